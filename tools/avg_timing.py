#!/usr/bin/env python3
"""What parameter averaging (``ema_decay``) and decoupled weight decay (``optim_alg='adamw'``) cost.

1. The captured train step at the sizes of bench.py's cfg 2 and cfg 5 (the wide configuration) on a resident batch, with
   off | average | AdamW | both: four engines captured in ONE process per workload and timed in alternating windows (device
   events around a run of replays; median, min .. max of the windows).
2. The optimiser sweep alone at 125 M parameters (``adam_stream_kernel``), the same four modes alternating, in ms and TB/s
   of the traffic each mode is derived to move (7 words per parameter, 9 with the average), next to the sweep of a PARENT
   library loaded into the same process (``--parent-lib``: a libdrvae_hip.so built from the parent commit; its
   ``dv_adam_l2`` reads the leading 32 bytes of the same ``dv_adam_hyper``).

  python tools/avg_timing.py [--windows 12] [--parent-lib PATH] [--out profiles/r18_avg.md]

There is no target: the table is the deliverable, and nothing here is asserted in a test."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

D = 0.999
MODES = (('off', {}), ('average', dict(ema_decay=D)), ('AdamW', dict(optim_alg='adamw')),
         ('both', dict(ema_decay=D, optim_alg='adamw')))
REPLAYS = {'cfg2': 1000, 'cfg5': 20}
N_SWEEP = 125 * 1000 * 1000


def build(workload, opts, device):
    """``bench.build``'s engine (same weights, same resident batch) with the options ``opts``, iteration 0 run and the
    steady-state step captured"""
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS[workload]
    cfg = E.StepConfig(kind=kind, L=L, **over, **opts)
    shapes = E.param_shapes(cfg)
    arena = ParamArena(shapes, device)
    rs, fan = np.random.RandomState(123), 1
    for k, shp in shapes.items():
        if k.endswith('W_mu') or k.endswith('bias_mu'):
            a = rs.uniform(-1e-4, 1e-4, shp)
        else:
            if k.endswith('.weight'):
                fan = shp[1]
            a = rs.uniform(-1, 1, shp) / np.sqrt(fan)
        arena.p(k).copy_(torch.as_tensor(a, dtype=torch.float32))
    eng = E.FusedStep(cfg, arena, seed=1000, concurrent=bool(tuning.get('concurrent')))
    batch = synth.make_batch(kind, rows, cfg.dim_x, cfg.dim_y, seed=1234)
    hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
    t = lambda k: torch.from_numpy(batch[k]).to(device)
    eng.set_batch(t('x1'), t('x2'), batch['y'], hx, hy)
    eng.train_step()
    eng.capture()
    return eng, desc, arena.n_live


def window(eng, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with eng.partition():
        e0.record()
        for _ in range(n):
            eng.replay()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure_step(workload, windows, device):
    replays = REPLAYS[workload]
    engs, desc, n_live = {}, '', 0
    for name, opts in MODES:
        engs[name], desc, n_live = build(workload, opts, device)
    for e in engs.values():
        window(e, max(2, replays // 4))
    ms = {name: [] for name, _ in MODES}
    for _ in range(windows):                     # alternating, so that drift of the box hits every mode alike
        for name, _ in MODES:
            ms[name].append(window(engs[name], replays))
    for e in engs.values():
        e.check_sync()
        assert all(np.isfinite(v) for v in e.losses().values())
    out = dict(workload=workload, desc=desc, replays=replays, windows=windows, n_live=n_live,
               dual={k: e._side_graph is not None for k, e in engs.items()}, ms=ms)
    del engs
    torch.cuda.empty_cache()
    return out


def measure_sweep(windows, device, parent_lib, n=N_SWEEP, reps=10):
    """the sweep alone: ``reps`` launches between two device events per window, modes alternating"""
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    g = torch.randn(n, device=device)
    p, m, v, e = (torch.zeros(n, device=device) for _ in range(4))
    v.fill_(1.0)
    step = torch.ones(1, dtype=torch.int32, device=device)
    hyper = dict(lr=5e-4, weight_decay=0.05)
    calls = {
        'off': lambda: K.adam_l2(p, g, m, v, step, **hyper),
        'average': lambda: K.adam_l2(p, g, m, v, step, avg=e, avg_decay=D, **hyper),
        'AdamW': lambda: K.adam_l2(p, g, m, v, step, decoupled=True, **hyper),
        'both': lambda: K.adam_l2(p, g, m, v, step, decoupled=True, avg=e, avg_decay=D, **hyper),
    }
    words = {'off': 7, 'average': 9, 'AdamW': 7, 'both': 9}
    if parent_lib:
        lib = C.CDLL(parent_lib)
        lib.dv_adam_l2.argtypes = _lib.SIGNATURES['dv_adam_l2']
        lib.dv_adam_l2.restype = C.c_int
        h = _lib.AdamHyper(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, gscale=1.0)

        def parent():
            rc = lib.dv_adam_l2(K._f32(p), K._f32(g), K._f32(m), K._f32(v), n, C.byref(h), K._i32(step), None, 0, K._stream())
            assert rc == 0, rc
        calls = dict(parent=parent, **calls)
        words['parent'] = 7
    ms = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(3):
            fn()
    for _ in range(windows):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return dict(n=n, reps=reps, ms=ms, words=words)


def _row(v):
    return '%.4f (%.4f .. %.4f)' % (statistics.median(v), min(v), max(v))


def report(steps, sw):
    lines = ['# Parameter averaging and AdamW in the optimiser sweep: what they cost', '',
             '`tools/avg_timing.py`, one MI355X.  Modes alternate in one process; median (min .. max) of the windows.  The absolute',
             'step times are this tool\'s (windows that start behind a host synchronise, a shared box): compare the modes with',
             'each other, not with `bench.py`\'s headline.  `off` is the step as it was; average: `ema_decay=%g`; AdamW:' % D,
             '`optim_alg=\'adamw\'`.', '']
    for r in steps:
        lines += ['## The captured step, %s (%s)' % (r['workload'], r['desc']), '',
                  '%d live parameters; %d windows of %d replays per mode, resident batch.' % (r['n_live'], r['windows'], r['replays']),
                  '', '| mode | ms / step | against off | schedule |', '|---|---|---|---|']
        base = statistics.median(r['ms']['off'])
        for name, _ in MODES:
            med = statistics.median(r['ms'][name])
            lines.append('| %s | %s | %+.2f %% | %s |' % (name, _row(r['ms'][name]), 100.0 * (med - base) / base,
                                                          'two flag-ordered graphs' if r['dual'][name] else 'one graph'))
        lines.append('')
    lines += ['## The sweep alone, %d parameters (`adam_stream_kernel`)' % sw['n'], '',
              '%d launches between two device events per window.  TB/s: the traffic each mode is DERIVED to move (words per'
              % sw['reps'],
              'parameter x 4 bytes: p, g, m, v read and p, m, v written = 7; the average read and written = 9) over the measured time.',
              '`parent`: `dv_adam_l2` of a library built from the parent commit, loaded into the same process.', '',
              '| sweep | words / parameter | ms | TB/s | time against off |', '|---|---|---|---|---|']
    base = statistics.median(sw['ms']['off'])
    for k, v in sw['ms'].items():
        med = statistics.median(v)
        lines.append('| %s | %d | %s | %.2f | x %.3f |' % (k, sw['words'][k], _row(v), sw['words'][k] * 4 * sw['n'] / med / 1e9,
                                                            med / base))
    avg = statistics.median(sw['ms']['average'])
    lines += ['', 'Derived expectation for the average: 9/7 = x 1.286 of the plain sweep\'s time at equal bandwidth.  Measured: x %.3f '
              '(average) and x %.3f (both).' % (avg / base, statistics.median(sw['ms']['both']) / base), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=12)
    ap.add_argument('--workloads', default='cfg2,cfg5')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('avg_timing: needs the GPU (a CPU run says nothing about the step\'s time)')
    dev = torch.device('cuda', 0)
    steps = [measure_step(w, args.windows, dev) for w in args.workloads.split(',') if w]
    text = report(steps, measure_sweep(args.windows, dev, args.parent_lib))
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
