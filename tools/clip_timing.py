#!/usr/bin/env python3
"""What gradient-norm clipping costs the captured train step: the step at the sizes of bench.py's cfg 2 and cfg 5 with
``max_grad_norm`` None (the switch off), inf (the non-finite guard alone) and a finite threshold at half of the step's gradient
norm, the three engines captured in ONE process and timed in alternating windows (medians of 20 windows, device events around a
run of replays), and the launches the clipped step adds and loses, by name (every C-ABI call of the capture is one launch; the norm pass is one call with two).

  python tools/clip_timing.py [--workloads cfg2,cfg5] [--windows 20] [--out profiles/r14_clip.md]

There is no target for the clipped step: the table is the deliverable.  The switch-off step is the step as it ever was (its
launch list is guarded by tests/test_gpu_engine.py and tests/test_gpu_clip.py)."""
import argparse
import collections
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MODES = ('off', 'inf', 'finite')
REPLAYS = {'cfg2': 200, 'cfg5': 4}        # replays per timed window: tens of milliseconds of device work at either size


def build(workload, max_grad_norm, device):
    """``bench.build`` (same weights, same batch) with a clip threshold"""
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS[workload]
    cfg = E.StepConfig(kind=kind, L=L, max_grad_norm=max_grad_norm, **over)
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
    t = lambda k: torch.from_numpy(batch[k]).to(device)
    eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'].astype(bool), batch['has_y'].astype(bool))
    return eng, desc


def capture_counting(eng):
    """capture the step; -> the names of its launches (the warm-up pass in front of the capture is not part of the step)"""
    from drvae_amd import _lib
    names, on = [], [False]
    real_check, real_main = _lib.check, eng._capture_main

    def check(code, what):
        if on[0] and not what.startswith('dv_gemm_set_option'):
            names.append(what)
        return real_check(code, what)

    def capture_main(*a, **k):
        on[0] = True
        return real_main(*a, **k)
    _lib.check, eng._capture_main = check, capture_main
    try:
        eng.capture()
    finally:
        _lib.check = real_check
        del eng._capture_main
    return names


def window(eng, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with eng.partition():
        e0.record()
        for _ in range(n):
            eng.replay()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def norm_pass_alone(eng, calls=50):
    """(ms per norm pass over the engine's live gradient slice, ms per norm pass over ONE element) by device events around
    ``calls`` back-to-back passes, nothing else on the device: the second is what the two launches cost with nothing to read"""
    from drvae_amd import kernels as K
    a, out = eng.arena, []
    for g in (a.grad[:a.n_live], a.grad[:1]):
        for _ in range(3):
            K.clip_norm(g, eng.clip_state)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            K.clip_norm(g, eng.clip_state)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def measure(workload, windows, device):
    engs, names, desc = {}, {}, ''
    # the finite threshold: half of the norm the guard-only engine reports for its first step
    probe, _ = build(workload, float('inf'), device)
    probe.train_step()
    norm0 = probe.clip_stats()['norm']
    del probe
    for mode in MODES:
        eng, desc = build(workload, {'off': None, 'inf': float('inf'), 'finite': 0.5 * norm0}[mode], device)
        eng.train_step()                       # iteration 0 (the annealing coefficient differs), eagerly
        names[mode] = capture_counting(eng)
        engs[mode] = eng
    n = REPLAYS[workload]
    for eng in engs.values():                  # warm every graph at the timed shape
        window(eng, max(2, n // 4))
    ms = {mode: [] for mode in MODES}
    for _ in range(windows):                   # alternating, so that drift of the box hits all alike
        for mode in MODES:
            ms[mode].append(window(engs[mode], n))
    for eng in engs.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values())
    diff = {}
    for mode in MODES[1:]:
        d = collections.Counter(names[mode])
        d.subtract(collections.Counter(names['off']))
        diff[mode] = {k: v for k, v in sorted(d.items()) if v}
    stats = {m: engs[m].clip_stats() for m in MODES[1:]}
    alone = norm_pass_alone(engs['finite'])
    out = dict(workload=workload, desc=desc, replays=n, windows=windows, n_live=engs['off'].arena.n_live, alone=alone,
               partials=engs['finite'].clip_part.numel(), norm0=norm0,
               stats=stats, ahead={m: bool(e.noise_ahead) for m, e in engs.items()},
               dual={m: e._side_graph is not None for m, e in engs.items()},
               launches={m: len(v) for m, v in names.items()}, diff=diff,
               median={m: statistics.median(v) for m, v in ms.items()}, lo={m: min(v) for m, v in ms.items()},
               hi={m: max(v) for m, v in ms.items()})
    del engs
    torch.cuda.empty_cache()
    return out


def report(results):
    lines = ['# Gradient-norm clipping in the captured train step', '',
             '`tools/clip_timing.py`: the three engines of a size live in one process; windows alternate between them; a window is',
             'a run of replays between two device events; medians (min .. max) of the windows, in ms per step; the default CU',
             'partition of the two-graph step (64 CUs reserved for the side chain, not tuned) for all.  The absolute times are',
             'this tool\'s (untuned partition, windows that start behind a host synchronise, a shared box): compare the three',
             'modes with each other, not with `bench.py`\'s headline.  `off`: `max_grad_norm=None`; `inf`: the non-finite guard',
             'alone; `finite`: a threshold at half of the first step\'s gradient norm.', '',
             '| size | max_grad_norm | ms / step | launches / step | schedule | noise drawn ahead |', '|---|---|---|---|---|---|']
    for r in results:
        for m in MODES:
            lines.append('| %s | %s | %.4f (%.4f .. %.4f) | %d | %s | %s |'
                         % (r['workload'], m, r['median'][m], r['lo'][m], r['hi'][m], r['launches'][m],
                            'two flag-ordered graphs' if r['dual'][m] else 'one graph', 'yes' if r['ahead'][m] else 'no'))
    lines.append('')
    for r in results:
        a = r['median']['off']
        lines += ['**%s** (%s): %d windows of %d replays per mode.  The norm launch reads %.2f M gradient elements (%.1f MB) into '
                  '%d double partials; first-step norm %.4g.  Against the switch-off step the guard alone takes %+.1f %% (%+.4f '
                  'ms), the finite threshold %+.1f %% (%+.4f ms).  Launches per step against the switch-off step: %s.  Last '
                  'step: coef %.4f, %d step(s) skipped.  The norm pass ALONE (both launches back to back, nothing else on the '
                  'device, device events around 50 passes): %.4f ms over this slice = %.2f TB/s, %.4f ms over one element (the '
                  'two launches with nothing to read; with the slice\'s number of partials the finalisation, one thread adding '
                  'them in index order, is in the first figure and was not timed by itself).'
                  % (r['workload'], r['desc'], r['windows'], r['replays'], r['n_live'] / 1e6, r['n_live'] * 4 / 1e6, r['partials'],
                     r['norm0'], 100.0 * (r['median']['inf'] - a) / a, r['median']['inf'] - a,
                     100.0 * (r['median']['finite'] - a) / a, r['median']['finite'] - a,
                     ', '.join('%s %+d' % kv for kv in r['diff']['finite'].items()) or 'none',
                     r['stats']['finite']['coef'], r['stats']['finite']['n_skipped'],
                     r['alone'][0], r['n_live'] * 4 / 1e9 / r['alone'][0], r['alone'][1]), '']
    lines += ['A clipped step needs every gradient final in front of the norm launch: where the switch-off step runs the',
              'classifier\'s weight gradient, the decoder heads\' half of the sweep, the loss scalars and the next step\'s draw on',
              'the side chain behind the join (`dv_adam_l2_gated` on the main chain, a second `dv_adam_l2` on the side chain), the',
              'clipped step keeps all of it in front of the join and sweeps the whole arena once, ungated (`dv_adam_l2_clipped`),',
              'behind the norm pass (`dv_grad_norm_clip`: one call, two launches -- the sum of squares and its finalisation).', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='cfg2,cfg5')
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('clip_timing: needs the GPU (a CPU run says nothing about the step\'s time)')
    dev = torch.device('cuda', 0)
    text = report([measure(w, args.windows, dev) for w in args.workloads.split(',')])
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
