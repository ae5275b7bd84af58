#!/usr/bin/env python3
"""What hidden-layer dropout costs the captured train step: the step at the sizes of bench.py's cfg 2 and cfg 5 with
``dropout_rate`` 0 and 0.5, both engines captured in ONE process and timed in alternating windows (medians of 20 windows, device
events around a run of replays), and the launches the dropped step adds, by name (every C-ABI call of the capture is one launch).

  python tools/dropout_timing.py [--workloads cfg2,cfg5] [--windows 20] [--out profiles/r13_dropout.md]

There is no target for the dropped step: the table is the deliverable.  The rate-0 step is the step as it ever was (its launch
list is guarded by tests/test_gpu_engine.py and tests/test_gpu_dropout.py)."""
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

RATES = (0.0, 0.5)
REPLAYS = {'cfg2': 200, 'cfg5': 4}        # replays per timed window: tens of milliseconds of device work at either size


def build(workload, rate, device):
    """``bench.build`` (same weights, same batch) with a dropout rate"""
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS[workload]
    cfg = E.StepConfig(kind=kind, L=L, dropout_rate=rate, **over)
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


def measure(workload, windows, device):
    engs, names, desc = {}, {}, ''
    for rate in RATES:
        eng, desc = build(workload, rate, device)
        eng.train_step()                       # iteration 0 (the annealing coefficient differs), eagerly
        names[rate] = capture_counting(eng)
        engs[rate] = eng
    n = REPLAYS[workload]
    for eng in engs.values():                  # warm every graph at the timed shape
        window(eng, max(2, n // 4))
    ms = {rate: [] for rate in RATES}
    for _ in range(windows):                   # alternating, so that drift of the box hits both alike
        for rate in RATES:
            ms[rate].append(window(engs[rate], n))
    for eng in engs.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values())
    added = collections.Counter(names[0.5])
    added.subtract(collections.Counter(names[0.0]))
    eng = engs[0.5]
    out = dict(workload=workload, desc=desc, replays=n, windows=windows, sites=len(eng.dropout_sites()),
               mask_elements=sum(s['M'] * s['N'] for s in eng.dropout_sites()),
               dual={r: e._side_graph is not None for r, e in engs.items()},
               launches={r: len(v) for r, v in names.items()}, added={k: v for k, v in sorted(added.items()) if v},
               median={r: statistics.median(v) for r, v in ms.items()}, lo={r: min(v) for r, v in ms.items()},
               hi={r: max(v) for r, v in ms.items()})
    del engs
    torch.cuda.empty_cache()
    return out


def report(results):
    lines = ['# Hidden-layer dropout in the captured train step', '',
             '`tools/dropout_timing.py`: both engines of a size live in one process; windows alternate between them; a window is',
             'a run of replays between two device events; medians (min .. max) of the windows, in ms per step; the default CU',
             'partition of the two-graph step (64 CUs reserved for the side chain, not tuned) for both rates.  The absolute',
             'times are this tool\'s (untuned partition, windows that start behind a host synchronise, a shared box): compare the',
             'two rates with each other, not with `bench.py`\'s headline.', '',
             '| size | rate | ms / step | launches / step | schedule |', '|---|---|---|---|---|']
    for r in results:
        for rate in RATES:
            lines.append('| %s | %.1f | %.4f (%.4f .. %.4f) | %d | %s |'
                         % (r['workload'], rate, r['median'][rate], r['lo'][rate], r['hi'][rate], r['launches'][rate],
                            'two flag-ordered graphs' if r['dual'][rate] else 'one graph'))
    lines.append('')
    for r in results:
        a, b = r['median'][0.0], r['median'][0.5]
        lines += ['**%s** (%s): %d windows of %d replays per rate.  %d dropout sites, %.2f M mask elements drawn per step.  The '
                  'dropped step takes %+.1f %% (%+.4f ms); launches added per step: %s.'
                  % (r['workload'], r['desc'], r['windows'], r['replays'], r['sites'], r['mask_elements'] / 1e6,
                     100.0 * (b - a) / a, b - a,
                     ', '.join('%s %+d' % kv for kv in r['added'].items()) or 'none'), '']
    lines += ['A plan with sites draws at the head of its step (the side chain does not draw ahead: the encoder backward reads its',
              'masks), so the plain `dv_fill_normal_rows` leaves the list and `dv_fill_noise_rows` joins it, next to one `dv_mask_scale` per',
              'site and pass.', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='cfg2,cfg5')
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('dropout_timing: needs the GPU (a CPU run says nothing about the step\'s time)')
    dev = torch.device('cuda', 0)
    text = report([measure(w, args.windows, dev) for w in args.workloads.split(',')])
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
