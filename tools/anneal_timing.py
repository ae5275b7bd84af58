#!/usr/bin/env python3
"""What the annealing schedules cost the captured train step: the step at the sizes of bench.py's cfg 2 on the sampler feed
(the batch-independent plan, every row may be a pair / labeled; 16384-row dataset, the captured step gathers its batch from the
epoch's index table) with every schedule off and with all three on (anneal_kl, anneal_yloss, anneal_learning_rate, mid-ramp),
the two engines captured in ONE process and timed in alternating windows (medians of the windows, device events around a run of
replays), the launches of either step by name, and what the next step's head spends parked on flag ``tail`` (wait site
``next_step``: the ticks the device itself counts).

  python tools/anneal_timing.py [--windows 20] [--replays 1000] [--out profiles/r17_anneal.md]

There is no target: the table is the deliverable.  The schedules-off step is the step as it ever was (its launch list is guarded
by tests/test_gpu_engine.py and tests/test_gpu_anneal.py)."""
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

MODES = ('off', 'on')
# mid-ramp for the whole measurement: ramps far longer than the replays timed (the coefficients change at every step)
ON = dict(anneal_kl=True, anneal_kl_itermax=1000000, anneal_yloss=True, anneal_yloss_itermax=1000000, anneal_yloss_offset=100,
          anneal_learning_rate=True, anneal_lr_itermax=1000000)
TICK_US = 0.01          # wall_clock64: the 100 MHz constant clock


def build(workload, sched, device, dataset_rows, n_table):
    """``bench.build``'s engine (same weights) with the schedules ``sched``, bound to the sampler feed over a synthetic dataset"""
    from drvae_amd import data as DD
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS[workload]
    cfg = E.StepConfig(kind=kind, L=L, **over, **sched)
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
    big = synth.make_batch(kind, dataset_rows, cfg.dim_x, cfg.dim_y, seed=77)
    tt = lambda k: torch.from_numpy(big[k]).to(device)
    ds = DD.DrVAEDataset(tt('x1'), tt('x2'), torch.zeros(dataset_rows, dtype=torch.int64, device=device), tt('y'), tt('has_x2'),
                         tt('has_y'))
    bat = DD.DeviceBatcher(ds, torch.ones(dataset_rows), rows, seed=5, mode='sampler')
    bat.bind(eng)
    bat.begin_epoch(n_batches=n_table)
    return eng, bat, desc


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


def window(eng, bat, n, n_table):
    """ms per step and ticks parked per step at site ``next_step`` over ``n`` replays behind a fresh index table"""
    from drvae_amd.schedule import SITE_INDEX
    bat.begin_epoch(n_batches=n_table)           # (drawn in place: the captured feed object stays)
    torch.cuda.synchronize()
    i = 2 * SITE_INDEX['next_step'] + 1
    t0 = int(eng.sync_err[i])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with eng.partition():
        e0.record()
        for _ in range(n):
            eng.replay()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (int(eng.sync_err[i]) - t0) / n


def measure(workload, windows, replays, device, dataset_rows=16384):
    n_table = max(1024, replays + 8)
    engs, bats, names, desc, tails = {}, {}, {}, '', {}
    for mode in MODES:
        eng, bat, desc = build(workload, ON if mode == 'on' else {}, device, dataset_rows, n_table)
        eng.train_step()                        # iteration 0, eagerly (the feed's first batch)
        names[mode] = capture_counting(eng)
        tails[mode] = eng._step_tail(False)
        engs[mode], bats[mode] = eng, bat
    for m in MODES:                              # warm every graph at the timed shape
        window(engs[m], bats[m], max(2, replays // 4), n_table)
    ms, park = {m: [] for m in MODES}, {m: [] for m in MODES}
    for _ in range(windows):                     # alternating, so that drift of the box hits both alike
        for m in MODES:
            t, p = window(engs[m], bats[m], replays, n_table)
            ms[m].append(t)
            park[m].append(p)
    for eng in engs.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values())
    d = collections.Counter(names['on'])
    d.subtract(collections.Counter(names['off']))
    out = dict(workload=workload, desc=desc, replays=replays, windows=windows, rows=dataset_rows,
               dual={m: e._side_graph is not None for m, e in engs.items()}, tails={m: t._asdict() for m, t in tails.items()},
               launches={m: len(v) for m, v in names.items()}, diff={k: v for k, v in sorted(d.items()) if v},
               same_order=names['on'] == names['off'], record=engs['on'].schedule_record(), iters=engs['on'].iters,
               median={m: statistics.median(v) for m, v in ms.items()}, lo={m: min(v) for m, v in ms.items()},
               hi={m: max(v) for m, v in ms.items()}, park={m: statistics.median(v) for m, v in park.items()},
               park_lo={m: min(v) for m, v in park.items()}, park_hi={m: max(v) for m, v in park.items()})
    del engs, bats
    torch.cuda.empty_cache()
    return out


def report(r):
    a, b = r['median']['off'], r['median']['on']
    t = r['tails']['on']
    lines = ['# Annealing schedules in the captured train step', '',
             '`tools/anneal_timing.py`: two engines at the sizes of `bench.py`\'s %s (%s) on the sampler feed (batch-independent plan,'
             % (r['workload'], r['desc']),
             'unbucketed; %d-row dataset, the captured step gathers its batch from the epoch\'s index table) live in one process;'
             % r['rows'],
             'windows alternate between them; a window is %d replays between two device events behind a freshly drawn table;'
             % r['replays'],
             'medians (min .. max) of %d windows per mode; the default CU partition of the two-graph step (64 CUs reserved for the'
             % r['windows'],
             'side chain, not tuned).  The absolute times are this tool\'s (untuned partition, windows that start behind a host',
             'synchronise, a shared box): compare the two modes with each other, not with `bench.py`\'s headline.  `off`: no',
             'schedule (the step as it was); `on`: anneal_kl + anneal_yloss (offset 100) + anneal_learning_rate, mid-ramp for the',
             'whole run (the coefficients change at every step).', '',
             '| schedules | ms / step | launches / step | schedule | parked on `tail` at the step\'s head (site `next_step`) |',
             '|---|---|---|---|---|']
    for m in MODES:
        lines.append('| %s | %.4f (%.4f .. %.4f) | %d | %s | %.0f ticks = %.2f us per step (%.0f .. %.0f ticks) |'
                     % (m, r['median'][m], r['lo'][m], r['hi'][m], r['launches'][m],
                        'two flag-ordered graphs' if r['dual'][m] else 'one graph', r['park'][m], r['park'][m] * TICK_US,
                        r['park_lo'][m], r['park_hi'][m]))
    lines += ['',
              'Against the schedules-off step the annealed step takes %+.2f %% (%+.4f ms).  Launches per step against the '
              'schedules-off step: %s; the two launch lists are %s.  The annealed engine\'s record after its last step (%d '
              'iterations): %s.' % (100.0 * (b - a) / a, b - a, ', '.join('%s %+d' % kv for kv in r['diff'].items()) or 'none',
                                    'identical, name for name and in order' if r['same_order'] else 'DIFFERENT in order',
                                    r['iters'], ', '.join('%s %.6g' % kv for kv in r['record'].items())), '',
              'The `tail` park: this step is recorded tail-gated (`Tail.tail_gated` = %s, `side_adam` = %s, `side_loss` = %s) with and '
              'without the schedules -- the feed launch, masks workgroup included, parks on flag `tail` at site `next_step` in BOTH '
              'modes, because that launch has always rewritten the per-row weights the tail\'s loss scalars read.  The schedules add '
              'no park and no launch; what the table\'s last column shows is what that existing park waits, per step, in either '
              'mode (ticks of the 100 MHz constant clock the device counts itself).  The schedule\'s own work is one thread\'s four '
              'double-precision divisions and 15 stores in the masks workgroup, and one 4-byte load per sweep launch.'
              % (t['tail_gated'], t['side_adam'], t['side_loss']), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg2')
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--replays', type=int, default=1000)       # (windows of 200 replays spread by 30 % on a shared box)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('anneal_timing: needs the GPU (a CPU run says nothing about the step\'s time)')
    text = report(measure(args.workload, args.windows, args.replays, torch.device('cuda', 0)))
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
