#!/usr/bin/env python3
"""Timing of the device-carried nuisance variable at config 4's sizes (VFAE, 978 genes, z = 100, B = 150, L = 2), in ONE
process, the legs alternating and the whole round repeated (spread = max - min over the rounds):

  A  captured step, use_s + use_MMD (rbf_fourier), host-list penalty on a resident batch   (bench.py's cfg4_mmd)
  B  the same model on DeviceBatcher(carry_s=True): resident epoch feed + the grouped penalty
  C  one training epoch of a use_s model WITHOUT the penalty, DeviceBatcher.feed() in front of every replay
  D  the same epoch on DeviceBatcher(carry_s=True): begin_epoch + replays

Every leg runs inside ``partition()`` with the default CU split (no per-leg tuning).  Prints one JSON line;
``--out FILE`` also writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def dataset(cfg, rows, device, seed=77):
    from drvae_amd import data as D, synth
    big = synth.make_batch(cfg.kind, rows, cfg.dim_x, cfg.dim_y, seed=seed)
    t = lambda k: torch.from_numpy(big[k]).to(device)
    s = torch.from_numpy((np.arange(rows) * 7 // 3 % cfg.dim_s).astype(np.int64)).to(device)
    return D.DrVAEDataset(t('x1'), t('x2'), s, t('y'), t('has_x2'), t('has_y'))


def leg(workload, device, carry, n_table, rows=8192):
    """(engine, batcher | None) of one leg, its step captured"""
    from drvae_amd import data as D
    cfg, eng, arena, batch, _ = bench.build(workload, device, 0, 1)
    eng.train_step()                     # iteration 0 runs eagerly (beta_pert = 0.01 only there)
    bat = None
    if carry is not None:
        hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
        gc = [int(((hy == bool(gy)) & (hx == bool(gx))).sum()) for (gy, gx) in D._GROUPS]
        bat = D.DeviceBatcher(dataset(cfg, rows, device), torch.ones(rows), len(hx), group_counts=gc, seed=5, carry_s=carry)
        bat.bind(eng)
        if carry:
            bat.begin_epoch(n_batches=n_table)
        else:
            bat.feed()
    eng.capture()
    return eng, bat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--epoch-batches', type=int, default=54)       # 8192 rows / 150
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    device = torch.device('cuda:0')
    bench.WORKLOADS['cfg4_s'] = ('vfae', 150, 2, {'add_noise_var': 0.0, 'use_s': True, 'dim_s': 2}, 'cfg 4 + use_s, no penalty')
    A = leg('cfg4_mmd', device, None, 0)
    B = leg('cfg4_mmd', device, True, args.steps + 8)
    Cc = leg('cfg4_s', device, False, 0)
    Dd = leg('cfg4_s', device, True, args.epoch_batches)

    def region(eng, n, before=None, each=None):
        with eng.partition():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if before is not None:
                before()
            for _ in range(n):
                if each is not None:
                    each()
                eng.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

    runs = {
        'A_hostlist_step_ms': lambda: region(A[0], args.steps),
        'B_device_step_ms': lambda: region(B[0], args.steps, before=lambda: B[1].begin_epoch(n_batches=args.steps + 8)),
        'C_feed_epoch_ms_per_step': lambda: region(Cc[0], args.epoch_batches, each=Cc[1].feed),
        'D_resident_epoch_ms_per_step': lambda: region(Dd[0], args.epoch_batches,
                                                        before=lambda: Dd[1].begin_epoch(n_batches=args.epoch_batches)),
    }
    for fn in runs.values():             # one untimed round: code objects, allocator, the first table
        fn()
    out = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            out[k].append(fn())
    res = {'steps': args.steps, 'epoch_batches': args.epoch_batches, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
    for k, v in out.items():
        res[k] = {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'spread': max(v) - min(v), 'all': v}
    for e, _ in (A, B, Cc, Dd):
        e.check_sync()
        assert all(np.isfinite(x) for x in e.losses().values())
    res['mmd_last'] = {'A': A[0].losses().get('MMD'), 'B': B[0].losses().get('MMD')}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
