#!/usr/bin/env python3
"""Timing of the nuisance variable on sampler-mode device batches at config 4's sizes (VFAE, 978 genes, z = 100, B = 150,
L = 2, use_s + use_MMD, rbf_fourier), in ONE process, the legs alternating and the whole round repeated (spread = max - min
over the rounds).  Every leg is one training epoch of 54 batches (8192 rows / 150), ms per step:

  a  sampler-drawn batches on DeviceBatcher(mode='sampler', carry_s='masked'): begin_epoch + replays of ONE captured step
  b  the SAME batches (a's epoch table) the way the host-list step takes them: per batch ``set_batch(..., s=host)`` -- a plan
     per batch structure, host row lists for the penalty -- and an eager ``train_step()`` (a captured step would hold for one
     composition of groups and classes only); the table and the dataset's s / has_y columns are on the host before the clock
     starts
  c  stratified batches on DeviceBatcher(carry_s=True): begin_epoch + replays (the cheaper plan, for context)

Legs a and c run inside ``partition()`` with the default CU split (no per-leg tuning).  Prints one JSON line; ``--out FILE``
also writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.nuisance_feed_timing import dataset  # noqa: E402


def engine(device):
    cfg, eng, arena, batch, _ = bench.build('cfg4_mmd', device, 0, 1)
    eng.train_step()                     # iteration 0 runs eagerly (beta_pert = 0.01 only there)
    return cfg, eng, batch


def main():
    from drvae_amd import data as D
    ap = argparse.ArgumentParser()
    ap.add_argument('--epoch-batches', type=int, default=54)       # 8192 rows / 150
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    device = torch.device('cuda:0')
    n_b, rows = args.epoch_batches, args.rows
    # a: the reference's sampler on the masked carry
    cfg, ea, batch = engine(device)
    ds = dataset(cfg, rows, device)
    B = len(batch['has_y'])
    ba = D.DeviceBatcher(ds, torch.ones(rows), B, seed=5, mode='sampler', carry_s='masked')
    ba.bind(ea)
    ba.begin_epoch(n_batches=n_b)
    ea.capture()
    ba.rebase()
    # b: host-list steps over a's table
    _, eb, _ = engine(device)
    host = {k: getattr(ds, k).reshape(-1).cpu().numpy() for k in ('s', 'has_y', 'y')}
    no_pairs = np.zeros(B, bool)
    # c: stratified carried step
    _, ec, _ = engine(device)
    hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
    gc = [int(((hy == bool(gy)) & (hx == bool(gx))).sum()) for (gy, gx) in D._GROUPS]
    bc = D.DeviceBatcher(ds, torch.ones(rows), B, group_counts=gc, seed=5, carry_s=True)
    bc.bind(ec)
    bc.begin_epoch(n_batches=n_b)
    ec.capture()
    bc.rebase()

    def resident(eng, bat):
        with eng.partition():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bat.begin_epoch(n_batches=n_b)
            for _ in range(n_b):
                eng.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n_b

    def hostlist():
        tab = ba.global_table.cpu().numpy()          # (before the clock starts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(n_b):
            r = tab[b]
            i = torch.from_numpy(r).to(device)
            eb.set_batch(ds.x1[i], None, host['y'][r], no_pairs, host['has_y'][r], s=host['s'][r])
            eb.train_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_b

    runs = {'a_masked_sampler_epoch_ms_per_step': lambda: resident(ea, ba),
            'b_hostlist_same_batches_ms_per_step': hostlist,
            'c_stratified_carried_epoch_ms_per_step': lambda: resident(ec, bc)}
    for fn in runs.values():             # one untimed round: code objects, allocator, the first tables
        fn()
    out = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            out[k].append(fn())
    res = {'epoch_batches': n_b, 'rounds': args.rounds, 'rows': rows, 'batch': B, 'device': torch.cuda.get_device_name(0),
           'plans': {'a': len(ea._plans), 'b': len(eb._plans), 'c': len(ec._plans)}}
    for k, v in out.items():
        res[k] = {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'spread': max(v) - min(v), 'all': v}
    for e in (ea, eb, ec):
        e.join_side()
        e.check_sync()
        assert all(np.isfinite(x) for x in e.losses().values())
    res['mmd_last'] = {'a': ea.losses().get('MMD'), 'b': eb.losses().get('MMD'), 'c': ec.losses().get('MMD')}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
