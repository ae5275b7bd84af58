#!/usr/bin/env python3
"""The precision ladder of the decoder-heads products -- ``matmul`` = 'fp32' | 'bf16x3' | 'bf16x2' | 'bf16x1' (``dv_gemm``,
``dv_gemm_x3``, ``dv_gemm_split`` with 2 and 1 parts) -- in ONE process, all four precisions ALTERNATING (A B C D A B C D ...:
clock state, cache state and whatever else drifts is shared), device events, warm-up first, >= 20 timed repetitions per figure:

  1. the three decoder-heads products of the wide configuration (cfg 5) alone;
  2. norm-wise error against float64 of all four at K = 2048, per layout;
  3. the captured cfg-5 train step with each ``matmul`` (the four engines resident together), and after 1 + warm-up +
     repetitions (= 24 by default) steps from one state the ELBO and the norm-wise parameter distance of every rung from
     the fp32 step.

The fp32 columns are the default path; nothing but an explicit ``matmul=`` / ``matmul_precision=`` selects another.  Its
output is the record profiles/r10_precision_ladder.txt:

    python tools/split_bench.py > profiles/r10_precision_ladder.txt

``--lab``: the K-tile depths of the cheaper rungs that the tuning build carries (a library compiled with -DDV_LAB, loaded
through DRVAE_HIP_LIB: ``dv_gemm_split(desc, parts + 16 * kt)`` runs the rung on a K tile of kt x 32), alternating, on the
three products -- the measurements behind profiles/r10_experiments.md.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import drvae_amd.kernels as K  # noqa: E402
from drvae_amd import _lib  # noqa: E402

LADDER = ('fp32', 'bf16x3', 'bf16x2', 'bf16x1')
KW = {'fp32': {}, 'bf16x3': dict(x3=True), 'bf16x2': dict(x3=True, parts=2), 'bf16x1': dict(x3=True, parts=1)}
ENTRY = {'fp32': 'dv_gemm', 'bf16x3': 'dv_gemm_x3', 'bf16x2': 'dv_gemm_split(2)', 'bf16x1': 'dv_gemm_split(1)'}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warm):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return {k: np.asarray(v) for k, v in out.items()}


def stats(v):
    return 'min %7.3f  median %7.3f  max %7.3f' % (v.min(), np.median(v), v.max())


def wide_operands(dev, rows=8192, X=20000, H=2048):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(rows, H, device=dev, generator=g)
    W = torch.randn(2 * X, H, device=dev, generator=g) * 0.02
    dpre = torch.randn(rows, 2 * X, device=dev, generator=g)
    yref = torch.randn(rows, H, device=dev, generator=g)
    out, dW, dx = torch.empty(rows, 2 * X, device=dev), torch.empty(2 * X, H, device=dev), torch.empty(rows, H, device=dev)
    # name -> (shape, launcher arguments, launcher keywords)
    return {
        'forward': ('%d x %d x %d  x W^T' % (rows, 2 * X, H), (out, x, W, True, True), dict(overread=True)),
        'dW': ('%d x %d x %d  dy^T x' % (2 * X, H, rows), (dW, dpre, x, False, False), dict(overread=True)),
        'dX': ('%d x %d x %d  (dy W) * act\'' % (rows, H, 2 * X), (dx, dpre, W, True, False),
               dict(epi=K.EPI_BWD, yref=yref, act0='elu', act1='elu', overread=True)),
    }, 2.0 * rows * 2 * X * H


def products(dev, reps, warm):
    calls, flop = wide_operands(dev)
    print('1. the three decoder-heads products of cfg 5, alone (ms; %d alternating repetitions after %d warm-up rounds;'
          ' TF/s = fp32-product-equivalent)' % (reps, warm))
    total = {k: 0.0 for k in LADDER}
    faster = {k: True for k in LADDER[1:]}
    for name, (shape, a, kw) in calls.items():
        t = alternate({k: (lambda k=k: K.gemm(*a, **kw, **KW[k])) for k in LADDER}, reps, warm)
        med = {k: float(np.median(t[k])) for k in LADDER}
        print('  %-8s %s' % (name, shape))
        for i, k in enumerate(LADDER):
            total[k] += med[k]
            print('      %-7s %-17s %s   %6.1f TF/s   %.2fx fp32%s'
                  % (k, ENTRY[k], stats(t[k]), flop / med[k] / 1e9, med['fp32'] / med[k],
                     '' if i == 0 else '   %.2fx %s' % (med[LADDER[i - 1]] / med[k], LADDER[i - 1])))
            if i > 0 and not med[k] < med[LADDER[i - 1]]:
                faster[k] = False
    print('  sum of the medians: ' + ', '.join('%s %.2f ms' % (k, total[k]) for k in LADDER))
    for k in LADDER[1:]:
        print('  %s is %s than the rung above it on all three products' % (k, 'faster' if faster[k] else 'NOT faster'))
    torch.cuda.empty_cache()


def accuracy(dev, Kd=2048, M=388, N=516):          # (dense operands: their rows must stay 16-B aligned in every layout)
    print('2. norm-wise error against float64 at K = %d (%d x %d, standard normal operands): ||c - c64|| / ||c64||' % (Kd, M, N))
    g = torch.Generator().manual_seed(11)
    Aop, Bop = torch.randn(M, Kd, generator=g), torch.randn(Kd, N, generator=g)
    c64 = Aop.double() @ Bop.double()
    for a_kc, b_kc in ((True, True), (True, False), (False, False)):
        A = (Aop if a_kc else Aop.t()).contiguous().to(dev)
        B = (Bop.t() if b_kc else Bop).contiguous().to(dev)
        err = {}
        for k in LADDER:
            Cm = torch.empty(M, N, device=dev)
            K.gemm(Cm, A, B, a_kc, b_kc, **KW[k])
            err[k] = float(torch.linalg.norm(Cm.cpu().double() - c64) / torch.linalg.norm(c64))
        print('  layout (a_kcontig, b_kcontig) = (%d, %d): ' % (a_kc, b_kc) + '   '.join('%s %.3e' % (k, err[k]) for k in LADDER))


def step(dev, reps, warm):
    kind, rows, L, over, desc = bench.WORKLOADS['wide']
    engs = {}
    for name in LADDER:
        wl = 'wide' if name == 'fp32' else 'wide_' + name
        if name != 'fp32':
            bench.WORKLOADS[wl] = (kind, rows, L, dict(over, matmul=name), desc)      # (this process only)
        cfg, eng, arena, batch, _ = bench.build(wl, dev, 0, 1)
        assert cfg.matmul == name and eng.plan.c_decx.x3_last == (name != 'fp32')
        eng.train_step()
        eng.capture()
        engs[name] = (eng, arena)
    t = alternate({k: e.replay for k, (e, _) in engs.items()}, reps, warm)
    for k, (e, _) in engs.items():
        e.check_sync()
    med = {k: float(np.median(t[k])) for k in LADDER}
    print('3. the captured cfg-5 train step (%s; ms per step, %d alternating repetitions after %d warm-up rounds)' % (desc, reps, warm))
    for k in LADDER:
        print('      matmul=%-7s %s   %.2fx fp32' % (k, stats(t[k]), med['fp32'] / med[k]))
    p32 = engs['fp32'][1].param
    print('      after %d steps each from the same state:' % (1 + warm + reps))
    for k in LADDER:
        e, a = engs[k]
        print('        %-7s ELBO %.4f   parameters norm-wise %.2e from the fp32 step\'s'
              % (k, e.losses()['ELBO'], float((a.param - p32).norm() / p32.norm())))


def lab(dev, reps, warm):
    lib = _lib.load()
    calls, flop = wide_operands(dev)
    variants = [('bf16x3 kt=1', 3, 0), ('bf16x2 kt=1', 2, 1), ('bf16x2 kt=2', 2, 2), ('bf16x1 kt=1', 1, 1), ('bf16x1 kt=2', 1, 2),
                ('bf16x1 kt=4', 1, 4)]
    print('lab: K tile = kt x 32 per rung (ms; %d alternating repetitions after %d warm-up rounds)' % (reps, warm))
    for name, (shape, a, kw) in calls.items():
        d = K._gemm_desc(*a, **kw)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fns = {}
        for label, parts, kt in variants:
            rc = lib.dv_gemm_split(ctypes.byref(d), parts + 16 * kt, stream)
            if rc != 0:
                print('      %-12s not in this library (status %d)' % (label, rc))
                continue
            fns[label] = lambda code=parts + 16 * kt: lib.dv_gemm_split(ctypes.byref(d), code, stream)
        t = alternate(fns, reps, warm)
        print('  %-8s %s' % (name, shape))
        for label in fns:
            print('      %-12s %s   %6.1f TF/s' % (label, stats(t[label]), flop / float(np.median(t[label])) / 1e9))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--lab', action='store_true')
    args = ap.parse_args()
    assert args.reps >= 20
    dev = torch.device('cuda', 0)
    print('dtype ladder (opt-in): bf16x3 (three bf16 parts per operand, six MFMA terms) | bf16x2 (two parts, three terms) | '
          'bf16x1 (one part, one term: a bf16 product), fp32 accumulation, against dtype: fp32 (MFMA, the default)')
    print('device: %s' % torch.cuda.get_device_name(dev))
    if args.lab:
        lab(dev, args.reps, args.warmup)
        sys.exit(0)
    products(dev, args.reps, args.warmup)
    accuracy(dev)
    if not args.skip_step:
        step(dev, args.reps, args.warmup)
