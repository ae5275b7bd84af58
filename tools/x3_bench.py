#!/usr/bin/env python3
"""The opt-in split-bf16 path (dtype: bf16x3 -- ``dv_gemm_x3``, ``StepConfig.matmul='bf16x3'``) next to the fp32 MFMA path, in
ONE process, the two precisions ALTERNATING (A B A B ...: clock state, cache state and whatever else drifts is shared), device
events, warm-up first, >= 20 timed repetitions per figure:

  1. the three decoder-heads products of the wide configuration (cfg 5) alone: fp32 ``dv_gemm`` against ``dv_gemm_x3``;
  2. norm-wise accuracy against float64 of both at K = 2048, per layout;
  3. the captured cfg-5 train step, ``matmul='fp32'`` against ``'bf16x3'`` (both engines resident together).

The fp32 columns are the default path.  The lab figures printed next to them are the library-GEMM form of
tools/bf16x3_step.py (profiles/r06_lab_bf16x3.txt).  Its output is the record profiles/r07_bf16x3.txt:

    python tools/x3_bench.py > profiles/r07_bf16x3.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import drvae_amd.kernels as K  # noqa: E402

LAB_MS = {'forward': 6.34, 'dW': 9.06, 'dX': 7.13, 'step': 27.03}      # profiles/r06_lab_bf16x3.txt (splits included)


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


def products(dev, reps, warm, rows=8192, X=20000, H=2048):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(rows, H, device=dev, generator=g)
    W = torch.randn(2 * X, H, device=dev, generator=g) * 0.02
    dpre = torch.randn(rows, 2 * X, device=dev, generator=g)
    yref = torch.randn(rows, H, device=dev, generator=g)
    out, dW, dx = torch.empty(rows, 2 * X, device=dev), torch.empty(2 * X, H, device=dev), torch.empty(rows, H, device=dev)
    calls = {
        'forward': ('%d x %d x %d  x W^T' % (rows, 2 * X, H), lambda k: K.gemm(out, x, W, True, True, overread=True, **k)),
        'dW': ('%d x %d x %d  dy^T x' % (2 * X, H, rows), lambda k: K.gemm(dW, dpre, x, False, False, overread=True, **k)),
        'dX': ('%d x %d x %d  (dy W) * act\'' % (rows, H, 2 * X),
               lambda k: K.gemm(dx, dpre, W, True, False, epi=K.EPI_BWD, yref=yref, act0='elu', act1='elu', overread=True, **k)),
    }
    flop = 2.0 * rows * 2 * X * H
    print('1. the three decoder-heads products of cfg 5, alone (ms; %d alternating repetitions after %d warm-up rounds)' % (reps, warm))
    total = {'fp32': 0.0, 'bf16x3': 0.0}
    for name, (shape, f) in calls.items():
        t = alternate({'fp32': lambda f=f: f({}), 'bf16x3': lambda f=f: f(dict(x3=True))}, reps, warm)
        m32, m3 = float(np.median(t['fp32'])), float(np.median(t['bf16x3']))
        total['fp32'] += m32
        total['bf16x3'] += m3
        print('  %-8s %s' % (name, shape))
        print('      fp32 dv_gemm      %s   %6.1f TF/s' % (stats(t['fp32']), flop / m32 / 1e9))
        print('      bf16x3 dv_gemm_x3 %s   %6.1f TF/s-equivalent   %.2fx   (lab form, library GEMM + split passes: %.2f ms)'
              % (stats(t['bf16x3']), flop / m3 / 1e9, m32 / m3, LAB_MS[name]))
    print('  sum of the medians: fp32 %.2f ms, bf16x3 %.2f ms (lab form %.2f ms)'
          % (total['fp32'], total['bf16x3'], LAB_MS['forward'] + LAB_MS['dW'] + LAB_MS['dX']))
    del x, W, dpre, yref, out, dW, dx
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
        for x3 in (False, True):
            Cm = torch.empty(M, N, device=dev)
            K.gemm(Cm, A, B, a_kc, b_kc, **(dict(x3=True) if x3 else {}))
            err[x3] = float(torch.linalg.norm(Cm.cpu().double() - c64) / torch.linalg.norm(c64))
        print('  layout (a_kcontig, b_kcontig) = (%d, %d): fp32 %.3e   bf16x3 %.3e   ratio %.2f   (lab form: 1.18)'
              % (a_kc, b_kc, err[False], err[True], err[True] / err[False]))


def step(dev, reps, warm):
    kind, rows, L, over, desc = bench.WORKLOADS['wide']
    bench.WORKLOADS['wide_bf16x3'] = (kind, rows, L, dict(over, matmul='bf16x3'), desc)      # (this process only)
    engs = {}
    for name, wl in (('fp32', 'wide'), ('bf16x3', 'wide_bf16x3')):
        cfg, eng, arena, batch, _ = bench.build(wl, dev, 0, 1)
        assert cfg.matmul == name and eng.plan.c_decx.x3_last == (name == 'bf16x3')
        eng.train_step()
        eng.capture()
        engs[name] = (eng, arena)
    t = alternate({k: e.replay for k, (e, _) in engs.items()}, reps, warm)
    for k, (e, _) in engs.items():
        e.check_sync()
    m32, m3 = float(np.median(t['fp32'])), float(np.median(t['bf16x3']))
    print('3. the captured cfg-5 train step (%s; ms per step, %d alternating repetitions after %d warm-up rounds)' % (desc, reps, warm))
    print('      matmul=fp32    %s' % stats(t['fp32']))
    print('      matmul=bf16x3  %s   %.2fx   (lab form: %.2f ms)' % (stats(t['bf16x3']), m32 / m3, LAB_MS['step']))
    l32, l3 = engs['fp32'][0].losses(), engs['bf16x3'][0].losses()
    pa, pb = engs['fp32'][1].param, engs['bf16x3'][1].param
    print('      after %d steps each from the same state: ELBO fp32 %.4f | bf16x3 %.4f; parameters norm-wise %.2e apart'
          % (1 + warm + reps, l32['ELBO'], l3['ELBO'], float((pa - pb).norm() / pa.norm())))
    if m3 >= LAB_MS['step']:
        print('      the hand-written kernel does NOT beat the lab form\'s %.2f ms step' % LAB_MS['step'])


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    assert args.reps >= 20
    dev = torch.device('cuda', 0)
    print('dtype: bf16x3 (opt-in; six bf16 MFMA terms per fp32 product, fp32 accumulation) against dtype: fp32 (MFMA, the default)')
    print('device: %s' % torch.cuda.get_device_name(dev))
    products(dev, args.reps, args.warmup)
    accuracy(dev)
    if not args.skip_step:
        step(dev, args.reps, args.warmup)
