#!/usr/bin/env python3
"""One latency-bound GEMM launch of the cfg-2 step on WARM and on COLD operands, per ring depth (GPU box only).

In the running step no operand of a launch sits in an XCD's L2: its left operand was written by the launch in front of it on
other XCDs, its weights by the optimiser a step earlier.  Re-issuing one launch back to back on one operand set -- what
tools/gemm_bench.py and tools/heads_bench.py time -- finds everything in the L2 instead.  Here each launch is timed in two modes:

  warm  a graph of C launches on ONE operand set;
  cold  a graph of C launches, each on its OWN copy of every operand and output; C is chosen so that the copies together
        pass COLD_BYTES (64 MiB = twice the aggregate L2 and a bit), far below the 256 MiB of the Infinity Cache: a replay
        finds a copy where the step finds its operands, in the Infinity Cache and in no L2.

Variants are the ring depths of drvae_amd/csrc/ring_route.h, forced through dv_gemm_tune.opt[7] (4: two slots, 3: three, 2:
four).  Modes and variants alternate in rounds inside one process; per (mode, variant) the minimum and the maximum over all
its replays are printed -- the maximum minus the minimum is the tool's spread, which a depth has to win by.

    python tools/gemm_cold_bench.py [--rounds 3] [--replays 5] [--only TAG[,TAG]] [--json FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drvae_amd.kernels as K  # noqa: E402
from drvae_amd import _lib  # noqa: E402

COLD_BYTES = 68 << 20
MAX_COPIES = 512
DEPTH_OPT = {2: 4, 3: 3, 4: 2}          # ring depth -> dv_gemm_tune.opt[7]

# (tag, kind, M, N, K): fwd = x W^T + bias, ELU (x: M x K, W: N x K); heads = sample-mode paired heads (N = 2 x split);
# pair = dW (N x K, reduction M) || dX (M x K, reduction N) of a layer with input width K and output width N
SHAPES = [
    ('enc L1 fwd', 'fwd', 224, 800, 980),
    ('dec L1 pair', 'pair', 596, 600, 100),
    ('z2Fz1 heads pair', 'pair', 300, 200, 100),
    ('enc heads pair', 'pair', 224, 200, 800),
    ('fprop pair 104', 'pair', 450, 200, 104),
    ('fprop pair 200', 'pair', 450, 200, 200),
    ('side heads', 'heads', 450, 200, 200),
    ('dec L1 fwd (K=100)', 'fwd', 596, 600, 100),
    ('fprop L1 fwd (K=104)', 'fwd', 450, 200, 104),
]


def _rows(r, c, dev, scale=1.0):
    """r x c with one spare row behind it (``overread``: a row may be read up to 3 floats past its end)"""
    return (torch.randn(r + 1, c, device=dev) * scale)[:-1]


def make_set(kind, M, N, Kd, dev):
    """one operand set of a launch: (closure that issues the launch, bytes of the set)"""
    if kind == 'fwd':
        x, W, b, out = _rows(M, Kd, dev), _rows(N, Kd, dev, Kd ** -0.5), torch.randn(N, device=dev), torch.empty(M, N, device=dev)
        ts = (x, W, b, out)
        fn = lambda: K.linear_fwd(out, x, W, b, act0='elu', act1='elu', overread=True)      # noqa: E731
    elif kind == 'heads':
        S, L = N // 2, 2
        x, W, b = _rows(M, Kd, dev), _rows(N, Kd, dev, Kd ** -0.5), torch.randn(N, device=dev)
        q, eps, z = torch.empty(M, N, device=dev), torch.randn(L * M, S, device=dev), torch.empty(L * M, S, device=dev)
        ptr = torch.arange(0, L * M + 1, L, dtype=torch.int32, device=dev)
        rws = torch.arange(L * M, dtype=torch.int32, device=dev)
        ts = (x, W, b, q, eps, z, ptr, rws)
        fn = lambda: K.linear_heads(q, x, W, b, sample=dict(eps=eps, out=z, n_src=M, seg_ptr=ptr, seg_rows=rws),      # noqa: E731
                                    overread=True, split=S, shift1=-2.0)
    else:
        x, W, dpre, yprev = _rows(M, Kd, dev), _rows(N, Kd, dev, Kd ** -0.5), _rows(M, N, dev), _rows(M, Kd, dev)
        dW, db, dx = _rows(N, Kd, dev), torch.empty(N, device=dev), _rows(M, Kd, dev)
        ts = (x, W, dpre, yprev, dW, db, dx)
        fn = lambda: K.linear_bwd_pair(dW, db, dx, dpre, x, W, yref=yprev, act='elu', overread=True)      # noqa: E731
    return fn, sum(t.numel() * t.element_size() for t in ts), ts


def capture(fns):
    g = torch.cuda.CUDAGraph()
    for f in fns:
        f()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    return g


def replay_us(g, n_launches, replays):
    ts = []
    g.replay()                                   # (the first replay of a graph uploads it)
    torch.cuda.synchronize()
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n_launches)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--replays', type=int, default=5)
    ap.add_argument('--depths', default='2,3,4')
    ap.add_argument('--only', default='', help='comma list of shape tags (substring match)')
    ap.add_argument('--json', default='', help='also write every replay time to this file')
    args = ap.parse_args()
    _lib.load()
    dev = torch.device('cuda:0')
    depths = [int(d) for d in args.depths.split(',')]
    only = [t for t in args.only.split(',') if t]
    record = []
    print('us per launch, min .. max over %d replays (%d rounds x %d); cold: every launch on its own operand copies'
          % (args.rounds * args.replays, args.rounds, args.replays), flush=True)
    for (tag, kind, M, N, Kd) in SHAPES:
        if only and not any(o in tag for o in only):
            continue
        first = make_set(kind, M, N, Kd, dev)
        copies = min(MAX_COPIES, -(-COLD_BYTES // first[1]))
        sets = [first] + [make_set(kind, M, N, Kd, dev) for _ in range(copies - 1)]
        graphs = {}
        for d in depths:
            K.gemm_set_option(7, DEPTH_OPT[d])
            graphs[('warm', d)] = capture([first[0]] * copies)
            graphs[('cold', d)] = capture([s[0] for s in sets])
        K.gemm_set_option(7, 0)
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for mode in ('warm', 'cold'):
                for d in depths:
                    res[(mode, d)] += replay_us(graphs[(mode, d)], copies, args.replays)
        print('%-22s %-5s %4d x %4d x %4d  %3d copies, %5.1f MiB' % (tag, kind, M, N, Kd, copies, copies * first[1] / 2.0 ** 20), flush=True)
        for mode in ('warm', 'cold'):
            print('    %s  ' % mode + '   '.join('depth %d: %6.2f .. %6.2f' % (d, min(res[(mode, d)]), max(res[(mode, d)])) for d in depths), flush=True)
        g2 = min(res[('cold', depths[0])]) - min(res[('warm', depths[0])])
        print('    cold - warm at depth %d (minima): %.2f us' % (depths[0], g2), flush=True)
        record.append(dict(tag=tag, kind=kind, M=M, N=N, K=Kd, copies=copies, bytes=copies * first[1],
                           times={'%s/%d' % k: v for k, v in res.items()}))
        del graphs, sets, first
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(record, fh)


if __name__ == '__main__':
    main()
