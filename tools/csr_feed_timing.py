#!/usr/bin/env python3
"""What sparse rows in the device batch feed cost and save -- every comparison against the dense feed on the same data:

1. the feed launch alone (``dv_batch_feed``, split form with log1p and the training noise: the count models' launch) at
   150 + 50 rows x 978 genes and at 1024 + 1024 rows x 20 000 genes, the data set at densities 0.05, 0.3 and 1.0, held dense
   against held as CSR (x1 and x2);
2. the captured ``type_rec='nb'`` train step (``x_transform='log1p'``, ``library_size=True``) on the graph-resident epoch feed at
   bench.py's cfg-2 sizes and at its wide sizes, a data set at density 0.07, dense against CSR -- the two engines share seed and
   index table, so their losses are compared bit for bit at the end;
3. HBM held by a 10^5 x 20 000 data set at density 0.07 (x1 + x2): allocated bytes, dense against CSR.

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), in the form of
``tools/depth_timing.py``.

  python tools/csr_feed_timing.py [--windows 9] [--replays 400] [--skip-wide] [--out profiles/r30_csr_feed.md]

``--out``: the measured section replaces the text between the two ``csr_feed_timing`` marker lines of the file.  There is no
target: the tables are the deliverable."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from nb_timing import time_graph, time_step  # noqa: E402

BEGIN, END = '<!-- csr_feed_timing:begin -->', '<!-- csr_feed_timing:end -->'
DENSITIES = (0.05, 0.3, 1.0)
SHAPES = (('150 + 50 rows x 978 genes', 150, 50, 978, 2048, 100), ('1024 + 1024 rows x 20000 genes', 1024, 1024, 20000, 4096, 10))


def counts(n, X, density, device, seed):
    """integer counts floor(|3 z|) + 1 kept with probability ``density`` (fp32, on the device, rows padded to 16-byte groups)"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.zeros(n, (X + 3) // 4 * 4, device=device)[:, :X]
    x.copy_(torch.floor((3 * torch.randn(n, X, generator=g, device=device)).abs()) + 1)
    if density < 1.0:
        x.mul_((torch.rand(n, X, generator=g, device=device) < density).float())
    return x


def _graph(fn, launches):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def feed_modes(device, wide=True):
    """(shape, density, 'dense' | 'csr') -> (graph, launches per graph, bytes the launch must move, tensors kept alive)"""
    import drvae_amd.kernels as K
    from drvae_amd.sparse_rows import CsrRows
    modes = {}
    for label, B, Np, X, N, launches in SHAPES[:2 if wide else 1]:
        g = torch.Generator().manual_seed(5)
        table = torch.randint(0, N, (8, B), generator=g).to(torch.int32).to(device)
        ctr, base = torch.tensor([3], dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)
        pair_rows = torch.arange(Np, dtype=torch.int32, device=device)
        pad = lambda: torch.zeros(B + Np, (X + 3) // 4 * 4, device=device)[:, :X]
        noise, xin, xt = pad(), pad(), pad()
        noise.normal_()
        for density in DENSITIES:
            x1, x2 = counts(N, X, density, device, 11), counts(N, X, density, device, 12)
            for held, (a, b) in (('dense', (x1, x2)), ('csr', (CsrRows.from_dense(x1).check(), CsrRows.from_dense(x2).check()))):
                fn = lambda a=a, b=b: K.batch_feed(xin, a, b, None, table, 8, ctr, base, pair_rows=pair_rows, noise=noise, sigma=0.01,
                                                   xt=xt, transform='log1p')
                rows = torch.cat([table[3].long(), table[3].long()[:Np]])
                nnz = int(((x1[rows[:B]] != 0).sum() + (x2[rows[B:]] != 0).sum()))
                out = 3 * (B + Np) * X * 4                  # noise read, xin and xt written
                moved = out + ((B + Np) * X * 4 if held == 'dense' else nnz * 8 + (B + Np) * 16)
                modes[(label, density, held)] = (_graph(fn, launches), launches, moved, (a, b, table, ctr, base, pair_rows, noise, xin, xt))
            del x1, x2
    return modes


def build_step(workload, device, sparse, density=0.07, n_rows=4096):
    """bench.py's engine of ``workload`` as a negative-binomial model with both count switches on the graph-resident epoch feed
    of a data set of ``n_rows`` rows, held dense or as CSR; captured"""
    from drvae_amd import data as D
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    from drvae_amd.sparse_rows import CsrRows
    kind, rows, L, over, desc = bench.WORKLOADS[workload]
    cfg = E.StepConfig(kind=kind, L=L, type_rec='nb', add_noise_var=0.01, x_transform='log1p', library_size=True, **over)
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
    batch = synth.make_batch(kind, rows, 8, cfg.dim_y, seed=1234)            # (its group composition only)
    hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
    gc = [int(((hy == bool(gy)) & (hx == bool(gx))).sum()) for (gy, gx) in D._GROUPS]
    rs = np.random.RandomState(7)
    flags = lambda f: torch.from_numpy(np.resize(f.astype(np.int64), n_rows)).to(device)
    x1, x2 = counts(n_rows, cfg.dim_x, density, device, 21), counts(n_rows, cfg.dim_x, density, device, 22)
    if sparse:
        x1, x2 = CsrRows.from_dense(x1), CsrRows.from_dense(x2)
    ds = D.DrVAEDataset(x1, x2, torch.zeros(n_rows, dtype=torch.int64, device=device),
                        torch.from_numpy(rs.randint(0, cfg.dim_y, n_rows)).to(device), flags(hx), flags(hy))
    bat = D.DeviceBatcher(ds, torch.ones(n_rows), rows, group_counts=gc, seed=5)
    bat.bind(eng)
    bat.begin_epoch(n_batches=16)
    eng.train_step()
    eng.capture()
    bat.rebase()
    return eng, desc, (ds, bat)


def held_bytes(device, n=100000, X=20000, density=0.07, chunk=10000):
    """allocated device bytes of an ``n`` x ``X`` data set (x1 + x2) at ``density``: dense fp32 against CSR, built chunk by chunk"""
    from drvae_amd.sparse_rows import CsrRows
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(device)
    dense = [torch.empty(n, X, device=device) for _ in range(2)]
    dense_b = torch.cuda.memory_allocated(device) - base
    del dense
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(device)
    held = []
    for m in range(2):
        parts = [CsrRows.from_dense(counts(min(chunk, n - r), X, density, device, 100 * m + r // chunk)) for r in range(0, n, chunk)]
        off = np.cumsum([0] + [p.nnz for p in parts])
        ptr = torch.cat([parts[0].ptr[:1]] + [p.ptr[1:] + int(o) for p, o in zip(parts, off)])
        held.append(CsrRows(ptr, torch.cat([p.idx for p in parts]), torch.cat([p.val for p in parts]), (n, X)))
        del parts, ptr
    torch.cuda.empty_cache()
    csr_b = torch.cuda.memory_allocated(device) - base
    nnz = sum(c.nnz for c in held)
    return dict(n=n, X=X, density=nnz / (2.0 * n * X), dense=dense_b, csr=csr_b, arrays=sum(c.nbytes() for c in held))


def measure(windows, replays, device, wide=True):
    feeds = feed_modes(device, wide)
    steps, descs = {}, {}
    for workload in ('cfg2', 'wide') if wide else ('cfg2',):
        for held in ('dense', 'csr'):
            steps[(workload, held)], descs[workload], _keep = build_step(workload, device, held == 'csr')
            steps[(workload, held)]._timing_keep = _keep
    n_rep = lambda k: replays if k[0] == 'cfg2' else max(10, replays // 20)
    for graph, launches, _, _ in feeds.values():
        time_graph(graph, max(1, replays // launches))
    for k, eng in steps.items():
        time_step(eng, max(2, n_rep(k) // 4))
    tf, ts = {k: [] for k in feeds}, {k: [] for k in steps}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for k, (graph, launches, _, _) in feeds.items():
            tf[k].append(1000.0 * time_graph(graph, max(1, replays // launches)) / launches)       # us per launch
        for k, eng in steps.items():
            ts[k].append(time_step(eng, n_rep(k)))
    same = {}
    for workload in descs:
        a, b = steps[(workload, 'dense')], steps[(workload, 'csr')]
        for eng in (a, b):
            eng.check_sync()
            assert all(np.isfinite(v) for v in eng.losses().values()), eng.losses()
        same[workload] = a.losses() == b.losses() and torch.equal(a.arena.param, b.arena.param)
    stat = lambda v: (statistics.median(v), min(v), max(v))
    mem = held_bytes(device) if wide else None
    return dict(windows=windows, replays=replays, descs=descs, feeds={k: stat(v) + (feeds[k][2],) for k, v in tf.items()},
                steps={k: stat(v) for k, v in ts.items()}, same=same, mem=mem, n_rep={k: n_rep(k) for k in steps})


def report(r):
    lines = [BEGIN, '## Measured: the feed launch, the captured step, the memory held', '',
             '`tools/csr_feed_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of %d'
             % r['windows'],
             'windows.  A launch window is about %d launches (hipGraphs of 100 back-to-back launches at 978 genes, of 10 at 20 000) between'
             % r['replays'],
             'two device events; times in a graph of back-to-back launches include the gap between two launches.  "bytes" is what the',
             'launch must move: the noise read, `xin` and `xt` written, and the source rows (dense: 4 B per element; CSR: 8 B per entry',
             'and two offsets per row).', '']
    shapes = sorted({k[0] for k in r['feeds']}, key=lambda s: len(s))
    for shape in shapes:
        lines += ['| `dv_batch_feed`, split + log1p + noise, %s | dense us / launch | CSR us / launch | CSR / dense | dense GB/s | CSR GB/s |' % shape,
                  '|---|---|---|---|---|---|']
        for d in DENSITIES:
            (a, alo, ahi, ab), (b, blo, bhi, bb) = r['feeds'][(shape, d, 'dense')], r['feeds'][(shape, d, 'csr')]
            lines.append('| density %.2f | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.2f | %.0f | %.0f |'
                         % (d, a, alo, ahi, b, blo, bhi, b / a, 1e-3 * ab / a, 1e-3 * bb / b))
        lines.append('')
    lines += ["| captured `type_rec='nb'` train step on the epoch feed (`x_transform='log1p'`, `library_size=True`), data set at density 0.07 "
              '| dense ms / step | CSR ms / step | difference | losses and parameters bit-equal |', '|---|---|---|---|---|']
    for w, desc in r['descs'].items():
        (a, alo, ahi), (b, blo, bhi) = r['steps'][(w, 'dense')], r['steps'][(w, 'csr')]
        lines.append('| %s (%s; windows of %d replays) | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %+.4f ms (%+.1f %%) | %s |'
                     % (w, desc, r['n_rep'][(w, 'dense')], a, alo, ahi, b, blo, bhi, b - a, 100.0 * (b - a) / a, 'yes' if r['same'][w] else 'NO'))
    if r['mem']:
        m = r['mem']
        lines += ['', 'HBM held by a %d x %d data set (x1 + x2) at density %.3f, allocated bytes: dense %.2f GB, CSR %.2f GB (its arrays: %.2f GB) '
                  '-- %.1f times less.' % (m['n'], m['X'], m['density'], m['dense'] / 1e9, m['csr'] / 1e9, m['arrays'] / 1e9, m['dense'] / m['csr'])]
    lines.append(END)
    return '\n'.join(lines)


def write(path, text):
    """the section between the marker lines of ``path`` replaced by ``text`` (a new file: the section alone)"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    old = open(path).read() if os.path.exists(path) else ''
    if BEGIN in old and END in old:
        text = old[:old.index(BEGIN)] + text + old[old.index(END) + len(END):]
    elif old:
        text = old.rstrip('\n') + '\n\n' + text + '\n'
    else:
        text += '\n'
    with open(path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--replays', type=int, default=400)
    ap.add_argument('--skip-wide', action='store_true', help='the 978-gene sizes only (no 20 000-gene launch, step or data set)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('csr_feed_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.replays, torch.device('cuda', 0), wide=not args.skip_wide))
    print(text)
    if args.out:
        write(args.out, text)
