#!/usr/bin/env python3
"""What the raw-count inputs (``x_transform='log1p'``, ``library_size=True``) cost:

1. the input launch ``dv_batch_feed`` at bench.py's cfg 2 input rows (150 x 978 + pairs): plain, split without a transform,
   split with log1p, each with the training noise;
2. the row pass ``dv_rec_nll_rows`` at cfg 2's decoder rows (900 stacked rows x 978 genes gathered from 150 data rows): Poisson
   and negative binomial, plain and library-scaled kinds, rows + gradient;
3. the captured cfg-2-sized ``type_rec='nb'`` train step on count data without the switches and with both.

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), in the form of
``tools/nb_timing.py``.

  python tools/counts_timing.py [--windows 15] [--replays 400] [--out profiles/r20_counts.md]

There is no target: the table is the deliverable."""
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
from nb_timing import PASS_LAUNCHES, time_graph, time_step  # noqa: E402


def _graph(fn):
    fn()                                   # warm (code object load) outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PASS_LAUNCHES):
            fn()
    return g


def feed_modes(device, B=150, Np=50, X=978, N=2048):
    """mode name -> (graph, words moved per launch, tensors kept alive)"""
    import drvae_amd.kernels as K
    g = torch.Generator().manual_seed(5)
    pad = lambda r: torch.zeros(r, X + 2, device=device)[:, :X]        # (rows of 980 floats: 16-byte access)
    x1, x2 = pad(N), pad(N)
    x1.copy_(torch.floor((30 * torch.randn(N, X, generator=g)).abs()))
    x2.copy_(torch.floor((30 * torch.randn(N, X, generator=g)).abs()))
    table = torch.randint(0, N, (8, B), generator=g).to(torch.int32).to(device)
    ctr, base = torch.tensor([3], dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)
    pair_rows = torch.arange(Np, dtype=torch.int32, device=device)
    noise, xin, xt = pad(B + Np), pad(B + Np), pad(B + Np)
    noise.copy_(torch.randn(B + Np, X, generator=g))
    rows = (B + Np) * X
    modes = {}
    for name, kw, words in (('plain', {}, 3), ('split, no transform', dict(xt=xt), 4), ('split, log1p', dict(xt=xt, transform='log1p'), 4)):
        fn = lambda kw=kw: K.batch_feed(xin, x1, x2, None, table, 8, ctr, base, pair_rows=pair_rows, noise=noise, sigma=0.01, **kw)
        modes[name] = (_graph(fn), words * rows, (x1, x2, table, ctr, base, pair_rows, noise, xin, xt))
    return modes


def row_modes(device, M=900, n_src=150, X=978):
    import drvae_amd.kernels as K
    g = torch.Generator().manual_seed(7)
    x = torch.floor((3 * torch.randn(n_src, X, generator=g)).abs()).to(device)
    xi = (torch.arange(M) % n_src).to(torch.int32).to(device)
    am, at = torch.randn(M, X, generator=g), torch.randn(M, X, generator=g)
    rate = (torch.nn.functional.softplus(am) + 1e-6).to(device)
    v = torch.cat([torch.nn.functional.softplus(am) + 1e-6, torch.nn.functional.softplus(at) + 1e-3], 1).to(device)
    coef, out = torch.randn(M, generator=g).to(device), torch.zeros(M, device=device)
    d1, d2 = torch.zeros(M, X, device=device), torch.zeros(M, 2 * X, device=device)
    modes = {}
    for kind, heads, dpre, words in (('poisson', rate, d1, 3), ('nb', v, d2, 5)):
        for lib in (False, True):
            fn = lambda kind=kind, heads=heads, dpre=dpre, lib=lib: K.rec_nll_rows(
                out, x, heads, kind=kind, shift=1e-6, xidx=xi, coef=coef, dpre=dpre, **(dict(library=True) if lib else {}))
            modes['%s%s' % (kind, ', library-scaled' if lib else '')] = (_graph(fn), words * M * X, (x, xi, heads, coef, out, dpre))
    return modes


def build_step(device, **switches):
    """``bench.build``'s cfg-2 engine as a negative-binomial model on count data, explicit batch (with the switches: through the
    split feed launch)"""
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS['cfg2']
    cfg = E.StepConfig(kind=kind, L=L, type_rec='nb', add_noise_var=0.01, **over, **switches)
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
    t = lambda k: torch.from_numpy(np.floor(np.abs(3 * batch[k])).astype(np.float32)).to(device)
    eng.set_batch(t('x1'), t('x2'), batch['y'], hx, hy)
    eng.train_step()
    eng.capture()
    return eng, desc


def measure(windows, replays, device):
    feeds, rows = feed_modes(device), row_modes(device)
    steps, desc = {}, ''
    for name, sw in (('plain', {}), ("x_transform='log1p', library_size=True", dict(x_transform='log1p', library_size=True))):
        steps[name], desc = build_step(device, **sw)
    n_pass = max(1, replays // PASS_LAUNCHES)
    for group in (feeds, rows):
        for graph, _, _ in group.values():
            time_graph(graph, n_pass)
    for eng in steps.values():
        time_step(eng, max(2, replays // 4))
    t = {id(g): {k: [] for k in g} for g in (feeds, rows, steps)}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for group in (feeds, rows):
            for name, (graph, _, _) in group.items():
                t[id(group)][name].append(1000.0 * time_graph(graph, n_pass) / PASS_LAUNCHES)       # us per launch
        for k, eng in steps.items():
            t[id(steps)][k].append(time_step(eng, replays))
    for eng in steps.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values()), eng.losses()
    stat = lambda v: (statistics.median(v), min(v), max(v))
    return dict(desc=desc, windows=windows, replays=replays, n_pass=n_pass * PASS_LAUNCHES,
                feeds={k: stat(v) + (feeds[k][1],) for k, v in t[id(feeds)].items()},
                rows={k: stat(v) + (rows[k][1],) for k, v in t[id(rows)].items()},
                steps={k: stat(v) for k, v in t[id(steps)].items()})


def report(r):
    lines = ['## Measured: split feed, library rows and the captured step', '',
             '`tools/counts_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of %d'
             % r['windows'],
             'windows.  A launch window is %d launches (hipGraphs of %d back-to-back launches) between two device events, a step'
             % (r['n_pass'], PASS_LAUNCHES),
             'window %d replays of the captured step.  Times in a graph of back-to-back launches include the gap between two launches.'
             % r['replays'], '',
             '| `dv_batch_feed`, 150 + 50 rows x 978 genes, with noise | us / launch | words moved | GB/s |', '|---|---|---|---|']
    for k, (med, lo, hi, words) in r['feeds'].items():
        lines.append('| %s | %.2f (%.2f .. %.2f) | %d | %.0f |' % (k, med, lo, hi, words, 4e-3 * words / med))
    lines += ['', '| `dv_rec_nll_rows`, 900 rows x 978 genes gathered from 150, rows + gradient | us / launch | words moved | GB/s |',
              '|---|---|---|---|']
    for k, (med, lo, hi, words) in r['rows'].items():
        lines.append('| %s | %.2f (%.2f .. %.2f) | %d | %.0f |' % (k, med, lo, hi, words, 4e-3 * words / med))
    lines += ['', "| captured `type_rec='nb'` train step, cfg-2 sizes (%s), count data, explicit batch | ms / step |" % r['desc'], '|---|---|']
    for k, (med, lo, hi) in r['steps'].items():
        lines.append('| %s | %.4f (%.4f .. %.4f) |' % (k, med, lo, hi))
    (a, _, _), (b, _, _) = r['steps'].values()
    lines += ['', 'The step with both switches takes %+.1f %% (%+.4f ms) against the step without.' % (100.0 * (b - a) / a, b - a), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('--replays', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('counts_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.replays, torch.device('cuda', 0)))
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
