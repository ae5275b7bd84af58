#!/usr/bin/env python3
"""What the negative-binomial data decoder (``type_rec='nb'``) costs next to the Poisson decoder:

1. the row pass ``dv_rec_nll_rows`` on the rows of bench.py's cfg 2 decoder (900 stacked rows x 978 genes gathered from 150
   data rows): Poisson and negative binomial, with and without the gradient (``coef``), plus 976 genes both ways (the negative
   binomial's 16-byte kernel, and the one-gene-per-thread kernel that 978 genes take, forced by heads one float off
   alignment) -- each mode a hipGraph of back-to-back launches, timed between device events;
2. the captured cfg-2-sized train step on count data with ``type_rec='poisson'`` and with ``'nb'`` (same trunk, one head
   against two).

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows).

  python tools/nb_timing.py [--windows 15] [--replays 400] [--out profiles/r19_nb.md]

There is no target: the table is the deliverable."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PASS_LAUNCHES = 100          # launches per graph of a row-pass mode


def pass_modes(device, M=900, n_src=150):
    """mode name -> (graph of PASS_LAUNCHES launches, words moved per launch)"""
    import drvae_amd.kernels as K
    g = torch.Generator().manual_seed(7)
    modes = {}
    for X in (978, 976):
        x = torch.floor((3 * torch.randn(n_src, X, generator=g)).abs()).to(device)
        xi = (torch.arange(M) % n_src).to(torch.int32).to(device)
        am, at = torch.randn(M, X, generator=g), torch.randn(M, X, generator=g)
        rate = (torch.nn.functional.softplus(am) + 1e-6).to(device)
        v = torch.cat([torch.nn.functional.softplus(am) + 1e-6, torch.nn.functional.softplus(at) + 1e-3], 1).to(device)
        coef = torch.randn(M, generator=g).to(device)
        out = torch.zeros(M, device=device)
        d1, d2 = torch.zeros(M, X, device=device), torch.zeros(M, 2 * X, device=device)
        # (the same heads one float off 16-byte alignment: the dispatcher takes the one-gene-per-thread kernel for them)
        v_off = torch.empty(M * 2 * X + 1, device=device)[1:].view(M, 2 * X).copy_(v)
        cases = [('poisson', 'poisson', rate, d1, 2), ('nb', 'nb', v, d2, 3)] if X == 978 else \
            [('nb', 'nb', v, d2, 3), ('nb, heads off 16-byte alignment', 'nb', v_off, d2, 3)]
        for label, kind, heads, dpre, words in cases:
            for with_coef in (False, True):
                kw = dict(kind=kind, shift=1e-6, xidx=xi)
                if with_coef:
                    kw.update(coef=coef, dpre=dpre)
                K.rec_nll_rows(out, x, heads, **kw)          # warm (code object load) outside the capture
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(PASS_LAUNCHES):
                        K.rec_nll_rows(out, x, heads, **kw)
                name = '%s, %d genes, %s' % (label, X, 'rows + gradient' if with_coef else 'rows only')
                modes[name] = (graph, (words + (words - 1 if with_coef else 0)) * M * X, (out, x, heads, xi, coef, dpre))
    return modes


def time_graph(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def build_step(type_rec, device):
    """``bench.build``'s cfg-2 engine with the given data decoder on count data (floor(|3 x|), as the Poisson tests use)"""
    from drvae_amd import engine as E
    from drvae_amd import synth, tuning
    from drvae_amd.arena import ParamArena
    kind, rows, L, over, desc = bench.WORKLOADS['cfg2']
    cfg = E.StepConfig(kind=kind, L=L, type_rec=type_rec, add_noise_var=0.0, **over)
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


def time_step(eng, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with eng.partition():
        e0.record()
        for _ in range(n):
            eng.replay()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure(windows, replays, device):
    passes = pass_modes(device)
    steps, desc = {}, ''
    for type_rec in ('poisson', 'nb'):
        steps[type_rec], desc = build_step(type_rec, device)
    n_pass = max(1, replays // PASS_LAUNCHES)
    for name, (graph, _, _) in passes.items():      # warm every graph at the timed shape
        time_graph(graph, n_pass)
    for eng in steps.values():
        time_step(eng, max(2, replays // 4))
    t_pass, t_step = {k: [] for k in passes}, {k: [] for k in steps}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for name, (graph, _, _) in passes.items():
            t_pass[name].append(1000.0 * time_graph(graph, n_pass) / PASS_LAUNCHES)       # us per launch
        for k, eng in steps.items():
            t_step[k].append(time_step(eng, replays))
    for eng in steps.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values()), eng.losses()
    stat = lambda v: (statistics.median(v), min(v), max(v))
    return dict(desc=desc, windows=windows, replays=replays, n_pass=n_pass * PASS_LAUNCHES,
                passes={k: stat(v) + (passes[k][1],) for k, v in t_pass.items()},
                steps={k: stat(v) for k, v in t_step.items()},
                dual={k: e._side_graph is not None for k, e in steps.items()})


def report(r):
    lines = ['## Measured: row pass and captured step', '',
             '`tools/nb_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of %d'
             % r['windows'],
             'windows.  A row-pass window is %d launches (hipGraphs of %d back-to-back launches) between two device events, a step'
             % (r['n_pass'], PASS_LAUNCHES),
             'window %d replays of the captured step.  Times in a graph of back-to-back launches include the gap between two launches.'
             % r['replays'], '',
             '| `dv_rec_nll_rows`, 900 rows gathered from 150 | us / launch | words moved | GB/s |', '|---|---|---|---|']
    for k, (med, lo, hi, words) in r['passes'].items():
        lines.append('| %s | %.2f (%.2f .. %.2f) | %d | %.0f |' % (k, med, lo, hi, words, 4e-3 * words / med))
    lines += ['', '| captured train step, cfg-2 sizes (%s), count data | ms / step | schedule |' % r['desc'], '|---|---|---|']
    for k, (med, lo, hi) in r['steps'].items():
        lines.append("| type_rec='%s' | %.4f (%.4f .. %.4f) | %s |" % (k, med, lo, hi, 'two flag-ordered graphs' if r['dual'][k] else 'one graph'))
    a, b = r['steps']['poisson'][0], r['steps']['nb'][0]
    lines += ['', "The negative-binomial step takes %+.1f %% (%+.4f ms) against the Poisson step: a second head on the decoder's last "
              'layer (its forward product and both gradient products are twice as wide) and the heavier row pass above.'
              % (100.0 * (b - a) / a, b - a), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('--replays', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('nb_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.replays, torch.device('cuda', 0)))
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
