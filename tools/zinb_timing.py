#!/usr/bin/env python3
"""What the zero-inflated negative-binomial data decoder (``type_rec='zinb'``) costs next to the negative binomial:

1. the row pass ``dv_rec_nll_rows`` on the rows of bench.py's cfg 2 decoder (900 stacked rows x 978 genes gathered from 150
   data rows): 'nb' and 'zinb', with and without the gradient (``coef``), and both library-scaled kinds -- each mode a hipGraph
   of back-to-back launches, timed between device events;
2. the captured cfg-2-sized train step on count data with ``type_rec='nb'`` and with ``'zinb'`` (same trunk, two heads against
   three: the third head's forward product is a launch of its own, the gradient products run over the fused (3X, K) view).

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), like
``tools/nb_timing.py``, whose helpers this reuses.

  python tools/zinb_timing.py [--windows 15] [--replays 400] [--out FILE]      # (its table: the 'Measured' section of profiles/r24_zinb.md)

There is no target: the table is the deliverable."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import nb_timing as NT  # noqa: E402

PASS_LAUNCHES = NT.PASS_LAUNCHES


def pass_modes(device, M=900, n_src=150, X=978):
    """mode name -> (graph of PASS_LAUNCHES launches, words moved per launch, the tensors kept alive)"""
    import drvae_amd.kernels as K
    g = torch.Generator().manual_seed(7)
    x = torch.floor((3 * torch.randn(n_src, X, generator=g)).abs())
    x[torch.rand(n_src, X, generator=g) < 0.3] = 0.0
    x = x.to(device)
    xi = (torch.arange(M) % n_src).to(torch.int32).to(device)
    sp = torch.nn.functional.softplus
    am, at, ad = (torch.randn(M, X, generator=g) for _ in range(3))
    v2 = torch.cat([sp(am) + 1e-6, sp(at) + 1e-3], 1).to(device)
    v3 = torch.cat([sp(am) + 1e-6, sp(at) + 1e-3, ad], 1).to(device)
    coef = torch.randn(M, generator=g).to(device)
    out = torch.zeros(M, device=device)
    d2, d3 = torch.zeros(M, 2 * X, device=device), torch.zeros(M, 3 * X, device=device)
    modes = {}
    for kind, heads, dpre, words in (('nb', v2, d2, 3), ('zinb', v3, d3, 4)):
        for library in (False, True):
            for with_coef in (False, True):
                kw = dict(kind=kind, shift=1e-6, xidx=xi, **(dict(library=True) if library else {}))
                if with_coef:
                    kw.update(coef=coef, dpre=dpre)
                K.rec_nll_rows(out, x, heads, **kw)          # warm (code object load) outside the capture
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(PASS_LAUNCHES):
                        K.rec_nll_rows(out, x, heads, **kw)
                name = '%s%s, %s' % (kind, '_lib' if library else '', 'rows + gradient' if with_coef else 'rows only')
                modes[name] = (graph, (words + (words - 1 if with_coef else 0)) * M * X, (out, x, heads, xi, coef, dpre))
    return modes


def measure(windows, replays, device):
    passes = pass_modes(device)
    steps, desc = {}, ''
    for type_rec in ('nb', 'zinb'):
        steps[type_rec], desc = NT.build_step(type_rec, device)
    n_pass = max(1, replays // PASS_LAUNCHES)
    for name, (graph, _, _) in passes.items():      # warm every graph at the timed shape
        NT.time_graph(graph, n_pass)
    for eng in steps.values():
        NT.time_step(eng, max(2, replays // 4))
    t_pass, t_step = {k: [] for k in passes}, {k: [] for k in steps}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for name, (graph, _, _) in passes.items():
            t_pass[name].append(1000.0 * NT.time_graph(graph, n_pass) / PASS_LAUNCHES)       # us per launch
        for k, eng in steps.items():
            t_step[k].append(NT.time_step(eng, replays))
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
             '`tools/zinb_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of %d'
             % r['windows'],
             'windows.  A row-pass window is %d launches (hipGraphs of %d back-to-back launches) between two device events, a step'
             % (r['n_pass'], PASS_LAUNCHES),
             'window %d replays of the captured step.  Times in a graph of back-to-back launches include the gap between two launches.'
             % r['replays'], '',
             '| `dv_rec_nll_rows`, 900 rows x 978 genes gathered from 150 | us / launch | words moved | GB/s |', '|---|---|---|---|']
    for k, (med, lo, hi, words) in r['passes'].items():
        lines.append('| %s | %.2f (%.2f .. %.2f) | %d | %.0f |' % (k, med, lo, hi, words, 4e-3 * words / med))
    lines += ['', '| captured train step, cfg-2 sizes (%s), count data | ms / step | schedule |' % r['desc'], '|---|---|---|']
    for k, (med, lo, hi) in r['steps'].items():
        lines.append("| type_rec='%s' | %.4f (%.4f .. %.4f) | %s |" % (k, med, lo, hi, 'two flag-ordered graphs' if r['dual'][k] else 'one graph'))
    a, b = r['steps']['nb'][0], r['steps']['zinb'][0]
    lines += ['', "The zero-inflated step takes %+.1f %% (%+.4f ms) against the negative-binomial step: the third head's forward "
              'product (one more launch from the same trunk activation), gradient products half as wide again, and the row pass above.'
              % (100.0 * (b - a) / a, b - a), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('--replays', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('zinb_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.replays, torch.device('cuda', 0)))
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
