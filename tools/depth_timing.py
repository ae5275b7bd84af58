#!/usr/bin/env python3
"""What the depth-normalised encoder input (``x_transform='log1p_norm'``) costs:

1. the input launch ``dv_batch_feed`` at bench.py's cfg 2 input rows (150 + 50 pairs = 200 rows x 978 genes), with the training
   noise: plain, split without a transform, split with log1p, split with log1p(x / s) -- the row sum in front of the transform
   and one division per element are what the last one adds;
2. the captured cfg-2-sized ``type_rec='nb'`` train step on count data with ``library_size=True`` and ``'log1p'`` against
   ``'log1p_norm'``.

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), in the form of
``tools/counts_timing.py``, whose feed operands and step builder these are.

  python tools/depth_timing.py [--windows 15] [--replays 400] [--out profiles/r25_depth_feed.md]

``--out``: the measured section replaces the text between the two ``depth_timing`` marker lines of the file (the file is
created with just that section if it does not exist).  There is no target: the table is the deliverable."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from counts_timing import _graph, build_step  # noqa: E402
from nb_timing import PASS_LAUNCHES, time_graph, time_step  # noqa: E402

BEGIN, END = '<!-- depth_timing:begin -->', '<!-- depth_timing:end -->'
FEEDS = (('plain', None, 3), ('split, no transform', {}, 4), ('split, log1p', dict(transform='log1p'), 4),
         ('split, log1p_norm', dict(transform='log1p_norm'), 4))
STEPS = ("x_transform='log1p', library_size=True", "x_transform='log1p_norm', library_size=True")


def feed_modes(device, B=150, Np=50, X=978, N=2048):
    """mode name -> (graph, words moved per launch, tensors kept alive); integer counts, every row total below 2^24"""
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
    modes = {}
    for name, kw, words in FEEDS:
        kw = {} if kw is None else dict(xt=xt, **kw)
        fn = lambda kw=kw: K.batch_feed(xin, x1, x2, None, table, 8, ctr, base, pair_rows=pair_rows, noise=noise, sigma=0.01, **kw)
        modes[name] = (_graph(fn), words * (B + Np) * X, (x1, x2, table, ctr, base, pair_rows, noise, xin, xt))
    return modes


def measure(windows, replays, device):
    feeds = feed_modes(device)
    steps, desc = {}, ''
    for name, tr in zip(STEPS, ('log1p', 'log1p_norm')):
        steps[name], desc = build_step(device, x_transform=tr, library_size=True)
    n_pass = max(1, replays // PASS_LAUNCHES)
    for graph, _, _ in feeds.values():
        time_graph(graph, n_pass)
    for eng in steps.values():
        time_step(eng, max(2, replays // 4))
    tf, ts = {k: [] for k in feeds}, {k: [] for k in steps}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for name, (graph, _, _) in feeds.items():
            tf[name].append(1000.0 * time_graph(graph, n_pass) / PASS_LAUNCHES)       # us per launch
        for k, eng in steps.items():
            ts[k].append(time_step(eng, replays))
    for eng in steps.values():
        eng.check_sync()
        assert all(np.isfinite(v) for v in eng.losses().values()), eng.losses()
    stat = lambda v: (statistics.median(v), min(v), max(v))
    return dict(desc=desc, windows=windows, replays=replays, n_pass=n_pass * PASS_LAUNCHES,
                feeds={k: stat(v) + (feeds[k][1],) for k, v in tf.items()}, steps={k: stat(v) for k, v in ts.items()})


def report(r):
    lines = [BEGIN, '## Measured: the feed launch and the captured step', '',
             '`tools/depth_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of %d'
             % r['windows'],
             'windows.  A launch window is %d launches (hipGraphs of %d back-to-back launches) between two device events, a step'
             % (r['n_pass'], PASS_LAUNCHES),
             'window %d replays of the captured step.  Times in a graph of back-to-back launches include the gap between two launches.'
             % r['replays'], '',
             '| `dv_batch_feed`, 150 + 50 rows x 978 genes, with noise | us / launch | words moved | GB/s |', '|---|---|---|---|']
    for k, (med, lo, hi, words) in r['feeds'].items():
        lines.append('| %s | %.2f (%.2f .. %.2f) | %d | %.0f |' % (k, med, lo, hi, words, 4e-3 * words / med))
    a, b = r['feeds']['split, log1p'][0], r['feeds']['split, log1p_norm'][0]
    lines += ['', 'The normalised feed takes %+.1f %% (%+.2f us) against the log1p feed of the same run.' % (100.0 * (b - a) / a, b - a), '',
              "| captured `type_rec='nb'` train step, cfg-2 sizes (%s), count data, explicit batch | ms / step |" % r['desc'], '|---|---|']
    for k, (med, lo, hi) in r['steps'].items():
        lines.append('| %s | %.4f (%.4f .. %.4f) |' % (k, med, lo, hi))
    (a, _, _), (b, _, _) = r['steps'].values()
    lines += ['', "The step with 'log1p_norm' takes %+.1f %% (%+.4f ms) against the step with 'log1p'." % (100.0 * (b - a) / a, b - a), END]
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
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('--replays', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('depth_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.replays, torch.device('cuda', 0)))
    print(text)
    if args.out:
        write(args.out, text)
