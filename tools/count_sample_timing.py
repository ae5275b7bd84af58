#!/usr/bin/env python3
"""What a posterior-predictive draw costs (``count_sample.draw``: the sampler form of ``dv_fill_normal``), per kind, at
900 x 978 and at 2048 x 20 000, one sample per launch -- next to ``kernels.recon_rows`` of the same kind on the same operands,
the yardstick: a pass that reads the same heads once -- and what divergence costs: the negative-binomial draw with ONE theta for
all elements against theta spread over nine decades (1e-3 .. 1e6), at the same means -- and the same draw through the scalar
path (rows one float off a 16-byte boundary: one gene per thread and step instead of four in turn).

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), as the other
timing tools do.

  python tools/count_sample_timing.py [--windows 7] [--launches 50] [--skip-wide] [--out profiles/r32_count_sample.md]

``--out``: the measured section replaces the text between the two ``count_sample_timing`` marker lines of the file.  There is
no target: the table is the deliverable, whatever loses included."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from csr_feed_timing import write  # noqa: E402

BEGIN, END = '<!-- count_sample_timing:begin -->', '<!-- count_sample_timing:end -->'
SHAPES = ((900, 978), (2048, 20000))
KINDS = ('diag_gaussian', 'binary', 'poisson', 'nb', 'zinb')


def operands(kind, M, X, device, theta='spread', misalign=False):
    """finished heads of a plausible count model on the device (rows padded to 16-byte groups): means log-uniform in
    1e-2 .. 1e2, theta log-uniform in 1e-3 .. 1e6 or all 2.0, logits in -4 .. 4.  ``misalign``: every row starts one float behind
    a 16-byte boundary, which forces the scalar path (one gene per thread and step) where the quad path would run"""
    g = torch.Generator(device=device).manual_seed(7)
    ld = (X + 3) // 4 * 4
    off = 1 if misalign else 0
    rows = lambda: torch.empty(M * ld + 4, device=device)[off:off + M * ld].view(M, ld)[:, :X]
    logu = lambda lo, hi: rows().copy_(torch.exp(torch.empty(M, X, device=device).uniform_(float(torch.tensor(lo).log()), float(torch.tensor(hi).log()), generator=g)))
    ops = {}
    if kind == 'diag_gaussian':
        ops['mu'] = rows().copy_(torch.randn(M, X, generator=g, device=device))
        ops['sd'] = logu(1e-2, 2.0)
    elif kind == 'binary':
        ops['mu'] = rows().copy_(torch.rand(M, X, generator=g, device=device).clamp(1e-6, 1 - 1e-6))
    else:
        ops['mu'] = logu(1e-2, 1e2)
    if kind in ('nb', 'zinb'):
        ops['theta'] = logu(1e-3, 1e6) if theta == 'spread' else rows().fill_(2.0)
    return ops, g


def modes(device, wide):
    from drvae_amd import count_sample as CS
    import drvae_amd.kernels as K
    out = {}
    for M, X in SHAPES[:2 if wide else 1]:
        for kind in KINDS:
            for theta in (('spread', 'uniform', 'spread, scalar path') if kind == 'nb' else ('spread',)):
                scalar = theta.endswith('scalar path')
                ops, g = operands(kind, M, X, device, theta.split(',')[0], misalign=scalar)
                res = torch.empty(1, M, X, device=device)
                if scalar:
                    out[(M, X, kind, theta, 'draw')] = (lambda res=res, ops=ops: CS.draw(res, ops['mu'], kind='nb', theta=ops['theta'], seed=11),
                                                        (res, ops))
                    continue
                kw = dict(ops)
                mu = kw.pop('mu')
                if kind == 'zinb':
                    both = torch.empty(M, 2 * X, device=device)
                    both[:, :X].copy_(ops['theta'])
                    both[:, X:].uniform_(-4, 4, generator=g)
                    kw['theta'], kw['logit'] = both[:, :X], both[:, X:]
                draw = lambda res=res, mu=mu, kw=kw, kind=kind: CS.draw(res, mu, kind=kind, seed=11, **kw)
                out[(M, X, kind, theta, 'draw')] = (draw, (res, mu, kw))
                # the yardstick: the evaluation pass over the same heads (targets: one draw of the sampler itself)
                draw()
                x = res[0].clone()
                stats, ll = torch.empty(M, 6, device=device), torch.empty(M, device=device)
                if kind == 'diag_gaussian':
                    if X > K.RECON_ROWS_MAX_X:
                        continue
                    rec = lambda x=x, mu=mu, sd=kw['sd'], stats=stats, ll=ll: K.recon_rows(stats, ll, x, mu, sd, sd_shift=0.0)
                else:
                    sd = both if kind == 'zinb' else kw.get('theta')
                    rec = lambda x=x, mu=mu, sd=sd, stats=stats, ll=ll, kind=kind: K.recon_rows(stats, ll, x, mu, sd, kind=kind)
                out[(M, X, kind, theta, 'recon_rows')] = (rec, (x, stats, ll))
    return out


def time_launches(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1000.0 * a.elapsed_time(b) / n            # us per launch


def measure(windows, launches, device, wide=True):
    ms = modes(device, wide)
    n_of = lambda k: launches if k[1] < 10000 else max(3, launches // 10)
    for k, (fn, _) in ms.items():
        time_launches(fn, 3)
    t = {k: [] for k in ms}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for k, (fn, _) in ms.items():
            t[k].append(time_launches(fn, n_of(k)))
    return dict(windows=windows, launches=launches, t={k: (statistics.median(v), min(v), max(v)) for k, v in t.items()})


def report(r):
    lines = [BEGIN, '## Measured: one sample per launch, next to the evaluation pass over the same heads', '',
             '`tools/count_sample_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of',
             '%d windows of %d back-to-back launches (a tenth of that at 20 000 genes) between two device events, launch gaps included.'
             % (r['windows'], r['launches']), '',
             '| rows x genes | kind | draw us / launch | elements / s | `recon_rows` us / launch | draw / recon_rows |', '|---|---|---|---|---|---|']
    for k in sorted(k for k in r['t'] if k[4] == 'draw'):
        M, X, kind, theta, _ = k
        a, alo, ahi = r['t'][k]
        y = r['t'].get((M, X, kind, theta, 'recon_rows'))
        label = {'spread': '1e-3 .. 1e6', 'uniform': '= 2 everywhere', 'spread, scalar path': '1e-3 .. 1e6; rows misaligned: the scalar path'}
        name = kind + (' (theta %s)' % label[theta] if kind in ('nb', 'zinb') else '')
        lines.append('| %d x %d | %s | %.1f (%.1f .. %.1f) | %.3g | %s | %s |' % (
            M, X, name, a, alo, ahi, M * X / (a * 1e-6), '%.1f (%.1f .. %.1f)' % y if y else ('beyond its width' if kind == 'diag_gaussian' else 'as above'), '%.2f' % (a / y[0]) if y else '-'))
    lines.append(END)
    return '\n'.join(lines)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--skip-wide', action='store_true', help='900 x 978 only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('count_sample_timing: needs the GPU (a CPU run says nothing about the time)')
    text = report(measure(args.windows, args.launches, torch.device('cuda', 0), wide=not args.skip_wide))
    print(text)
    if args.out:
        write(args.out, text)
