#!/usr/bin/env python3
"""What the effect reduction costs (``effect.effect_cols``: the ``dv_draw_desc.fx`` form of ``dv_fill_normal``) at 900 x 978 and
2048 x 20 000 with 1 and 8 groups, next to two yardsticks on the same two matrices -- ``kernels.col_moments``, a launch that
reads the same bytes and leaves three float64 sums per (block, gene), and an ATen composition of the same seven statistics
(elementwise passes and one ``index_add_``) -- and what ``perturbation_effect`` costs end to end at both sizes with one pass at
the means and with 16 sampled passes, split into the reduction launches, the folds and the rest (encoder, latents, decoders).

The geometry of the launch is fixed (64 genes x one row block x one group per workgroup); its free parameter is the number of
row blocks, measured at the rule's value (``effect.row_blocks_for``), at half and at twice that.

All modes live in ONE process and are timed in alternating windows (medians and the spread of the windows), as the other
timing tools do.

  python tools/effect_timing.py [--windows 7] [--launches 50] [--skip-wide] [--out profiles/r33_effect.md]

``--out``: the measured section replaces the text between the two ``effect_timing`` marker lines of the file.  There is no
target: the table is the deliverable, whatever loses included."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = '<!-- effect_timing:begin -->', '<!-- effect_timing:end -->'
SHAPES = ((900, 978), (2048, 20000))
GROUPS = (1, 8)
DELTA, PSEUDO = 0.25, 1.0


def heads(M, X, device):
    """two finished mean heads of a plausible count model, as the columns of ONE (M, 2 X') buffer (X' = X rounded up to four):
    means log-uniform in 1e-2 .. 1e2, a log2 fold change of sd 0.7"""
    g = torch.Generator(device=device).manual_seed(7)
    ld = (X + 3) // 4 * 4
    buf = torch.empty(M, 2 * ld, device=device)
    a, b = buf[:, :X], buf[:, ld:ld + X]
    a.copy_(torch.exp(torch.empty(M, X, device=device).uniform_(-4.6, 4.6, generator=g)))
    b.copy_(a * torch.exp2(0.7 * torch.randn(M, X, device=device, generator=g)))
    return a, b


def aten_stats(a, b, grp, G):
    e = torch.log2(b + PSEUDO) - torch.log2(a + PSEUDO)
    v = torch.isfinite(e)
    ed = torch.where(v, e, torch.zeros_like(e)).double()
    z = torch.zeros_like(a)
    terms = torch.stack([v.double(), ed, ed * ed, (v & (e > DELTA)).double(), (v & (e < -DELTA)).double(),
                         torch.where(v, a, z).double(), torch.where(v, b, z).double()], 1)
    if G == 1:
        return terms.sum(0, keepdim=True)
    return torch.zeros(G, 7, a.shape[1], dtype=torch.float64, device=a.device).index_add_(0, grp, terms)


def kernel_modes(device, wide):
    from drvae_amd import effect as E
    import drvae_amd.kernels as K
    out = {}
    for M, X in SHAPES[:2 if wide else 1]:
        a, b = heads(M, X, device)
        nb = K.col_moment_blocks(M)
        cm = torch.empty(nb, 3, X, dtype=torch.float64, device=device)
        out[(M, X, 0, 'col_moments', nb)] = (lambda a=a, b=b, cm=cm: K.col_moments(None, a, b, part=cm), 8 * M * X + cm.numel() * 8)
        for G in GROUPS:
            grp = (torch.arange(M, device=device) % G).to(torch.int32)
            rule = E.row_blocks_for(M, X, G)
            for rb in sorted({max(1, rule // 2), rule, min(M, rule * 2)}):
                part = torch.empty(rb, G, 7, X, dtype=torch.float64, device=device)
                fn = lambda a=a, b=b, part=part, grp=grp, G=G: E.effect_cols(part, a, b, grp=grp if G > 1 else None, n_groups=G,
                                                                              mode=0, delta=DELTA, pseudocount=PSEUDO)
                out[(M, X, G, 'effect_cols' + (' (the rule)' if rb == rule else ''), rb)] = (fn, 8 * M * X + part.numel() * 8)
            gl = grp.long()
            out[(M, X, G, 'ATen composition', 0)] = (lambda a=a, b=b, gl=gl, G=G: aten_stats(a, b, gl, G), 8 * M * X)
    return out


def time_launches(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1000.0 * a.elapsed_time(b) / n            # us per launch


def measure_kernels(windows, launches, device, wide):
    ms = kernel_modes(device, wide)
    n_of = lambda k: launches if k[1] < 10000 else max(3, launches // 10)
    for k, (fn, _) in ms.items():
        time_launches(fn, 3)
    t = {k: [] for k in ms}
    for _ in range(windows):                         # alternating, so that drift of the box hits all modes alike
        for k, (fn, _) in ms.items():
            t[k].append(time_launches(fn, n_of(k)))
    return {k: (statistics.median(v), min(v), max(v), ms[k][1]) for k, v in t.items()}


# ------------------------------------------------------------------------------------------- end to end
def tiny_count_model(X, device):
    import warnings
    from drvae_amd.PVAE import PVAE
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return PVAE(dim_x=X, dim_s=1, dim_y=2, dim_h_en_z1=[256], dim_h_de_x=[256], dim_z1=32, type_rec='nb', dispersion='gene',
                    library_size=True, x_transform='log1p_norm', nonlinearity='elu', learning_rate=1e-3, L=1, use_MMD=False,
                    random_seed=5, epochs=1, batch_size=64, pertloss_rate=0.05, device=str(device))


def count_set(M, X, device):
    from drvae_amd import data as D
    g = torch.Generator(device=device).manual_seed(3)
    x1 = torch.poisson(torch.empty(M, X, device=device).uniform_(0.0, 3.0, generator=g), generator=g)
    zi = torch.zeros(M, dtype=torch.int64, device=device)
    return D.DrVAEDataset(x1, torch.zeros_like(x1), zi, zi, zi, zi)


def measure_end_to_end(windows, device, wide):
    """-> {(M, X, S): (total us, effect launches us, folds us) medians} -- the launcher and the fold are wrapped so that each
    call sits between two device events; the events are read after the call has been synchronised, the loop itself never waits"""
    from drvae_amd import effect as E
    out = {}
    real_cols, real_fold = E.effect_cols, E.fold
    for M, X in SHAPES[:2 if wide else 1]:
        model, ds = tiny_count_model(X, device), count_set(M, X, device)
        grp = torch.arange(M, device=device) % 8
        for S in (1, 16):
            kw = dict(n_samples=S, latent='mean' if S == 1 else 'sample', groups=grp, n_groups=8, pseudocount=PSEUDO)
            rec = {'cols': [], 'fold': []}

            def wrap(fn, key):
                def inner(*a, **k):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = fn(*a, **k)
                    e1.record()
                    rec[key].append((e0, e1))
                    return r
                return inner
            tot, cols, fold = [], [], []
            try:
                E.effect_cols, E.fold = wrap(real_cols, 'cols'), wrap(real_fold, 'fold')
                for w in range(windows + 1):         # (the first window warms every shape up and is dropped)
                    rec['cols'], rec['fold'] = [], []
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    model.perturbation_effect(ds, **kw)
                    b.record()
                    b.synchronize()
                    if w:
                        tot.append(1000.0 * a.elapsed_time(b))
                        cols.append(sum(1000.0 * x.elapsed_time(y) for x, y in rec['cols']))
                        fold.append(sum(1000.0 * x.elapsed_time(y) for x, y in rec['fold']))
            finally:
                E.effect_cols, E.fold = real_cols, real_fold
            out[(M, X, S)] = (statistics.median(tot), min(tot), max(tot), statistics.median(cols), statistics.median(fold))
    return out


def report(kern, e2e, windows, launches):
    lines = [BEGIN, '## Measured: the reduction launch next to its yardsticks', '',
             '`tools/effect_timing.py`: every mode lives in one process; windows alternate between the modes; medians (min .. max) of',
             '%d windows of %d back-to-back launches (a tenth of that at 20 000 genes) between two device events, launch gaps included.'
             % (windows, launches),
             'Bytes: the two matrices read once (8 per row and gene) plus the float64 partials written; the ATen composition is charged',
             'the reads alone (its intermediates are not counted), so its figure is the useful rate.  Mode 0, pseudocount 1, delta 0.25.', '',
             '| rows x genes | groups | launch | row blocks | us / launch | bytes / s |', '|---|---|---|---|---|---|']
    for k in sorted(kern, key=lambda k: (k[0], k[1], k[2], k[3] == 'ATen composition', k[4])):
        M, X, G, name, rb = k
        t, lo, hi, nbytes = kern[k]
        lines.append('| %d x %d | %s | %s | %s | %.1f (%.1f .. %.1f) | %.3g |' % (
            M, X, G or '-', name, rb or '-', t, lo, hi, nbytes / (t * 1e-6)))
    lines += ['', '## Measured: `perturbation_effect` end to end', '',
              'A PVAE with a negative-binomial decoder (hidden layers of 256, 32 latent dimensions, `library_size`, gene-wise dispersion),',
              '8 groups, one chunk; S = 1 is `latent=\'mean\'`, S = 16 is `latent=\'sample\'`.  Medians of %d calls after a warm-up call; the' % windows,
              'reduction launches and the folds each between device events of their own, the rest (encoder, latent noise, the two decoder',
              'passes per sample, host time between launches) is the difference.', '',
              '| rows x genes | S | call us (min .. max) | reduction launches | folds | the rest |', '|---|---|---|---|---|---|']
    for (M, X, S), (t, lo, hi, c, f) in sorted(e2e.items()):
        lines.append('| %d x %d | %d | %.0f (%.0f .. %.0f) | %.0f us, %.1f %% | %.0f us, %.1f %% | %.1f %% |' % (
            M, X, S, t, lo, hi, c, 100 * c / t, f, 100 * f / t, 100 * (t - c - f) / t))
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
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--skip-wide', action='store_true', help='900 x 978 only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('effect_timing: needs the GPU (a CPU run says nothing about the time)')
    dev = torch.device('cuda', 0)
    text = report(measure_kernels(args.windows, args.launches, dev, not args.skip_wide),
                  measure_end_to_end(args.windows, dev, not args.skip_wide), args.windows, args.launches)
    print(text)
    if args.out:
        write(args.out, text)
