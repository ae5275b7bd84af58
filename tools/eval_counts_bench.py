#!/usr/bin/env python3
"""Whole-set evaluation of the count-decoder models on an HBM-resident set: the captured path
(``evaluate_performance_on_dataset``: one graph replay + one copy) against the step-by-step path ``model._evaluate`` on the
same model and set, taken in alternation in one process (profiler off, shapes warmed up, host clock around work that ends in
a device synchronise -- both paths end in a device-to-host copy of their scalars); then the count kinds of ``dv_recon_rows``
alone (device events around a captured graph of 20 launches, divided by 20).

Cases: the 'nb' model with x_transform='log1p' + library_size=True and the plain 'poisson' model, 8192 rows at cfg-2 sizes
(978 genes); one wide case, 'nb' with both switches on 2048 rows x 20 000 genes; the zero-inflated model ('zinb') plain and with
both switches at 8192 x 978 and with both switches at 2048 x 20 000; the launch alone per kind at 8192 x 978.

``python tools/eval_counts_bench.py [reps] [--only CASE[,CASE...]|kernel] [--stepwise-only] [--out FILE]`` (GPU box only).  Prints
markdown tables -- median with min .. max -- and with ``--out [FILE]`` replaces the text between the ``<!-- timings -->``
markers of FILE (``--out`` alone: profiles/r22_eval_counts.md; the file is created when missing) by them.  ``--stepwise-only``:
the step-by-step path alone, nothing asked of the captured one (a tree whose evaluation declines the model: the baseline)."""
import gc
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drvae_amd import data as D                 # noqa: E402
from drvae_amd.DrVAE import DrVAE               # noqa: E402

CASES = {'nb': dict(type_rec='nb', x_transform='log1p', library_size=True, n=8192, X=978),
         'poisson': dict(type_rec='poisson', n=8192, X=978),
         'wide': dict(type_rec='nb', x_transform='log1p', library_size=True, n=2048, X=20000),
         'zinb-plain': dict(type_rec='zinb', n=8192, X=978),
         'zinb': dict(type_rec='zinb', x_transform='log1p', library_size=True, n=8192, X=978),
         'zinb-wide': dict(type_rec='zinb', x_transform='log1p', library_size=True, n=2048, X=20000)}
BEGIN, END = '<!-- timings:begin -->', '<!-- timings:end -->'
BATCH = 20          # launches of ``dv_recon_rows`` per timed graph replay


def counts(n, X, seed):
    """Gamma-Poisson counts (theta = 2), gene means 0.5 .. 8, depths log-uniform over one decade; x2 = a 1.3 x deeper draw"""
    rs = np.random.RandomState(seed)
    mean = rs.uniform(0.5, 8.0, X)[None, :] * 10 ** rs.uniform(-0.5, 0.5, n)[:, None]
    x1 = rs.poisson(rs.gamma(2.0, mean / 2.0)).astype(np.float32)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    x2 = (rs.poisson(rs.gamma(2.0, 1.3 * mean / 2.0)) * hx[:, None]).astype(np.float32)
    return x1, x2, hx, rs.randint(0, 2, n), (np.arange(n) % 4 != 1).astype(np.int64)


def model_and_set(case, seed=1, dev='cuda'):
    c = dict(CASES[case])
    n, X = c.pop('n'), c.pop('X')
    model = DrVAE(dim_x=X, dim_s=1, dim_y=2, dim_h_en_z1=[800], dim_h_de_z1=[200], dim_h_en_z3=[200], dim_h_de_x=[600], dim_h_clf=[],
                  dim_z1=100, dim_z3=100, nonlinearity='elu', learning_rate=5e-4, L=2, weight_decay=0.05, add_noise_var=0.0,
                  use_MMD=False, pertloss_rate=0.05, random_seed=123, epochs=1, batch_size=150, **c).to(dev)
    model.w2log = lambda *a: None
    x1, x2, hx, y, hy = counts(n, X, seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return model, D.DrVAEDataset(t(x1), t(x2), t(np.zeros(n, np.int64)), t(y), t(hx), t(hy))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def row(label, path, v):
    v = np.asarray(v)
    return '| %s | %s | %d | %.3f | %.3f .. %.3f |' % (label, path, len(v), np.median(v), v.min(), v.max())


def models(reps, only, out, stepwise_only=False):
    from drvae_amd import fit as F
    out += ['| model | path | n | median ms | min .. max |', '|---|---|---|---|---|']
    for case in CASES:
        if only is not None and case not in only:
            continue
        model, ds = model_and_set(case)
        g = lambda k: getattr(ds, k, None)
        captured = lambda: model.evaluate_performance_on_dataset(ds)
        stepwise = lambda: model._evaluate(g('x1'), g('x2'), g('s'), g('y'), g('has_x2'), g('has_y'))
        paths = [('captured', captured), ('step by step', stepwise)]
        if stepwise_only:
            paths = paths[1:]
        else:
            captured()
            assert F._EvalGraph.get(model, ds) is not None, 'the captured path was not taken'
        for _, fn in paths:
            fn(), fn()
        ms = {name: [] for name, _ in paths}
        for _ in range(reps if not case.endswith('wide') else max(5, reps // 4)):
            for name, fn in paths:
                ms[name].append(timed(fn))
        c = CASES[case]
        label = "drvae '%s'%s, %d x %d" % (c['type_rec'], ' log1p + library size' if c.get('library_size') else '', c['n'], c['X'])
        for name, _ in paths:
            out.append(row(label, name, ms[name]))
            print(out[-1], flush=True)
        del model, ds
        torch.cuda.empty_cache()


def kernel(reps, out, M=8192, X=978, dev='cuda'):
    import drvae_amd.kernels as K
    out += ['', '| dv_recon_rows, %d x %d | operands | n | median us per launch | min .. max |' % (M, X), '|---|---|---|---|---|']
    x1, x2, _, _, _ = counts(M, X, 3)
    g = torch.Generator(device='cpu').manual_seed(5)
    x1, x2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    mu = (torch.rand(M, X, generator=g) * 4 + 0.05).to(dev)
    th = (torch.rand(M, X, generator=g) * 3 + 0.5).to(dev)
    p = torch.rand(M, X, generator=g).clamp(1e-3, 1 - 1e-3).to(dev)
    xb = (x1 > 2).float()
    tl = torch.cat([th, (torch.rand(M, X, generator=g) * 8 - 4).to(dev)], 1)          # [theta | dropout logit] for 'zinb'
    rows, ll, rec = torch.empty(M, 6, device=dev), torch.empty(M, device=dev), torch.empty(M, X, device=dev)
    forms = [('binary', 'rows + ll', lambda: K.recon_rows(rows, ll, xb, p, None, kind='binary')),
             ('poisson', 'rows + ll', lambda: K.recon_rows(rows, ll, x1, mu, None, kind='poisson')),
             ('poisson', 'rows + ll + stored mean, size source = target', lambda: K.recon_rows(rows, ll, x1, mu, None, kind='poisson', size_from=x1, rec_out=rec)),
             ('nb', 'rows + ll', lambda: K.recon_rows(rows, ll, x1, mu, th, kind='nb')),
             ('nb', 'rows + ll + stored mean, size source = target', lambda: K.recon_rows(rows, ll, x1, mu, th, kind='nb', size_from=x1, rec_out=rec)),
             ('nb', 'rows + ll + stored mean, size source = another matrix', lambda: K.recon_rows(rows, ll, x2, mu, th, kind='nb', size_from=x1, rec_out=rec)),
             ('zinb', 'rows + ll', lambda: K.recon_rows(rows, ll, x1, mu, tl, kind='zinb')),
             ('zinb', 'rows + ll + stored mean, size source = target', lambda: K.recon_rows(rows, ll, x1, mu, tl, kind='zinb', size_from=x1, rec_out=rec)),
             ('zinb', 'rows + ll + stored mean, size source = another matrix', lambda: K.recon_rows(rows, ll, x2, mu, tl, kind='zinb', size_from=x1, rec_out=rec)),
             ('gaussian (kind=None)', 'rows + ll', lambda: K.recon_rows(rows, ll, x1, mu, th))]
    for kind, what, fn in forms:
        fn(), fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()          # BATCH launches per replay: the event pair's own time is shared by all of them
        gc.collect()                            # (a dead model's evaluation graph must not be destroyed inside the capture)
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                for _ in range(BATCH):
                    fn()
        finally:
            gc.enable()
        graph.replay()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            us.append(1e3 * a.elapsed_time(b) / BATCH)
        v = np.asarray(us)
        out.append('| %s | %s | %d x %d | %.1f | %.1f .. %.1f |' % (kind, what, len(v), BATCH, np.median(v), v.min(), v.max()))
        print(out[-1], flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('reps', nargs='?', type=int, default=60)
    ap.add_argument('--only', default=None, metavar='CASE[,CASE...]', help='of: %s, kernel' % ', '.join(CASES))
    ap.add_argument('--stepwise-only', action='store_true')
    ap.add_argument('--out', nargs='?', default=None, const=os.path.join(ROOT, 'profiles', 'r22_eval_counts.md'), metavar='FILE')
    a = ap.parse_args()
    only = a.only.split(',') if a.only is not None else None
    if only is not None and not set(only) <= set(CASES) | {'kernel'}:
        ap.error('--only: unknown case in %s' % a.only)
    out = []
    if only != ['kernel']:
        models(a.reps, only, out, a.stepwise_only)
    if (only is None or 'kernel' in only) and not a.stepwise_only:
        kernel(max(a.reps, 50), out)
    if a.out is not None:
        text = open(a.out).read() if os.path.exists(a.out) else '# Whole-set evaluation of the count-decoder models\n\n%s\n%s\n' % (BEGIN, END)
        head, rest = text.split(BEGIN, 1)
        tail = rest.split(END, 1)[1]
        open(a.out, 'w').write(head + BEGIN + '\n' + '\n'.join(out) + '\n' + END + tail)


if __name__ == '__main__':
    main()
