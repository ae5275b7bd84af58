#!/usr/bin/env python3
"""Row-chunked whole-set evaluation (``evaluate_performance_on_dataset(chunk_rows=C)``, ``evaluate._ChunkedEval``) against the
one-replay evaluation (``evaluate._EvalGraph``) on the same model and HBM-resident set, the modes alternating inside one process
(shapes warmed up, evaluators built before the clock starts; host clock around a call that ends in the evaluation's one
device-to-host copy), and a large ``CsrRows`` set: time and peak device memory of the chunked evaluation and of the densifying path.

Cases: 'cfg2' (DrVAE, Gaussian decoder, 8192 x 978 at the cfg-2 sizes), 'wide' ('nb' with x_transform='log1p' +
library_size=True, 2048 x 20 000), each at C = 1024 / 2048 / 4096; 'csr' (a CSR set of 65 536 x 20 000 at 7 % density, 'nb' with
both switches, C = 2048).

``python tools/eval_chunk_bench.py [reps] [--only cfg2,wide,csr] [--csr-rows N] [--out [FILE]]`` (GPU box only).  Prints markdown
tables -- median with min .. max -- and with ``--out`` replaces the text between the ``<!-- timings -->`` markers of FILE
(default profiles/r31_eval_chunks.md)."""
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
from drvae_amd.sparse_rows import CsrRows       # noqa: E402

BEGIN, END = '<!-- timings:begin -->', '<!-- timings:end -->'
CASES = {'cfg2': dict(n=8192, X=978), 'wide': dict(type_rec='nb', x_transform='log1p', library_size=True, n=2048, X=20000)}
CHUNKS = (1024, 2048, 4096)


def model_for(X, dev='cuda', **kw):
    model = DrVAE(dim_x=X, dim_s=1, dim_y=2, dim_h_en_z1=[800], dim_h_de_z1=[200], dim_h_en_z3=[200], dim_h_de_x=[600], dim_h_clf=[],
                  dim_z1=100, dim_z3=100, nonlinearity='elu', learning_rate=5e-4, L=2, weight_decay=0.05, add_noise_var=0.0,
                  use_MMD=False, pertloss_rate=0.05, random_seed=123, epochs=1, batch_size=150, **kw).to(dev)
    model.w2log = lambda *a: None
    return model


def flags(n, dev):
    i = torch.arange(n, device=dev)
    return (i % 3 == 0).long(), (i % 4 != 1).long(), torch.randint(0, 2, (n,), device=dev, generator=torch.Generator(dev).manual_seed(7))


def dense_set(n, X, dev='cuda', seed=1):
    g = torch.Generator(dev).manual_seed(seed)
    hx, hy, y = flags(n, dev)
    draw = lambda: torch.poisson(torch.rand(n, X, device=dev, generator=g) * 6.0, generator=g)
    x1 = draw()
    x2 = draw() * hx[:, None].float()
    return D.DrVAEDataset(x1, x2, torch.zeros(n, dtype=torch.int64, device=dev), y, hx, hy)


def csr_matrix(n, X, density, dev, seed, keep_rows=None, block=4096):
    """``n`` x ``X`` counts at ``density`` as CSR rows, built on the device a block of rows at a time (the dense matrix never
    exists); ``keep_rows`` (n, 0/1): the other rows are empty"""
    g = torch.Generator(dev).manual_seed(seed)
    ptr, idx, val, base = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], 0
    for a in range(0, n, block):
        b = min(n, a + block)
        keep = torch.rand(b - a, X, device=dev, generator=g) < density
        if keep_rows is not None:
            keep &= keep_rows[a:b, None] != 0
        r, c = torch.nonzero(keep, as_tuple=True)
        ptr.append(base + keep.sum(1).cumsum(0))
        base = int(ptr[-1][-1])
        idx.append(c.to(torch.int32))
        val.append(1.0 + torch.poisson(torch.full((c.numel(),), 2.0, device=dev), generator=g))
        del keep, r, c
    return CsrRows(torch.cat(ptr), torch.cat(idx), torch.cat(val), (n, X))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def cell(v):
    v = np.asarray(v)
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v.min(), v.max())


def dense_cases(reps, only, out):
    from drvae_amd import fit as F
    out += ['| model, set | one replay ms | ' + ' | '.join('C = %d ms (chunks)' % c for c in CHUNKS) + ' |',
            '|---|---|' + '---|' * len(CHUNKS)]
    for case, c in CASES.items():
        if case not in only:
            continue
        c = dict(c)
        n, X = c.pop('n'), c.pop('X')
        model, ds = model_for(X, **c), dense_set(n, X)
        modes = [('one replay', lambda: model.evaluate_performance_on_dataset(ds))]
        for C in CHUNKS:
            modes.append(('C=%d' % C, lambda C=C: model.evaluate_performance_on_dataset(ds, chunk_rows=C)))
        for _, fn in modes:
            fn(), fn()
        assert F._EvalGraph.get(model, ds) is not None, 'the one-replay path was not taken'
        ms = {name: [] for name, _ in modes}
        for _ in range(reps if case != 'wide' else max(5, reps // 3)):
            for name, fn in modes:           # (the modes alternate inside one process)
                ms[name].append(timed(fn))
        n_chunks = [len(model._eval_chunked[(id(ds), C)].spans) for C in CHUNKS]
        label = "drvae %s, %d x %d" % ("'%s' log1p + library size" % c['type_rec'] if c else 'Gaussian (cfg-2 sizes)', n, X)
        out.append('| %s | %s | ' % (label, cell(ms['one replay'])) +
                   ' | '.join('%s (%d)' % (cell(ms['C=%d' % C]), k) for C, k in zip(CHUNKS, n_chunks)) + ' |')
        print(out[-1], flush=True)
        base = np.median(ms['one replay'])
        spread = max(ms['one replay']) - min(ms['one replay'])
        out.append('| ... chunked minus one replay (the one-replay windows span %.3f ms) | | ' % spread +
                   ' | '.join('%+.3f ms (%+.1f %%)' % (np.median(ms['C=%d' % C]) - base, 100 * (np.median(ms['C=%d' % C]) / base - 1))
                              for C in CHUNKS) + ' |')
        print(out[-1], flush=True)
        del model, ds, modes
        gc.collect()
        torch.cuda.empty_cache()


def peak_of(fn):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ms = timed(fn)
    return ms, torch.cuda.max_memory_allocated() - before


def csr_case(reps, n, out, X=20000, density=0.07, C=2048, dev='cuda'):
    hx, hy, y = flags(n, dev)
    x1 = csr_matrix(n, X, density, dev, 11)
    x2 = csr_matrix(n, X, density, dev, 12, keep_rows=hx)
    ds = D.DrVAEDataset(x1, x2, torch.zeros(n, dtype=torch.int64, device=dev), y, hx, hy)
    held = x1.nbytes() + x2.nbytes()
    model = model_for(X, type_rec='nb', x_transform='log1p', library_size=True)
    model.engine()
    out += ['', '| CSR set %d x %d at density %.2f (arrays: %.2f GB; one dense matrix: %.2f GB) | ms | peak device memory above the set |'
            % (n, X, density, held / 1e9, n * X * 4 / 1e9), '|---|---|---|']
    chunked = lambda: model.evaluate_performance_on_dataset(ds, chunk_rows=C)
    ms0, peak = peak_of(chunked)              # (evaluators built inside: the first call)
    runs = [timed(chunked) for _ in range(reps)]
    out.append('| chunked, C = %d (%d chunks): first call, evaluators built inside | %.1f | %.3f GB |'
               % (C, len(model._eval_chunked[(id(ds), C)].spans), ms0, peak / 1e9))
    out.append('| chunked, C = %d: later calls | %s | |' % (C, cell(runs)))
    model.__dict__.pop('_eval_chunked', None)
    try:
        ms1, peak1 = peak_of(lambda: model.evaluate_performance_on_dataset(ds))
        runs1 = [timed(lambda: model.evaluate_performance_on_dataset(ds)) for _ in range(max(2, reps // 3))]
        out.append('| densifying path (``eval_chunk_rows=None``): first call | %.1f | %.3f GB |' % (ms1, peak1 / 1e9))
        out.append('| densifying path: later calls | %s | |' % cell(runs1))
    except torch.cuda.OutOfMemoryError as e:
        out.append('| densifying path (``eval_chunk_rows=None``) | did not complete: %s | |' % str(e).split('.')[0])
    for line in out[-6:]:
        print(line, flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('reps', nargs='?', type=int, default=15)
    ap.add_argument('--only', default='cfg2,wide,csr')
    ap.add_argument('--csr-rows', type=int, default=65536)
    ap.add_argument('--out', nargs='?', default=None, const=os.path.join(ROOT, 'profiles', 'r31_eval_chunks.md'), metavar='FILE')
    a = ap.parse_args()
    only = a.only.split(',')
    if not set(only) <= set(CASES) | {'csr'}:
        ap.error('--only: unknown case in %s' % a.only)
    out = []
    dense_cases(a.reps, only, out)
    if 'csr' in only:
        csr_case(max(3, a.reps // 3), a.csr_rows, out)
    if a.out is not None:
        text = open(a.out).read() if os.path.exists(a.out) else '# Row-chunked whole-set evaluation\n\n%s\n%s\n' % (BEGIN, END)
        head, rest = text.split(BEGIN, 1)
        tail = rest.split(END, 1)[1]
        open(a.out, 'w').write(head + BEGIN + '\n' + '\n'.join(out) + '\n' + END + tail)


if __name__ == '__main__':
    main()
