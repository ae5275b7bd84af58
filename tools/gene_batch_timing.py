"""Timings of the inverse dispersion per (nuisance class, gene) (``dispersion='gene-batch'``), on the GPU:

1. the row pass -- ``gene_batch_rows.gene_batch_rows`` + the ``colsum`` of its workspace for S = 1, 2, 8 classes, balanced and
   90/10, over the candidates of the row-block rule, against ``gene_rows.gene_rows`` + ``colsum`` (the 'gene' pass at its own rule)
   in the same process -- at 900 x 978 and 2048 x 20000, 'nb' and 'zinb', plain and library-scaled.  S = 1 against 'gene' at the
   same row blocks is the cost of the class scan and of the launch's class dimension;
2. the captured train step at cfg-2 sizes (DrVAE, 150 rows, L = 2, 978 genes) and at the wide count sizes (1024 rows, L = 4,
   20000 genes): 'gene-batch' against 'gene' and 'gene-cell', all three on the same ``use_s`` model with 2 and with 8 classes.

Modes alternate inside one process (leg after leg, every mode once per leg); times are host clocks around work that ends in a
device synchronise; every figure is printed as a markdown table row.  ``python tools/gene_batch_timing.py [legs] [--rows-only |
--steps-only] [--no-wide]``."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from drvae_amd import engine as E                      # noqa: E402
from drvae_amd import gene_batch_rows as GB            # noqa: E402
from drvae_amd import gene_rows as G                   # noqa: E402
from drvae_amd import kernels as K                     # noqa: E402
from drvae_amd.arena import ParamArena                 # noqa: E402
from tools.gene_disp_timing import BOTH, DEV, ROW_SIZES, STEP_SIZES, counts, line, timed      # noqa: E402

ROWS_PER_BLOCK = (1, 2, 4, 8, 16, 32)
CLASSES = ((1, 'one class'), (2, 'balanced'), (2, '90/10'), (8, 'balanced'), (8, '90/10'))


def first_form(M, X, S):
    """the rule derived from the 'gene' rule by giving each class its share (``gene_batch_rows.row_blocks_for`` as first written)"""
    chunks = -(-X // G.CHUNK)
    return max(1, min(-(-G.TARGET_WORKGROUPS // (chunks * S)), -(-M // (G.MIN_ROWS * S)), M))


def classes(M, S, split, seed=0):
    """the class of every row, in random order: balanced, or class 0 on nine rows in ten and the others sharing the rest"""
    rs = np.random.RandomState(seed)
    if S == 1:
        return np.zeros(M, np.int32)
    if split == 'balanced':
        return rs.permutation(np.arange(M) % S).astype(np.int32)
    c = np.where(rs.rand(M) < 0.9, 0, 1 + rs.randint(0, S - 1, M))
    return c.astype(np.int32)


def row_pass(legs, calls=50):
    print('\n| row pass | mode | legs | median us | min .. max |\n|---|---|---|---|---|')
    for M, X in ROW_SIZES:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        rs = np.random.RandomState(M)
        ldp = (X + 3) // 4 * 4
        x = torch.zeros(M, ldp, device=DEV)[:, :X]
        x.copy_(t(counts(M, X, 1)))
        coef = torch.full((M,), 1.0 / M, device=DEV)
        table = t(rs.normal(0, 1, (8, X)).astype(np.float32))
        for family in ('nb', 'zinb'):
            nh = 2 if family == 'zinb' else 1
            heads = torch.zeros(M, nh * ldp, device=DEV)      # [mean | logit]
            mu, logit = heads[:, :X], heads[:, ldp:ldp + X] if nh == 2 else None
            mu.copy_(torch.nn.functional.softplus(t(rs.uniform(-2, 3, (M, X)).astype(np.float32))) + 1e-6)
            if logit is not None:
                logit.copy_(t(rs.normal(0, 2, (M, X)).astype(np.float32)))
            dh = torch.zeros_like(heads)
            dmu, dlogit = dh[:, :X], dh[:, ldp:ldp + X] if nh == 2 else None
            size = torch.zeros(M, device=DEV)
            part = torch.zeros(M, -(-X // G.CHUNK), device=DEV)
            for library in (False, True):
                kw = dict(kind=family, shift=1e-6, logit=logit, coef=coef, dmu=dmu, dlogit=dlogit, library=library,
                          size=size if library else None)
                modes = {}
                rb0 = G.row_blocks_for(M, X)
                ws0, g0 = torch.zeros(rb0, ldp, device=DEV), torch.zeros(X, device=DEV)

                def gene(ws=ws0, g=g0):
                    G.gene_rows(part, x, mu, table[0], ws=ws, **kw)
                    K.colsum(g, ws[:, :X])
                modes["'gene' rows + colsum, %d row blocks (R = %d) <- its rule" % (rb0, -(-M // rb0))] = gene
                for S, split in CLASSES:
                    cls = t(classes(M, S, split))
                    marks = {first_form(M, X, S): 'first form', GB.row_blocks_for(M, X, S): 'the rule', rb0: "'gene' rule"}
                    for rb in sorted({-(-M // r) for r in ROWS_PER_BLOCK} | set(marks), reverse=True):
                        ws, g = torch.zeros(rb, (S * X + 3) // 4 * 4, device=DEV), torch.zeros(S * X, device=DEV)

                        def run(ws=ws, g=g, cls=cls, S=S):
                            GB.gene_batch_rows(part, x, mu, table[:S], cls, ws=ws, **kw)
                            K.colsum(g, ws[:, :S * X])
                        note = ', '.join(sorted({v for k, v in marks.items() if k == rb}))
                        modes["'gene-batch' S = %d %s, %d row blocks (R = %d)%s" % (S, split, rb, -(-M // rb), ' <- ' + note if note else '')] = run
                res = {k: [] for k in modes}
                for fn in modes.values():
                    timed(fn, 3)
                for _ in range(legs):
                    for k, fn in modes.items():
                        res[k].append(timed(fn, calls if X < 5000 else max(5, calls // 5)))
                for k, vv in res.items():
                    line('%d x %d %s%s' % (M, X, family, ' lib' if library else ''), k, vv)


def build_step(size, family, dispersion, switches, S):
    rows, L, over = STEP_SIZES[size]
    cfg = E.StepConfig(kind='drvae', L=L, type_rec=family, dispersion=dispersion, add_noise_var=0.01 if switches else 0.0,
                       use_s=True, dim_s=S, **over, **switches)
    shapes = E.param_shapes(cfg)
    arena = ParamArena(shapes, DEV)
    rs = np.random.RandomState(123)
    fan = 1
    for k, shp in shapes.items():
        if k == E.GENE_THETA:
            continue
        if k.endswith('W_mu') or k.endswith('bias_mu'):
            a = rs.uniform(-1e-4, 1e-4, shp)
        else:
            if k.endswith('.weight'):
                fan = shp[1]
            a = rs.uniform(-1, 1, shp) / np.sqrt(fan)
        arena.p(k).copy_(torch.as_tensor(a, dtype=torch.float32))
    eng = E.FusedStep(cfg, arena, seed=1000)
    X = cfg.dim_x
    x1 = counts(rows, X, 1)
    hx = (np.arange(rows) % 3 == 0).astype(np.int64)
    x2 = counts(rows, X, 2) * hx[:, None].astype(np.float32)
    hy = (np.arange(rows) % 4 != 1).astype(np.int64)
    y = np.random.RandomState(3).randint(0, cfg.dim_y, rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    eng.set_batch(t(x1), t(x2), y, hx, hy, s=classes(rows, S, 'balanced').astype(np.int64))
    return eng


def steps(legs, wide=True):
    print('\n| captured step | mode | legs | median us | min .. max |\n|---|---|---|---|---|')
    for size in ('cfg2',) + (('wide',) if wide else ()):
        n = 100 if size == 'cfg2' else 5
        for family in ('nb', 'zinb'):
            for sw_name, sw in (('plain', {}), ('log1p + library size', BOTH)):
                for S in (2, 8):
                    engines = {}
                    for disp in ('gene-cell', 'gene', 'gene-batch'):
                        eng = build_step(size, family, disp, sw, S)
                        for _ in range(3):
                            eng.train_step()
                        eng.capture()
                        timed(eng.replay, 5 if size == 'cfg2' else 2)
                        engines[disp] = eng
                    res = {d: [] for d in engines}
                    for _ in range(legs):
                        for d, eng in engines.items():
                            res[d].append(timed(eng.replay, n))
                    for d, vv in res.items():
                        line('%s %s %s, use_s with %d classes' % (size, family, sw_name, S), "dispersion='%s'" % d, vv)
                    fin = {d: all(np.isfinite(v) for v in e.losses().values()) for d, e in engines.items()}
                    print('|  | losses finite: %s |  |  |  |' % fin, flush=True)
                    del engines
                    torch.cuda.empty_cache()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    legs = int(args[0]) if args else 5
    if '--steps-only' not in sys.argv:
        row_pass(legs)
    if '--rows-only' not in sys.argv:
        steps(legs, wide='--no-wide' not in sys.argv)


if __name__ == '__main__':
    main()
