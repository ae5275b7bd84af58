"""Float64 reference, fp32 emulations and the CPU stand-in of the count rows with an inverse dispersion PER (NUISANCE CLASS, GENE)
(``drvae_amd.gene_batch_rows``; the count kinds of ``dv_gauss_nll_rows_raw_cs`` with ``n_cls >= 1``; ``dispersion='gene-batch'``),
a model-level float64 reference and a generator of counts whose classes differ in their dispersion.  Test-only; everything is
built from ``tests/gene_disp_ref.py``: for each class k the launch IS the ``'gene'`` launch at ``theta_raw[k]`` on that class's
rows, so

* the float64 reference is ``gene_disp_ref.reference`` per class, at row k of the table, on the rows of class k;
* the bounds are that file's own -- the per-element bounds, the chunk-sum bound of a row partial, and its derived ``ws`` bound
  (sum of the addends' bounds + (n - 1) U sum |addend|, any order) applied per (row block, class) to the n rows of that class
  in that block.  No new constant.

The class of row r is ``cls[cls_src[r]]`` (``cls_src``: the batch row of a decoder row), without ``cls_src`` ``cls[r]``.  The
faulty emulations (``emulate(..., fault=...)``) are listed in ``FAULTS``."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import counts_ref as CR
from tests import gene_disp_ref as GR
from tests import nb_ref as R
from tests import ref64
from tests.gene_disp_ref import CHUNK, RAW, blocks, theta32      # noqa: F401
from tests.ref64 import U

FAULTS = ('neighbour_theta',   # class k reads the table's row (k + 1) % S
          'cls_direct',        # the class taken from cls[r], not from cls[cls_src[r]]
          'pair_neighbour',    # a pair row (r >= pair_from) under the class of x1's NEIGHBOUR: cls[(cls_src[r] + 1) % B]
          'ws_swapped',        # the segments of classes 0 and 1 of ``ws`` swapped
          'short_block',       # the rows of one class in the short last row block dropped
          'no_clear',          # accumulators not cleared between classes: class k's sums start from class k - 1's
          'stale_partial')     # behind a skipped row, the partial of the last TAKEN row of the slot summed into out_part
CALLS = {'gene_batch_rows': 0, 'gene_batch_rows_lib': 0}


def row_classes(cls, cls_src, M):
    cls = np.asarray(cls, np.int64).reshape(-1)
    return cls[:M] if cls_src is None else cls[np.asarray(cls_src, np.int64).reshape(-1)[:M]]


def shape(M, X, S, row_blocks=None):
    from drvae_amd import gene_batch_rows as GB
    return -(-X // CHUNK), GB.row_blocks_for(M, X, S) if row_blocks is None else int(row_blocks)


def row_blocks_for(M, X, S):
    from drvae_amd import gene_batch_rows as GB
    return GB.row_blocks_for(M, X, S)


# --------------------------------------------------------------------------------------------- float64 reference
def reference(kind, x, mu, raw, cls, logit=None, coef=None, shift=R.MU_SHIFT, library=False, s=None, row_blocks=1):
    """``gene_disp_ref.reference`` per class: ``x`` the TARGET row of every row (gathered already), ``raw`` the (S, X) table,
    ``cls`` the class of every row (resolved through ``cls_src`` already), ``s`` fp32 size factors per row.  Keys: parts /
    parts_bound (M, chunks), theta (S, X) fp32, with ``coef`` gm, gd (zinb) and their bounds (M, X), ws / ws_bound
    (row_blocks, S, X): per (block, class), grad / grad_bound (S, X): the blocks summed"""
    M, X = mu.shape
    S = raw.shape[0]
    cls = np.asarray(cls, np.int64).reshape(-1)
    chunks = -(-X // CHUNK)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float64)
    out = dict(parts=z(M, chunks), parts_bound=z(M, chunks), theta=torch.stack([theta32(raw[k]) for k in range(S)]))
    if coef is not None:
        out.update(gm=z(M, X), gm_bound=z(M, X), ws=z(row_blocks, S, X), ws_bound=z(row_blocks, S, X), grad=z(S, X),
                   grad_bound=z(S, X))
        if kind == 'zinb':
            out.update(gd=z(M, X), gd_bound=z(M, X))
    t = lambda a: None if a is None else torch.as_tensor(a)
    for k in range(S):
        rows = torch.as_tensor(np.nonzero(cls == k)[0])
        if rows.numel() == 0:
            continue
        sub = lambda a: None if a is None else t(a)[rows]
        r = GR.reference(kind, t(x)[rows], t(mu)[rows], raw[k], sub(logit), coef=sub(coef), shift=shift, library=library,
                         s=None if s is None else np.asarray(s)[rows.numpy()])
        out['parts'][rows], out['parts_bound'][rows] = r['parts'], r['parts_bound']
        if coef is None:
            continue
        for key in ('gm', 'gm_bound') + (('gd', 'gd_bound') if kind == 'zinb' else ()):
            out[key][rows] = r[key]
        # the table's gradient, the blocks summed: ``gene_disp_ref.reference``'s ws and its any-order bound over the class's rows
        out['grad'][k], out['grad_bound'][k] = r['ws'], r['ws_bound']
        # ... and the same two formed over the class's rows of one block
        for b, (r0, r1) in enumerate(blocks(M, row_blocks)):
            m = (rows >= r0) & (rows < r1)
            n = int(m.sum())
            if n:
                out['ws'][b, k] = r['gt'][m].sum(0)
                out['ws_bound'][b, k] = r['gt_bound'][m].sum(0) + (n - 1) * U * r['gt'][m].abs().sum(0)
    return out


# ----------------------------------------------------------------------------------------------- fp32 emulation
def emulate(kind, x, mu, raw, cls, logit=None, coef=None, shift=R.MU_SHIFT, library=False, xidx=None, cls_src=None,
            row_blocks=1, fault=None, pair_from=None):
    """the launch in numpy float32 (``gene_disp_ref.emulate`` per row at the row's class's theta, the kernel's summation orders):
    dict(parts (M, chunks), size, cls (M,), and with ``coef`` gm, gd (zinb), ws_blocks (row_blocks, S X)).  ``fault``: one
    of ``FAULTS`` (``pair_from``: the first pair row, for 'pair_neighbour')"""
    assert fault is None or fault in FAULTS
    f = np.float32
    x, mu, raw = R._f(x), R._f(mu), R._f(raw)
    M, X = mu.shape
    S = raw.shape[0]
    cvec = np.asarray(cls, np.int64).reshape(-1)
    c = row_classes(cvec, cls_src, M).copy()
    if fault == 'cls_direct' and cls_src is not None:
        c = cvec[np.arange(M) % cvec.size]
    if fault == 'pair_neighbour' and cls_src is not None:
        src = np.asarray(cls_src, np.int64)[:M].copy()
        src[pair_from:] = (src[pair_from:] + 1) % cvec.size
        c = cvec[src]
    idx = np.arange(M) if xidx is None else np.asarray(xidx, np.int64)
    chunks = -(-X // CHUNK)
    parts, gm, gd, add = np.zeros((M, chunks), f), np.zeros((M, X), f), np.zeros((M, X), f), np.zeros((M, X), f)
    size = np.zeros(M, f) if library else None
    live = (c >= 0) & (c < S)             # (a class outside the table: no workgroup takes the row)
    for k in range(S):
        rows = np.nonzero(c == k)[0]
        if rows.size == 0:
            continue
        th = raw[(k + 1) % S] if fault == 'neighbour_theta' else raw[k]
        # one row per block: ws_blocks[i] is then row i's own addend coef * d/da_t (0 + a == a)
        e = GR.emulate(kind, x, mu[rows], th, None if logit is None else R._f(logit)[rows],
                       None if coef is None else R._f(coef).reshape(-1)[rows], shift=shift, library=library, xidx=idx[rows],
                       row_blocks=rows.size)
        parts[rows] = e['parts']
        if library:
            size[rows] = e['size']
        if coef is not None:
            gm[rows], add[rows] = e['gm'], e['ws_blocks']
            if kind == 'zinb':
                gd[rows] = e['gd']
    blk = blocks(M, row_blocks)
    if fault == 'short_block' and blk[-1][1] - blk[-1][0] < blk[0][1] - blk[0][0] and blk[-1][1] > blk[-1][0]:
        k0 = c[blk[-1][0]]
        live = live & ~((np.arange(M) >= blk[-1][0]) & (c == k0))
    if fault == 'stale_partial':
        good = parts.copy()
        for r0, r1 in blk:
            for k in range(S):
                taken = [r for r in range(r0, r1) if c[r] == k]
                # (slot = (r - r0) & 1 with one barrier a row: the partial two slots back is still there when a row was skipped)
                for i in range(1, len(taken)):
                    if taken[i] - taken[i - 1] > 1:
                        parts[taken[i]] = (good[taken[i]] + good[taken[i - 1]]).astype(f)
    parts[~live] = 0
    out = dict(parts=parts, size=size, cls=c)
    if coef is None:
        return out
    gm[~live], gd[~live] = 0, 0
    wsb = np.zeros((row_blocks, S, X), f)
    for b, (r0, r1) in enumerate(blk):
        acc = np.zeros(X, f)
        for k in range(S):
            if fault != 'no_clear':
                acc = np.zeros(X, f)
            for r in range(r0, r1):
                if live[r] and c[r] == k:
                    acc = (acc + add[r]).astype(f)
            wsb[b, k] = acc
    if fault == 'ws_swapped' and S > 1:
        wsb[:, [0, 1]] = wsb[:, [1, 0]]
    out.update(gm=gm, ws_blocks=wsb.reshape(row_blocks, S * X))
    if kind == 'zinb':
        out['gd'] = gd
    return out


def excess(emu, ref, coef=None):
    """|emulation or launch - reference| / bound per output: dict of worst fractions (<= 1 passes; a non-finite output: inf)"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))

    def worst(a, r, b):
        a = t(a).reshape(r.shape)
        if not bool(torch.isfinite(a).all()):
            return float('inf')
        return float(ref64.excess(a, r, b).max()) if a.numel() else 0.0
    e = dict(parts=worst(emu['parts'], ref['parts'], ref['parts_bound']))
    if coef is not None:
        e['gm'] = worst(emu['gm'], ref['gm'], ref['gm_bound'])
        if 'gd' in ref:
            e['gd'] = worst(emu['gd'], ref['gd'], ref['gd_bound'])
        e['ws'] = worst(emu['ws_blocks'], ref['ws'], ref['ws_bound'])
        if 'grad' in emu:       # (the column sum over the blocks, where the caller formed it)
            e['grad'] = worst(emu['grad'], ref['grad'], ref['grad_bound'])
    return e


# ------------------------------------------------------------------------------------------------ CPU stand-in
def gene_batch_rows(out_part, x, mu, theta_raw, cls, *, kind, cls_src=None, shift=0.0, logit=None, xidx=None, coef=None,
                    dmu=None, dlogit=None, ws=None, library=False, size=None, row_blocks=None):
    """stand-in of ``drvae_amd.gene_batch_rows.gene_batch_rows``: the careful fp32 emulation of the launch (or, ``exact``, the
    float64 reference rounded once), written into the caller's buffers the way the launch writes them"""
    assert kind in ('nb', 'zinb') and (logit is not None) == (kind == 'zinb')
    CALLS['gene_batch_rows_lib' if library else 'gene_batch_rows'] += 1
    M, X = mu.shape
    assert theta_raw.dim() == 2 and theta_raw.shape[1] == X
    S = theta_raw.shape[0]
    grad = dmu is not None
    if row_blocks is None:
        row_blocks = ws.shape[0] if grad else None
    chunks, rbs = shape(M, X, S, row_blocks)
    assert tuple(out_part.shape) == (M, chunks)
    assert 1 <= rbs <= max(M, 1) and (not grad or (ws.shape[0] == rbs and ws.shape[1] >= S * X and coef is not None))
    assert grad or (ws is None and dlogit is None)
    assert (dlogit is not None) == (grad and kind == 'zinb')
    assert not (library and chunks > 1 and size is None)
    assert cls.dtype == torch.int32 and (cls_src is None or (cls_src.dtype == torch.int32 and cls_src.numel() >= M))
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    c = row_classes(n(cls), n(cls_src), M)
    assert c.size == M and (M == 0 or (c.min() >= 0 and c.max() < S)), 'a class outside the table'
    if GR.MODE['exact']:
        e = _exact(kind, x, mu, theta_raw, c, logit, coef if grad else None, shift, library, xidx, rbs)
    else:
        e = emulate(kind, n(x), n(mu), n(theta_raw), c, n(logit), n(coef) if grad else None, shift=shift, library=library,
                    xidx=n(xidx), row_blocks=rbs)
    put = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.device))
    put(out_part, e['parts'])
    if library and size is not None:
        put(size[:M], e['size'])
    if grad:
        put(dmu, e['gm'])
        if kind == 'zinb':
            put(dlogit, e['gd'])
        put(ws[:, :S * X], e['ws_blocks'])


def _exact(kind, x, mu, raw, c, logit, coef, shift, library, xidx, rbs):
    xs = x[xidx.long()] if xidx is not None else x
    cp = lambda t: None if t is None else t.detach().cpu()
    r = reference(kind, cp(xs), cp(mu), cp(raw), c, cp(logit), coef=cp(coef), shift=shift, library=library, row_blocks=rbs)
    f = lambda t: t.to(torch.float32).numpy()
    out = dict(parts=f(r['parts']), size=CR.size_factor32(xs) if library else None)
    if coef is not None:
        out.update(gm=f(r['gm']), gd=f(r['gd']) if kind == 'zinb' else None, ws_blocks=f(r['ws']).reshape(rbs, -1))
    return out


FUNCTIONS = ('gene_batch_rows', 'row_blocks_for', 'shape')


def install(monkeypatch, exact=False):
    """``gene_disp_ref.install`` (and with it ``kernel_ref.install``) plus the stand-in of the launch over
    ``drvae_amd.gene_batch_rows`` for one CPU test: the careful fp32 emulation, or with ``exact`` float64 rounded once"""
    import drvae_amd.gene_batch_rows as GB
    GR.install(monkeypatch, exact=exact)
    monkeypatch.setattr(GB, 'gene_batch_rows', gene_batch_rows)
    for k in CALLS:
        CALLS[k] = 0


# ------------------------------------------------------------------------------- model-level float64 reference
def ModelRef(family, spec, seed=9, norm=False, **kw):
    """the float64 model-level reference of a ``dispersion='gene-batch'`` model: ``gene_disp_ref.ModelRef`` with ``RAW`` a
    (dim_s, dim_x) table (small random values) and every decoder row reading the row of its class -- the class the one-hot block
    names that is the decoder's last input"""
    assert spec.use_s
    ref = GR.ModelRef(family, spec, seed=seed, norm=norm, **kw)
    base = type(ref)

    class _Batch(base):
        @contextlib.contextmanager
        def context(self):
            from oracle import blocks_ref as B
            from tests import zinb_ref as Z
            with super().context():
                inner = B.diag_gaussian_sigma

                def heads(inputs, p, prefix, n_hidden, nonlin, constrain_means=False):
                    h = B.mlp(inputs, p, prefix + '.nnet', n_hidden, nonlin)
                    mu = F.softplus(B.linear(h, p, prefix + '.encoder_mu.linear_mu')) + R.MU_SHIFT
                    theta = (F.softplus(p[RAW]) + ref64.f32(R.THETA_SHIFT))[inputs[-1].argmax(1)]
                    return (mu, theta, B.linear(h, p, Z.LOGIT_HEAD)) if family == 'zinb' else (mu, theta)
                B.diag_gaussian_sigma = heads
                try:
                    yield
                finally:
                    B.diag_gaussian_sigma = inner

    from oracle import models_ref as M
    ref.__class__ = _Batch
    rs = np.random.RandomState(seed + 177)
    init = type(ref.init32)(ref.init32)
    init[RAW] = (0.5 * rs.standard_normal((spec.dim_s, spec.dim_x))).astype(np.float32)
    ref.init32 = init
    params = type(init)((k, torch.tensor(v.astype(np.float64), requires_grad=True)) for k, v in init.items())
    ref.tr = M.RefTrainer(spec, params)
    ref.avg = {k: v.detach().clone() for k, v in ref.tr.params.items()}
    return ref


# ------------------------------------------------------------------- counts whose classes differ in dispersion
def class_counts(n, X=13, seed=0, thetas=(0.5, 20.0), depth_spread=4.0):
    """(x, s, y): Gamma-Poisson counts of ``len(thetas)`` nuisance classes, class k with true inverse dispersion thetas[k] in
    EVERY gene; gene means 3 (1 .. 4) times a per-row depth spread log-uniformly over ``depth_spread``; y shifts every third gene"""
    rs = np.random.RandomState(seed)
    s = rs.randint(0, len(thetas), n)
    y = rs.randint(0, 2, n)
    depth = np.exp(rs.uniform(-0.5, 0.5, n) * np.log(depth_spread))
    mean = 3.0 * depth[:, None] * (1.0 + (np.arange(X) % 4))[None, :] * \
        np.where((np.arange(X) % 3 == 0)[None, :], 1.0 + 0.8 * y[:, None], 1.0)
    th = np.asarray(thetas)[s][:, None]
    x = rs.poisson(rs.gamma(np.broadcast_to(th, mean.shape), mean / th))
    return x.astype(np.float32), s.astype(np.int64), y.astype(np.int64)


def class_dataset(kind, n, seed, dev='cpu', **kw):
    """a dataset of ``class_counts`` for model ``kind`` (the layout of ``gene_disp_ref.gp_dataset``, with the classes as s)"""
    from drvae_amd import data as D
    x1, s, y = class_counts(n, seed=seed, **kw)
    x2, _, _ = class_counts(n, seed=seed + 500, **kw)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(s), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2 * hx[:, None].astype(np.float32)), t(s), t(y), t(hx), t(hy))
