"""Float64 reference, bounds, fp32 emulations and the CPU stand-in of the count rows with a GENE-WISE inverse dispersion
(``drvae_amd.gene_rows``; the count kinds of ``dv_gauss_nll_rows_raw_cs``; ``dispersion='gene'``), a model-level float64
reference and a generator of counts with a per-gene theta.  Test-only; builds on ``tests/nb_ref.py``, ``tests/counts_ref.py``
and ``tests/zinb_ref.py``.

theta is one pre-activation vector ``raw`` (X,): theta_g = softplus(raw_g) + fl32(1e-3), formed by the kernel in double and
rounded ONCE to fp32.  ``theta32`` forms the same number in float64 and rounds it once: it is the fp32 theta the row formula
receives, so the per-element terms, d/da_m and d/da_d are held to the bounds of ``nb_ref`` / ``counts_ref`` / ``zinb_ref``
UNCHANGED, with that theta broadcast over the rows.

What is new is the two sums:

* a row partial ``out_part[r, c]`` sums the <= 1024 terms of one gene chunk: per-thread partials of four terms (3 roundings), the
  wave's butterfly (6), the four waves (2) -- 11 roundings of partial sums, granted as ``ref64.row_sum_bound(., 1024)`` (20 U
  times the sum of the components), on top of the sum of the elements' own bounds;
* ``ws`` summed over the row blocks, the gradient of ``raw``: sum_r c_r g_t[r, g].  Each addend carries its own bound (the
  d/da_t bound of the element, which already holds |c_r|), and a sum of M addends adds at most (M - 1) roundings of partial
  sums, each at most U sum_r |c_r g_t| to first order: ``ws_bound = sum_r gt_bound + (M - 1) U sum_r |c_r g_t|``.  It holds in
  ANY summation order -- ascending rows inside a block, the blocks in ``dv_colsum``'s order -- so it is derived, not measured.

The faulty emulations (``emulate(..., fault=...)``) and what catches them are listed in ``FAULTS``."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import counts_ref as CR
from tests import nb_ref as R
from tests import ref64
from tests import zinb_ref as Z
from tests.ref64 import U, f64

CHUNK = 1024
RAW = 'decoder_x.decoder_t.raw_theta'
SG_HEAD = 'decoder_x.encoder_sg.linear_sg'            # the oracle's second head: the theta head a gene-wise model does not have
FAULTS = ('seam',           # theta of the neighbouring gene at a chunk seam (gene 1024 c reads theta[1024 c - 1])
          'short_block',    # the last, short row block dropped: its rows are never walked
          'no_coef',        # coef missing from the theta sum
          'no_slope',       # the theta slope missing from d/da_t
          'no_clear',       # accumulators not cleared between chunks: chunk c's sums start from chunk c - 1's
          'wrong_s')        # (library kinds, with xidx) s taken from row r of x, not from its target row xidx[r]
CALLS = {'gene_rows': 0, 'gene_rows_lib': 0}


def theta32(raw):
    """the fp32 theta of every gene: softplus(raw) + fl32(1e-3) in float64, rounded once"""
    r = f64(raw).reshape(-1)
    return (F.softplus(r) + ref64.f32(R.THETA_SHIFT)).to(torch.float32)


def shape(M, X, row_blocks=None):
    from drvae_amd import gene_rows as G
    return -(-X // CHUNK), G.row_blocks_for(M, X) if row_blocks is None else int(row_blocks)


def row_blocks_for(M, X):
    from drvae_amd import gene_rows as G
    return G.row_blocks_for(M, X)


def blocks(M, row_blocks):
    """[(r0, r1)] of every row block: R = ceil(M / row_blocks) rows each, the last one short or empty"""
    Rr = -(-M // row_blocks) if M else 0
    return [(min(M, b * Rr), min(M, (b + 1) * Rr)) for b in range(row_blocks)]


# --------------------------------------------------------------------------------------------- float64 reference
def reference(kind, x, mu, raw, logit=None, coef=None, shift=R.MU_SHIFT, library=False, s=None):
    """everything the tests compare a launch with, from the exact fp32 values it received.  ``x``: the TARGET row of every
    decoder row (gathered through ``xidx`` already); ``s``: fp32 size factors per row (library; default: those of ``x``).
    Keys: ll / ll_bound per element, parts / parts_bound (M, chunks), with ``coef`` gm, gd (zinb), gt and their bounds, ws /
    ws_bound (X,); theta (X,) fp32"""
    th = theta32(raw)
    M, X = mu.shape
    TH = th[None, :].expand(M, X)
    if kind == 'zinb':
        r = Z.reference(x, mu, TH, logit, coef=coef, shift=shift, library=library, s=s)
    elif library:
        r = CR.reference('nb', x, mu, TH, coef=coef, shift=shift, s=s)
    else:
        r = R.reference(x, mu, TH, coef=coef, shift=shift)
        r['ll_bound'] = ref64.bound(R.C_ROW, r['comps'])
    out = dict(r, theta=th)
    chunks = -(-X // CHUNK)
    cut = lambda t, c: t[:, c * CHUNK:(c + 1) * CHUNK]
    out['parts'] = torch.stack([cut(r['ll'], c).sum(1) for c in range(chunks)], 1)
    out['parts_bound'] = torch.stack([cut(r['ll_bound'], c).sum(1) + ref64.row_sum_bound(cut(r['comps'], c), CHUNK)
                                      for c in range(chunks)], 1)
    if coef is not None:
        out['ws'] = r['gt'].sum(0)
        out['ws_bound'] = r['gt_bound'].sum(0) + max(M - 1, 0) * U * r['gt'].abs().sum(0)
    return out


# ----------------------------------------------------------------------------------------------- fp32 emulation
def _elem32(kind, x, mu, th, logit, shift, s):
    if kind == 'zinb':
        return Z.emulate_fp32(x, mu, th, logit, shift=shift, s=s)
    ll, gm, gt = CR.emulate_fp32(x, mu, th, s, shift=shift) if s is not None else R.emulate_fp32(x, mu, th, shift=shift)
    return ll, gm, gt, None


def emulate(kind, x, mu, raw, logit=None, coef=None, shift=R.MU_SHIFT, library=False, xidx=None, row_blocks=1, fault=None):
    """the launch in numpy float32: ``x`` the UNGATHERED targets with ``xidx``, as the launcher gets them.  Returns dict(parts
    (M, chunks), size (M,) or None, and with ``coef`` gm, gd (zinb), ws_blocks (row_blocks, X), ws (X,)).  Careful = the
    kernel's construction: the elements by the careful emulations of ``nb_ref`` / ``counts_ref`` / ``zinb_ref`` at the once-rounded
    theta, chunk sums and column sums accumulated in fp32 (rows ascending inside a block, then the blocks ascending);
    ``fault``: one of ``FAULTS``"""
    assert fault is None or fault in FAULTS
    f = np.float32
    x, mu = R._f(x), R._f(mu)
    M, X = mu.shape
    idx = np.arange(M) if xidx is None else np.asarray(xidx, np.int64)
    xs = x[idx]
    th = theta32(torch.as_tensor(np.asarray(raw, np.float32))).numpy()
    if fault == 'seam':
        th = th.copy()
        for g in range(CHUNK, X, CHUNK):
            th[g] = th[g - 1]
    size = None
    if library:
        src = x[:M] if fault == 'wrong_s' else xs
        size = (np.maximum(src.astype(np.float64).sum(1), 1.0).astype(f) / f(X)).astype(f)
    TH = np.broadcast_to(th[None, :], (M, X))
    ll, gm, gt, gd = _elem32(kind, xs, mu, TH, None if logit is None else R._f(logit), shift, size)
    if fault == 'no_slope':
        with np.errstate(all='ignore'):
            gt = (gt / -np.expm1(-(TH - f(R.THETA_SHIFT)))).astype(f)
    live = np.ones(M, bool)
    blk = blocks(M, row_blocks)
    if fault == 'short_block' and blk[-1][1] - blk[-1][0] < blk[0][1] - blk[0][0]:
        live[blk[-1][0]:] = False
    chunks = -(-X // CHUNK)
    parts = np.zeros((M, chunks), f)
    for c in range(chunks):
        parts[:, c] = np.add.reduce(ll[:, c * CHUNK:(c + 1) * CHUNK], axis=1, dtype=f)
    parts[~live] = 0
    out = dict(parts=parts, size=size, theta=th)
    if coef is None:
        return out
    c32 = R._f(coef).reshape(-1, 1)
    out['gm'] = np.where(live[:, None], c32 * gm, f(0)).astype(f)
    if gd is not None:
        out['gd'] = np.where(live[:, None], c32 * gd, f(0)).astype(f)
    add = gt if fault == 'no_coef' else (c32 * gt).astype(f)
    wsb = np.zeros((row_blocks, X), f)
    for b, (r0, r1) in enumerate(blk):
        acc = np.zeros(X, f)
        for r in range(r0, r1):
            if live[r]:
                acc = (acc + add[r]).astype(f)
        wsb[b] = acc
    if fault == 'no_clear':
        for c in range(1, chunks):
            w = min(CHUNK, X - c * CHUNK)
            wsb[:, c * CHUNK:c * CHUNK + w] += wsb[:, (c - 1) * CHUNK:(c - 1) * CHUNK + w]
    ws = np.zeros(X, f)
    for b in range(row_blocks):
        ws = (ws + wsb[b]).astype(f)
    out.update(ws_blocks=wsb, ws=ws)
    return out


def excess(emu, ref, coef=None):
    """|emulation or launch - reference| / bound per output: dict of worst fractions (<= 1 passes)"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    e = dict(parts=ref64.excess(t(emu['parts']), ref['parts'], ref['parts_bound']))
    if coef is not None:
        e['gm'] = ref64.excess(t(emu['gm']), ref['gm'], ref['gm_bound'])
        if 'gd' in ref:
            e['gd'] = ref64.excess(t(emu['gd']), ref['gd'], ref['gd_bound'])
        e['ws'] = ref64.excess(t(emu['ws']), ref['ws'], ref['ws_bound'])
    return {k: float(v.max()) for k, v in e.items()}


# ------------------------------------------------------------------------------------------------ CPU stand-in
def gene_rows(out_part, x, mu, theta_raw, *, kind, shift=0.0, logit=None, xidx=None, coef=None, dmu=None, dlogit=None,
              ws=None, library=False, size=None, row_blocks=None):
    """stand-in of ``drvae_amd.gene_rows.gene_rows``: the careful fp32 emulation of the launch, written into the caller's
    buffers the way the launch writes them"""
    assert kind in ('nb', 'zinb') and (logit is not None) == (kind == 'zinb')
    CALLS['gene_rows_lib' if library else 'gene_rows'] += 1
    M, X = mu.shape
    grad = dmu is not None
    if row_blocks is None:
        row_blocks = ws.shape[0] if grad else None
    chunks, rbs = shape(M, X, row_blocks)
    assert tuple(out_part.shape) == (M, chunks) and theta_raw.numel() == X
    assert 1 <= rbs <= max(M, 1) and (not grad or (ws.shape[0] == rbs and ws.shape[1] >= X and coef is not None))
    assert grad or (ws is None and dlogit is None)
    assert (dlogit is not None) == (grad and kind == 'zinb')
    assert not (library and chunks > 1 and size is None)
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    if MODE['exact']:
        e = _exact(kind, x, mu, theta_raw, logit, coef if grad else None, shift, library, xidx, rbs)
    else:
        e = emulate(kind, n(x), n(mu), n(theta_raw), n(logit), n(coef) if grad else None, shift=shift, library=library,
                    xidx=n(xidx), row_blocks=rbs)
    put = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.device))
    put(out_part, e['parts'])
    if library and size is not None:
        put(size[:M], e['size'])
    if grad:
        put(dmu, e['gm'])
        if kind == 'zinb':
            put(dlogit, e['gd'])
        put(ws[:, :X], e['ws_blocks'])


def _exact(kind, x, mu, raw, logit, coef, shift, library, xidx, rbs):
    """the same outputs stated the way ``tests/kernel_ref.py`` states its rows: float64 on the fp32 values handed in, rounded
    once (``reference``) -- for the model-level tests, whose tolerances are those of a step on such stand-ins"""
    xs = x[xidx.long()] if xidx is not None else x
    r = reference(kind, xs.cpu(), mu.cpu(), raw.cpu(), None if logit is None else logit.cpu(), coef=None if coef is None else coef.cpu(),
                  shift=shift, library=library)
    f = lambda t: t.to(torch.float32).numpy()
    out = dict(parts=f(r['parts']), size=CR.size_factor32(xs) if library else None)
    if coef is not None:
        out.update(gm=f(r['gm']), gd=f(r['gd']) if kind == 'zinb' else None,
                   ws_blocks=np.stack([f(r['gt'][r0:r1].sum(0)) for r0, r1 in blocks(mu.shape[0], rbs)]))
    return out


FUNCTIONS = ('gene_rows', 'row_blocks_for', 'shape')
MODE = {'exact': False}


def install(monkeypatch, exact=False):
    """``kernel_ref.install`` plus the stand-in of the launch over ``drvae_amd.gene_rows`` for one CPU test: the careful fp32
    emulation, or with ``exact`` float64 rounded once"""
    import drvae_amd.gene_rows as G
    from tests import kernel_ref
    kernel_ref.install(monkeypatch)
    monkeypatch.setattr(G, 'gene_rows', gene_rows)
    monkeypatch.setitem(MODE, 'exact', bool(exact))
    for k in CALLS:
        CALLS[k] = 0


# ------------------------------------------------------------------------------- model-level float64 reference
class ModelRef:
    """the float64 model-level reference of a ``dispersion='gene'`` model: ``zinb_ref.ModelRef`` ('zinb') or
    ``counts_ref.RidersRef`` ('nb') -- switches and riders as theirs -- without the theta head's parameters and with the vector
    ``RAW`` (started at small random values, so that its gradient, its weight decay and its softplus all show): the decoder
    returns theta = softplus(RAW) + 1e-3 broadcast over its rows.  One more run-time substitution inside their contexts"""

    def __new__(cls, family, spec, seed=9, norm=False, **kw):
        """``norm`` ('nb' only): the encoder reads the depth-normalised rows (``depth_ref.ModelRef``, x_transform='log1p_norm')"""
        from tests import depth_ref as DR
        assert not (norm and family == 'zinb')
        base = Z.ModelRef if family == 'zinb' else DR.ModelRef if norm else CR.RidersRef

        class _Ref(base):
            def __init__(self):
                from oracle import models_ref as M
                super().__init__(spec, seed, **kw)
                rs = np.random.RandomState(seed + 177)
                init = type(self.init32)((k, v) for k, v in self.init32.items() if not k.startswith(SG_HEAD + '.'))
                init[RAW] = (0.5 * rs.standard_normal(spec.dim_x)).astype(np.float32)
                self.init32 = init
                params = type(init)((k, torch.tensor(v.astype(np.float64), requires_grad=True)) for k, v in init.items())
                self.tr = M.RefTrainer(spec, params)
                self.avg = {k: v.detach().clone() for k, v in self.tr.params.items()}

            @contextlib.contextmanager
            def context(self):
                from oracle import blocks_ref as B
                with super().context():
                    inner = B.diag_gaussian_sigma

                    def heads(inputs, p, prefix, n_hidden, nonlin, constrain_means=False):
                        h = B.mlp(inputs, p, prefix + '.nnet', n_hidden, nonlin)
                        mu = F.softplus(B.linear(h, p, prefix + '.encoder_mu.linear_mu')) + R.MU_SHIFT
                        theta = (F.softplus(p[RAW]) + ref64.f32(R.THETA_SHIFT))[None, :].expand_as(mu)
                        return (mu, theta, B.linear(h, p, Z.LOGIT_HEAD)) if family == 'zinb' else (mu, theta)
                    B.diag_gaussian_sigma = heads
                    try:
                        yield
                    finally:
                        B.diag_gaussian_sigma = inner
        return _Ref()


# --------------------------------------------------------------------------------- counts with a per-gene theta
def gene_theta(X, seed=0):
    """the generator's true inverse dispersions: log-uniform over 0.3 .. 30, one per gene"""
    return np.exp(np.random.RandomState(seed + 31).uniform(np.log(0.3), np.log(30.0), X))


def gp_counts(n, X=13, seed=0, depth=6.0, zero_inflated=False):
    """(x, y, theta): Gamma-Poisson counts with ``gene_theta`` around gene means depth * (1 .. 4) (a class shifts every third
    gene); ``zero_inflated``: each entry then zeroed with its gene's structural-zero probability, 0.1 .. 0.6"""
    rs = np.random.RandomState(seed)
    th = gene_theta(X, seed=1)          # (one set of genes: train and held-out sets share their dispersions)
    y = rs.randint(0, 2, n)
    mean = depth * (1.0 + (np.arange(X) % 4))[None, :] * np.where((np.arange(X) % 3 == 0)[None, :], 1.0 + 0.8 * y[:, None], 1.0)
    x = rs.poisson(rs.gamma(th[None, :], mean / th[None, :]))
    if zero_inflated:
        x = np.where(rs.rand(n, X) < np.linspace(0.1, 0.6, X)[None, :], 0, x)
    return x.astype(np.float32), y.astype(np.int64), th


def gp_dataset(kind, n, seed, dev='cpu', **kw):
    """a dataset of ``gp_counts`` for model ``kind`` (the layout of ``zinb_ref.zi_dataset``)"""
    from drvae_amd import data as D
    x1, y, _ = gp_counts(n, seed=seed, **kw)
    x2, _, _ = gp_counts(n, seed=seed + 500, **dict(kw, depth=1.3 * kw.get('depth', 6.0)))
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(np.zeros(n, np.int64)), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2 * hx[:, None].astype(np.float32)), t(np.zeros(n, np.int64)), t(y), t(hx), t(hy))
