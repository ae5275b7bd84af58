"""Float64 reference of the count kinds of ``dv_recon_rows`` (``kernels.recon_rows(kind='binary' | 'poisson' | 'nb',
size_from=..., rec_out=...)``: the whole-set evaluation of the count decoders), the bounds its outputs are held to, an fp32
emulation -- a careful one and five faulty ones the bounds catch -- and a float64 evaluation of the reported metrics (the
launcher's CPU stand-in: ``tests/kernel_ref.py``).  Test-only.

What the launch forms, per target row x[i,:], from the POST-activation heads v (and theta for 'nb'):

    r       = v                      without a size source
    r       = fl(s v),  s = max(sum_g xs[i,g], 1) / X      with one (xs: the target itself or another matrix; theta as it is)
    rows    = [ sum (x-r)^2, mean x, mean r, sum (x-mx)^2, sum (r-mr)^2, sum (x-mx)(r-mr) ]     (the centred sums: a second walk)
    ll      = sum_g log p(x_g | r_g [, theta_g])
    rec_out = r

The log-likelihood rows are ``dv_rec_nll_rows``' terms (the same device functions), so their bounds are reused as they
stand: ``nb_ref.reference`` ('nb'), ``counts_ref.reference`` (the scaled kinds: nb_ref's plus the one rounding of m = s v),
C = 16 for the Poisson and C = 8 for the Bernoulli row (``tests/test_gpu_numerics.py``).  ``rec_out`` is one product: C = 1.

The six statistics, by ``tests/ref64.py``'s rule |got - ref| <= C U sum |components| (U = 2^-24; a row sum of X terms adds
``row_sum_bound``), counting roundings to first order.  With d = x - r, p = x - mx, q = r - mr and dr = U |r| the rounding
of the scaled mean (0 without a size source):

* sum d^2:  the difference (1) enters the square twice, the square (1): 3 U d^2, and the mean's rounding moves d^2 by
  2 |d| dr.  C = 3 on the components d^2 + |d| |r|  (3 >= 2: the second component's factor).
* mean x:   the targets are integer counts (0 / 1 for 'binary') with a row total below 2^24 -- asserted here, the contract
  of these kinds -- so every partial sum is an integer below 2^24, exact in fp32 in any order (the argument of
  ``counts_ref.size_factor32``): the quotient alone rounds, C = 1 on |mx|.  mean r: the sum (``row_sum_bound`` on |r|),
  the quotient (1) and dr per element, over X.
* the centred sums carry the MEANS' errors, 2 |p| |d mx| per element and its likes -- counted here for what they amount to,
  by algebra rather than term by term.  The kernel centres at mx' = mx + a and mr' = mr + e_bar + b (a, b: what summation and
  quotient lose, |a| <= d mx, |b| <= d mr; e_i = fl(s v_i) - s v_i, |e_i| <= dr_i, e_bar its mean), ONE number per row each.
  The exact deviations obey sum p = sum q = 0 identically, so with p' = p - a and q' = q + e - e_bar - b:
      sum p'^2  = sum p^2 + X a^2
      sum q'^2  = sum q^2 + 2 sum q e + sum (e - e_bar - b)^2
      sum p' q' = sum p q + sum p e + X a b
  -- the means' errors enter through their PRODUCTS only (the term-by-term count 2 |p| |d mx| is sum-free: it held the careful
  emulation at 0.001 of the bound and let a raw-moment covariance pass at 3 x).  What is left to first order is the rounding of
  the scaled mean element by element, which no identity cancels: 2 |q| dr and |p| dr.
* sum p^2:  3 U p^2 as above (difference, square) + X (d mx)^2.
* sum q^2:  3 U q^2 + 2 |q| dr + X (max dr + d mr)^2.
* sum p q:  each factor's difference (1 + 1) and the product (1): 3 U |p q|, plus |p| dr + X d mx d mr.

Every C is at most 3; none comes from what the kernel returns.  A kernel that takes the centred sums from raw moments
(sum x^2 - X mx^2) loses what cancels -- counts ~ 3e3 with a spread of ~ 55: sum x^2 ~ 9e6 X against sum p^2 ~ 3e3 X -- and
lands far outside in all three of them (``emulate(fault='raw_moments')``)."""
import numpy as np
import torch

from tests import counts_ref as CR
from tests import nb_ref as R
from tests.ref64 import U, bound, f64, row_sum_bound

KINDS = ('binary', 'poisson', 'nb')
C_BERN, C_POIS = 8, CR.C_POIS
C_STAT = 3
P_MIN = 1e-10
COMBOS = (('binary', False), ('poisson', False), ('poisson', True), ('nb', False), ('nb', True))      # (kind, scaled)
FAULTS = ('raw_moments', 'size_target', 'stats_unscaled', 'll_unscaled', 'theta_scaled')


# ------------------------------------------------------------------------------------------- float64 reference
def reference(kind, x, mu, theta=None, size_from=None):
    """everything the tests compare with, from the exact fp32 values the kernel received: ``rows`` (M, 6), ``ll`` (M),
    ``rec`` (M, X) and their bounds (``*_bound``)"""
    assert kind in KINDS and (theta is not None) == (kind == 'nb') and not (kind == 'binary' and size_from is not None)
    M, X = x.shape
    xx, V = f64(x), f64(mu)
    lib = size_from is not None
    s32 = CR.size_factor32(size_from) if lib else None
    r = f64(s32)[:, None] * V if lib else V
    dr = U * r.abs() if lib else torch.zeros_like(r)
    out = dict(rec=r, rec_bound=dr, s=s32)
    # ---- the log-likelihood rows: the bounds of the row kernels, as they stand
    if kind == 'nb':
        ref = CR.reference('nb', x, mu, theta, s=s32) if lib else R.reference(x, mu, theta)
        out['ll'], out['ll_bound'] = ref['rows'], ref['rows_bound']
    elif kind == 'poisson' and lib:
        ref = CR.reference('poisson', x, mu, s=s32)
        out['ll'], out['ll_bound'] = ref['rows'], ref['rows_bound']
    elif kind == 'poisson':
        lgam, xl = torch.lgamma(xx + 1), xx * torch.log(V)
        comps = xl.abs() + V + lgam
        out['ll'], out['ll_bound'] = (xl - V - lgam).sum(1), bound(C_POIS, comps).sum(1) + row_sum_bound(comps, X)
    else:
        pc = V.clamp(P_MIN, 1.0)
        comps = xx.abs() * (torch.log(pc).abs() + 1) + (1 - xx).abs() * (torch.log1p(-pc).abs() + 1)
        out['ll'] = (xx * torch.log(pc) + (1 - xx) * torch.log1p(-pc)).sum(1)
        out['ll_bound'] = bound(C_BERN, comps).sum(1) + row_sum_bound(comps, X)
    # ---- the six statistics
    d = xx - r
    mx, mr = xx.sum(1) / X, r.sum(1) / X
    p, q = xx - mx[:, None], r - mr[:, None]
    rows = torch.stack([(d * d).sum(1), mx, mr, (p * p).sum(1), (q * q).sum(1), (p * q).sum(1)], 1)
    ax, ar = xx.abs(), r.abs()
    tot = ax.sum(1)
    assert bool((xx == xx.floor()).all()) and bool((xx >= 0).all()) and float(tot.max()) < 2 ** 24, 'integer counts, totals < 2^24'
    dmx = bound(1, tot) / X
    dmr = (row_sum_bound(ar, X) + bound(1, ar.sum(1)) + dr.sum(1)) / X
    c_d = d * d + d.abs() * ar * (1.0 if lib else 0.0)
    b_sse = bound(C_STAT, c_d).sum(1) + row_sum_bound(d * d, X)
    b_xx = bound(C_STAT, p * p).sum(1) + row_sum_bound(p * p, X) + X * dmx ** 2
    b_rr = bound(C_STAT, q * q).sum(1) + row_sum_bound(q * q, X) + 2 * (q.abs() * dr).sum(1) + X * (dr.max(1)[0] + dmr) ** 2
    pq = (p * q).abs()
    b_xr = bound(C_STAT, pq).sum(1) + row_sum_bound(pq, X) + (p.abs() * dr).sum(1) + X * dmx * dmr
    out['rows'], out['rows_bound'] = rows, torch.stack([b_sse, dmx, dmr, b_xx, b_rr, b_xr], 1)
    return out


# ---------------------------------------------------------------------------------------------- fp32 emulation
def _sum32(a):
    """a row sum in fp32 the way the kernel takes it: 256 strided per-thread partials in index order, then a tree"""
    a = np.asarray(a, np.float32)
    M, X = a.shape
    pad = np.zeros((M, -(-X // 256) * 256), np.float32)
    pad[:, :X] = a
    part = np.zeros((M, 256), np.float32)
    for k in range(pad.shape[1] // 256):
        part = (part + pad[:, k * 256:(k + 1) * 256]).astype(np.float32)
    n = 256
    while n > 1:
        n //= 2
        part = (part[:, :n] + part[:, n:2 * n]).astype(np.float32)
    return part[:, 0]


def emulate(kind, x, mu, theta=None, size_from=None, fault=None):
    """the launch in numpy float32, operation by operation -> dict(rows, ll, rec).  ``fault`` None: the kernel's
    construction.  FAULTY on purpose (``FAULTS``): 'raw_moments' (the centred sums as sum a b - X ma mb), 'size_target'
    (the size factor of the TARGET row whatever the source), 'stats_unscaled' / 'll_unscaled' (statistics / log-likelihood
    at the head v instead of s v), 'theta_scaled' (theta multiplied by s too)"""
    import scipy.special as sp
    f = np.float32
    assert fault is None or fault in FAULTS
    x, v = R._f(x.numpy() if torch.is_tensor(x) else x), R._f(mu.numpy() if torch.is_tensor(mu) else mu)
    t = R._f(theta.numpy() if torch.is_tensor(theta) else theta) if theta is not None else None
    M, X = x.shape
    lib = size_from is not None
    with np.errstate(all='ignore'):
        if lib:
            s = CR.size_factor32(x if fault == 'size_target' else size_from).reshape(-1, 1)
            r = (s * v).astype(f)
        else:
            s, r = None, v
        rs = v if fault == 'stats_unscaled' else r          # what the statistics see
        rl = v if fault == 'll_unscaled' else r             # what the log-likelihood sees
        if kind == 'nb':
            tl = (t * s).astype(f) if (fault == 'theta_scaled' and lib) else t
            ll = R.emulate_fp32(x, rl, tl)[0]
        elif kind == 'poisson':
            ll = (x * np.log(rl) - rl - R._f(sp.gammaln(x + f(1)))).astype(f)
        else:
            pc = np.minimum(np.maximum(rl, f(P_MIN)), f(1.0 - 1e-10))
            ll = (x * np.log(pc) + (f(1) - x) * np.log(f(1) - pc)).astype(f)
        d = (x - rs).astype(f)
        sse = _sum32(d * d)
        mx, mr = (_sum32(x) / f(X)).astype(f), (_sum32(rs) / f(X)).astype(f)
        if fault == 'raw_moments':
            cxx = (_sum32(x * x) - f(X) * mx * mx).astype(f)
            crr = (_sum32(rs * rs) - f(X) * mr * mr).astype(f)
            cxr = (_sum32(x * rs) - f(X) * mx * mr).astype(f)
        else:
            p, q = (x - mx[:, None]).astype(f), (rs - mr[:, None]).astype(f)
            cxx, crr, cxr = _sum32(p * p), _sum32(q * q), _sum32(p * q)
    return dict(rows=np.stack([sse, mx, mr, cxx, crr, cxr], 1), ll=_sum32(ll), rec=rs)


# ------------------------------------------------------------------------------------------------- test data
def case(kind, M, X, seed=0, scaled=False, other=False, counts='mixed'):
    """fp32 host tensors (x, mu, theta | None, size_from | None) of one kernel case: integer counts with row totals below
    2^24 (row 0 all zero: the max(., 1) clamp; ``counts='thousands'``: ~ 3e3 with a Poisson-like spread of ~ 55; 'mixed': mostly small
    with a few up to 30 000), heads on the ranges of the models ('binary': probabilities and 0 / 1 targets).  ``other``:
    the size source is another matrix, ~ 10 x as deep as the target"""
    rs = np.random.RandomState(1000 * seed + 7 * M + X)
    if kind == 'binary':
        x = (rs.uniform(size=(M, X)) < 0.3).astype(np.float32)
        mu = rs.uniform(1e-4, 1 - 1e-4, (M, X)).astype(np.float32)
    else:
        if counts == 'thousands':
            x = np.floor(rs.normal(3000.0, 55.0, (M, X)).clip(0)).astype(np.float32)
        else:
            x = np.floor(rs.gamma(0.6, 8.0, (M, X))).astype(np.float32)
            hot = rs.uniform(size=(M, X)) < min(0.02, 4.0 / X)
            x[hot] = np.floor(rs.uniform(1000, 30000, int(hot.sum()))).astype(np.float32)
            x.reshape(-1)[-1] = 30000.0
        mu = np.exp(rs.uniform(np.log(1e-6), np.log(1e4), (M, X))).astype(np.float32)
        if counts == 'thousands':
            mu = (rs.normal(1.0, 0.03, (M, X)).clip(0.5) * (3000.0 if not scaled else 1.0)).astype(np.float32)
    x[0] = 0.0
    theta = np.exp(rs.uniform(np.log(1e-3), np.log(1e6), (M, X))).astype(np.float32) if kind == 'nb' else None
    size = None
    if scaled:
        size = x
        if other:
            size = np.floor(x * 10.0 + rs.poisson(3.0, (M, X))).astype(np.float32)
            size[0] = 0.0
            if M > 1:
                size[1] = x[1]
        assert float(np.asarray(size, np.float64).sum(1).max()) < 2 ** 24
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return t(x), t(mu), t(theta), t(size)


# -------------------------------------------------------------------------- the reported metrics, in float64
def metrics64(x, r, ll_rows=None):
    """``eval_x_reconstruction`` in float64 on the given rows: dict(rmse, r2, pearr, ll) -- the formulas of
    ``dv_recon_finalize`` (sklearn's variance-weighted R^2, the mean per-row Pearson r)"""
    x, r = f64(x), f64(r)
    n, X = x.shape
    out = dict(rmse=float(torch.sqrt(((x - r) ** 2).sum() / (n * X))))
    ss_tot = ((x - x.mean(0)) ** 2).sum(0)
    out['r2'] = float(1.0 - ((x - r) ** 2).sum() / ss_tot.sum())
    p, q = x - x.mean(1, keepdim=True), r - r.mean(1, keepdim=True)
    out['pearr'] = float(((p * q).sum(1) / torch.sqrt((p * p).sum(1) * (q * q).sum(1))).mean())
    out['ll'] = float(f64(ll_rows).mean()) if ll_rows is not None else float('nan')
    return out


def metrics_bound(x, r, rows_bound, ll_bound=None):
    """the kernel-level bounds of the rows (``reference``) propagated to the four metrics, to first order:
    rmse = sqrt(S / nX): dS / (2 sqrt(S nX));  r2 = 1 - S / T (S by float64 column sums of fp32 values: only the stored
    mean's rounding, 2 |d| U |r|, enters);  pearr = mean c / sqrt(a b): |dc| / sqrt(ab) + |c| (da / a + db / b) / (2 sqrt(ab));
    ll: the mean of the rows' bounds"""
    x, r, rb = f64(x), f64(r), f64(rows_bound)
    n, X = x.shape
    S = ((x - r) ** 2).sum()
    out = dict(rmse=float(rb[:, 0].sum() / (2 * torch.sqrt(S * n * X))))
    ss_tot = ((x - x.mean(0)) ** 2).sum()
    out['r2'] = float((2 * (x - r).abs() * U * r.abs()).sum() / ss_tot)
    p, q = x - x.mean(1, keepdim=True), r - r.mean(1, keepdim=True)
    a, b, c = (p * p).sum(1), (q * q).sum(1), (p * q).sum(1)
    ok = (a > 0) & (b > 0)
    den = torch.sqrt(a * b)
    t = rb[:, 5] / den + c.abs() * (rb[:, 3] / a + rb[:, 4] / b) / (2 * den)
    out['pearr'] = float(torch.where(ok, t, torch.zeros_like(t)).mean())
    out['ll'] = float(f64(ll_bound).mean()) if ll_bound is not None else 0.0
    return out
