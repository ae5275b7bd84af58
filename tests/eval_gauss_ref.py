"""Float64 references of the Gaussian half of the whole-set evaluation tail -- ``dv_recon_row_stats``, ``dv_recon_rows``
(kind 0: finished and raw heads), ``dv_col_moments``, ``dv_recon_finalize``, ``dv_rank_metrics`` -- the bounds their
outputs are held to, the input profiles the CPU and GPU tests share, an emulation of each launch in its own arithmetic
(a careful one and faulty ones the bounds catch) and the exact rank metrics.  Test-only.

Every reference is evaluated on the exact fp32 values the launch receives; every bound counts roundings under
``tests/ref64.py``'s rule |got - ref| <= C U sum |components| (U = 2^-24), to first order; no constant comes from what a
kernel returns.

THE SUMMATION RULE of the row launches.  ``recon_row_stats_kernel`` and ``recon_rows_kernel`` give a WAVE to a row: lane l
adds the terms of its columns one after the other -- ceil(X / 64) of them on the dword path, 2 ceil(X / 128) <= ceil(X / 64) + 1
on the pair path (at most 16 in ``dv_recon_rows``, any number in ``dv_recon_row_stats``) -- the first onto an exact zero,
and a butterfly of 6 levels adds the 64 lanes.  A term therefore passes through at most ceil(X / 64) + 6 rounded additions,
each relative to a partial sum of magnitude <= sum |terms|:

    wave_sum_bound = (ceil(X / 64) + 6) U sum |terms|

``ref64.row_sum_bound`` ((ceil(X / 256) + 16) U sum |terms|) describes the launches that give a row 256 threads; at X = 4100
it allows 33 U where a lane of ``recon_row_stats_kernel`` alone makes 65 additions, so it is not used here.

THE SIX ROW STATISTICS, general x (the algebra of ``tests/eval_counts_ref.py``, which see).  With d = x - r, p = x - mx,
q = r - mr: each term is a difference (1 rounding, entering the product twice) and a product (1): C = 3 on d^2, p^2, q^2,
|p q|, plus ``wave_sum_bound`` of those terms.  The means: d mx = (wave_sum_bound(|x|) + U sum |x|) / X -- the summation and
the quotient's rounding; x is no integer count here, so the sum is not exact -- and d mr likewise.  The means' errors enter
the centred sums through their PRODUCTS only (sum p = sum q = 0 identically): + X dmx^2, + X dmr^2, + X dmx dmr.  With raw
heads r = fl32(mu + bias_mu) is formed HERE, exactly rounded, before anything else: it is the kernel's first operation and
IEEE addition leaves no choice, so r carries no error of its own.

THE LOG-LIKELIHOOD ROWS are the terms ``tests/test_gpu_numerics.py`` holds ``dv_gauss_nll_rows_fwd`` to:
``ref64.nll_sigma_finished`` (finished heads) / ``ref64.nll_sigma_pre`` (raw heads, pre = fl32(sd + bias_sd) formed here) with
C_NLL = 16 and the hardware-exp extra, under the summation rule above:  0.5 (sum bound(C_NLL, term_c, term_x) + wave_sum_bound).

``dv_col_moments`` accumulates fp32 values in float64: squares of fp32 values are exact, a difference of two and its square
round at 2^-53, and otherwise only the ORDER of at most M additions differs from the reference: M 2^-53 sum |terms| per
output.  ``COL_MARGIN`` = 100 multiplies it -- the two orders ``tests/test_gpu_reg_metrics.py`` allows for the same argument, so
that neither the reduction tree nor the reference's own float64 sum matters; an fp32 accumulation (2^-24) stays 10^4 outside
at M = 8193.  With ``r_bias`` the reference first rounds r + r_bias to fp32, as the kernel does.

``dv_recon_finalize`` is taken from GIVEN rows / part / ll (exact inputs), in extended precision (numpy longdouble), so the
reference's own error is nil.  One workgroup of 1024 threads: a thread adds ceil(n / 1024) row terms (ceil(X / 1024) column
terms), a 6-level butterfly and 16 wave sums follow: k_n = ceil(n / 1024) + 22 additions, k_X = ceil(X / 1024) + 22.  A
float64 division or square root is counted as 2 roundings (1 if correctly rounded; the count does not rely on it).  u = 2^-53:
  rmse   = sqrt(S / (n X)):  the sum's k_n u halves under the root, quotient 2, root 2:  (k_n / 2 + 4) u rmse
  pearr  = mean t_i, t_i = c / sqrt(a b): product 1, root 2, quotient 2:  ((5 + k_n) sum |t_i| / n + 2 |pearr|) u
  ll     = mean ll_i (conversions exact):  (k_n sum |ll_i| / n + 2 |ll|) u
  R^2    = 1 - num / den, num = sum_g c2, den = sum_g (c1 - c0^2 / n), c. = sum over B row blocks in order (B u each,
           relative to sum_b |c._b|).  Per column with m_g = c1 + (sum_b |c0_b|)^2 / n: c1 B, c0^2 / n 2 B + 3 (square,
           quotient), the difference 1: (2 B + 4) u m_g; the sum over columns k_X u sum m_g.  num: (B + k_X) u num.  So
           |d R^2| <= u { |R^2| + (num / |den|) [ (B + k_X + 2) + (2 B + 4 + k_X) sum_g m_g / |den| ] }
           -- the conditioning sum m_g / den is computed per case, never fixed.

THE RANK METRICS are exact: ROC-AUC = (2 #pos_above + #pos_tied) summed over the negatives / (2 n_pos n_neg) as ONE division
of Python integers (correctly rounded: the kernel's value, an exact integer times 0.5 over an exact product, is the same
rational and must be bit-equal); AP = 1 / n_pos sum over positives of #pos(>= s_i) / #rows(>= s_i), the header's definition,
summed with ``math.fsum``.  Scores compare as IEEE fp32 values: -0.0 ties with +0.0, subnormals are distinct.

THE ``pred = NULL`` CONTRACT: without a prediction the accuracy slot is NaN ("none given" is not "0 % correct"), as it is
for n = 0."""
import math

import numpy as np
import torch

from tests import ref64
from tests.ref64 import U, bound, f64

C_STAT = 3
C_NLL = 16            # tests/test_gpu_numerics.py's, as it stands
SHIFT = 1e-3
U64 = 2.0 ** -53
COL_MARGIN = 100.0
PROFILES = ('normal', 'expression', 'offset', 'zero_rows', 'const_rows')
ROW_FAULTS = ('raw_moments', 'mean_over_ld', 'drop_last_odd', 'pair_bias')
COL_FAULTS = ('sel_ignored', 'fp32')
FIN_FAULTS = ('fp32', 'll_position')
ACC_WITHOUT_PRED = float('nan')          # the settled contract of dv_rank_metrics' out[2 n_cls] for pred = NULL
RANK_MAX_ROWS = 32768
f = np.float32


def wave_sum_bound(comps, X):
    """the summation rule of the module header for row sums (rows along dim 1)"""
    return (math.ceil(X / 64) + 6) * U * f64(comps).sum(1)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---------------------------------------------------------------------------------------------- input profiles
def profile(name, M, X, seed=0):
    """fp32 host arrays of one row-launch case: dict(x, r, sd, pre, bm, bs, mu_raw, sd_raw).  Finished heads: (x, r, sd),
    sd = fl32(softplus(pre) + SHIFT); raw heads: (x, mu_raw, sd_raw, bm, bs) with fl32(mu_raw + bm) ~ r, fl32(sd_raw + bs) ~ pre.
    'zero_rows': row 0 of x exactly zero, row 1 (M > 1) of r exactly zero -- and of fl32(mu_raw + bm): mu_raw = -bm there;
    'const_rows': row 0 of x constant 2.5, row 1 of r constant -0.75 (the raw heads: to within the rounding of the sum)"""
    assert name in PROFILES
    rs = np.random.RandomState(100003 * PROFILES.index(name) + 1009 * seed + 7 * M + X)
    if name in ('normal', 'zero_rows', 'const_rows'):
        x = rs.standard_normal((M, X))
        r = rs.standard_normal((M, X))
    elif name == 'expression':
        depth = rs.uniform(1.0, 3.0, (M, 1))                  # row means of log1p(counts) between ~1 and ~3
        x = np.log1p(rs.poisson(np.expm1(depth) * rs.gamma(4.0, 0.25, (M, X))))
        r = x + 0.05 * rs.standard_normal((M, X))
    else:
        x = 1000.0 + rs.standard_normal((M, X))
        r = x.astype(f).astype(np.float64) + 0.1 * rs.standard_normal((M, X))
    x, r = x.astype(f), r.astype(f)
    if name == 'zero_rows':
        x[0] = 0.0
        if M > 1:
            r[1] = 0.0
    if name == 'const_rows':
        x[0] = 2.5
        if M > 1:
            r[1] = -0.75
    pre = rs.uniform(-3.0, 2.0, (M, X)).astype(f)
    sd = (np.log1p(np.exp(pre.astype(np.float64))) + SHIFT).astype(f)
    bm, bs = rs.standard_normal(X).astype(f), (0.3 * rs.standard_normal(X)).astype(f)
    mu_raw, sd_raw = (r - bm).astype(f), (pre - bs).astype(f)
    if name == 'zero_rows' and M > 1:
        mu_raw[1] = -bm
    return dict(x=x, r=r, sd=sd, pre=pre, bm=bm, bs=bs, mu_raw=mu_raw, sd_raw=sd_raw)


def finished(c, raw):
    """(r, sd | None, pre | None) as the launch sees them: raw heads are finished in fp32, exactly rounded sums"""
    if raw:
        return (c['mu_raw'] + c['bm']).astype(f), None, (c['sd_raw'] + c['bs']).astype(f)
    return c['r'], c['sd'], None


# ------------------------------------------------------------------------------------------- float64 references
def rows_reference(x, r):
    """the six statistics between fp32 x and the FINISHED fp32 r, float64, and their bounds: (rows, bound), each (M, 6)"""
    xx, rr = f64(x), f64(r)
    M, X = xx.shape
    d = xx - rr
    mx, mr = xx.sum(1) / X, rr.sum(1) / X
    p, q = xx - mx[:, None], rr - mr[:, None]
    rows = torch.stack([(d * d).sum(1), mx, mr, (p * p).sum(1), (q * q).sum(1), (p * q).sum(1)], 1)
    ax, ar = xx.abs(), rr.abs()
    dmx = (wave_sum_bound(ax, X) + bound(1, ax.sum(1))) / X
    dmr = (wave_sum_bound(ar, X) + bound(1, ar.sum(1))) / X
    pq = (p * q).abs()
    b_sse = bound(C_STAT, d * d).sum(1) + wave_sum_bound(d * d, X)
    b_xx = bound(C_STAT, p * p).sum(1) + wave_sum_bound(p * p, X) + X * dmx ** 2
    b_rr = bound(C_STAT, q * q).sum(1) + wave_sum_bound(q * q, X) + X * dmr ** 2
    b_xr = bound(C_STAT, pq).sum(1) + wave_sum_bound(pq, X) + X * dmx * dmr
    return rows, torch.stack([b_sse, dmx, dmr, b_xx, b_rr, b_xr], 1)


def ll_reference(x, r, sd=None, pre=None, shift=SHIFT):
    """the Gaussian log-likelihood rows -0.5 sum term: finished heads (``sd``) or raw (``pre`` = fl32(sd_raw + bias_sd)) -> (ll, bound)"""
    X = x.shape[1]
    if pre is None:
        t = ref64.nll_sigma_finished(x, r, sd, shift, 'softplus')
        own = bound(C_NLL, t['term_c'])
    else:
        t = ref64.nll_sigma_pre(x, r, pre, ref64.f32(shift))
        own = bound(C_NLL, t['term_c'], t['term_x'])
    return -0.5 * t['term'].sum(1), 0.5 * (own.sum(1) + wave_sum_bound(t['term_c'], X))


def col_reference(x, r, sel=None, r_bias=None):
    """sum x, sum x^2, sum (x - r)^2 per column over the selected rows in float64 -> (cols (3, X), bound (3, X))"""
    x, r = _np(x).astype(f), _np(r).astype(f)
    if r_bias is not None:
        r = (r + _np(r_bias).astype(f)[None, :]).astype(f)
    if sel is not None:
        idx = _np(sel).astype(np.int64)
        x, r = x[idx], r[idx]
    a, b = x.astype(np.float64), r.astype(np.float64)
    M = a.shape[0]
    e = (a - b) ** 2
    cols = np.stack([a.sum(0), (a * a).sum(0), e.sum(0)], 0)
    mags = np.stack([np.abs(a).sum(0), (a * a).sum(0), e.sum(0)], 0)
    return cols, COL_MARGIN * max(M, 1) * U64 * mags


def finalize_reference(rows, part, ll, sel, n, X):
    """[rmse, R^2, mean Pearson r, mean ll] from the given fp32 rows / ll and float64 part (row_blocks, 3, X), in extended
    precision, and the bounds of the module header -> (out (4,) float64, bound (4,) float64).  Non-finite values carry a zero bound
    (they are compared for identity)"""
    L = np.longdouble
    assert np.finfo(L).eps < 1e-18, 'extended precision expected'
    nan = float('nan')
    rows, part = _np(rows), _np(part)
    B = part.shape[0]
    idx = _np(sel).astype(np.int64)[:n] if sel is not None else np.arange(n)
    out, bnd = np.full(4, nan), np.zeros(4)
    kn, kx = math.ceil(max(n, 1) / 1024) + 22, math.ceil(X / 1024) + 22
    with np.errstate(all='ignore'):
        o = rows[idx].astype(L)
        if n:
            rmse = np.sqrt(o[:, 0].sum() / (L(n) * X))
            out[0], bnd[0] = float(rmse), float((kn / 2 + 4) * U64 * abs(rmse))
            t = o[:, 5] / np.sqrt(o[:, 3] * o[:, 4])
            pe = t.sum() / n
            out[2], bnd[2] = float(pe), float(((5 + kn) * np.abs(t).sum() / n + 2 * abs(pe)) * U64)
            if ll is not None:
                lv = _np(ll)[idx].astype(L)
                m = lv.sum() / n
                out[3], bnd[3] = float(m), float((kn * np.abs(lv).sum() / n + 2 * abs(m)) * U64)
        p = part.astype(L)
        c0, c1, c2 = p[:, 0].sum(0), p[:, 1].sum(0), p[:, 2].sum(0)
        num, den = c2.sum(), (c1 - c0 * c0 / L(n)).sum()
        r2 = 1 - num / den
        out[1] = float(r2)
        mg = (c1 + np.abs(p[:, 0]).sum(0) ** 2 / L(n)).sum()
        bnd[1] = float(U64 * (abs(r2) + num / abs(den) * ((B + kx + 2) + (2 * B + 4 + kx) * mg / abs(den))))
    bnd[~np.isfinite(out)] = 0.0
    bnd[~np.isfinite(bnd)] = 0.0
    return out, bnd


def fin_excess(got, ref, bnd):
    """per output |got - ref| / bound; a non-finite reference wants the identical value (nan = nan, inf by sign): 0 or inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ex = np.zeros(len(ref))
    for k in range(len(ref)):
        if not np.isfinite(ref[k]):
            same = (np.isnan(got[k]) and np.isnan(ref[k])) or got[k] == ref[k]
            ex[k] = 0.0 if same else math.inf
        elif not np.isfinite(got[k]):
            ex[k] = math.inf
        else:
            err = abs(got[k] - ref[k])
            ex[k] = 0.0 if err == 0 else err / max(bnd[k], 1e-300)
    return ex


# ------------------------------------------------------------------------------- emulations of the row launches
def _lane_terms(a, v2):
    """(M, T, 64): the terms of a row in the order lane l of the wave holds them -- dword path: column l + 64 t; pair path
    (``v2``): column 2 (l + 64 (t / 2)) + t % 2; zero beyond X"""
    M, X = a.shape
    if v2:
        assert X % 2 == 0
        K = -(-X // 128)
        pad = np.zeros((M, K * 128), a.dtype)
        pad[:, :X] = a
        return pad.reshape(M, K, 64, 2).transpose(0, 1, 3, 2).reshape(M, 2 * K, 64)
    T = -(-X // 64)
    pad = np.zeros((M, T * 64), a.dtype)
    pad[:, :X] = a
    return pad.reshape(M, T, 64)


def _butterfly(v):
    """the wave's xor butterfly (offsets 32 .. 1) over the last axis of 64 lanes -> lane 0's value"""
    n = 64
    while n > 1:
        n //= 2
        v = (v[..., :n] + v[..., n:2 * n]).astype(v.dtype)
    return v[..., 0]


def _wave_sum(a, v2=False):
    t = _lane_terms(np.asarray(a, f), v2)
    acc = np.zeros((t.shape[0], 64), f)
    for k in range(t.shape[1]):
        acc = (acc + t[:, k]).astype(f)
    return _butterfly(acc)


def _wave_sum_ll(a, X, v2=False):
    """the log-likelihood terms in ``recon_rows_kernel``'s order: four per trip, (t0 + t1) + (t2 + t3), while the lane's four fit"""
    t = _lane_terms(np.asarray(a, f), v2)
    M, T, _ = t.shape
    T4 = -(-T // 4) * 4
    tt = np.zeros((M, T4, 64), f)
    tt[:, :T] = t
    lane = np.arange(64)
    col = (lambda e: 2 * (lane + 64 * (e >> 1)) + (e & 1)) if v2 else (lambda e: lane + 64 * e)
    acc = np.zeros((M, 64), f)
    for k in range(0, T4, 4):
        full = (col(k + 3) < X) & (col(k) < X)
        quad = (acc + ((tt[:, k] + tt[:, k + 1]).astype(f) + (tt[:, k + 2] + tt[:, k + 3]).astype(f)).astype(f)).astype(f)
        seq = acc
        for q in range(4):
            seq = (seq + tt[:, k + q]).astype(f)
        acc = np.where(full[None, :], quad, seq)
    return _butterfly(acc)


def _softplus32(a):
    a = np.asarray(a, f)
    return (np.maximum(a, f(0)) + np.log1p(np.exp(-np.abs(a)).astype(f)).astype(f)).astype(f)


def emulate_rows(x, mu, sd=None, bias=None, shift=SHIFT, v2=False, fault=None, ld=None):
    """``dv_recon_row_stats`` (``sd`` None; any X) / ``dv_recon_rows`` kind 0 in numpy float32, operation by operation, in the
    wave's summation order (``v2``: the pair path) -> dict(rows (M, 6), ll (M) | None).  ``bias`` = (bm, bs): raw heads.
    FAULTY on purpose (``ROW_FAULTS``): 'raw_moments' (centred sums as sum a b - X ma mb), 'mean_over_ld' (the means divided
    by the row stride ``ld``), 'drop_last_odd' (the last column of an odd-width row never read), 'pair_bias' (pair path, raw
    heads: column 2c finished with column 2c + 1's biases)"""
    assert fault is None or fault in ROW_FAULTS
    x, mu = np.asarray(x, f), np.asarray(mu, f)
    M, X = x.shape
    with np.errstate(all='ignore'):
        if bias is not None:
            bm, bs = np.asarray(bias[0], f).copy(), np.asarray(bias[1], f).copy()
            if fault == 'pair_bias':
                assert v2
                bm[0::2], bs[0::2] = bm[1::2].copy(), bs[1::2].copy()
            r = (mu + bm[None, :]).astype(f)
        else:
            r = mu
        ll = None
        if sd is not None:
            if bias is not None:
                s = (_softplus32((np.asarray(sd, f) + bs[None, :]).astype(f)) + f(shift)).astype(f)
                t = ((x - r).astype(f) / s).astype(f)
                term = (f(ref64.LOG_2PI) + (f(2) * np.log(s)).astype(f) + (t * t).astype(f)).astype(f)
            else:
                s = np.asarray(sd, f)
                v, d = (s * s).astype(f), (x - r).astype(f)
                term = (f(ref64.LOG_2PI) + np.log(v).astype(f) + ((d * d).astype(f) / v).astype(f)).astype(f)
        xs, rs_ = x, r
        if fault == 'drop_last_odd' and X % 2:
            xs, rs_ = x.copy(), r.copy()          # (a zero term is what a column never read contributes)
            xs[:, -1] = 0
            rs_[:, -1] = 0
            if sd is not None:
                term = term.copy()
                term[:, -1] = 0
        if sd is not None:
            ll = (f(-0.5) * _wave_sum_ll(term, X, v2)).astype(f)
        d = (xs - rs_).astype(f)
        sse = _wave_sum(d * d, v2)
        div = f(ld if fault == 'mean_over_ld' else X)
        mx, mr = (_wave_sum(xs, v2) / div).astype(f), (_wave_sum(rs_, v2) / div).astype(f)
        if fault == 'raw_moments':
            cxx = (_wave_sum(xs * xs, v2) - f(X) * mx * mx).astype(f)
            crr = (_wave_sum(rs_ * rs_, v2) - f(X) * mr * mr).astype(f)
            cxr = (_wave_sum(xs * rs_, v2) - f(X) * mx * mr).astype(f)
        else:
            p, q = (xs - mx[:, None]).astype(f), (rs_ - mr[:, None]).astype(f)
            if fault == 'drop_last_odd' and X % 2:
                p[:, -1] = 0
                q[:, -1] = 0
            cxx, crr, cxr = _wave_sum(p * p, v2), _wave_sum(q * q, v2), _wave_sum(p * q, v2)
    return dict(rows=np.stack([sse, mx, mr, cxx, crr, cxr], 1), ll=ll)


def emulate_col(x, r, sel=None, r_bias=None, row_blocks=1, fault=None):
    """``dv_col_moments`` -> part (row_blocks, 3, X) float64, in the kernel's order: row block b = rows [b rpb, (b + 1) rpb) of
    the list, 16 row groups walking every 16th row, the groups added in order.  FAULTY (``COL_FAULTS``): 'sel_ignored' (row ii
    of the matrix instead of row sel[ii]), 'fp32' (the accumulators in fp32)"""
    assert fault is None or fault in COL_FAULTS
    x, r = np.asarray(x, f), np.asarray(r, f)
    X = x.shape[1]
    M = len(sel) if sel is not None else x.shape[0]
    idx = np.asarray(sel, np.int64) if (sel is not None and fault != 'sel_ignored') else np.arange(M)
    acc = f if fault == 'fp32' else np.float64
    rpb = max(1, -(-M // row_blocks))
    part = np.zeros((row_blocks, 3, X), np.float64)
    for b in range(row_blocks):
        i0, i1 = b * rpb, min(M, (b + 1) * rpb)
        tot = np.zeros((3, X), acc)
        for rg in range(16):
            rows_ = idx[i0 + rg:i1:16] if i0 + rg < i1 else idx[:0]
            a = x[rows_].astype(acc)
            bb = (r[rows_] + np.asarray(r_bias, f)[None, :]).astype(f).astype(acc) if r_bias is not None else r[rows_].astype(acc)
            e = ((a - bb).astype(acc) * (a - bb).astype(acc)).astype(acc)
            g = [np.add.accumulate(v, 0, dtype=acc)[-1] if len(rows_) else np.zeros(X, acc) for v in (a, (a * a).astype(acc), e)]
            tot = (tot + np.stack(g, 0)).astype(acc)
        part[b] = tot
    return part


def emulate_finalize(rows, part, ll, sel, n, X, fault=None):
    """``dv_recon_finalize`` in its own order (1024 threads striding the rows / the columns, a 6-level butterfly, 16 wave sums in
    order) -> (4,) float64.  FAULTY (``FIN_FAULTS``): 'fp32' (every accumulator in fp32), 'll_position' (ll[e] for ll[sel[e]])"""
    assert fault is None or fault in FIN_FAULTS
    acc = f if fault == 'fp32' else np.float64
    rows, part = np.asarray(rows, f), np.asarray(part, np.float64)
    idx = np.asarray(sel, np.int64)[:n] if sel is not None else np.arange(n)

    def block_sum(v):
        v = np.asarray(v, acc)
        T = max(1, -(-len(v) // 1024))
        pad = np.zeros(T * 1024, acc)
        pad[:len(v)] = v
        th = np.add.accumulate(pad.reshape(T, 1024), 0, dtype=acc)[-1]
        waves = _butterfly(th.reshape(16, 64))
        return np.add.accumulate(waves, dtype=acc)[-1]
    nan = float('nan')
    with np.errstate(all='ignore'):
        o = rows[idx].astype(np.float64)
        t = [block_sum(o[:, 0]), block_sum(o[:, 5] / np.sqrt(o[:, 3] * o[:, 4]))]
        if ll is not None:
            lv = np.asarray(ll, f)
            t.append(block_sum(lv[np.arange(n)] if fault == 'll_position' else lv[idx]))
        c = np.add.accumulate(part.astype(acc), 0, dtype=acc)[-1]
        num = block_sum(c[2])
        den = block_sum((c[1] - (c[0] * c[0]).astype(acc) / acc(n)).astype(acc))
        out = np.array([np.sqrt(np.float64(t[0]) / (float(n) * X)) if n else nan, 1.0 - np.float64(num) / np.float64(den),
                        np.float64(t[1]) / n if n else nan, np.float64(t[2]) / n if (ll is not None and n) else nan])
    return out


# -------------------------------------------------------------------- synthetic inputs of the finalizer
def finalize_case(n, X, row_blocks, with_sel, seed=0):
    """random exact inputs of ``dv_recon_finalize``: fp32 rows (n_all, 6) / ll (n_all), float64 part (row_blocks, 3, X) whose first
    ``used`` blocks hold the column sums of n rows split at random and whose other blocks are zero -- the layout the sharded
    evaluation leaves -- and an UNSORTED int32 ``sel`` into a larger rows array (or None).  n = 1: the part of one fp32 row
    (den = 0 exactly); n = 0: all zero"""
    rs = np.random.RandomState(7919 * seed + 31 * n + 3 * X + row_blocks + 1000 * int(with_sel))
    n_all = n + 37 if with_sel else max(n, 1)         # (rows is never an empty array: the launch is given a pointer)
    a, b = rs.gamma(3.0, 1.0, n_all), rs.gamma(3.0, 1.0, n_all)
    rho = rs.uniform(-1, 1, n_all)
    rows = np.stack([rs.gamma(2.0, 5.0, n_all), rs.standard_normal(n_all), rs.standard_normal(n_all), a, b, rho * np.sqrt(a * b)], 1).astype(f)
    ll = (-50.0 + 30.0 * rs.standard_normal(n_all)).astype(f)
    sel = rs.permutation(n_all)[:n].astype(np.int32) if with_sel else None
    part = np.zeros((row_blocks, 3, X), np.float64)
    used = max(1, min(row_blocks, -(-row_blocks * 2 // 3)))
    if n == 1:
        xr, rr = rs.standard_normal(X).astype(f).astype(np.float64), rs.standard_normal(X).astype(f).astype(np.float64)
        part[0] = np.stack([xr, xr * xr, (xr - rr) ** 2], 0)
    elif n > 1:
        m, v, e = 3.0 * rs.standard_normal(X), rs.gamma(2.0, 0.5, X) + 0.1, rs.gamma(2.0, 0.2, X)
        w = rs.dirichlet(np.ones(used))
        tot = np.stack([n * m, n * (v + m * m), n * e], 0)
        part[:used] = w[:, None, None] * tot[None]
    return rows, part, ll, sel


# ---------------------------------------------------------------------------------------------- rank metrics
def rank_reference(score, pos):
    """(ROC-AUC, AP) of fp32 scores and a boolean positive mask: the AUC as ONE correctly rounded division of Python integers,
    AP by the header's definition with exact counts, summed with fsum; nan / 0 for the degenerate cases"""
    s = np.asarray(score, f).reshape(-1)
    s = np.where(s == 0, f(0), s)                # (-0.0 and +0.0 tie; np.unique sorts them as equal, this keeps it explicit)
    pos = np.asarray(pos, bool).reshape(-1)
    n, n_pos = len(s), int(pos.sum())
    n_neg = n - n_pos
    if n == 0 or n_pos == 0:
        return float('nan'), 0.0
    vals, inv = np.unique(s, return_inverse=True)           # ascending distinct scores
    P = np.bincount(inv, weights=pos, minlength=len(vals)).astype(np.int64)
    A = np.bincount(inv, minlength=len(vals)).astype(np.int64)
    Pge, Age = np.cumsum(P[::-1])[::-1], np.cumsum(A[::-1])[::-1]        # counts at scores >= the value
    ap = math.fsum(int(P[k]) * (int(Pge[k]) / int(Age[k])) for k in range(len(vals)) if P[k]) / n_pos
    if n_neg == 0:
        return float('nan'), ap
    num = sum(int(A[k] - P[k]) * (2 * int(Pge[k] - P[k]) + int(P[k])) for k in range(len(vals)))
    return num / (2 * n_pos * n_neg), ap


RANK_PATTERNS = ('continuous', 'grid3', 'equal', 'saturated', 'signed_zero', 'subnormal')


def rank_scores(pattern, n_all, Y, seed=0):
    """fp32 (n_all, Y) score matrix of one pattern: softmax rows; a three-value grid (heavy ties); all equal; saturated softmax
    rows holding exact 0.0 and 1.0; -0.0 next to +0.0 (a tie); values that differ only among fp32 subnormals (distinct)"""
    rs = np.random.RandomState(104729 * RANK_PATTERNS.index(pattern) + 13 * n_all + Y + seed)
    if pattern == 'continuous':
        z = 2.0 * rs.standard_normal((n_all, Y))
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(f)
    if pattern == 'grid3':
        return rs.choice(np.asarray([0.25, 0.5, 0.75], f), (n_all, Y))
    if pattern == 'equal':
        return np.full((n_all, Y), 0.5, f)
    if pattern == 'saturated':
        z = 200.0 * rs.standard_normal((n_all, Y))
        e = np.exp((z - z.max(1, keepdims=True)).astype(f)).astype(f)
        p = (e / e.sum(1, keepdims=True).astype(f)).astype(f)
        assert (p == 0).any() and (p == 1).any()
        return p
    if pattern == 'signed_zero':
        return rs.choice(np.asarray([-0.0, 0.0, 0.5], f), (n_all, Y))
    p = rs.choice(np.asarray([0.0, 1e-40, 2e-40, 3e-40], f), (n_all, Y))
    assert f(1e-40) != f(2e-40) and f(1e-40) > 0
    return p


def rank_case(n, pattern, Y, seed=0, extra=29):
    """(proba (n + extra, Y) fp32, y int32, pred int32, sel int32: an UNSORTED choice of n of the n + extra rows)"""
    rs = np.random.RandomState(31 * n + Y + 7 * seed + 1)
    proba = rank_scores(pattern, n + extra, Y, seed)
    y = rs.randint(0, Y, n + extra).astype(np.int32)
    pred = np.where(rs.rand(n + extra) < 0.7, y, rs.randint(0, Y, n + extra)).astype(np.int32)
    sel = rs.permutation(n + extra)[:n].astype(np.int32)
    return proba, y, pred, sel


def rank_expected(proba, y, pred, sel, c0, n_cls, binary):
    """out (2 n_cls + 1) float64 of ``dv_rank_metrics`` by the reference: [auc, ap] per class, then the accuracy -- hits / n
    in fp32 as the kernel divides (NaN for n = 0 and, the settled contract, for ``pred`` None)"""
    idx = np.asarray(sel, np.int64) if sel is not None else np.arange(len(y))
    out = np.zeros(2 * n_cls + 1)
    for c in range(n_cls):
        pos = (y[idx] > 0) if binary else (y[idx] == c0 + c)
        out[2 * c], out[2 * c + 1] = rank_reference(proba[idx, c0 + c], pos)
    n = len(idx)
    out[2 * n_cls] = float(f(int((pred[idx] == y[idx]).sum())) / f(n)) if (pred is not None and n) else ACC_WITHOUT_PRED
    return out
