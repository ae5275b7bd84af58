"""-m gpu: the element-wise math of the row kernels and GEMM epilogues against the float64 reference of
``tests/ref64.py``, at the inputs where fp32 formulas lose accuracy: sigma heads down to the sd floor (pre-activations to
-30), residuals from 0 to 10, log-variances over [-30, 30], probabilities at the 1e-10 clamp, small Poisson rates.

Every bound is the componentwise rule of ``ref64`` (|got - ref| <= C U sum|components| + 2 U extra); each check states
its C.  The GEMM paths receive exact pre-activations through a one-hot product: x = I, W[j, i] = pre[i, j], no bias --
a sum with one non-zero product is exact in every tiling, so the chosen values reach the epilogue unchanged."""
import math

import numpy as np
import pytest
import torch

from tests import ref64
from tests.ref64 import ACTS, U, bound, check, f32, f64

pytestmark = pytest.mark.gpu

PRODUCT_TILINGS = (0, 1, 2, 3, 17, 40, 46)      # dv_gemm_has_tiling of the product library
SHIFT = f32(1e-3)                               # the models' sd floor (sd = softplus(pre) + 1e-3)
D_VALUES = (0.0, 1e-3, 0.1, 1.0, 10.0)          # residuals x - mu
SIGMA, LOGVAR = 1, 0                            # GAUSS_SIGMA / GAUSS_LOGVAR of the C-ABI
# C of the NLL checks: a log, one or two divisions, a square, the sum of three terms -- a few roundings each, the log's
# argument (sd^2 or sd) carrying the rounding of sd
C_NLL = 16


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert (_lib.GAUSS_SIGMA, _lib.GAUSS_LOGVAR) == (SIGMA, LOGVAR)
    return K


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def rows_bound(C, comps, extra, X, scale=0.5):
    """bound of scale * (row sum of X terms): the terms' own bounds plus the summation bound"""
    return scale * (bound(C, comps, extra).sum(1) + ref64.row_sum_bound(f64(comps), X))


# ------------------------------------------------------------------------------------------------ activations
AM, AN = 128, 256


def act_grid():
    """AM x AN fp32 pre-activations: a dense grid over [-30, 30], the edges (0, +-0.5: ELU's Taylor switch, +-20: the
    softplus threshold, and their fp32 neighbours) and finite-only points at +-88 / +-100 (returned as a mask)"""
    edges = [0.0, 0.5, -0.5, 20.0, -20.0]
    nb = [float(np.nextafter(np.float32(e), np.float32(s))) for e in (0.5, -0.5, 20.0, -20.0) for s in (-np.inf, np.inf)]
    finite = [88.0, -88.0, 100.0, -100.0]
    dense = np.linspace(-30.0, 30.0, AM * AN - len(edges) - len(nb) - len(finite))
    v = np.concatenate([dense, edges, nb, finite]).astype(np.float32)
    fin = np.zeros(v.size, bool)
    fin[-len(finite):] = True
    return torch.from_numpy(v).reshape(AM, AN), torch.from_numpy(fin).reshape(AM, AN)


@pytest.mark.parametrize('tiling', PRODUCT_TILINGS)
def test_activations_forward_and_derivative(K, dev, tiling):
    """all eight activations: dv_act in the forward epilogue (linear_fwd), dv_dact_from_y in the backward-data epilogue
    (linear_bwd_data with yref) on every product tiling, and act_bwd_"""
    pre, fin = act_grid()
    ok = ~fin
    eye = torch.eye(AM, device=dev)
    W = pre.t().contiguous().to(dev)
    ones = torch.ones(AM, AN, device=dev)
    assert K.gemm_force_tiling(tiling) == 0, 'product tiling %d missing from the library' % tiling
    try:
        for a in ACTS:
            y = torch.full((AM, AN), 7.0, device=dev)
            K.linear_fwd(y, eye, W, act0=a, act1=a)
            yr = ref64.act(a, pre)
            # C = 8: the library transcendentals' few ulp and the epilogue's own roundings
            check('dv_act(%s), forward epilogue, tiling %d' % (a, tiling), host(y)[ok], yr[ok],
                  bound(8, yr.abs(), ref64.act_exp_extra(a, pre))[ok], pre=pre[ok])
            assert bool(torch.isfinite(y).all()), a
            ys = yr.float()                                    # the forward's stored output
            gr = ref64.dact(a, pre)
            # C = 8: the derivative's few roundings; the stored output's rounding enters through |y g'(y)|
            bd = bound(8, gr.abs() + ys.double().abs() * ref64.dact_from_y_slope(a, ys))
            dx = torch.full((AM, AN), 7.0, device=dev)
            K.linear_bwd_data(dx, eye, ones, yref=ys.to(dev), act=a)
            check('dv_dact_from_y(%s), backward epilogue (gemm_common.inc / gemm_pipe.inc), tiling %d' % (a, tiling),
                  host(dx)[ok], gr[ok], bd[ok], y=ys[ok], pre=pre[ok])
            assert bool(torch.isfinite(dx).all()), a
            if tiling == 0:
                dY = torch.ones(AM, AN, device=dev)
                K.act_bwd_(dY, ys.to(dev), act0=a, act1=a)
                check('dv_dact_from_y(%s), act_bwd (rows.hip)' % a, host(dY)[ok], gr[ok], bd[ok], y=ys[ok], pre=pre[ok])
                assert bool(torch.isfinite(dY).all()), a
    finally:
        K.gemm_force_tiling(0)


# ------------------------------------------------------------------------------------- Gaussian sigma-head NLL
PRE_GRID = np.arange(-30 * 64, 30 * 64 + 1) / 64.0       # [-30, 30] in steps of 1/64 (exact in fp32, with +-0.5, +-20)


def nll_case(X, grid=PRE_GRID, seed=0):
    """M x X elements covering every (grid value, residual) pair; bias columns are small integers so that raw = value -
    bias is exact and the kernel's raw + bias gives the grid value back"""
    n = grid.size * len(D_VALUES)
    M = max(4, -(-n // X))
    k = np.arange(M * X)
    rng = np.random.default_rng(seed + X)
    pre = grid[k % grid.size]
    d = np.asarray(D_VALUES)[(k // grid.size) % len(D_VALUES)]
    mu = np.round(rng.uniform(-2.0, 2.0, M * X) * 1024) / 1024
    x = (mu + d).astype(np.float32)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).reshape(M, X)   # noqa: E731
    return dict(M=M, X=X, pre=t(pre), x=t(x), mu=t(mu),
                coef=torch.tensor([1.0, -0.5, 2.0, 0.25])[torch.arange(M) % 4],
                bm=torch.from_numpy(rng.integers(-2, 3, X).astype(np.float32)),
                bs=torch.from_numpy(rng.integers(-3, 4, X).astype(np.float32)))


def _dev(dev, *ts):
    return [t.to(dev).contiguous() for t in ts]


@pytest.mark.parametrize('X', [13, 978, 4100])
def test_sigma_nll_finished_heads(K, dev, X):
    """nll_rows_fwd / nll_rows_bwd / nll_rows_fwdbwd on finished heads s = fl(softplus(pre) + 1e-3): the value on the
    stored s, the derivative through the softplus taken from s - shift (X = 13 / 978 / 4100: scalar, float2, float4)"""
    c = nll_case(X)
    M = c['M']
    s = (ref64.act('softplus', c['pre']) + SHIFT).float()
    r = ref64.nll_sigma_finished(c['x'], c['mu'], s, SHIFT, 'softplus', coef=c['coef'][:, None])
    x, mu, sd, coef = _dev(dev, c['x'], c['mu'], s, c['coef'])
    rows_ref = -0.5 * r['term'].sum(1)
    rows_bd = rows_bound(C_NLL, r['term_c'], None, X)
    info = dict(pre=c['pre'], x=c['x'], mu=c['mu'], s=s)
    out = torch.full((M,), 7.0, device=dev)
    K.nll_rows_fwd(out, x, mu, sd, mode=SIGMA)
    check('nll_rows_fwd (finished)', host(out), rows_ref, rows_bd)
    D = torch.full((M, 2 * X), 7.0, device=dev)
    dx = torch.full((M, X), 7.0, device=dev)
    K.nll_rows_bwd(D[:, :X], D[:, X:], coef, x, mu, sd, mode=SIGMA, sd_act='softplus', sd_shift=SHIFT, dx=dx)
    D = host(D)
    check('nll_rows_bwd d/dmu', D[:, :X], r['gm'], bound(C_NLL, r['gm_c']), **info)
    check('nll_rows_bwd d/dx', host(dx), -r['gm'], bound(C_NLL, r['gm_c']), **info)
    check('nll_rows_bwd d/dpre (dv_dact_from_y softplus)', D[:, X:], r['gs'], bound(C_NLL, r['gs_c']), **info)
    out = torch.full((M,), 7.0, device=dev)
    D = torch.full((M, 2 * X), 7.0, device=dev)
    K.nll_rows_fwdbwd(out, D[:, :X], D[:, X:], coef, x, mu, sd, mode=SIGMA, sd_act='softplus', sd_shift=SHIFT)
    D = host(D)
    check('nll_rows_fwdbwd (finished) rows', host(out), rows_ref, rows_bd)
    check('nll_rows_fwdbwd (finished) d/dmu', D[:, :X], r['gm'], bound(C_NLL, r['gm_c']), **info)
    check('nll_rows_fwdbwd (finished) d/dpre (nll_fb_elem, dv_dact_from_y softplus)', D[:, X:], r['gs'],
          bound(C_NLL, r['gs_c']), **info)


@pytest.mark.parametrize('X', [13, 978, 4100])
def test_sigma_nll_raw_heads(K, dev, X):
    """the raw-heads passes, which receive x W^T and finish sd = softplus(raw + b) + 1e-3 themselves: nll_rows_fwd
    (nll_raw_term), nll_rows_fwdbwd with bias (nll_fb_elem's raw branch; the float4 pass nll_raw_sp_elem at X = 4100)
    and nll_rows_raw_cs with its folded bias gradient"""
    c = nll_case(X)
    M = c['M']
    r = ref64.nll_sigma_pre(c['x'], c['mu'], c['pre'], SHIFT, coef=c['coef'][:, None])
    mraw, sraw = c['mu'] - c['bm'], c['pre'] - c['bs']
    assert torch.equal(mraw + c['bm'], c['mu']) and torch.equal(sraw + c['bs'], c['pre'])
    x, mr, sr, bm, bs, coef = _dev(dev, c['x'], mraw, sraw, c['bm'], c['bs'], c['coef'])
    rows_ref = -0.5 * r['term'].sum(1)
    rows_bd = rows_bound(C_NLL, r['term_c'], r['term_x'], X)
    info = dict(pre=c['pre'], x=c['x'], mu=c['mu'])
    out = torch.full((M,), 7.0, device=dev)
    K.nll_rows_fwd(out, x, mr, sr, mode=SIGMA, bias=(bm, bs), sd_shift=SHIFT)
    check('nll_rows_fwd (raw: nll_raw_term)', host(out), rows_ref, rows_bd)
    site = 'nll_raw_sp_elem' if X % 4 == 0 else 'nll_fb_elem raw branch'
    out = torch.full((M,), 7.0, device=dev)
    D = torch.full((M, 2 * X), 7.0, device=dev)
    K.nll_rows_fwdbwd(out, D[:, :X], D[:, X:], coef, x, mr, sr, mode=SIGMA, sd_act='softplus', sd_shift=SHIFT,
                      bias=(bm, bs))
    D = host(D)
    check('nll_rows_fwdbwd (raw, %s) rows' % site, host(out), rows_ref, rows_bd)
    check('nll_rows_fwdbwd (raw, %s) d/dmu' % site, D[:, :X], r['gm'], bound(C_NLL, r['gm_c'], r['gm_x']), **info)
    check('nll_rows_fwdbwd (raw, %s) d/dpre' % site, D[:, X:], r['gs'], bound(C_NLL, r['gs_c'], r['gs_x']), **info)
    if X % 4:
        return
    chunks, rbs = K.nll_raw_cs_shape(M, X)
    part = torch.full((M, chunks), 7.0, device=dev)
    K.nll_rows_raw_cs(part, None, None, None, None, x, mr, sr, (bm, bs), sd_shift=SHIFT)
    check('nll_rows_raw_cs (forward only) rows', host(part).double().sum(1), rows_ref, rows_bd)
    part = torch.full((M, chunks), 7.0, device=dev)
    D = torch.full((M, 2 * X), 7.0, device=dev)
    ws = torch.full((rbs, 2 * X), 7.0, device=dev)
    K.nll_rows_raw_cs(part, D[:, :X], D[:, X:], ws, coef, x, mr, sr, (bm, bs), sd_shift=SHIFT)
    D, ws = host(D), host(ws)
    check('nll_rows_raw_cs rows', host(part).double().sum(1), rows_ref, rows_bd)
    check('nll_rows_raw_cs (nll_raw_sp_elem) d/dmu', D[:, :X], r['gm'], bound(C_NLL, r['gm_c'], r['gm_x']), **info)
    check('nll_rows_raw_cs (nll_raw_sp_elem) d/dpre', D[:, X:], r['gs'], bound(C_NLL, r['gs_c'], r['gs_x']), **info)
    # the folded bias gradient: column sums over blocks of 64 rows
    for key, lo in (('gm', 0), ('gs', X)):
        g, bd = r[key], bound(C_NLL, r[key + '_c'], r[key + '_x'])
        for b in range(rbs):
            sl = slice(64 * b, 64 * (b + 1))
            colb = bd[sl].sum(0) + ref64.row_sum_bound(r[key + '_c'][sl].t(), 64)
            check('nll_rows_raw_cs column sums of %s, row block %d' % (key, b), ws[b, lo:lo + X], g[sl].sum(0), colb)


@pytest.mark.parametrize('M_S', [(978, 'softplus'), (13, 'softplus'), (978, 'sigmoid')])
def test_heads_nll_epilogue(K, dev, M_S):
    """linear_heads(nll=...): the fused sigma-head epilogue (act1 = softplus, the cfg-2 path) and the general heads-NLL
    branch (another act1: the derivative from the output a1 - shift1), pre-activations reaching it exactly (one-hot)"""
    S, act1 = M_S
    c = nll_case(S)
    M = c['M']
    fused = act1 == 'softplus'
    r = ref64.nll_sigma_pre(c['x'], c['mu'], c['pre'], SHIFT, coef=c['coef'][:, None], sd_act=act1, hw_exp=fused,
                            from_output=not fused)
    W = torch.cat([c['mu'].t(), c['pre'].t()], 0).contiguous().to(dev)
    eye = torch.eye(M, device=dev)
    xt, coef = _dev(dev, c['x'], c['coef'])
    nt = K.heads_tiles(S)
    out = torch.full((M, 2 * S), 7.0, device=dev)
    part = torch.full((M, nt), 7.0, device=dev)
    K.linear_heads(out, eye, W, None, split=S, act0='identity', act1=act1, shift1=SHIFT,
                   nll=dict(x=xt, coef=coef, part=part))
    out = host(out)
    site = 'linear_heads fused softplus epilogue' if fused else 'linear_heads general NLL branch (%s)' % act1
    info = dict(pre=c['pre'], x=c['x'], mu=c['mu'])
    check(site + ' rows', host(part).double().sum(1), -0.5 * r['term'].sum(1),
          rows_bound(C_NLL, r['term_c'], r['term_x'], S))
    check(site + ' d/dmu', out[:, :S], r['gm'], bound(C_NLL, r['gm_c'], r['gm_x']), **info)
    check(site + ' d/dpre', out[:, S:], r['gs'], bound(C_NLL, r['gs_c'], r['gs_x']), **info)


# ------------------------------------------------------------------------------------------------ logvar mode
@pytest.mark.parametrize('X', [13, 978, 4100])
def test_logvar_nll(K, dev, X):
    """the Gaussian NLL in log-variance mode (nll_rows_fwd / nll_rows_bwd / nll_rows_fwdbwd), logvar over [-30, 30]"""
    c = nll_case(X)
    M = c['M']
    lv = c['pre']
    r = ref64.nll_logvar(c['x'], c['mu'], lv, coef=c['coef'][:, None])
    x, mu, sd, coef = _dev(dev, c['x'], c['mu'], lv, c['coef'])
    rows_ref, rows_bd = -0.5 * r['term'].sum(1), rows_bound(C_NLL, r['term_c'], None, X)
    info = dict(lv=lv, x=c['x'], mu=c['mu'])
    out = torch.full((M,), 7.0, device=dev)
    K.nll_rows_fwd(out, x, mu, sd, mode=LOGVAR)
    check('nll_rows_fwd (logvar)', host(out), rows_ref, rows_bd)
    for fused in (False, True):
        D = torch.full((M, 2 * X), 7.0, device=dev)
        if fused:
            out = torch.full((M,), 7.0, device=dev)
            K.nll_rows_fwdbwd(out, D[:, :X], D[:, X:], coef, x, mu, sd, mode=LOGVAR)
            check('nll_rows_fwdbwd (logvar) rows', host(out), rows_ref, rows_bd)
        else:
            K.nll_rows_bwd(D[:, :X], D[:, X:], coef, x, mu, sd, mode=LOGVAR)
        D = host(D)
        name = 'nll_rows_fwdbwd' if fused else 'nll_rows_bwd'
        check(name + ' (logvar) d/dmu', D[:, :X], r['gm'], bound(C_NLL, r['gm_c']), **info)
        check(name + ' (logvar) d/dlogvar', D[:, X:], r['gs'], bound(C_NLL, r['gs_c']), **info)


def test_logvar_kl_rows_and_reparam(K, dev):
    """kl_rows_fwd / kl_rows_bwd (KL(q || p) of two diagonal Gaussians) and reparam_fwd / reparam_bwd in log-variance
    mode, both log-variances over [-30, 30]"""
    Z = 100
    g = np.arange(-30 * 8, 30 * 8 + 1) / 8.0
    rng = np.random.default_rng(7)
    sq = np.repeat(g, 5)
    sp = rng.permutation(sq)
    dm = np.tile(np.asarray(D_VALUES), g.size)
    n = -(-sq.size // Z)
    pad = n * Z - sq.size
    sq, sp, dm = (np.concatenate([v, np.zeros(pad)]) for v in (sq, sp, dm))
    mp = np.round(rng.uniform(-2, 2, n * Z) * 1024) / 1024
    mq = (mp + dm).astype(np.float32)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(n, Z)   # noqa: E731
    MQ, SQ, MP, SP = t(mq), t(sq), t(mp), t(sp)
    mq_d, sq_d, mp_d, sp_d = _dev(dev, MQ, SQ, MP, SP)
    # fp64 reference through autograd: raw = -0.5 sum_d (1 - sp + sq - (dm^2 + e^sq) e^-sp)
    leaves = [f64(v).requires_grad_(True) for v in (MQ, SQ, MP, SP)]
    a, b, cc, e = leaves
    kl = 1 - e + b - ((a - cc) ** 2 + torch.exp(b)) * torch.exp(-e)
    raw_ref = -0.5 * kl.sum(1)
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25])[torch.arange(n) % 4].double()
    (raw_ref * coef).sum().backward()
    q = (f64(MQ) - f64(MP)) ** 2 * torch.exp(-f64(SP))
    evq = torch.exp(f64(SQ) - f64(SP))
    kl_c = 1 + f64(SP).abs() + f64(SQ).abs() + q + evq
    out, raw = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    K.kl_rows_fwd(out, raw, mq_d, sq_d, mp_d, sp_d, mode=LOGVAR)
    # C = 16: two exps, a division and a sum of four terms per element
    check('kl_rows_fwd (logvar) raw', host(raw), raw_ref.detach(), rows_bound(16, kl_c, None, Z))
    check('kl_rows_fwd (logvar) out', host(out), raw_ref.detach(), rows_bound(16, kl_c, None, Z))
    G = [torch.full((n, Z), 7.0, device=dev) for _ in range(4)]
    K.kl_rows_bwd(G[0], G[1], G[2], G[3], coef.float().to(dev), raw, mq_d, sq_d, mp_d, sp_d, mode=LOGVAR)
    cab = coef.abs()[:, None]
    comps = [cab * (f64(MQ) - f64(MP)).abs() * torch.exp(-f64(SP)), 0.5 * cab * (1 + evq),
             cab * (f64(MQ) - f64(MP)).abs() * torch.exp(-f64(SP)), 0.5 * cab * (1 + q + evq)]
    for name, got, lf, cp in zip(('mu_q', 'logvar_q', 'mu_p', 'logvar_p'), G, leaves, comps):
        # C = 16: as the forward
        check('kl_rows_bwd (logvar) d/d' + name, host(got), lf.grad, bound(16, cp), sq=SQ, sp=SP)
    eps = t(rng.standard_normal(n * Z))
    z = torch.full((n, Z), 7.0, device=dev)
    K.reparam_fwd(z, mp_d, sq_d, eps.to(dev), mode=LOGVAR)
    std = torch.exp(0.5 * f64(SQ))
    # C = 8: one exp, a product and a sum
    check('reparam_fwd (logvar)', host(z), f64(eps) * std + f64(MP), bound(8, (f64(eps) * std).abs() + f64(MP).abs()),
          lv=SQ)
    dz = t(rng.standard_normal(n * Z))
    dmu, dlv = torch.full((n, Z), 7.0, device=dev), torch.full((n, Z), 7.0, device=dev)
    K.reparam_bwd(dmu, dlv, dz.to(dev), eps.to(dev), sq_d, mode=LOGVAR)
    check('reparam_bwd (logvar) d/dmu', host(dmu), f64(dz), bound(1, f64(dz).abs()))
    gl = f64(dz) * f64(eps) * 0.5 * std
    check('reparam_bwd (logvar) d/dlogvar', host(dlv), gl, bound(8, gl.abs()), lv=SQ)


# ----------------------------------------------------------------------------------------------- categorical
P_MIN = f32(1e-10)


@pytest.mark.parametrize('Y,sig', [(2, False), (3, False), (2, True)])
def test_softmax_clamp_and_cat_terms_at_the_clamp(K, dev, Y, sig):
    """softmax_clamp_fwd / _bwd and cat_terms_fwd / _bwd with probabilities on both sides of the 1e-10 clamp"""
    L = np.concatenate([np.linspace(18.0, 28.0, 2001), [math.log(1e10) + e for e in (-1e-6, 0.0, 1e-6)], [0.0, 3.0]])
    M = L.size
    lg = np.zeros((M, 1 if sig else Y), np.float32)
    if sig:
        lg[:, 0] = L
    else:
        lg[:, 1:] = -L[:, None]
        lg[:, Y - 1] -= 0.5 * (Y - 2)
    logits = torch.from_numpy(lg)
    a64 = f64(logits)
    if sig:
        s = torch.sigmoid(a64[:, :1])
        p64 = torch.cat([1 - s, s], 1)
    else:
        p64 = torch.softmax(a64, 1)
    pref = p64.clamp(P_MIN, 1.0)
    probs = torch.full((M, Y), 7.0, device=dev)
    K.softmax_clamp_fwd(probs, logits.to(dev), sig)
    probs_h = host(probs)
    if sig:
        # C = 8: 1 / (1 + exp(-a)) and 1 - s, which carries the rounding of s (condition term |s|)
        comps = pref + p64[:, 1:2].abs()
    else:
        # C = 8: exp(a - max) sees a rounded argument (|a - max| U relative), a sum of Y terms and a division
        comps = pref * (Y + (a64 - a64.max(1, keepdim=True)[0]).abs())
    check('softmax_clamp_fwd', probs_h, pref, bound(8, comps), L=torch.from_numpy(L)[:, None].expand(M, Y))
    # backward and the categorical terms on the kernel's stored probabilities
    P = f64(probs_h)
    rng = np.random.default_rng(Y)
    gp = torch.from_numpy(rng.standard_normal((M, Y)).astype(np.float32))
    dl = torch.full((M, 1 if sig else Y), 7.0, device=dev)
    K.softmax_clamp_bwd(dl, gp.to(dev), probs, sig)
    gm = torch.where(P > P_MIN, f64(gp), torch.zeros_like(P))
    if sig:
        sp = P[:, 1:2]
        ref = (gm[:, 1:2] - gm[:, 0:1]) * sp * (1 - sp)
        comps = (gm[:, 1:2].abs() + gm[:, 0:1].abs()) * sp * (1 - sp)
    else:
        dot = (gm * P).sum(1, keepdim=True)
        ref = P * (gm - dot)
        comps = P * (gm.abs() + (gm * P).abs().sum(1, keepdim=True))
    # C = 8: a dot product of Y terms, a difference and a product
    check('softmax_clamp_bwd', host(dl), ref, bound(8, comps))
    labels = torch.from_numpy((np.arange(M) % Y).astype(np.int32))
    prior = torch.softmax(torch.from_numpy(rng.standard_normal((M, Y)).astype(np.float32)), 1)
    logp, kl, ent = (torch.full(s_, 7.0, device=dev) for s_ in ((M,), (M, Y), (M,)))
    best = torch.zeros(M, dtype=torch.int32, device=dev)
    K.cat_terms_fwd(probs, labels=labels.to(dev), prior=prior.to(dev), logp=logp, kl=kl, ent=ent, best=best)
    lp, lq = torch.log(P), torch.log(f64(prior))
    lab = labels.long()[:, None]
    # C = 8: one log per probability and a few products / sums
    check('cat_terms_fwd logp', host(logp), lp.gather(1, lab)[:, 0], bound(8, lp.gather(1, lab)[:, 0].abs()))
    check('cat_terms_fwd kl', host(kl), -P * (lq - lp), bound(8, P * (lq.abs() + lp.abs())))
    check('cat_terms_fwd ent', host(ent), -(P * lp).sum(1), bound(8, (P * lp).abs().sum(1)))
    c1 = torch.from_numpy(rng.standard_normal(M).astype(np.float32))
    gk = torch.from_numpy(rng.standard_normal((M, Y)).astype(np.float32))
    c2 = torch.from_numpy(rng.standard_normal(M).astype(np.float32))
    dp = torch.full((M, Y), 7.0, device=dev)
    K.cat_terms_bwd(dp, probs, labels=labels.to(dev), prior=prior.to(dev), c_logp=c1.to(dev), g_kl=gk.to(dev),
                    c_ent=c2.to(dev))
    oh = torch.nn.functional.one_hot(labels.long(), Y).double()
    ref = oh * (f64(c1)[:, None] / P) + f64(gk) * (lp - lq + 1) - f64(c2)[:, None] * (lp + 1)
    comps = oh * (f64(c1)[:, None] / P).abs() + f64(gk).abs() * (lp.abs() + lq.abs() + 1) + \
        f64(c2).abs()[:, None] * (lp.abs() + 1)
    check('cat_terms_bwd', host(dp), ref, bound(8, comps))


# ---------------------------------------------------------------------------------------------- rec_nll_rows
@pytest.mark.parametrize('shift', [0.0, SHIFT])
def test_rec_nll_poisson_small_rates(K, dev, shift):
    """rec_nll_rows (Poisson): rates v = softplus(a) + shift with a down to -30, counts 0..20; the gradient w.r.t. a is
    taken from the stored rate (rows.hip rec_term)"""
    a = np.arange(-30 * 16, 10 * 16 + 1) / 16.0
    counts = np.asarray([0.0, 1.0, 3.0, 20.0])
    X = 256
    n = a.size * counts.size
    M = -(-n // X)
    k = np.arange(M * X)
    A = a[k % a.size]
    xs = counts[(k // a.size) % counts.size]
    v = (ref64.act('softplus', torch.from_numpy(A)) + shift).float().reshape(M, X)
    x = torch.from_numpy(xs.astype(np.float32)).reshape(M, X)
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25])[torch.arange(M) % 4]
    out, dpre = torch.full((M,), 7.0, device=dev), torch.full((M, X), 7.0, device=dev)
    K.rec_nll_rows(out, x.to(dev), v.to(dev), kind='poisson', shift=shift, coef=coef.to(dev), dpre=dpre)
    V, XX = f64(v), f64(x)
    lgam = torch.lgamma(XX + 1)
    ll = XX * torch.log(V) - V - lgam
    # C = 16: a log, lgamma (a few ulp) and two products / sums per term
    check('rec_nll_rows (poisson) rows', host(out), ll.sum(1),
          bound(16, (XX * torch.log(V)).abs() + V + lgam).sum(1) +
          ref64.row_sum_bound((XX * torch.log(V)).abs() + V + lgam, X))
    y = V - shift
    g = ref64.dact_from_y('softplus', y)
    ref = f64(coef)[:, None] * (XX / V - 1) * g
    comps = f64(coef).abs()[:, None] * (XX / V + 1) * (g + y.abs() * ref64.dact_from_y_slope('softplus', y))
    # C = 16: a division, a difference and the softplus derivative from the rate
    check('rec_nll_rows (poisson) d/dpre (rec_term softplus derivative)', host(dpre), ref, bound(16, comps),
          a=torch.from_numpy(A).reshape(M, X), v=v)


def test_rec_nll_bernoulli_at_the_clamp(K, dev):
    """rec_nll_rows (Bernoulli): probabilities on both sides of the 1e-10 clamp and just below 1"""
    vals = [1e-12, 5e-11, P_MIN * (1 - 2.0 ** -20), P_MIN, P_MIN * (1 + 2.0 ** -20), 2e-10, 1e-8, 1e-4, 0.5,
            1 - 2.0 ** -20, 1 - 2.0 ** -23, 1 - 2.0 ** -24]
    X = 64
    n = len(vals) * 2
    M = 4
    k = np.arange(M * X)
    v = torch.from_numpy(np.asarray(vals, np.float32)[k % len(vals)].reshape(M, X))
    x = torch.from_numpy(((k // len(vals)) % 2).astype(np.float32).reshape(M, X))
    assert n <= M * X
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25])
    out, dpre = torch.full((M,), 7.0, device=dev), torch.full((M, X), 7.0, device=dev)
    K.rec_nll_rows(out, x.to(dev), v.to(dev), kind='binary', coef=coef.to(dev), dpre=dpre)
    V, XX = f64(v), f64(x)
    pc = V.clamp(P_MIN, 1.0)
    ll = XX * torch.log(pc) + (1 - XX) * torch.log1p(-pc)
    # C = 8: two logs, the second of the rounded 1 - pc (+1: U absolute)
    comps = XX.abs() * (torch.log(pc).abs() + 1) + (1 - XX).abs() * (torch.log1p(-pc).abs() + 1)
    check('rec_nll_rows (bernoulli) rows', host(out), ll.sum(1), bound(8, comps).sum(1) + ref64.row_sum_bound(comps, X))
    inside = (V > P_MIN) & (V < 1.0)
    ref = f64(coef)[:, None] * torch.where(inside, XX - V, torch.zeros_like(V))
    check('rec_nll_rows (bernoulli) d/dpre', host(dpre), ref, bound(4, f64(coef).abs()[:, None] * (XX + V)), v=v)
