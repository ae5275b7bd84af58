"""The sampler form of ``dv_fill_normal`` (``dv_draw_desc``) as SPECIFIED, in numpy: written from the paragraph "THE SAMPLER" of
``include/drvae_hip.h`` and from ``tests/philox_ref.py``; it shares nothing with ``drvae_amd/csrc/optim.hip``.  Test-only.

``draw(...)`` evaluates the specification in float64 on the fp32 operands and fp32 uniforms a conforming kernel holds, and
returns per element

* ``value``: the draw;
* ``cap``: whether a loop ran into its cap (8 Gamma attempts, 64 inversion steps, 16 PTRS attempts);
* ``margin``: the smallest margin of any DECISION the element took -- a Gamma accept test, ``t > -1``, the dropout gate, the
  ``lam < 10`` / ``lam < 2^24`` switches, every CDF comparison of the inversion, the PTRS squeeze, its rejection region, its
  accept test and the distance of its ``floor`` argument to an integer -- in units of a bound on what fp32 rounding of the
  specified arithmetic can move that decision by.  ``margin < 1``: the element is UNDECIDED, a conforming fp32 kernel may
  take the other branch there; every other element must come out EQUAL;
* ``tol``: 0 for the count kinds and Bernoulli, except where the result is the rate itself (``lam >= 2^24``): there, and for
  the Gaussian kind, the absolute error a conforming kernel may have.

The bounds count roundings by the rule of ``tests/nb_ref.py`` / ``tests/test_gpu_numerics.py`` (a transcendental: 3; a
product, quotient, sum or square root: 1; U = 2^-24), propagate the error of every intermediate into the decision that reads it
(``_Elem`` carries the rate's relative error ``rho`` into the Poisson draw), and are doubled (``SAFETY``): fused
multiply-adds and the order of a sum are the implementation's.  The normal's error is the bound of
``tests/test_gpu_philox.py``, C U (r + r a) with C = 4.

``ft=np.float32`` runs the same statements in fp32: an EMULATION of a conforming kernel (what share of elements flips
against float64: ``tests/test_count_sample_cpu.py``), and with ``fault=...`` one of the faulty emulations that the tests must
catch:

  'gamma_scale'  Gamma scale m instead of m / theta        'no_boost'   the theta < 1 factor u^(1/theta) left out
  'gate_flip'    the dropout gate on 1 - pi                 'no_size'    the size factor dropped
  'swap_blocks'  the gate from block 0, the Gamma draw from blocks 16 .. 23
  'no_sample'    the sample index left out of the counter   'naive'      the accept test as d - d v + d ln v
"""
import numpy as np
import torch

from tests import philox_ref as P

GAUSS, BERNOULLI, POISSON, NEGBIN, ZINB = range(5)
KIND = {'diag_gaussian': GAUSS, 'binary': BERNOULLI, 'poisson': POISSON, 'nb': NEGBIN, 'zinb': ZINB}
U = 2.0 ** -24
C_NORMAL = 4.0            # tests/test_gpu_philox.py: C_BOUND
T = 3.0                   # roundings of a transcendental
SAFETY = 2.0
GAMMA_TRIES, POIS_BLOCK0, PTRS_TRIES, INV_STEPS, GATE_BLOCK = 8, 8, 16, 64, 16
LAM_MAX = 2.0 ** 24
FLT_MAX = float(np.finfo(np.float32).max)
FAULTS = ('gamma_scale', 'no_boost', 'gate_flip', 'no_size', 'swap_blocks', 'no_sample', 'naive')


def _lgamma(x):
    return torch.lgamma(torch.from_numpy(np.ascontiguousarray(x))).numpy()


class _Elem:
    """the flat elements of one draw: their counter coordinates, results and decision margins"""

    def __init__(self, g, R, k, seed, event, ft):
        self.g, self.R, self.k, self.ft = g, R, k, ft
        s_lo, s_hi = P._split(seed)
        e_lo, e_hi = P._split(event)
        self.key, self.e_lo = (s_lo, s_hi ^ e_hi), e_lo
        n = g.size
        self.value = np.full(n, np.nan)
        self.cap = np.zeros(n, bool)
        self.margin = np.full(n, np.inf)
        self.tol = np.zeros(n)

    def block(self, idx, b):
        """the four words of block ``b`` of the elements ``idx``"""
        return P.philox4x32_10(self.g[idx], self.R[idx], (self.k[idx] << 8) | int(b), self.e_lo, *self.key)

    def u(self, w):
        return P.u01(w).astype(self.ft)

    def decide(self, idx, dist, bound):
        """a decision of the elements ``idx`` that stands ``dist`` from its threshold where fp32 rounding moves it by at most
        ``bound``; bound 0: the decision is exact in fp32 (both sides are fp32 numbers)"""
        dist, bound = np.abs(np.asarray(dist, np.float64)), SAFETY * np.asarray(bound, np.float64)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            m = np.where(bound > 0, dist / bound, np.inf)
        m = np.where(np.isnan(m), 0.0, m)
        self.margin[idx] = np.minimum(self.margin[idx], m)

    def normal(self, w):
        """N(b) of a block's words: (x, its error bound)"""
        ft = self.ft
        r = np.sqrt(ft(-2.0) * np.log(self.u(w[0])))
        a = ft(2.0 * np.pi) * self.u(w[1])
        return r * np.cos(a), C_NORMAL * U * (r + r * a).astype(np.float64)


def _gamma_rate(E, idx, m, theta, fault):
    """(lam, rho) of the negative-binomial elements ``idx``: the Marsaglia-Tsang rate and a bound on its relative error"""
    ft = E.ft
    lam, rho = m.copy(), np.zeros(idx.size)
    live = np.flatnonzero(np.isfinite(theta))          # (theta = +inf: lam = m)
    if not live.size:
        return lam, rho
    th, mm = theta[live], m[live]
    boost = th < 1
    d = np.where(boost, th + ft(1), th) - ft(1.0 / 3.0)
    c = ft(1) / np.sqrt(ft(9) * d)
    first = 16 if fault == 'swap_blocks' else 0
    ub = E.u(E.block(idx[live], first)[3])
    lg, dlg = np.zeros(live.size, ft), np.zeros(live.size)
    todo = np.arange(live.size)
    for j in range(GAMMA_TRIES):
        if not todo.size:
            break
        ii = idx[live[todo]]
        w = E.block(ii, first + j)
        x, dx = E.normal(w)
        dd, cc = d[todo], c[todo]
        t = cc * x
        t64, d64, x64 = t.astype(np.float64), dd.astype(np.float64), x.astype(np.float64)
        dt = np.abs(t64) * 5 * U + cc * dx               # c: difference, product, root, quotient (4); the product (1)
        E.decide(ii, t64 + 1, dt)
        inside = t > -1
        lu = np.log(E.u(w[2]))
        with np.errstate(invalid='ignore', divide='ignore'):
            l1 = np.log1p(t)
            if fault == 'naive':
                v = (ft(1) + t) * (ft(1) + t) * (ft(1) + t)
                h = ft(0.5) * x * x + (dd - dd * v + dd * np.log(v))
            else:
                h = ft(0.5) * x * x + dd * (ft(3) * l1 - t * (ft(3) + t * (ft(3) + t)))
            l64, a64 = np.abs(np.log1p(t64)), np.abs(t64)
            poly = a64 * (3 + a64 * (3 + a64))
            slope = np.abs(3 / (1 + t64) - 3 - 6 * t64 - 3 * t64 * t64)
            bound = (np.abs(x64) * dx + 2 * U * x64 * x64                       # x^2 / 2
                     + d64 * (slope * dt + U * (T + 3) * 3 * l64 + U * 6 * poly)  # d g(t): through t, and g's own roundings
                     + T * U * np.abs(lu) + U * np.abs(h))
        E.decide(ii[inside], (lu.astype(np.float64) - h)[inside], bound[inside])
        acc = inside & (lu < h)
        with np.errstate(invalid='ignore', divide='ignore'):
            lr = np.log(dd if fault == 'gamma_scale' else dd / theta[live[todo]])
            lgd = lr + ft(3) * l1
        lg[todo[acc]] = lgd[acc]
        # ln(d / theta): difference and quotient (2) through the logarithm, the logarithm (T); 3 log1p(t) through t; the sum
        dlg[todo[acc]] = (2 * U + T * U * np.abs(lr) + 3 * (dt / (1 + t64) + T * U * l64) + 2 * U * np.abs(lgd))[acc]
        todo = todo[~acc]
    E.cap[idx[live[todo]]] = True                      # (past the cap: the Gamma's mean, lam = m)
    ok = np.ones(live.size, bool)
    ok[todo] = False
    if fault != 'no_boost':
        with np.errstate(divide='ignore'):
            add = np.where(boost, np.log(ub) / th, ft(0))
        lg = lg + add
        dlg = dlg + (T + 2) * U * np.abs(add)
    # q not finite in fp32 (a denormal theta: d / theta or ln u / theta beyond FLT_MAX): lam = 0
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        lost = (d.astype(np.float64) / th.astype(np.float64) > FLT_MAX) | ~np.isfinite(lg)
        if fault != 'no_boost':
            lost |= np.abs(add.astype(np.float64)) > FLT_MAX
        lam[live[ok]] = np.where(lost, ft(0), mm * np.exp(lg))[ok]
        dlg = np.where(lost, 0.0, dlg)
    dex = dlg + U                                       # (the product with m)
    rho[live[ok]] = np.where(lost, 0.0, dex + T * U)[ok]
    return lam, rho


def _poisson(E, idx, b0, lam, rho):
    """P(b0, lam) of the elements ``idx`` (lam >= 0, no NaN), whose rate carries the relative error bound ``rho``"""
    ft = E.ft
    lam64 = lam.astype(np.float64)
    with np.errstate(invalid='ignore'):
        dlam = rho * lam64
    E.decide(idx, lam64 - LAM_MAX, dlam)
    big = ~(lam < LAM_MAX)
    E.value[idx[big]] = np.minimum(lam64[big], FLT_MAX)
    E.tol[idx[big]] = np.where(np.isfinite(lam64[big]), SAFETY * dlam[big], 0.0)      # (+inf: FLT_MAX itself)
    rest = np.flatnonzero(~big)
    E.decide(idx[rest], lam64[rest] - 10, dlam[rest])
    small = rest[lam[rest] < 10]
    large = rest[~(lam[rest] < 10)]
    # ---- inversion by sequential search
    if small.size:
        ii, la, dl = idx[small], lam[small], dlam[small]
        u = E.u(E.block(ii, b0)[0])
        p = np.exp(-la)
        cdf = p.copy()
        todo = np.arange(small.size)
        for i in range(INV_STEPS + 1):
            if i:
                p[todo] = p[todo] * (la[todo] / ft(i))
                cdf[todo] = cdf[todo] + p[todo]
            E.decide(ii[todo], (u[todo] - cdf[todo]).astype(np.float64),
                     dl[todo] * p[todo] + U * (T + 3 * i) * cdf[todo].astype(np.float64))
            hit = ~(u[todo] > cdf[todo])
            E.value[ii[todo[hit]]] = i
            todo = todo[~hit]
            if not todo.size:
                break
        E.cap[ii[todo]] = True
        E.value[ii[todo]] = np.rint(la[todo])
    # ---- PTRS
    if large.size:
        ii, la, rh = idx[large], lam[large], rho[large]
        la64 = la.astype(np.float64)
        slam, loglam = np.sqrt(la), np.log(la)
        b = ft(0.931) + ft(2.53) * slam
        a = ft(-0.059) + ft(0.02483) * b
        ia = ft(1.1239) + ft(1.1328) / (b - ft(3.4))
        lia = np.log(ia)
        vr = ft(0.9277) - ft(3.6224) / (b - ft(2))
        b64, a64 = b.astype(np.float64), a.astype(np.float64)
        rb = 3 * U + rh / 2                             # relative error of b (root, product, sum; the rate's own)
        ra = rb + 2 * U * (1 + 0.059 / a64)
        dvr = U * (0.9277 + 2 * 3.6224 / (b64 - 2)) + 3.6224 / (b64 - 2) ** 2 * b64 * rb + U
        dlia = T * U * np.abs(lia) + (2 * U * ia + 1.1328 / (b64 - 3.4) ** 2 * b64 * rb) / ia
        todo = np.arange(large.size)
        w = None
        for j in range(PTRS_TRIES):
            if not todo.size:
                break
            it = ii[todo]
            if not j & 1:
                w = E.block(it, b0 + (j >> 1))
                keep = np.arange(todo.size)
            wU, wV = (w[2][keep], w[3][keep]) if j & 1 else (w[0][keep], w[1][keep])
            UU, V = E.u(wU) - ft(0.5), E.u(wV)
            us = ft(0.5) - np.abs(UU)
            l, l6, bb, aa = la[todo], la64[todo], b[todo], a[todo]
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                term = (ft(2) * aa / us + bb) * UU
                arg = term + l + ft(0.43)
                k = np.floor(arg)
                us6, U6, a6, b6 = us.astype(np.float64), np.abs(UU.astype(np.float64)), a64[todo], b64[todo]
                darg = (2 * a6 / us6 * U6 * (5 * U + ra[todo] + U / us6) + b6 * U6 * (2 * U + rb[todo]) + rh[todo] * l6
                        + 3 * U * (np.abs(term) + l6 + 0.43))
                frac = (arg - k).astype(np.float64)
            nz = us > 0                                # (us = 0: k = +inf, the attempt is rejected whatever rounding does)
            E.decide(it[nz], np.minimum(frac, 1 - frac)[nz], darg[nz])
            E.decide(it, us6 - 0.07, np.full(todo.size, U))
            wide = us >= ft(0.07)
            E.decide(it[wide], (V - vr[todo]).astype(np.float64)[wide], dvr[todo][wide])
            quick = wide & (V <= vr[todo])
            E.decide(it[~quick], us6[~quick] - 0.013, np.full(int((~quick).sum()), U))
            narrow = ~quick & (us < ft(0.013))
            E.decide(it[narrow], (V - us).astype(np.float64)[narrow], np.full(int(narrow.sum()), U))
            rej = ~quick & ((k < 0) | (narrow & (V > us)))
            slow = np.flatnonzero(~quick & ~rej)
            acc = quick.copy()
            if slow.size:
                ks, ls, l6s = k[slow], l[slow], l6[slow]
                q = aa[slow] / (us[slow] * us[slow]) + bb[slow]
                lgk = _lgamma(ks + ft(1))
                lhs = np.log(V[slow]) + lia[todo][slow] - np.log(q)
                rhs = -ls + ks * loglam[todo][slow] - lgk
                q6, k6, ll6 = q.astype(np.float64), ks.astype(np.float64), np.abs(loglam[todo][slow].astype(np.float64))
                dq = (a6[slow] / us6[slow] ** 2 * (3 * U + ra[todo][slow] + 2 * U / us6[slow]) + b6[slow] * rb[todo][slow]) / q6
                bound = (T * U * np.abs(np.log(V[slow].astype(np.float64))) + dlia[todo][slow] + T * U * np.abs(np.log(q6)) + dq
                         + 2 * U * (np.abs(lhs) + np.abs(np.log(q6)))
                         + rh[todo][slow] * (1 + np.abs(k6 - l6s)) + (T + 1) * U * k6 * ll6 + 8 * U * np.abs(lgk)
                         + 2 * U * (l6s + k6 * ll6 + np.abs(lgk)))
                E.decide(it[slow], (lhs - rhs).astype(np.float64), bound)
                acc[slow] = lhs <= rhs
            E.value[it[acc]] = k[acc]
            todo = todo[~acc]
            keep = keep[~acc]
        E.cap[ii[todo]] = True
        E.value[ii[todo]] = np.rint(la[todo])


def draw(kind, mu, *, sd=None, theta=None, logit=None, size=None, S=1, seed=0, event=0, row0=0, grow=None, sample0=0,
         ft=np.float64, fault=None):
    """the specification on the heads ``mu`` (M, X) and their companions (``theta``: (M, X) or the shared (X,) row), for the
    samples sample0 .. sample0 + S - 1 of the global rows ``row0 + r`` or ``grow``: -> dict(value, cap, margin, tol), each
    (S, M, X) -- see the module's docstring"""
    kind = KIND.get(kind, kind)
    assert kind in range(5) and (fault is None or fault in FAULTS)
    mu = np.asarray(mu, np.float32)
    M, X = mu.shape
    shape = (S, M, X)
    rows = (int(row0) + np.arange(M)) if grow is None else np.asarray(grow).reshape(M)
    g = np.broadcast_to(np.arange(X, dtype=np.int64), shape).reshape(-1)
    R = np.broadcast_to(rows.astype(np.int64)[None, :, None], shape).reshape(-1)
    k = np.broadcast_to((sample0 + np.arange(S, dtype=np.int64))[:, None, None], shape).reshape(-1)
    if fault == 'no_sample':
        k = np.zeros_like(k)
    E = _Elem(g, R, k, seed, event, ft)
    op = lambda v: None if v is None else np.broadcast_to(np.asarray(v, np.float32), (M, X))[None].repeat(S, 0).reshape(-1).astype(ft)
    mu_e, sd_e, th_e, lg_e = op(mu), op(sd), op(theta), op(logit)
    every = np.arange(g.size)
    if kind == GAUSS:
        x, dx = E.normal(E.block(every, 0))
        E.value[:] = mu_e + sd_e * x
        E.tol[:] = np.abs(sd_e) * dx + 2 * U * (np.abs(mu_e) + np.abs(sd_e * x))
    elif kind == BERNOULLI:
        u = E.u(E.block(every, 0)[0])
        E.value[:] = np.where(np.isnan(mu_e), np.nan, (u <= mu_e).astype(np.float64))
    else:
        m = mu_e
        if size is not None and fault != 'no_size':
            s32 = np.broadcast_to(np.asarray(size, np.float32).reshape(1, M, 1), shape).reshape(-1)
            with np.errstate(over='ignore', invalid='ignore'):
                m = (s32 * mu.reshape(1, M, X).repeat(S, 0).reshape(-1)).astype(ft)       # ONE fp32 product
        live = ~np.isnan(m)
        if kind == POISSON:
            E.value[live & ~(m > 0)] = 0
            idx = np.flatnonzero(live & (m > 0))
            _poisson(E, idx, 0, m[idx], np.zeros(idx.size))
        else:
            live &= ~np.isnan(th_e) & (th_e > 0)
            if kind == ZINB:
                live &= ~np.isnan(lg_e)
                idx = np.flatnonzero(live)
                u = E.u(E.block(idx, 0 if fault == 'swap_blocks' else GATE_BLOCK)[0])
                with np.errstate(over='ignore'):
                    pi = ft(1) / (ft(1) + np.exp(-lg_e[idx]))
                if fault == 'gate_flip':
                    pi = ft(1) - pi
                E.decide(idx, (u - pi).astype(np.float64), (T + 2) * U * pi.astype(np.float64))
                drop = u <= pi
                E.value[idx[drop]] = 0
                live[idx[drop]] = False
            E.value[live & ~(m > 0)] = 0
            E.value[live & np.isposinf(m)] = FLT_MAX
            idx = np.flatnonzero(live & (m > 0) & np.isfinite(m))
            lam, rho = _gamma_rate(E, idx, m[idx], th_e[idx], fault)
            _poisson(E, idx, POIS_BLOCK0, lam, rho)
    return dict(value=E.value.reshape(shape), cap=E.cap.reshape(shape), margin=E.margin.reshape(shape),
                tol=E.tol.reshape(shape))


def compare(got, ref):
    """``got`` (any float array shaped like the reference's) against ``draw``'s result: -> (wrong, undecided), boolean arrays --
    a DECIDED element is wrong unless |got - value| <= tol (NaN matches NaN); an undecided one unless it is finite,
    non-negative and integral"""
    got = np.asarray(got, np.float64)
    val, und = ref['value'], ref['margin'] < 1
    with np.errstate(invalid='ignore'):
        same = (np.abs(got - val) <= ref['tol']) | (np.isnan(got) & np.isnan(val))
        loose = np.isfinite(got) & (got >= 0) & (got == np.floor(got))
    return np.where(und, ~loose, ~same), und


# ------------------------------------------------------------------------------------------- analytic laws
def nb_pmf(kmax, mean, theta):
    """P(x = 0 .. kmax) of the negative binomial (mean, inverse dispersion theta; theta = inf: Poisson), float64, from
    math.lgamma"""
    import math
    out = np.empty(kmax + 1)
    for x in range(kmax + 1):
        if math.isinf(theta):
            out[x] = math.exp(x * math.log(mean) - mean - math.lgamma(x + 1))
        else:
            out[x] = math.exp(math.lgamma(x + theta) - math.lgamma(theta) - math.lgamma(x + 1)
                              + theta * math.log(theta / (theta + mean)) + x * math.log(mean / (theta + mean)))
    return out


def law(mean, theta, pi=0.0):
    """(mean, sd, P(x = 0), P(x <= floor(mean))) of the zero-inflated negative binomial: x = 0 with probability pi, else
    NB(mean, theta); ``mean`` is the NB's mean, the returned mean the mixture's"""
    var_nb = mean + (0.0 if np.isinf(theta) else mean * mean / theta)
    mix_mean = (1 - pi) * mean
    var = (1 - pi) * (var_nb + mean * mean) - mix_mean ** 2
    kq = int(np.floor(mix_mean))
    pmf = nb_pmf(kq, mean, theta)
    return mix_mean, float(np.sqrt(var)), pi + (1 - pi) * pmf[0], pi + (1 - pi) * float(pmf.sum())


# ------------------------------------------------------------------------------------------- the kernel tests' grid
UNDECIDED_CAP = 0.02
# (X, M, S): both sides of the quad path (X % 4) and of the 1024-gene chunk seam; 1, 2 and 9 rows; 1 and 3 samples
GRID_SHAPES = ((1, 9, 3), (3, 2, 1), (4, 9, 3), (5, 1, 3), (1020, 2, 3), (1024, 9, 1), (1028, 1, 3), (2052, 2, 3))
GRID_KINDS = ('diag_gaussian', 'binary', 'poisson', 'nb', 'zinb')


def grid_case(kind, i):
    """the operands of grid case ``i`` (a shape of GRID_SHAPES) of ``kind``, float32 numpy: mu 1e-6 .. 1e4, theta 1e-3 .. 1e6 (every
    other case ONE shared row: stride 0), logits -20 .. 20, size factors 1e-2 .. 1e2 (every other case none; mu <= 1e2 next to
    one for 'nb' / 'zinb'), a seed, an event and a first row of their own"""
    X, M, S = GRID_SHAPES[i]
    rs = np.random.RandomState(1000 * (KIND[kind] + 1) + i)
    logu = lambda lo, hi, *shape: np.exp(rs.uniform(np.log(lo), np.log(hi), shape)).astype(np.float32)
    c = dict(kind=kind, X=X, M=M, S=S, seed=int(rs.randint(1, 2 ** 31)) * 0x100000001 + 12345 * i, event=(i % 3) * (2 ** 33 + 5),
             row0=(0, 7, 2 ** 20 + 3)[i % 3], ops={})
    if kind == 'diag_gaussian':
        c['ops'] = dict(mu=rs.normal(0, 3, (M, X)).astype(np.float32), sd=logu(1e-3, 10, M, X))
    elif kind == 'binary':
        c['ops'] = dict(mu=np.clip(rs.uniform(0, 1, (M, X)), 1e-10, 1 - 1e-10).astype(np.float32))
    else:
        # (a Gamma-Poisson rate carries a relative error of some 1e-6 in ANY fp32 arithmetic and PTRS takes floor(... + lam):
        # above lam ~ 1e4 most elements are undecided by nature.  The cases with a size factor keep s mu <= 1e4 like the others)
        sized = i % 2 == 0
        c['ops'] = dict(mu=logu(1e-6, 1e2 if sized and kind != 'poisson' else 1e4, M, X))
        if sized:
            c['ops']['size'] = logu(1e-2, 1e2, M)
        if kind in ('nb', 'zinb'):
            c['ops']['theta'] = logu(1e-3, 1e6, X) if i % 2 else logu(1e-3, 1e6, M, X)
        if kind == 'zinb':
            c['ops']['logit'] = rs.uniform(-20, 20, (M, X)).astype(np.float32)
    return c


def grid_reference(kind, i, **kw):
    c = grid_case(kind, i)
    return c, draw(kind, S=c['S'], seed=c['seed'], event=c['event'], row0=c['row0'], **c['ops'], **kw)
