"""The optimiser sweeps (``dv_adam_l2``, ``dv_adam_l2_gated``, ``dv_adamax_l2``; drvae_amd/csrc/optim.hip) below model level:
a float64 reference of ONE step with its componentwise bound, two fp32 host emulations of the kernels' operation sequence,
the case classes, the memory frame and the faulty emulations the CPU file (tests/test_optim_cpu.py) proves the checks
against.  tests/test_gpu_optim.py holds the device to the same reference.  Plain numpy on the host: no device, no library.

Staging (as tests/clf_launch_ref.py).  A sequence of steps is checked step by step: the reference of step k reads the fp32
``p, m, v`` that the code under test STORED after step k-1, so every bound below is the bound of one step and never has to
carry an earlier step's rounding.  ``t = 0`` is outside the contract (bc1 = 1 - beta1^0 = 0: the step size is infinite) and
no case uses it.

What the ABI carries.  ``dv_adam_hyper`` holds lr, beta1, beta2, eps, weight_decay and gscale as fp32, so the reference
rounds them to fp32 first and computes in float64 from there: w1 = 1 - beta1, w2 = 1 - beta2 (both exact in fp32 for a
beta in [0.5, 1)), step = lr / (1 - beta1^t), c2 = sqrt(1 - beta2^t).  That is a self-consistent Adam whose betas are the
fp32 neighbours of python's 0.9 and 0.999: 1 - fp32(0.999) = 0.00099998713, 1.29e-5 (relative) off python's 0.001.  How far
that moves a trajectory is measured in tests/test_optim_cpu.py (``trajectory_bounds`` below is what can be derived).

The operation sequence of ``adam_one`` (fl: one fp32 rounding; the kernel writes its four multiply-adds as fma):

    g1 = fl(gscale g)           g2 = fma(wd, p, g1)   [wd != 0; else g2 = g1]
    d  = fl(g2 - m)             m' = fma(w1, d, m)
    a  = fl(w2 g2)  vb = fl(v beta2)     v' = fma(a, g2, vb)
    s  = fl(sqrt v')  q = fl(s / c2)  den = fl(q + eps)  r = fl(m' / den)     p' = fma(-step, r, p)

The componentwise bound (derived, not chosen).  First-order running error analysis: every fp32 operation costs one
rounding of ITS RESULT's magnitude, rnd(x) = U |x| + ETA (U = 2^-24; ETA = 2^-149, the spacing of the subnormals a product
may land among: gradual underflow, nothing is flushed), the fp32 casts of step and c2 cost one rounding each (of the
quantities they scale), and the errors travel through the sensitivities of the operations that follow.  Written for the
sequence with EVERY operation rounded, so it admits the fused sequence too (a fused operation drops a rounding, it adds
none); hipcc contracts where it is not told otherwise, and the bound must not depend on that.

    E_g   = rnd(gscale g) + [wd != 0] (rnd(wd p) + rnd(g2))
    E_m   = w1 (E_g + rnd(d)) + 2 rnd(w1 d) + rnd(m')
    E_v   = |g2| (w2 E_g + 2 rnd(a)) + |a| E_g + w2 E_g^2 + rnd(a g2) + rnd(vb) + rnd(v')
    E_s   = dsqrt(v', E_v) + rnd(s)
    E_den = (E_s / c2 + 2 rnd(q)) + rnd(den)
    E_r   = (E_m + |r| E_den) / (den - E_den) + rnd(r)
    E_p   = step E_r + 2 rnd(step r) + rnd(p')

The terms are operand magnitudes, not the result's: with wd != 0, g1 + wd p cancels, E_g stays of the size of
U (|gscale g| + |wd p|) whatever is left of g2, and everything downstream inherits it (|g2| E_g in v': an fp32 emulation
is thousands of ulps of v' off float64 where g2 has cancelled, and within this bound).  ``2 rnd``: the product's rounding
and that of its fp32 factor (w1, w2, c2, step).  dsqrt(v, E) = 1.001 E / (2 sqrt v) where E <= v / 1000 and the rigorous
min(E / sqrt v, sqrt E) elsewhere (|sqrt(v + e) - sqrt v| = |e| / (sqrt(v + e) + sqrt v)).  The quotient's (den - E_den) is
the exact form of the first-order E_den / den; where E_den >= den the bound is infinite (the element is not held; the
cases count such elements and allow none).  Everything is multiplied by SLACK = 1.01 for the remaining second-order
terms -- the constant tests/gemm_contract.py uses for the same purpose, and the only place it enters.

Adamax (``adamax_kernel``): g2 and m' as above; u' = max(fl(u beta2), fl(|g2| + eps)) moves by no more than the larger of
its two arguments' errors, E_u = max(rnd(u beta2), E_g + rnd(|g2| + eps)); r = m' / u' and p' as above with u' for den and
no second bias correction.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149
SLACK = 1.01                    # second-order terms, as in tests/gemm_contract.py
F32 = np.float32
HYPER = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8)
TS = (1, 2, 3, 1000, 100000)
GSCALES = (1.0, 0.125)
DECAYS = (0.0, 0.05)
N_CASE = 4099                   # odd, 3 past a multiple of 4: a float4 sweep has a scalar tail, more than one workgroup
GUARD = 64
KINDS = ('adam', 'adamax')
STORED = {'adam': ('p', 'm', 'v'), 'adamax': ('p', 'm', 'u')}


def hyper32(weight_decay=0.0, gscale=1.0, **kw):
    """the hyper-parameters as ``dv_adam_hyper`` carries them: python floats holding fp32 values"""
    h = dict(HYPER, weight_decay=weight_decay, gscale=gscale)
    h.update(kw)
    return {k: float(F32(v)) for k, v in h.items()}


def consts64(h, t, betas=None):
    """(step, c2, w1, w2, beta2) in float64; ``betas`` = (beta1, beta2) replaces the carried ones (python doubles)"""
    assert t >= 1, 't = 0 is outside the contract'
    b1, b2 = betas if betas is not None else (h['beta1'], h['beta2'])
    return h['lr'] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 - b1, 1.0 - b2, b2


def rnd(x):
    return U * np.abs(x) + ETA


def _dsqrt(v, E):
    s = np.sqrt(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        first = 1.001 * E / (2 * s)
        rig = np.minimum(np.where(s > 0, E / s, np.inf), np.sqrt(E))
    return np.where(E <= v / 1000, first, rig)


def _grad64(p, g, h):
    gs, wd = h['gscale'], h['weight_decay']
    g1 = gs * g
    if wd == 0.0:
        return g1, rnd(g1)
    wp = wd * p
    g2 = g1 + wp
    return g2, rnd(g1) + rnd(wp) + rnd(g2)


def _quot(m1, Em, den, Eden):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(den > 0, m1 / den, 0.0)
        room = den - Eden
        Er = np.where(room > 0, (Em + np.abs(r) * Eden) / room, np.inf) + rnd(r)
    return r, Er


def ref_adam(p, g, m, v, t, h, betas=None):
    """one Adam step in float64 on the fp32 arrays: dict(p, m, v, upd) and the bounds dict(p, m, v)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    step, c2, w1, w2, b2 = consts64(h, t, betas)
    g2, Eg = _grad64(p, g, h)
    d = g2 - m
    m1 = m + w1 * d
    Em = w1 * (Eg + rnd(d)) + 2 * rnd(w1 * d) + rnd(m1)
    a, vb = w2 * g2, v * b2
    v1 = vb + a * g2
    Ev = np.abs(g2) * (w2 * Eg + 2 * rnd(a)) + np.abs(a) * Eg + w2 * Eg * Eg + rnd(a * g2) + rnd(vb) + rnd(v1)
    s = np.sqrt(v1)
    q = s / c2
    den = q + h['eps']
    Eden = (_dsqrt(v1, Ev) + rnd(s)) / c2 + 2 * rnd(q) + rnd(den)
    r, Er = _quot(m1, Em, den, Eden)
    upd = -step * r
    p1 = p + upd
    Ep = step * Er + 2 * rnd(upd) + rnd(p1)
    return dict(p=p1, m=m1, v=v1, upd=upd), dict(p=SLACK * Ep, m=SLACK * Em, v=SLACK * Ev)


def ref_adamax(p, g, m, u, t, h, betas=None):
    """one Adamax step in float64: dict(p, m, u, upd) and the bounds dict(p, m, u)"""
    p, g, m, u = (np.asarray(a, np.float64) for a in (p, g, m, u))
    step, _, w1, _, b2 = consts64(h, t, betas)
    g2, Eg = _grad64(p, g, h)
    d = g2 - m
    m1 = m + w1 * d
    Em = w1 * (Eg + rnd(d)) + 2 * rnd(w1 * d) + rnd(m1)
    ub, ge = u * b2, np.abs(g2) + h['eps']
    u1 = np.maximum(ub, ge)
    Eu = np.maximum(rnd(ub), Eg + rnd(ge))
    r, Er = _quot(m1, Em, u1, Eu)
    upd = -step * r
    p1 = p + upd
    Ep = step * Er + 2 * rnd(upd) + rnd(p1)
    return dict(p=p1, m=m1, u=u1, upd=upd), dict(p=SLACK * Ep, m=SLACK * Em, u=SLACK * Eu)


def reference(kind, p, g, m, v, t, h, betas=None):
    return (ref_adam if kind == 'adam' else ref_adamax)(p, g, m, v, t, h, betas)


# ------------------------------------------------------------------------------------------------ fp32 host emulations
def fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the sum rounds to 53 bits and then to 24 (a double rounding
    that differs from the single one in about one case in 2^29: far below what any check here resolves)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def consts32(h, t):
    step, c2, w1, w2, b2 = consts64(h, t)
    return F32(step), F32(c2), F32(w1), F32(w2), F32(b2)


# FAULTY arithmetic -> the checks (stored quantities) it must fail, and no others: m and v are stored before p is formed
ADAM_FAULTS = {'eps_in_root': {'p'}, 'eps_before_bc2': {'p'}, 'decoupled_decay': {'p', 'm', 'v'},
               'gscale_after_decay': {'p', 'm', 'v'}, 'bias_at_t_minus_1': {'p'}, 'v_from_raw_g': {'p', 'v'},
               'p_from_old_m': {'p'}}
ADAMAX_FAULTS = {'eps_after_max': {'p', 'u'}, 'second_bias_correction': {'p'}}


def emulate(kind, p, g, m, v, t, h, fused, fault=None):
    """the kernels' sequence in fp32 on the host, every operation rounded (``fused`` False) or with the multiply-adds
    fused as the kernel writes them (True).  ``fault``: one of ``ADAM_FAULTS`` / ``ADAMAX_FAULTS``.  Returns dict(p, m, v|u)"""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    mad = fma if fused else (lambda a, b, c: (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32) + np.asarray(c, F32))
    step, c2, w1, w2, b2 = consts32(h, t)
    if fault == 'bias_at_t_minus_1':                  # (t = 1: both corrections are 0, the step size is infinite)
        step, c2 = consts32(h, t - 1)[:2] if t > 1 else (F32(np.inf), F32(0))
    gs, wd, eps = F32(h['gscale']), F32(h['weight_decay']), F32(h['eps'])
    with np.errstate(all='ignore'):
        if fault == 'gscale_after_decay':
            g2 = (mad(wd, p, g) if wd != 0 else g) * gs
        else:
            g2 = g * gs
            if wd != 0 and fault != 'decoupled_decay':
                g2 = mad(wd, p, g2)
        m1 = mad(w1, g2 - m, m)
        if fault == 'decoupled_decay':
            p = p - (F32(h['lr']) * wd) * p
        if kind == 'adam':
            gv = g if fault == 'v_from_raw_g' else g2
            v1 = mad(w2 * gv, gv, v * b2)
            if fault == 'eps_in_root':
                den = np.sqrt(v1 + eps) / c2
            elif fault == 'eps_before_bc2':
                den = (np.sqrt(v1) + eps) / c2
            else:
                den = np.sqrt(v1) / c2 + eps
        else:
            if fault == 'eps_after_max':
                v1 = np.maximum(v * b2, np.abs(g2)) + eps
            else:
                v1 = np.maximum(v * b2, np.abs(g2) + eps)
            den = v1 / c2 if fault == 'second_bias_correction' else v1
        p1 = mad(-step, (m if fault == 'p_from_old_m' else m1) / den, p)
    return {'p': p1.astype(F32), 'm': m1.astype(F32), STORED[kind][2]: v1.astype(F32)}


# ------------------------------------------------------------------------------------------------ case classes
CLASSES = ('normal', 'tiny', 'underflow', 'huge', 'mixed', 'pads', 'warm')


def _logu(rs, n, lo, hi):
    return np.exp(rs.uniform(math.log(lo), math.log(hi), n)) * rs.choice([-1.0, 1.0], n)


def case(cls, n=N_CASE, seed=0):
    """(p, g, m, v) in fp32; v >= 0.  Fixed seeds: the same arrays on every call"""
    rs = np.random.RandomState(1000 * CLASSES.index(cls) + seed + 17)
    z = np.zeros(n)
    if cls == 'normal':           # standard normal parameters and gradients, zero moments
        a = rs.randn(n), rs.randn(n), z, z
    elif cls == 'tiny':           # sqrt(v) of the order of eps
        a = 1e-3 * rs.randn(n), 1e-9 * rs.randn(n), z, z
    elif cls == 'underflow':      # (w2 g) g underflows; only without weight decay
        a = 1e-3 * rs.randn(n), 1e-22 * rs.randn(n), z, z
    elif cls == 'huge':
        a = rs.randn(n), 1e15 * rs.randn(n), z, z
    elif cls == 'mixed':
        g = _logu(rs, n, 1e-30, 1e18)
        g[::7] = 0.0
        a = _logu(rs, n, 1e-30, 1e18), g, _logu(rs, n, 1e-30, 1e18), np.abs(_logu(rs, n, 1e-30, 1e18))
    elif cls == 'pads':
        a = z, z, z, z
    elif cls == 'warm':
        a = rs.randn(n), rs.randn(n), 0.3 * rs.randn(n), 0.5 * rs.randn(n) ** 2 + 1e-3
    else:
        raise KeyError(cls)
    return tuple(np.ascontiguousarray(x, F32) for x in a)


def shrinking(n=N_CASE, seed=0):
    """Adamax: a running max u carried in that decides against the gradient on about half the elements"""
    rs = np.random.RandomState(seed + 991)
    return tuple(np.ascontiguousarray(x, F32) for x in (rs.randn(n), 0.5 * rs.randn(n), 0.3 * rs.randn(n), np.abs(rs.randn(n)) * 0.7))


def settings(cls):
    """every (t, gscale, weight_decay) a class is run at"""
    return [(t, gs, wd) for t in TS for gs in GSCALES for wd in DECAYS if not (cls == 'underflow' and wd != 0.0)]


def cases(kind):
    """(name, arrays) of every class of ``kind``"""
    out = [(c, case(c)) for c in CLASSES]
    if kind == 'adamax':
        out.append(('shrinking', shrinking()))
    return out


# ------------------------------------------------------------------------------------------------ the checks
def excess(got, want, bound):
    """|got - want| / bound per element; 0 where both agree exactly, inf for a non-finite ``got``"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got), r, np.inf)


def distance(got, want, bound):
    """how far ``got`` is from float64, as one number per stored quantity: the root mean square of the error in units of
    the bound, over the elements the bound holds.  (The GEMM contract compares Frobenius norms of the error; an optimiser
    sweep is element-wise and the 'mixed' class spans 48 decades, where a Frobenius norm would be the error of the one
    largest element.  In units of the bound every element counts alike.)"""
    r = excess(got, want, bound)
    r = r[np.isfinite(bound)]
    return float(np.sqrt(np.mean(r * r))) if r.size else 0.0


def verify(kind, got, inputs, t, h, site='', ref=None):
    """hold the stored ``got`` = dict(p, m, v|u) of one step on ``inputs`` = (p, g, m, v|u) to the reference (``ref``: the
    pair ``reference`` returned for the same inputs, if the caller has it).  Returns (set of failed checks, {quantity:
    worst excess}, {quantity: distance}).  A check is named for the stored quantity"""
    want, bound = ref if ref is not None else reference(kind, *inputs, t, h)
    failed, worst, dist = set(), {}, {}
    for k in STORED[kind]:
        assert np.isfinite(bound[k]).all(), '%s: %s has elements the bound does not hold' % (site, k)
        r = excess(got[k], want[k], bound[k])
        worst[k], dist[k] = float(r.max()), distance(got[k], want[k], bound[k])
        if not worst[k] <= 1.0:
            failed.add(k)
    return failed, worst, dist


@functools.lru_cache(maxsize=None)
def case_ref(kind, cls, t, gs, wd):
    """(arrays, hyper-parameters, (reference, bound)) of one class at one setting; computed once, never modified"""
    arrays = dict(cases(kind))[cls]
    h = hyper32(weight_decay=wd, gscale=gs)
    return arrays, h, reference(kind, *arrays, t, h)


@functools.lru_cache(maxsize=None)
def yardstick(kind, cls, t, gs, wd):
    """{quantity: the larger ``distance`` of the two host emulations} on one class at one setting.  The device may be at
    most twice as far from float64 (the rule of the GEMM contract, with ``distance`` for the Frobenius norm)"""
    arrays, h, (want, bound) = case_ref(kind, cls, t, gs, wd)
    runs = [emulate(kind, *arrays, t, h, fused=f) for f in (False, True)]
    return {q: max(distance(r[q], want[q], bound[q]) for r in runs) for q in STORED[kind]}


# ------------------------------------------------------------------------------------------------ the memory frame
def sentinel_m(n):
    """a first moment no update reproduces: 1000 + (i mod 7) against gradients of order 1 -- m' = m + 0.1 (g - m) is
    about 0.9 m, a hundred units away"""
    return (1000.0 + np.arange(n) % 7).astype(F32)


def frame_inputs(n, seed=0):
    """(p, g, m, v) of the memory-contract tests: every element of p, m and v changes in an update (m: the sentinel;
    v = 1000: v' = 999 + 0.001 g^2 with g^2 far below 1000; p: at t = 1 the update is about lr * 9000 / 1000 = 0.0045)"""
    rs = np.random.RandomState(seed + 5 * n + 3)
    return (rs.randn(n).astype(F32), rs.randn(n).astype(F32), sentinel_m(n), np.full(n, 1000.0, F32))


def framed(a, guard=GUARD, lead=0):
    """``a`` cut out of a NaN-filled buffer with ``guard`` elements on both sides (``lead`` more in front: shifts the
    view's alignment).  Returns (buffer, slice of the view)"""
    buf = np.full(lead + guard + a.size + guard, np.nan, F32)
    sl = slice(lead + guard, lead + guard + a.size)
    buf[sl] = a
    return buf, sl


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def memory_faults(before, after, sl):
    """the memory contract on buffers dict(p, g, m, v) -> set of violated checks: 'guards' (an element outside the views,
    or any of g, changed bits), 'written' (an element of p, m or v inside [0, n) kept its bits)"""
    bad = set()
    inside = np.zeros(before['p'].size, bool)
    inside[sl] = True
    for k in before:
        same = bits(before[k]) == bits(after[k])
        if not same[~inside].all() or (k == 'g' and not same.all()):
            bad.add('guards')
        if k != 'g' and same[inside].any():
            bad.add('written')
    return bad


# FAULTY indexing -> the checks it must fail: an element left alone is neither written nor right, a group filled from its
# neighbour is written but wrong, an element past n breaks nothing but the guard
INDEX_FAULTS = {'tail_untouched': {'written', 'p', 'm', 'v'}, 'group_from_neighbour': {'p', 'm', 'v'}, 'past_n': {'guards'}}


def index_fault(name, before, after, sl):
    """FAULTY sweeps, applied to a good emulation's output buffers (copies are returned)"""
    out = {k: a.copy() for k, a in after.items()}
    n, o = sl.stop - sl.start, sl.start
    for k in ('p', 'm', 'v'):
        if name == 'tail_untouched' and n % 4:        # the last n % 4 elements keep what they held
            out[k][o + n - n % 4:o + n] = before[k][o + n - n % 4:o + n]
        elif name == 'group_from_neighbour':          # one group of 4 written with the values of the next
            grp = max(n // 8 - 1, 0) * 4
            out[k][o + grp:o + grp + 4] = after[k][o + grp + 4:o + grp + 8]
        elif name == 'past_n':                        # one element too many
            out[k][o + n] = after[k][o + n - 1]
    return out


# ------------------------------------------------------------------------------------------------ the betas
T_LONG = 200
RHO = 3.0


def long_scale(k):
    """the 200-step run: step k (from 1) sees the gradient ``long_scale(k) * gamma`` for ONE fixed fp32 array gamma, no
    weight decay -- every moment is then a weighted mean of known terms, per element, whatever the parameters do"""
    return 1.0 + (k % 3)


def trajectory_bounds(T, h, gamma, pmax, py=(0.9, 0.999)):
    """How far T steps of the fp32-beta, fp32-arithmetic Adam may end from T steps of a python-beta, fp32-arithmetic Adam
    (torch.optim.Adam) on the gradients s_k gamma, 1 <= s_k <= RHO, weight_decay = 0: element-wise bounds dict(p, m, v) and
    the beta part alone, dict(p, m, v) too.  Derived from the perturbation of the betas and from fp32 rounding, nothing else.

    Betas.  e_i = |d(1 - beta_i)| / (1 - beta_i) (2.4e-7 and 1.29e-5) and l_i = |d log beta_i| (2.6e-8 and 1.29e-8).
    m_t = sum_k w1 b1^(t-k) g_k: every weight moves by at most (e1 + t l1) relatively, and sum_k weights |g_k| <=
    RHO |gamma| bc1_t, so |dm_t| <= (e1 + t l1) RHO |gamma| bc1_t; likewise |dv_t| <= (e2 + t l2) RHO^2 gamma^2 bc2_t.  The
    bias-corrected m^_t and v^_t are weighted MEANS (their weights sum to 1: the factor 1 - beta cancels against the bias
    correction, which is why the 1.29e-5 is not seen in the parameters): a weight moves by at most t l_i relatively, so
    |dm^_t| <= t l1 RHO |gamma| and |dv^_t| / v^_t <= t l2, and with |m^| / sqrt v^ <= RHO the update lr m^ / (sqrt v^ + eps)
    moves by at most lr RHO t (l1 + l2 / 2).  Without weight decay the parameters do not feed back:
    |dp_T| <= lr RHO (l1 + l2 / 2) T (T + 1) / 2.

    Rounding, per party (there are two), first order, worst case.  m: a step rounds d = g - m (<= 2 RHO |gamma| U, weighted
    w1), the product (the same) and the sum (RHO |gamma| U): 1.4 U RHO |gamma| a step, carried with b1: <= 14 U RHO |gamma|
    bc1_t.  v: a step rounds v b2, w2 g (twice into the product), the product and the sum: <= U RHO^2 gamma^2 (2 bc2_t + 3 w2),
    carried with b2 and bc2_t <= t w2: <= U RHO^2 gamma^2 bc2_t (2 t + 3).  The update: the relative error of m^ against
    |gamma| (14 U RHO), half that of v^ (U RHO^2 (2 t + 3) / 2, times |m^| / sqrt v^ <= RHO) and six more roundings (root,
    two quotients, eps, the casts of step and c2; the fma's own goes with p): lr U (20 RHO + RHO^3 (t + 1.5)); and p rounds
    once a step: U pmax.  Summed over t <= T."""
    e = [abs((1 - h[k]) - (1 - b)) / (1 - b) for k, b in (('beta1', py[0]), ('beta2', py[1]))]
    l = [abs(math.log(h[k] / b)) for k, b in (('beta1', py[0]), ('beta2', py[1]))]
    ga = np.abs(np.asarray(gamma, np.float64))
    bc1, bc2 = 1 - py[0] ** T, 1 - py[1] ** T
    lr = h['lr']
    beta = dict(p=np.full(ga.shape, lr * RHO * (l[0] + l[1] / 2) * T * (T + 1) / 2),
                m=(e[0] + T * l[0]) * RHO * ga * bc1, v=(e[1] + T * l[1]) * RHO ** 2 * ga ** 2 * bc2)
    rnd_p = T * U * pmax + lr * U * (20 * RHO * T + RHO ** 3 * (T * (T + 1) / 2 + 1.5 * T))
    both = dict(p=beta['p'] + 2 * rnd_p, m=beta['m'] + 2 * 14 * U * RHO * ga * bc1,
                v=beta['v'] + 2 * U * RHO ** 2 * ga ** 2 * bc2 * (2 * T + 3))
    return {k: SLACK * b for k, b in both.items()}, {k: SLACK * b for k, b in beta.items()}
