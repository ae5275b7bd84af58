"""The classifier-head launch (``dv_smalln_linear_fwd`` with a ``dv_ymarg`` and a ``dv_fprop_kl`` argument) below model
level: its cases, a staged float64 reference, and faulty host emulations that show the checks have teeth.  Plain torch on
the host, no library call; ``tests/test_clf_launch_cpu.py`` runs it without a device, ``tests/test_gpu_clf_launch.py``
holds the two kernels of the launch (the generic one and the register-resident one of the train step's common shape) and
the separate launches it replaces to it.

One launch computes, per classifier row r with fprop rows [fp_ptr[r], fp_ptr[r + 1]):

    raw1[t], raw3[t], klfp[t]      the fprop rows' two KL terms with their own free bits
    logits[r], probs[r]            the classifier's dot products, the softmax and the 1e-10 clamp
    yl[r], kld[r], cfp[t], dqy[r]  the y-marginalisation forward and backward
    dq[t], dp[t]                   the backward of the z1 KL term with the coefficients cfp, gated on raw1

The reference is STAGED: each stage takes as exact inputs the fp32 values the previous stage stored (read back from the
launch), so every bound stays componentwise and tight -- the rule of ``tests/ref64.py``, each stage with its C.

Row kinds (every case mixes all three, so fp_ptr is ragged): unlabeled (nf == Y, label == 0), labeled with one slot
(nf == 1, label == class), labeled with all slots (nf == Y, label == -2 - class)."""
import math

import numpy as np
import torch

from tests import kernel_ref
from tests.ref64 import U, bound, check, excess, f32, f64, row_sum_bound

SENTINEL = 7.0
PAD_COLS, PAD_ROWS = 3, 2
P_MIN = f32(1e-10)

# the constants of the same arithmetic elsewhere in the suite (tests/test_gpu_numerics.py)
C_KL = 16       # KL forward and backward: two exps, a division and a sum of four terms per element
C_SOFTMAX = 8   # exp(a - max) on a rounded argument, a sum of Y terms and a division
C_YMARG = 8     # one log per probability, a product, a sum of Y terms (as cat_terms)
C_DOT = 2       # a dot product's terms (one rounding each) and the bias add; the summation itself: row_sum_bound

STAGES = ('logits', 'probs', 'raw1', 'raw3', 'klfp', 'yl', 'kld', 'cfp', 'dqy', 'dq', 'dp')
OUT_2D = ('logits', 'probs', 'dqy', 'dq', 'dp')
OUT_1D = ('yl', 'kld', 'cfp', 'raw1', 'raw3', 'klfp')

# residuals and grids of tests/test_gpu_numerics.py (test_logvar_kl_rows_and_reparam,
# test_softmax_clamp_and_cat_terms_at_the_clamp)
D_VALUES = (0.0, 1e-3, 0.1, 1.0, 10.0)
LOGVAR_GRID = np.arange(-30 * 8, 30 * 8 + 1) / 8.0
CLAMP_LOGITS = np.concatenate([np.linspace(18.0, 28.0, 2001), [math.log(1e10) + e for e in (-1e-6, 0.0, 1e-6)], [0.0, 3.0]])


def route(shape):
    """which kernel the entry point takes for a launch with both riders (rows.hip, dv_smalln_linear_fwd)"""
    M, Y, K1, K2, Z1, Z3 = shape
    return 'fast' if Y <= 2 and K1 + K2 <= 256 and Z1 <= 128 and Z3 <= 128 else 'generic'


def case_id(case):
    return case['name']


# ------------------------------------------------------------------------------------------------------ cases
def _wide(t, junk=1e3):
    """t as a view into a wider buffer whose pad columns hold a value that no result survives"""
    buf = torch.full((t.shape[0], t.shape[1] + PAD_COLS), junk, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


def _plan(M, Y):
    r = torch.arange(M)
    kind = r % 3                                   # 0 unlabeled, 1 labeled with one slot, 2 labeled with all slots
    cls = (5 * r + 1) % Y
    label = torch.where(kind == 1, cls, torch.where(kind == 2, -2 - cls, torch.zeros_like(cls))).to(torch.int32)
    nf = torch.where(kind == 1, torch.ones_like(r), torch.full_like(r, Y))
    fp_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), nf.cumsum(0)]).to(torch.int32)
    return kind, label, fp_ptr


def plan_rows(fp_ptr):
    """owner row and slot index of every fprop row"""
    f0 = fp_ptr[:-1].long()
    nf = (fp_ptr[1:] - fp_ptr[:-1]).long()
    own = torch.repeat_interleave(torch.arange(nf.numel()), nf)
    return own, torch.arange(int(nf.sum())) - f0[own]


def make_case(shape, seed=0, name=None, a1=None, W=None, bias=True, kl=None, need_split=True):
    """one case, deterministically from (M, Y, K1, K2, Z1, Z3): fp32 host tensors -- every matrix a view into a wider
    buffer (``bufs``) --, the prior vector, and the three kl_min settings.  ``a1`` / ``W`` / ``kl`` = (Q, qidx, P, Q3)
    override the random operands (edge cases)."""
    M, Y, K1, K2, Z1, Z3 = shape
    g = torch.Generator().manual_seed(7919 * seed + sum(shape))
    rn = lambda *s: torch.randn(*s, generator=g)              # noqa: E731
    kind, label, fp_ptr = _plan(M, Y)
    own, slot = plan_rows(fp_ptr)
    F_ = own.numel()
    Kt = K1 + K2
    ops = dict(label=label, fp_ptr=fp_ptr, c_kld=rn(M), c_yl=rn(M))
    mats = dict(a1=rn(M, K1) if a1 is None else a1, W=rn(Y, Kt) * (1.5 / math.sqrt(Kt)) if W is None else W)
    if K2:
        mats['a2'] = rn(M, K2)
    ops['bias'] = rn(Y) * 0.5 if bias else None
    if kl is None:
        nq = max(2, (M + 1) // 2)
        qidx = ((3 * own + slot) % nq).to(torch.int32)        # many-to-one, with repeats
        # per-row spreads over 1.5 decades: the raw KL terms of a case cover a wide range (both sides of a free-bits gate)
        spread = lambda: torch.exp(torch.rand(F_, 1, generator=g) * math.log(30.0) + math.log(0.05))   # noqa: E731
        Q = rn(nq, 2 * Z1) * 0.5
        P = Q[qidx.long()] + spread() * rn(F_, 2 * Z1)
        Q3 = spread() * rn(F_, 2 * Z3)
    else:
        Q, qidx, P, Q3 = kl
    mats.update(Q=Q, P=P, Q3=Q3)
    ops['qidx'] = qidx
    bufs = {k: _wide(v.float()) for k, v in mats.items()}
    case = dict(name=name or '%s-%s' % (route(shape), 'x'.join(str(v) for v in shape)), shape=tuple(shape), F=F_, kind=kind,
                ops=ops, bufs=bufs, cols={k: v.shape[1] for k, v in mats.items()},
                prior_scalar=f32(math.log(1.0 / Y)), prior_vector=torch.log_softmax(rn(Y), 0))
    raw1, raw3 = (f64(v) for v in _raw_ref(operands(case))[:2])
    case['kl_min_above'] = f32(2.0 * float(torch.max(raw1.max(), raw3.max())) + 1.0)
    # between the extremes: the midpoint of two neighbouring raw values that leaves most rows on its smaller side, for
    # both terms (fp32-exact, and far from either neighbour on the scale of the rounding of a raw value)
    pooled = torch.sort(torch.cat([raw1, raw3]))[0]
    mids = 0.5 * (pooled[:-1] + pooled[1:])
    best, best_frac = 0.0, -1.0
    for m in mids[torch.linspace(0, mids.numel() - 1, min(mids.numel(), 64)).long()].tolist():
        frac = min(side_fractions(raw1, raw3, m))
        if frac > best_frac:
            best, best_frac = f32(m), frac
    case['kl_min_between'] = best
    if need_split:
        assert min(side_fractions(raw1, raw3, best)) >= 0.25, (case['name'], side_fractions(raw1, raw3, best))
    return case


def side_fractions(raw1, raw3, kl_min):
    """fractions of the fprop rows below and above kl_min, for the z1 and the z3 term"""
    return tuple(float((v < kl_min).double().mean()) if below else float((v > kl_min).double().mean())
                 for v in (raw1, raw3) for below in (True, False))


def kl_min_settings(case):
    return (('0', 0.0), ('above', case['kl_min_above']), ('between', case['kl_min_between']))


def priors(case):
    return (('scalar', case['prior_scalar']), ('vector', case['prior_vector']))


def operands(case, dev=None):
    """the launch's inputs on ``dev`` (host: None): the matrices as views into their wider buffers"""
    o = {}
    for k, buf in case['bufs'].items():
        b = buf if dev is None else buf.to(dev)
        o[k] = b[:, :case['cols'][k]]
    for k, v in case['ops'].items():
        o[k] = v if (dev is None or v is None) else v.to(dev)
    o.setdefault('a2', None)
    return o


def alloc(case, dev=None, klfp=None):
    """every output prefilled with the sentinel, as a view into a larger buffer (pad columns, rows beyond the extent):
    {name: (buffer, view)}.  ``klfp``: its values where it is an input of the launch (no fprop rider)"""
    M, Y, K1, K2, Z1, Z3 = case['shape']
    F_ = case['F']
    dev = dev or torch.device('cpu')
    out = {}
    for k in OUT_2D:
        rows, cols = (M, Y) if k in ('logits', 'probs', 'dqy') else (F_, 2 * Z1)
        buf = torch.full((rows + PAD_ROWS, cols + PAD_COLS), SENTINEL, device=dev)
        out[k] = (buf, buf[:rows, :cols])
    for k in OUT_1D:
        n = M if k in ('yl', 'kld') else F_
        buf = torch.full((n + PAD_COLS,), SENTINEL, device=dev)
        out[k] = (buf, buf[:n])
    if klfp is not None:
        out['klfp'][1].copy_(klfp.to(dev))
    return out


def launch(mod, case, o, out, kl_min, log_prior, fprop=True, logits=True):
    """the fused launch through ``mod`` (drvae_amd.kernels, tests.kernel_ref or a faulty emulation)"""
    M, Y, K1, K2, Z1, Z3 = case['shape']
    v = {k: b[1] for k, b in out.items()}
    ym = (v['yl'], v['kld'], v['cfp'], v['dqy'], o['label'], o['fp_ptr'], v['klfp'], log_prior, o['c_kld'], o['c_yl'])
    kf = dict(Q=o['Q'], qidx=o['qidx'], P=o['P'], Q3=o['Q3'], Z1=Z1, Z3=Z3, kl_min=kl_min, raw1=v['raw1'], raw3=v['raw3'],
              dq=v['dq'], dp=v['dp']) if fprop else None
    mod.smalln_fwd(v['probs'], v['logits'] if logits else None, o['a1'], o['W'], o['bias'], o['a2'], ymarg=ym, fprop_kl=kf)


def launch_separate(mod, case, o, out, kl_min, log_prior):
    """the same results from the separate launches the fused one replaces"""
    M, Y, K1, K2, Z1, Z3 = case['shape']
    v = {k: b[1] for k, b in out.items()}
    Q, P, Q3 = o['Q'], o['P'], o['Q3']
    mod.kl_rows_fwd(v['klfp'], v['raw1'], Q[:, :Z1], Q[:, Z1:], P[:, :Z1], P[:, Z1:], qidx=o['qidx'], free_bits=True,
                    kl_min=kl_min, prior=(0.0, 0.0), second=(Q3[:, :Z3], Q3[:, Z3:], v['raw3']))
    mod.smalln_fwd(v['probs'], v['logits'], o['a1'], o['W'], o['bias'], o['a2'])
    mod.ymarg_fwdbwd(v['yl'], v['kld'], v['cfp'], v['dqy'], v['probs'], o['label'], o['fp_ptr'], v['klfp'], log_prior,
                     o['c_kld'], o['c_yl'])
    mod.kl_rows_bwd(v['dq'][:, :Z1], v['dq'][:, Z1:], v['dp'][:, :Z1], v['dp'][:, Z1:], v['cfp'], v['raw1'], Q[:, :Z1],
                    Q[:, Z1:], P[:, :Z1], P[:, Z1:], qidx=o['qidx'], free_bits=True, kl_min=kl_min)


def to_host(out):
    res = {}
    for k, (b, v) in out.items():
        hb = b.detach().cpu().clone()
        res[k] = (hb, torch.as_strided(hb, v.size(), v.stride(), v.storage_offset()))
    return res


# -------------------------------------------------------------------------------------------------- reference
def _raw_ref(o):
    """float64 raw KL terms of the fprop rows with their bounds, and the z1 term's operands"""
    Z1, Z3 = o['Q'].shape[1] // 2, o['Q3'].shape[1] // 2
    Q, P, Q3 = f64(o['Q'])[o['qidx'].long()], f64(o['P']), f64(o['Q3'])
    mq, sq, mp, sp = Q[:, :Z1], Q[:, Z1:], P[:, :Z1], P[:, Z1:]
    dm, ivp, vq = mq - mp, torch.exp(-sp), torch.exp(sq)
    raw1 = -0.5 * (1 - sp + sq - (dm * dm + vq) * ivp).sum(1)
    c1 = 1 + sp.abs() + sq.abs() + dm * dm * ivp + vq * ivp
    m3, s3 = Q3[:, :Z3], Q3[:, Z3:]
    raw3 = -0.5 * (1 + s3 - (m3 * m3 + torch.exp(s3))).sum(1)
    c3 = 1 + s3.abs() + m3 * m3 + torch.exp(s3)
    b1 = 0.5 * (bound(C_KL, c1).sum(1) + row_sum_bound(c1, Z1))
    b3 = 0.5 * (bound(C_KL, c3).sum(1) + row_sum_bound(c3, Z3))
    return raw1, raw3, b1, b3, (dm, ivp, vq)


def reference(case, stored, kl_min, log_prior, fprop=True):
    """{stage: (ref, bound)} in float64.  ``stored``: the fp32 values a launch stored (host tensors by name); a stage
    reads from it what the stage in front of it produced -- logits for probs, raw1 / raw3 for klfp, probs and klfp for
    the y-marginalisation, cfp and raw1 (the gate) for dq / dp.  A bound of 0 marks a selection: the value is exact."""
    M, Y, K1, K2, Z1, Z3 = case['shape']
    o = operands(case)
    ref = {}
    # logits: C_DOT on the terms and the bias, the summation by row_sum_bound over K1 + K2 terms
    x = f64(torch.cat([o['a1'], o['a2']], 1) if o['a2'] is not None else o['a1'])
    W = f64(o['W'])
    b = f64(o['bias']) if o['bias'] is not None else torch.zeros(Y, dtype=torch.float64)
    comps = x.abs() @ W.abs().t()
    ref['logits'] = (x @ W.t() + b, (math.ceil((K1 + K2) / 256) + 16) * U * comps + bound(C_DOT, comps + b.abs()))
    # probs on the stored logits: C_SOFTMAX
    a = f64(stored['logits'])
    p64 = torch.softmax(a, 1)
    pref = p64.clamp(P_MIN, 1.0)            # (the upper clamp 1 - 1e-10 is 1 in fp32)
    ref['probs'] = (pref, bound(C_SOFTMAX, pref * (Y + (a - a.max(1, keepdim=True)[0]).abs())))
    m = f64(f32(kl_min))
    if fprop:
        # the raw KL terms: C_KL per element and the row sum; klfp on the stored raw terms: one rounding
        raw1, raw3, b1, b3, (dm, ivp, vq) = _raw_ref(o)
        ref['raw1'], ref['raw3'] = (raw1, b1), (raw3, b3)
        t1, t3 = torch.clamp(f64(stored['raw1']), min=m), torch.clamp(f64(stored['raw3']), min=m)
        ref['klfp'] = (t1 + t3, bound(1, t1.abs() + t3.abs()))
    # the y-marginalisation on the stored probabilities and klfp: C_YMARG (selections exact)
    q, klfp = f64(stored['probs']), f64(stored['klfp'])
    ck, cy = f64(o['c_kld']), f64(o['c_yl'])
    lp = f64(log_prior).expand(Y) if torch.is_tensor(log_prior) else torch.full((Y,), f32(log_prior), dtype=torch.float64)
    label, f0 = o['label'].long(), o['fp_ptr'][:-1].long()
    one = (o['fp_ptr'][1:] - o['fp_ptr'][:-1]).long() == 1
    slots = ~one & (label <= -2)
    lab = one | slots
    cls = torch.where(slots, -2 - label, torch.where(one, label, torch.zeros_like(label)))
    j = torch.arange(Y)[None, :]
    kf = klfp[torch.where(one[:, None], f0[:, None].expand(M, Y), f0[:, None] + j).clamp(max=klfp.numel() - 1)]
    lq = torch.log(q)
    pick = lambda t: t.gather(1, cls[:, None])[:, 0]                      # noqa: E731
    zero = torch.zeros(M, dtype=torch.float64)
    yl = torch.where(lab, pick(lq), zero)
    ref['yl'] = (yl, bound(C_YMARG, yl.abs()))
    marg = (q * kf).sum(1) + (-q * (lp - lq)).sum(1)
    marg_c = (q * kf.abs()).sum(1) + (q * (lp.abs() + lq.abs())).sum(1)
    ref['kld'] = (torch.where(one, kf[:, 0], torch.where(slots, pick(kf), marg)), bound(C_YMARG, torch.where(lab, zero, marg_c)))
    oh = (j == cls[:, None]).double()
    dqy_l = oh * (cy[:, None] / q)
    dqy_u = ck[:, None] * (kf + lq - lp + 1)
    dqy_c = torch.where(lab[:, None], dqy_l.abs(), ck.abs()[:, None] * (kf.abs() + lq.abs() + lp.abs() + 1))
    ref['dqy'] = (torch.where(lab[:, None], dqy_l, dqy_u), bound(C_YMARG, dqy_c))
    own, slot = plan_rows(o['fp_ptr'])
    cfp_u = ck[own] * q[own, slot.clamp(max=Y - 1)]
    cfp = torch.where(one[own], ck[own], torch.where(slots[own], ck[own] * (slot == cls[own]).double(), cfp_u))
    ref['cfp'] = (cfp, bound(1, torch.where(lab[own], torch.zeros_like(cfp), cfp_u.abs())))      # (one product)
    if fprop:
        # backward of the z1 term with the stored coefficients, the gate on the stored raw1: C_KL; gate 0: exactly 0
        r1 = f64(stored['raw1'])
        gate = torch.where(r1 > m, 1.0, torch.where(r1 == m, 0.5, 0.0)).double()
        c = (f64(stored['cfp']) * gate)[:, None]
        gmq = dm * ivp
        ref['dq'] = (torch.cat([c * gmq, c * (-0.5 * (1 - vq * ivp))], 1),
                     bound(C_KL, torch.cat([c.abs() * gmq.abs(), 0.5 * c.abs() * (1 + vq * ivp)], 1)))
        ref['dp'] = (torch.cat([-c * gmq, c * (-0.5 * (-1 + (dm * dm + vq) * ivp))], 1),
                     bound(C_KL, torch.cat([c.abs() * gmq.abs(), 0.5 * c.abs() * (1 + (dm * dm + vq) * ivp)], 1)))
    return ref


def verify(case, host, kl_min, log_prior, fprop=True, logits=True, raises=True, site=''):
    """hold what a launch left (``host`` = ``to_host`` of its outputs) to the reference, stage by stage, and to the memory
    contract: {check: worst excess} -- 'pads': 0 if everything outside the outputs' extent still holds the sentinel, 'written':
    0 if every element inside it was written (inf otherwise).  ``raises``: a failed check is an AssertionError naming it"""
    stored = {k: v for k, (_, v) in host.items()}
    ref = reference(case, stored, kl_min, log_prior, fprop)
    skip = set() if fprop else {'raw1', 'raw3', 'dq', 'dp'}
    skip |= set() if logits else {'logits'}
    # (without the stored logits the probabilities have no exact input to be held to: the caller compares them with the launch
    # that stores both)
    no_stage = skip | (set() if logits else {'probs'})
    worst = {}
    untouched, written = True, True
    for k, (buf, view) in host.items():
        outside = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(outside, view.size(), view.stride(), view.storage_offset()).fill_(False)
        untouched &= bool((buf[outside] == SENTINEL).all())
        if k == 'klfp' and not fprop:          # (an input of this launch)
            continue
        if k in skip:                          # (not an output of this launch: nothing of it is written)
            untouched &= bool((view == SENTINEL).all())
        else:
            written &= bool((view != SENTINEL).all())
    worst['pads'] = 0.0 if untouched else math.inf
    worst['written'] = 0.0 if written else math.inf
    if raises:
        assert untouched, '%s pads: an element outside the outputs\' extent lost the sentinel' % site
        assert written, '%s written: an element inside the outputs\' extent still holds the sentinel' % site
    for k in STAGES:
        if k in no_stage or (k == 'klfp' and not fprop):
            continue
        r, b = ref[k]
        if raises:
            worst[k] = check('%s %s' % (site, k), stored[k], r, b)
        else:
            e = excess(stored[k], r, b)
            worst[k] = float(e.max()) if e.numel() else 0.0
    return worst


def selections(case, host, kl_min):
    """the results that are a selection and not arithmetic, as exact statements: the names of those that do not hold"""
    M, Y, K1, K2, Z1, Z3 = case['shape']
    o = operands(case)
    s = {k: v for k, (_, v) in host.items()}
    own, slot = plan_rows(o['fp_ptr'])
    kind, label = case['kind'], o['label'].long()
    cls = torch.where(kind == 2, -2 - label, label)
    bad = []
    labeled = (kind != 0)[own]
    hit = (kind[own] == 1) | (slot == cls[own])
    if not torch.equal(s['cfp'][labeled & hit], o['c_kld'][own][labeled & hit]):
        bad.append('cfp of labeled rows equals c_kld')
    if not bool((s['cfp'][labeled & ~hit] == 0.0).all()):
        bad.append('cfp is 0 in the other slots of a labeled-slot row')
    off = (torch.arange(Y)[None, :] != cls[:, None]) & (kind != 0)[:, None]
    if not bool((s['dqy'][off] == 0.0).all()):
        bad.append('dqy is zero off the label')
    if not bool((s['yl'][kind == 0] == 0.0).all()):
        bad.append('yl is zero on unlabeled rows')
    f0 = o['fp_ptr'][:-1].long()
    if not torch.equal(s['kld'][kind != 0], s['klfp'][(f0 + torch.where(kind == 2, cls, torch.zeros_like(cls)))[kind != 0]]):
        bad.append('kld of labeled rows is the klfp of their slot')
    closed = s['raw1'] < f32(kl_min)
    if not (bool((s['dq'][closed] == 0.0).all()) and bool((s['dp'][closed] == 0.0).all())):
        bad.append('gate-0 rows of dq and dp equal 0.0')
    return bad


# ----------------------------------------------------------------------------------------------------- faults
class Faulty:
    """the fused launch on the host in fp32 -- the sequence of ``kernel_ref.smalln_fwd(ymarg=, fprop_kl=)`` -- with ONE
    defect (``fault`` None: none, bitwise that sequence)"""

    def __init__(self, fault=None):
        self.fault = fault

    def smalln_fwd(self, probs, logits, a1, W, bias=None, a2=None, ymarg=None, park=None, fprop_kl=None):
        R, fault, f = kernel_ref, self.fault, fprop_kl
        yl, kld, cfp, dqy, label, fp_ptr, klfp, log_prior, c_kld, c_yl = ymarg
        Z1, Z3, m = f['Z1'], f['Z3'], f['kl_min']
        Y = W.shape[0]
        own, slot = plan_rows(fp_ptr)
        F_ = own.numel()
        rows = slot < 2 if fault == 'nf_clamped_to_2' else torch.ones(F_, dtype=torch.bool)
        w1, w3 = (min(Z1, 64), min(Z3, 64)) if fault == 'columns_from_64_dropped' else (Z1, Z3)
        Q, P, Q3, qidx = f['Q'], f['P'], f['Q3'], f['qidx']
        t_kl, t_r1, t_r3 = torch.empty(F_), torch.empty(F_), torch.empty(F_)
        R.kl_rows_fwd(t_kl, t_r1, Q[:, :w1], Q[:, Z1:Z1 + w1], P[:, :w1], P[:, Z1:Z1 + w1], qidx=qidx, free_bits=True,
                      kl_min=m, prior=(0.0, 0.0), second=(Q3[:, :w3], Q3[:, Z3:Z3 + w3], t_r3))
        for dst, src in ((klfp, t_kl), (f['raw1'], t_r1), (f['raw3'], t_r3)):
            dst[rows] = src[rows]
        R.smalln_fwd(probs, logits, a1, W, bias, a2)
        lp = 0.0 if (fault == 'prior_vector_ignored' and torch.is_tensor(log_prior)) else log_prior
        R.ymarg_fwdbwd(yl, kld, cfp, dqy, probs, label, fp_ptr, klfp, lp, c_kld, c_yl)
        if fault == 'slot_row_reads_first_slot':
            nf = (fp_ptr[1:] - fp_ptr[:-1]).long()
            s = (nf != 1) & (label.long() <= -2)
            kld[s] = klfp[fp_ptr[:-1].long()[s]]
        src = klfp if fault == 'gate_from_klfp' else f['raw1']
        tie = 1.0 if fault == 'tie_weighted_1' else 0.5
        gate = torch.where(src > m, torch.ones(F_), torch.where(src == m, torch.full((F_,), tie), torch.zeros(F_)))
        g = [torch.empty(F_, Z1) for _ in range(4)]
        R.kl_rows_bwd(g[0], g[1], g[2], g[3], cfp * gate, f['raw1'], Q[:, :Z1], Q[:, Z1:], P[:, :Z1], P[:, Z1:], qidx=qidx,
                      free_bits=False)
        if fault == 'dp_mean_with_the_sign_of_dq':
            g[2] = -g[2]
        for dst, (gm, gs) in ((f['dq'], g[:2]), (f['dp'], g[2:])):
            v = torch.cat([gm, gs], 1)
            keep = torch.zeros(F_, 2 * Z1, dtype=torch.bool)
            keep[:, :w1] = True
            keep[:, Z1:Z1 + w1] = True
            keep &= rows[:, None]
            dst[keep] = v[keep]
        if fault == 'pad_column_written':
            d = f['dq']
            torch.as_strided(d, (F_, 2 * Z1 + 1), d.stride(), d.storage_offset())[:, -1] = 0.0


# fault -> the check meant to catch it
FAULTS = {
    'tie_weighted_1': 'dq',
    'gate_from_klfp': 'dq',
    'dp_mean_with_the_sign_of_dq': 'dp',
    'columns_from_64_dropped': 'raw1',
    'nf_clamped_to_2': 'written',
    'slot_row_reads_first_slot': 'kld',
    'prior_vector_ignored': 'kld',
    'pad_column_written': 'pads',
}


# ------------------------------------------------------------------------------------------------ the cases
SHAPES = (
    (9, 2, 5, 5, 5, 4),                   # fast: the goldens' size
    (37, 2, 100, 100, 100, 100),          # fast: cfg 2's widths, the second lane chunk partly full
    (6, 2, 33, 32, 65, 63),               # fast: one element into the second chunk; Z3 one short of it
    (6, 2, 128, 128, 128, 128),           # fast: the last lane of the last chunk, on every limit at once
    (6, 2, 129, 128, 128, 128),           # generic: one past each limit, one limit at a time
    (6, 2, 128, 128, 129, 128),
    (6, 2, 128, 128, 128, 129),
    (21, 3, 100, 0, 100, 37),             # generic: single input (VFAE form), three classes
    (10, 8, 200, 200, 200, 200),          # generic: kMaxSmallN fprop rows per unlabeled row; cfg 5's widths
)
CASES = tuple(make_case(s, seed=i) for i, s in enumerate(SHAPES))


def _grid_rows(values, rows, cols):
    return torch.from_numpy(np.resize(np.asarray(values, dtype=np.float64), rows * cols).astype(np.float32)).reshape(rows, cols)


def _logvar_case(Z1, Z3, name):
    """both log-variances of the z1 term over [-30, 30] against each other, the z3 term's over the same grid, mean
    residuals D_VALUES: the grid of test_logvar_kl_rows_and_reparam laid out over the fprop rows of a 15-row plan"""
    shape = (15, 2, 5, 0, Z1, Z3)
    F_ = int(_plan(15, 2)[2][-1])
    rng = np.random.default_rng(7)
    sq = np.repeat(LOGVAR_GRID, len(D_VALUES))
    sp = rng.permutation(sq)
    dm = np.tile(np.asarray(D_VALUES), LOGVAR_GRID.size)
    mp = _grid_rows(np.round(rng.uniform(-2, 2, F_ * Z1) * 1024) / 1024, F_, Z1)
    Q = torch.cat([mp + _grid_rows(dm, F_, Z1), _grid_rows(sq, F_, Z1)], 1)
    P = torch.cat([mp, _grid_rows(sp, F_, Z1)], 1)
    Q3 = torch.cat([_grid_rows(dm, F_, Z3), _grid_rows(sp, F_, Z3)], 1)
    qidx = torch.arange(F_, dtype=torch.int32)
    return make_case(shape, seed=11, name=name, kl=(Q, qidx, P, Q3), need_split=False)


def _clamp_case(Y, name):
    """classifier probabilities on both sides of the 1e-10 clamp: K1 = Y, W = I and no bias, so the chosen logits reach the
    softmax exactly (a sum with one non-zero product is exact); the grid of test_softmax_clamp_and_cat_terms_at_the_clamp"""
    L = CLAMP_LOGITS
    lg = np.zeros((L.size, Y), np.float32)
    lg[:, 1:] = -L[:, None]
    lg[:, Y - 1] -= 0.5 * (Y - 2)
    return make_case((L.size, Y, Y, 0, 5, 4), seed=12, name=name, a1=torch.from_numpy(lg), W=torch.eye(Y), bias=False,
                     need_split=False)


EDGE_CASES = (_logvar_case(100, 100, 'edge-logvar-fast'), _logvar_case(129, 100, 'edge-logvar-generic'),
              _clamp_case(2, 'edge-clamp-fast'), _clamp_case(3, 'edge-clamp-generic'))
