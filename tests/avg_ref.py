"""The two options riding on the optimiser sweeps (``dv_adam_hyper.decoupled`` / ``.avg``; drvae_amd/csrc/optim.hip) below model
level: float64 references of ONE sweep with their componentwise bounds, fp32 host emulations of the kernels' operation
sequence and the faulty emulations the CPU file (tests/test_avg_cpu.py) proves the bounds against.  tests/test_gpu_avg.py holds
the device to the same references.  Built on tests/optim_ref.py (its case classes, ``HYPER``, ``TS``, ``GSCALES``, ``DECAYS``,
its ``rnd`` / ``excess`` / ``framed``), which stays as it is.  Plain numpy on the host: no device, no library.

What the ABI carries.  The sweep runs at ONE fp32 rate lr_eff -- ``lr`` itself, or fl32(lr * lr_scale[0]) under learning-rate
annealing -- and ONE fp32 gradient scale -- ``gscale`` itself, or fl32(gscale * coef) in a clipped sweep.  ``effective`` forms
both; every reference below computes in float64 from those fp32 values, as tests/optim_ref.py does from its hyper-parameters.

Decoupled decay (AdamW; torch 2.x ``_single_tensor_adam`` under ``torch.optim.AdamW``).  The kernel's sequence:

    dk = fl(1 - lr_eff wd)   [in double, rounded once]      p0 = fl(p dk)
    g1 = fl(gscale g)        [no wd p term]                 m', v', p' = the coupled sequence on (p0, g1) with wd = 0

so the reference is ``optim_ref.ref_adam`` at weight_decay = 0 started from p0 = p (1 - lr_eff wd) in float64, and the bound is
its bound plus what p0 brings along: one rounding of the product and one of its fp32 factor dk, 2 rnd(p0), which travel into
p' with sensitivity 1 (p' = p0 + update; the update does not read p0).  m and v do not read p at all: their bounds are the
coupled ones at wd = 0.  The same first-order running error analysis, the same SLACK = 1.01 for the second-order terms.

The average.  e' = fma(w, fl(p' - e), e) with w = fl(1 - d), d = avg_decay as the ABI carries it (fp32), w computed in double
and rounded once (for a d in [0.5, 1) the difference is exact in fp32).  The reference is evaluated at the DEVICE's own stored
p' and old e -- whatever error p' carries does not leak in -- so with D = p' - e (float64):

    E_e = w rnd(D) + 2 rnd(w D) + rnd(e')

the subtraction's rounding scaled by w, the product's rounding and that of its fp32 factor w, and the result's rounding: written
with every operation rounded, so it admits the fused form (which drops the product's rounding) too.  A sweep that is not taken
(halted, skipped, a timed-out gate's parked workgroups) leaves e's BITS: no bound, equality.
"""
import numpy as np

from tests import optim_ref as R

F32 = R.F32
AVG_DECAYS = (0.5, 0.9, 0.999)              # d of the average: the edge of exactness, a short and a long memory
LR_SCALE = 0.37                             # an annealing coefficient that is no power of two
CLIP_COEF = 0.5625                          # a clip coefficient < 1

ADAMW_FAULTS = ('coupled_decay', 'decay_after_update', 'decay_with_unannealed_lr', 'decay_scaled_by_clip')
AVG_FAULTS = ('lerp_from_old_p', 'decay_on_wrong_side', 'moved_on_skipped_step', 'tail_untouched')


def effective(h, lr_scale=None, coef=None):
    """the hyper-parameters a sweep RUNS at: lr_eff = fl32(lr * lr_scale) (the product in double), gscale_eff =
    fl32(gscale * coef) (an fp32 product); both None: ``h`` itself"""
    out = dict(h)
    if lr_scale is not None:
        out['lr'] = float(F32(np.float64(F32(h['lr'])) * np.float64(F32(lr_scale))))
    if coef is not None:
        out['gscale'] = float(F32(h['gscale']) * F32(coef))
    return out


def decay64(h):
    """1 - lr_eff wd in float64 from the carried fp32 values"""
    return 1.0 - float(F32(h['lr'])) * float(F32(h['weight_decay']))


def ref_adamw(p, g, m, v, t, h):
    """one AdamW step in float64 at the EFFECTIVE hyper-parameters ``h``: dict(p, m, v, upd) and the bounds dict(p, m, v)"""
    p0 = np.asarray(p, np.float64) * decay64(h)
    want, bound = R.ref_adam(p0, g, m, v, t, dict(h, weight_decay=0.0))
    bound = dict(bound, p=bound['p'] + R.SLACK * 2 * R.rnd(p0))
    return want, bound


def reference(kind, p, g, m, v, t, h):
    """``kind``: 'adam' | 'adamax' (``optim_ref.reference``) | 'adamw'"""
    if kind == 'adamw':
        return ref_adamw(p, g, m, v, t, h)
    return R.reference(kind, p, g, m, v, t, h)


def stored(kind):
    return R.STORED['adamax' if kind == 'adamax' else 'adam']


def ref_avg(e, p_new, d):
    """(e', bound) of the average's move at the stored ``p_new`` and the old ``e``, float64"""
    e, p_new = np.asarray(e, np.float64), np.asarray(p_new, np.float64)
    w = 1.0 - float(F32(d))
    D = p_new - e
    e1 = e + w * D
    return e1, R.SLACK * (w * R.rnd(D) + 2 * R.rnd(w * D) + R.rnd(e1))


# ------------------------------------------------------------------------------------------------ fp32 host emulations
def emulate_adamw(p, g, m, v, t, h, fused, fault=None, lr_scale=None, coef=None):
    """the kernel's AdamW sequence in fp32 (``optim_ref.emulate`` behind the decay) at the BASE hyper-parameters ``h`` with the
    step's ``lr_scale`` / ``coef``; ``fault``: one of ``ADAMW_FAULTS``.  Returns dict(p, m, v)"""
    he = effective(h, lr_scale, coef)
    p = np.asarray(p, F32)
    if fault == 'coupled_decay':
        return R.emulate('adam', p, g, m, v, t, he, fused)
    dk = decay64(he)
    if fault == 'decay_with_unannealed_lr':
        dk = decay64(h)
    if fault == 'decay_scaled_by_clip':
        dk = 1.0 - float(F32(he['lr'])) * float(F32(he['weight_decay'])) * float(F32(1.0 if coef is None else coef))
    dk = F32(dk)
    h0 = dict(he, weight_decay=0.0)
    if fault == 'decay_after_update':
        out = R.emulate('adam', p, g, m, v, t, h0, fused)
        return dict(out, p=(out['p'] * dk).astype(F32))
    return R.emulate('adam', (p * dk).astype(F32), g, m, v, t, h0, fused)


def emulate(kind, p, g, m, v, t, h, fused, lr_scale=None, coef=None):
    if kind == 'adamw':
        return emulate_adamw(p, g, m, v, t, h, fused, lr_scale=lr_scale, coef=coef)
    return R.emulate(kind, p, g, m, v, t, effective(h, lr_scale, coef), fused)


def emulate_avg(e, p_old, p_new, d, fused=True, fault=None, taken=True):
    """the average's move in fp32; ``taken`` False: the sweep returned early.  ``fault``: one of ``AVG_FAULTS``"""
    e, p_old, p_new = (np.asarray(a, F32) for a in (e, p_old, p_new))
    if not taken and fault != 'moved_on_skipped_step':
        return e.copy()
    w = F32(1.0 - float(F32(d)))
    if fault == 'decay_on_wrong_side':                  # e = d p + (1 - d) e
        w = F32(d)
    src = p_old if fault == 'lerp_from_old_p' else p_new
    D = (src - e).astype(F32)
    out = R.fma(w, D, e) if fused else ((w * D).astype(F32) + e).astype(F32)
    if fault == 'tail_untouched' and e.size % 4:
        out[e.size - e.size % 4:] = e[e.size - e.size % 4:]
    return out.astype(F32)


def avg_start(cls, n=R.N_CASE, seed=0):
    """the old average of a case class: the class's parameters moved by a relative amount that no rounding explains (so that
    an average that did not move, or moved toward the wrong point, is seen); zeros stay zeros ('pads')"""
    p = R.case(cls, n, seed)[0].astype(np.float64)
    rs = np.random.RandomState(7000 + R.CLASSES.index(cls) + seed)
    return np.ascontiguousarray(p * (1.0 + 0.25 * rs.randn(n)) + 0.01 * np.abs(p).mean() * rs.randn(n), F32)


def verify_avg(got, e_old, p_new, d, taken=True):
    """hold a stored average to the reference -> (failed?, worst excess).  Not taken: bit equality with the old average"""
    if not taken:
        same = bool((R.bits(np.asarray(got, F32)) == R.bits(np.asarray(e_old, F32))).all())
        return (not same), (0.0 if same else np.inf)
    want, bound = ref_avg(e_old, p_new, d)
    worst = float(R.excess(got, want, bound).max())
    return (not worst <= 1.0), worst


def verify(kind, got, inputs, t, h, site=''):
    """``optim_ref.verify`` for the three kinds: (set of failed checks, {quantity: worst excess})"""
    want, bound = reference(kind, *inputs, t, h)
    failed, worst = set(), {}
    for k in stored(kind):
        assert np.isfinite(bound[k]).all(), '%s: %s has elements the bound does not hold' % (site, k)
        worst[k] = float(R.excess(got[k], want[k], bound[k]).max())
        if not worst[k] <= 1.0:
            failed.add(k)
    return failed, worst
