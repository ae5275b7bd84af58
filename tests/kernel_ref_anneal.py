"""Plain-PyTorch stand-ins of the launchers the annealing schedules extend (``drvae_amd.kernels.batch_masks`` / ``batch_feed``
with their ``anneal`` argument, the four optimiser sweeps with ``lr_scale``): same names, same signatures, same output
tensors -- the companion of ``tests/kernel_ref.py`` / ``tests/kernel_ref_clip.py`` for these, test-only, CPU or GPU tensors.
Without the new arguments every stand-in IS the one it wraps, call for call.

The schedule record is evaluated the way ``dv_batch_masks`` does: in double from the integer step counter and the integer
schedule parameters, one rounding to fp32 per coefficient (``record``); ``record_fp32`` is the deliberately WRONG emulation
(every operation in fp32) the tests show their check to catch."""
import numpy as np
import torch

from tests import kernel_ref
from tests import kernel_ref_clip

CALLS = {'batch_masks': 0, 'batch_feed': 0, 'lr_scaled_sweeps': 0}


def _coef64(it, itermax, offset):
    if itermax <= 0:
        return 1.0
    d = it - offset
    if d <= 0:
        return 0.01
    return min(1.0, 0.01 + float(d) / float(itermax))


def record(it, pert, kl, yl, lr):
    """{beta_pert, beta_kl, beta_yr, lr_scale} as fp32: ``pert`` / ``yl`` = (itermax, offset), ``kl`` / ``lr`` = itermax; an
    itermax <= 0 switches that schedule off (value 1)"""
    lr_s = max(0.01, 1.0 - _coef64(it, lr, 0)) if lr > 0 else 1.0
    return np.array([np.float32(_coef64(it, pert[0], pert[1])), np.float32(_coef64(it, kl, 0)),
                     np.float32(_coef64(it, yl[0], yl[1])), np.float32(lr_s)], np.float32)


def _coef32(it, itermax, offset):
    f = np.float32
    if itermax <= 0:
        return f(1.0)
    d = it - offset
    if d <= 0:
        return f(0.01)
    return min(f(1.0), f(f(0.01) + f(f(d) / f(itermax))))


def record_fp32(it, pert, kl, yl, lr):
    """FAULTY on purpose: the same record with every operation rounded to fp32 (what a kernel evaluating the schedule in
    single precision would store)"""
    f = np.float32
    lr_s = max(f(0.01), f(f(1.0) - _coef32(it, lr, 0))) if lr > 0 else f(1.0)
    return np.array([_coef32(it, pert[0], pert[1]), _coef32(it, kl, 0), _coef32(it, yl[0], yl[1]), lr_s], np.float32)


def _apply_schedule(B, L, an, m, rec):
    """what the extended launch does behind the plain masks: the record, beta_kl / beta_yr folded into the coefficients, the
    copies without beta_kl, the ELBO / CMPL weights (fp32 arithmetic on the fp32 record, like the kernel)"""
    dev = m['c_nll'].device
    r = torch.from_numpy(rec).to(dev)
    an['sched'].copy_(r)
    b_kl, b_yr = r[1], r[2]
    if m.get('c_klz2') is not None and m.get('hx') is not None:
        if an.get('w_klz2') is not None:
            an['w_klz2'].copy_(m['c_klz2'])
        m['c_klz2'].mul_(b_kl)
    if m.get('c_klp') is not None:
        if an.get('w_klp') is not None:
            an['w_klp'].copy_(m['c_klp'])
        m['c_klp'].mul_(b_kl)
    if m.get('hy') is not None:
        m['c_yl'].mul_(b_yr)
    if an.get('c_kld') is not None:
        c_tot = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(L), dtype=torch.float32) * torch.tensor(m['n_tot'], dtype=torch.float32))
        an['c_kld'][:L * B] = (b_kl.cpu() * c_tot).to(dev)
    has_pert, has_y = m.get('hx') is not None, m.get('hy') is not None
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    an['w_elbo'][:3] = torch.stack([f(1.0), -r[1].cpu(), r[0].cpu() * f(m['pert_rate']) if has_pert else f(0.0)]).to(dev)
    w = torch.zeros(8)
    w[3] = -(r[2].cpu() * f(m['yl_rate'])) if has_y else 0.0
    mmd = float(an.get('mmd_rate', 0.0))
    w[4] = -np.float32(mmd) if mmd != 0.0 else 0.0
    w[5] = -1.0
    an['w_cmpl'][:8] = w.to(dev)


def _record_of(an):
    return record(int(an['step'].reshape(-1)[0]), an['pert'], an['kl'], an['yl'], an['lr'])


def batch_masks(B, L, *, anneal=None, **m):
    CALLS['batch_masks'] += 1
    if anneal is None:
        return kernel_ref.batch_masks(B, L, **m)
    rec = _record_of(anneal)
    beta = torch.from_numpy(rec[0:1].copy()).to(m['c_nll'].device)       # the launch's OWN beta_pert: ``beta`` is not read
    if m.get('gcounts') is not None:      # (an explicit batch's one pair of global counts: the wrapped stand-in indexes rows)
        m = dict(m, gcounts=m['gcounts'].reshape(-1, 2))
    kernel_ref.batch_masks(B, L, **dict(m, beta=beta))
    _apply_schedule(B, L, anneal, m, rec)


def batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, *, masks=None, **kw):
    CALLS['batch_feed'] += 1
    if masks is None or masks.get('anneal') is None:
        return kernel_ref.batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, masks=masks, **kw)
    m = {k: v for k, v in masks.items() if k != 'anneal'}
    an = masks['anneal']
    rec = _record_of(an)
    m['beta'] = torch.from_numpy(rec[0:1].copy()).to(xin.device)
    kernel_ref.batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, masks=m, **kw)
    _apply_schedule(table.shape[1], kw.get('L', 1), an, m, rec)


def lr_effective(lr, lr_scale):
    """the rate a sweep with ``lr_scale`` runs at: (float)((double)lr * (double)lr_scale[0]) of the fp32 ``lr`` it is handed"""
    return float(np.float32(np.float64(np.float32(lr)) * np.float64(np.float32(float(lr_scale.reshape(-1)[0])))))


def _scaled(fn, args, kw):
    ls = kw.pop('lr_scale', None)
    if ls is not None:
        CALLS['lr_scaled_sweeps'] += 1
        kw['lr'] = lr_effective(kw['lr'], ls)
    return fn(*args, **kw)


def adam_l2(*a, **kw):
    return _scaled(kernel_ref.adam_l2, a, kw)


def adamax_l2(*a, **kw):
    return _scaled(kernel_ref.adamax_l2, a, kw)


def adam_l2_clip(*a, **kw):
    return _scaled(kernel_ref_clip.adam_l2_clip, a, kw)


def adamax_l2_clip(*a, **kw):
    return _scaled(kernel_ref_clip.adamax_l2_clip, a, kw)


FUNCTIONS = ['batch_masks', 'batch_feed', 'adam_l2', 'adamax_l2', 'adam_l2_clip', 'adamax_l2_clip']


def install(monkeypatch):
    """``kernel_ref_clip.install`` (which is ``kernel_ref.install`` plus the clipped launchers) plus the launchers of this
    module, for one CPU test (pytest monkeypatch); resets the call counts"""
    import drvae_amd.kernels as K
    kernel_ref_clip.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
    for name in CALLS:
        CALLS[name] = 0
