"""Plain-PyTorch stand-ins of the optimiser sweeps with the two options the parameter-averaging work adds
(``drvae_amd.kernels.adam_l2`` / ``adamax_l2`` / ``adam_l2_clip`` / ``adamax_l2_clip`` with ``decoupled``, ``avg``,
``avg_decay``): same names, same signatures, same output tensors -- the companion of ``tests/kernel_ref_anneal.py`` (which they
wrap, and through it ``kernel_ref`` / ``kernel_ref_clip``), test-only, CPU or GPU tensors.  Without the new arguments every
stand-in IS the one it wraps, call for call.

A sweep is TAKEN unless a halt word is set (behind the gate's wait, where there is one) or the clip record says skip; a sweep
that is not taken touches nothing, the average included.  Decoupled decay: p *= fl32(1 - lr_eff wd) first (the factor in double
from the fp32 rate the sweep runs at), then the wrapped sweep at weight_decay = 0.  The average: e += fl32(1 - avg_decay)
(p_new - e) behind the wrapped sweep."""
import numpy as np
import torch

from tests import kernel_ref
from tests import kernel_ref_anneal as KA

CALLS = {'decoupled_sweeps': 0, 'averaged_sweeps': 0}
FAULT = {'name': None}          # tests only: 'moved_on_skipped_step' makes the stand-in wrong on purpose


def _taken(kw, state):
    gate = kw.get('gate')
    if gate is not None:
        kernel_ref.flag_wait(gate[0], gate[1], gate[3], gate[2])      # (what the wrapped sweep does first: idempotent)
    if kernel_ref._halted(kw.get('halt')):
        return False
    if state is not None:
        import drvae_amd.kernels as K
        if int(K.clip_record(state)[2]):
            return False
    return True


def _extended(fn, args, kw, state=None, adamax=False):
    decoupled, avg, avg_decay = kw.pop('decoupled', False), kw.pop('avg', None), kw.pop('avg_decay', None)
    if not decoupled and avg is None:
        return fn(*args, **kw)
    if decoupled and adamax:
        raise RuntimeError('drvae_amd: dv_adamax_l2 failed: invalid argument (-1)')       # (as ``_lib.check`` raises)
    if avg is not None:
        if avg_decay is None:
            raise ValueError('an average needs its avg_decay')
        if not 0.0 < float(np.float32(avg_decay)) < 1.0:
            raise RuntimeError('drvae_amd: dv_adam_l2 failed: invalid argument (-1)')
    p = args[0]
    taken = _taken(kw, state)
    if decoupled:
        CALLS['decoupled_sweeps'] += 1
        if taken:
            lr = KA.lr_effective(kw['lr'], kw['lr_scale']) if kw.get('lr_scale') is not None else float(np.float32(kw['lr']))
            dk = np.float32(1.0 - np.float64(np.float32(lr)) * np.float64(np.float32(kw.get('weight_decay', 0.0))))
            p.mul_(float(dk))
        kw = dict(kw, weight_decay=0.0)
    out = fn(*args, **kw)
    if avg is not None:
        CALLS['averaged_sweeps'] += 1
        assert avg.shape == p.shape
        if taken or FAULT['name'] == 'moved_on_skipped_step':
            avg.add_((p - avg) * float(np.float32(1.0 - np.float64(np.float32(avg_decay)))))
    return out


def adam_l2(*a, **kw):
    return _extended(KA.adam_l2, a, kw)


def adamax_l2(*a, **kw):
    return _extended(KA.adamax_l2, a, kw, adamax=True)


def adam_l2_clip(*a, **kw):
    return _extended(KA.adam_l2_clip, a, kw, state=a[4])


def adamax_l2_clip(*a, **kw):
    return _extended(KA.adamax_l2_clip, a, kw, state=a[4], adamax=True)


FUNCTIONS = ['adam_l2', 'adamax_l2', 'adam_l2_clip', 'adamax_l2_clip']


def install(monkeypatch):
    """``kernel_ref_anneal.install`` plus the launchers of this module, for one CPU test (pytest monkeypatch); resets the
    call counts"""
    import drvae_amd.kernels as K
    KA.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
    for name in CALLS:
        CALLS[name] = 0
    FAULT['name'] = None
