"""Plain-PyTorch stand-in of ``drvae_amd.kernels.rec_nll_rows`` with the negative-binomial kind (``kind='nb'``: ``v`` =
[mu | theta], ``dpre`` = [d/da_m | d/da_t]) -- the companion of ``tests/kernel_ref.py`` for it, test-only, CPU or GPU tensors.
Every other kind IS the stand-in it wraps, call for call.

The formula is the header's, evaluated in float64 on the fp32 values handed in and rounded once (``tests/nb_ref.py``): the
stand-in states WHAT the launch computes; how the kernel keeps that in fp32 is held to the bound of ``tests/nb_ref.py``."""
import torch

from tests import kernel_ref
from tests import nb_ref

CALLS = {'nb': 0, 'other': 0}


def rec_nll_rows(out, x, v, *, kind, shift=0.0, xidx=None, coef=None, dpre=None):
    if kind != 'nb':
        CALLS['other'] += 1
        return kernel_ref.rec_nll_rows(out, x, v, kind=kind, shift=shift, xidx=xidx, coef=coef, dpre=dpre)
    CALLS['nb'] += 1
    X = x.shape[1]
    assert v.shape[1] == 2 * X
    xs = (x[xidx.long()] if xidx is not None else x).double()
    mu, th = v[:, :X].double(), v[:, X:].double()
    out.copy_(nb_ref.logp64(xs, mu, th).sum(1).to(out.dtype))
    if coef is not None:
        gm, gt, _, _ = nb_ref.grads64(xs, mu, th)
        sm = -torch.expm1(-(mu - nb_ref.ref64.f32(shift)))
        st = -torch.expm1(-(th - nb_ref.ref64.f32(nb_ref.THETA_SHIFT)))
        c = coef.double()[:, None]
        dpre[:, :X] = (c * gm * sm).to(dpre.dtype)
        dpre[:, X:] = (c * gt * st).to(dpre.dtype)


def install(monkeypatch):
    """``kernel_ref.install`` plus this module's ``rec_nll_rows``, for one CPU test (pytest monkeypatch); resets the counts"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    monkeypatch.setattr(K, 'rec_nll_rows', rec_nll_rows)
    for k in CALLS:
        CALLS[k] = 0
