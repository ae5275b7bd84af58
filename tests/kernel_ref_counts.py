"""Plain-PyTorch stand-ins of the two launchers the raw-count inputs extend -- ``drvae_amd.kernels.batch_feed`` with its split
form (``xt`` / ``transform``) and ``rec_nll_rows`` with ``library=True`` -- the companion of ``tests/kernel_ref.py`` /
``tests/kernel_ref_nb.py`` for them, test-only, CPU or GPU tensors.  Without the new keywords every call IS the stand-in it
wraps, call for call.

The formulas are the header's: the feed writes the raw rows to ``xt`` and T(x) + sigma * noise to ``xin`` (fp32, like the
wrapped stand-in); the library rows are evaluated in float64 on the fp32 values handed in and rounded once
(``tests/counts_ref.py``), with the size factor the fp32 quotient the kernel forms."""
import torch

from tests import counts_ref as CR
from tests import kernel_ref
from tests import kernel_ref_nb
from tests import nb_ref

CALLS = {'split_feed': 0, 'plain_feed': 0, 'lib_rows': 0, 'plain_rows': 0}
INNER = {'feed': kernel_ref.batch_feed}      # the feed stand-in this module's wraps (``install(riders=True)``: the annealed one)


def batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, *, xt=None, transform=None, noise=None, sigma=0.0, **kw):
    if xt is None:
        assert transform is None
        CALLS['plain_feed'] += 1
        return INNER['feed'](xin, x1, x2, y32, table, n_batches, ctr, base, noise=noise, sigma=sigma, **kw)
    CALLS['split_feed'] += 1
    assert transform in (None, 'log1p') and tuple(xt.shape) == tuple(xin.shape)
    INNER['feed'](xt, x1, x2, y32, table, n_batches, ctr, base, **kw)        # the gather (and labels, masks, park)
    t = torch.log1p(xt) if transform == 'log1p' else xt
    xin.copy_(t + sigma * noise if noise is not None else t)


def rec_nll_rows(out, x, v, *, kind, library=False, **kw):
    if not library:
        CALLS['plain_rows'] += 1
        return kernel_ref_nb.rec_nll_rows(out, x, v, kind=kind, **kw)
    CALLS['lib_rows'] += 1
    assert kind in ('poisson', 'nb')
    shift, xidx, coef, dpre = kw.get('shift', 0.0), kw.get('xidx'), kw.get('coef'), kw.get('dpre')
    X = x.shape[1]
    xs = x[xidx.long()] if xidx is not None else x
    ref = CR.reference(kind, xs, v[:, :X], v[:, X:] if kind == 'nb' else None, coef=coef, shift=shift)
    out.copy_(ref['rows'].to(out.dtype))
    if coef is not None:
        dpre[:, :X] = ref['gm'].to(dpre.dtype)
        if kind == 'nb':
            dpre[:, X:] = ref['gt'].to(dpre.dtype)


def install(monkeypatch, riders=False):
    """``kernel_ref_nb.install`` plus this module's two stand-ins, for one CPU test (pytest monkeypatch); resets the counts.
    ``riders``: on top of the stand-ins of dropout, clipping, annealing and the parameter average (``kernel_ref_avg.install``
    and ``kernel_ref_dropout``'s launchers) -- the feed this module's wraps is then the annealed one"""
    import drvae_amd.kernels as K
    if riders:
        from tests import kernel_ref_avg, kernel_ref_dropout
        kernel_ref_avg.install(monkeypatch)
        for name in kernel_ref_dropout.FUNCTIONS:
            monkeypatch.setattr(K, name, getattr(kernel_ref_dropout, name))
    else:
        kernel_ref_nb.install(monkeypatch)
    install_over(monkeypatch)


def install_over(monkeypatch):
    """this module's two stand-ins over whatever set of stand-ins is installed now (its feed is the one wrapped); resets the counts"""
    import drvae_amd.kernels as K
    if K.batch_feed is not batch_feed:
        monkeypatch.setitem(INNER, 'feed', K.batch_feed)
    monkeypatch.setattr(K, 'batch_feed', batch_feed)
    monkeypatch.setattr(K, 'rec_nll_rows', rec_nll_rows)
    for k in CALLS:
        CALLS[k] = 0


assert nb_ref.MU_SHIFT == 1e-6
