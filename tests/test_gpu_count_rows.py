"""The row loop of ``count_nll_rows_kernel`` (``dv_rec_nll_rows``) on its SECOND trip: the launch caps its grid at 4096
workgroups, so rows beyond 4096 are walked by a workgroup that has already finished one -- a part of the shared walker the
per-family tests (5 to 7 rows) never reach.  4100 decoder rows gathered through a permuting, repeating ``xidx`` from 37 target
rows; X = 8: the 16-byte walk of the two- and three-head kinds, X = 7: the scalar walk; all seven kinds, with ``coef`` and
without.  Rows, and gradients, within the bounds of the float64 references the per-family tests use (``tests/counts_ref.py``,
``tests/nb_ref.py``, ``tests/zinb_ref.py``; plain Poisson and Bernoulli: the formulas and constants of
``tests/test_gpu_numerics.py``), and rows r and r + 4096, given equal inputs, equal bit for bit.  The same cases hold the CPU
stand-in of ``tests/kernel_ref.py`` to the same references (no GPU)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import counts_ref as CR
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests import zinb_ref as Z
from tests.ref64 import bound, f64

M, SRC, WRAP = 4100, 37, 4096
KINDS = [('binary', False), ('poisson', False), ('poisson', True), ('nb', False), ('nb', True), ('zinb', False), ('zinb', True)]
GRADS = {'binary': ('gm',), 'poisson': ('gm',), 'nb': ('gm', 'gt'), 'zinb': ('gm', 'gt', 'gd')}
P_MIN = ref64.f32(1e-10)


def cases(fn):
    fn = pytest.mark.parametrize('kind,library', KINDS, ids=[k + ('_lib' if lib else '') for k, lib in KINDS])(fn)
    return pytest.mark.parametrize('X', [8, 7])(fn)


@functools.lru_cache(None)
def case(kind, X):
    """(target rows, xidx, post-activation heads, coef) on the host; rows 4096.. repeat the inputs of rows 0.."""
    g = torch.Generator().manual_seed(977 * X + len(kind))
    src = torch.poisson(torch.rand(SRC, X, generator=g) * 6)
    src[torch.rand(SRC, X, generator=g) < 0.33] = 0.0
    src[torch.rand(SRC, X, generator=g) < 0.05] = 1500.0
    xidx = (torch.arange(M) * 11 + 5) % SRC
    a = torch.randn(M, len(GRADS[kind]) * X, generator=g) * 3
    if kind == 'binary':
        src, v = (src > 2).float(), torch.sigmoid(a.clamp(-10, 10))
    else:
        v = F.softplus(a) + R.MU_SHIFT
        if kind != 'poisson':
            v[:, X:2 * X] = F.softplus(a[:, X:2 * X]) + R.THETA_SHIFT
        if kind == 'zinb':
            v[:, 2 * X:] = a[:, 2 * X:] * (4.0 / 3.0)           # (the dropout logit: raw)
    coef = torch.randn(M, generator=g)
    for t in (xidx, v, coef):
        t[WRAP:] = t[:M - WRAP]
    return src, xidx.int(), v, coef


@functools.lru_cache(None)
def reference(kind, library, X):
    """rows / rows_bound / g* / g*_bound in float64 from the fp32 values of ``case`` -- computed once per case"""
    src, xidx, v, coef = case(kind, X)
    xs = src[xidx.long()]
    if kind == 'zinb':
        return Z.reference(xs, v[:, :X], v[:, X:2 * X], v[:, 2 * X:], coef=coef, library=library)
    if library:
        return CR.reference(kind, xs, v[:, :X], v[:, X:] if kind == 'nb' else None, coef=coef)
    if kind == 'nb':
        return R.reference(xs, v[:, :X], v[:, X:], coef=coef)
    V, XX, c = f64(v), f64(xs), f64(coef)[:, None]
    if kind == 'poisson':       # (tests/test_gpu_numerics.py::test_rec_nll_poisson_small_rates: C = 16 both ways)
        lgam, xl = torch.lgamma(XX + 1), XX * torch.log(V)
        comps = xl.abs() + V + lgam
        y = V - ref64.f32(R.MU_SHIFT)
        sl = ref64.dact_from_y('softplus', y)
        return dict(rows=(xl - V - lgam).sum(1), rows_bound=bound(16, comps).sum(1) + ref64.row_sum_bound(comps, X),
                    gm=c * (XX / V - 1) * sl,
                    gm_bound=bound(16, c.abs() * (XX / V + 1) * (sl + y.abs() * ref64.dact_from_y_slope('softplus', y))))
    # (tests/test_gpu_numerics.py::test_rec_nll_bernoulli_at_the_clamp: C = 8 for the rows, 4 for the gradient)
    pc = V.clamp(P_MIN, 1.0)
    comps = XX.abs() * (torch.log(pc).abs() + 1) + (1 - XX).abs() * (torch.log1p(-pc).abs() + 1)
    inside = (V > P_MIN) & (V < 1.0)
    return dict(rows=(XX * torch.log(pc) + (1 - XX) * torch.log1p(-pc)).sum(1),
                rows_bound=bound(8, comps).sum(1) + ref64.row_sum_bound(comps, X),
                gm=c * torch.where(inside, XX - V, torch.zeros_like(V)), gm_bound=bound(4, c.abs() * (XX + V)))


def hold(rec_nll_rows, dev, kind, library, X):
    """launch with ``coef`` and without; everything within the bound, the second trip's rows equal to their twins' bits"""
    src, xidx, v, coef = case(kind, X)
    ref = reference(kind, library, X)
    shift = 0.0 if kind == 'binary' else R.MU_SHIFT
    tag = '%s%s X=%d' % (kind, '_lib' if library else '', X)
    for with_coef in (True, False):
        out = torch.full((M,), 7.0, device=dev)
        dpre = torch.full((M, v.shape[1]), 7.0, device=dev) if with_coef else None
        rec_nll_rows(out, src.to(dev), v.to(dev), kind=kind, shift=shift, xidx=xidx.to(dev),
                     coef=coef.to(dev) if with_coef else None, dpre=dpre, library=library)
        out = out.cpu()
        worst = [ref64.check(tag + ' rows', out, ref['rows'], ref['rows_bound'])]
        assert torch.equal(out[WRAP:], out[:M - WRAP])
        if with_coef:
            dpre = dpre.cpu()
            for i, k in enumerate(GRADS[kind]):
                worst.append(ref64.check('%s %s' % (tag, k), dpre[:, i * X:(i + 1) * X], ref[k], ref[k + '_bound']))
            assert torch.equal(dpre[WRAP:], dpre[:M - WRAP])
        print('%s%s, worst |err| / bound: %s' % (tag, '' if with_coef else ', no coef', '  '.join('%.3g' % w for w in worst)))


@pytest.mark.gpu
@cases
def test_rows_beyond_the_grid_cap_within_the_bound_and_bit_equal_to_their_twins(dev, kind, library, X):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    hold(K.rec_nll_rows, dev, kind, library, X)


@cases
def test_the_stand_in_holds_the_same_cases(kind, library, X):
    hold(kernel_ref.rec_nll_rows, torch.device('cpu'), kind, library, X)
