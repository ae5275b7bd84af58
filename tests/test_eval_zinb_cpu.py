"""CPU checks of the zero-inflated kind of ``dv_recon_rows`` (``DV_RECON_ZINB``: the whole-set evaluation of ``type_rec='zinb'``
models in one graph replay): the float64 reference and its bounds (``tests/eval_zinb_ref.py``) against a plain recomputation,
a careful fp32 emulation inside them and six faulty ones outside; the C entry point's refusals through ctypes on the
cross-compiled library (nothing launched: no GPU here); the kind's code beside the frozen table; ``_EvalGraph.get``'s decision
for a host dataset."""
import ctypes as C
import inspect
import warnings

import numpy as np
import pytest
import torch

from tests import eval_counts_ref as ER
from tests import eval_zinb_ref as EZ
from tests import kernel_ref
from tests import ref64
from tests import zinb_ref as Z

SHAPES = ((1, 1), (5, 13), (3, 16), (4, 257), (2, 1028))


def _worst(got, ref, bnd):
    return float(ref64.excess(torch.from_numpy(np.asarray(got, np.float64)), ref, bnd).max())


def _grid_size(x):
    """the size source of the scaled edge grid: small counts with an all-zero row (``tests/test_gpu_eval_counts.py``'s)"""
    rs = np.random.RandomState(5)
    size = torch.from_numpy(rs.poisson(rs.gamma(2.0, 2.0, tuple(x.shape))).astype(np.float32))
    size[0] = 0.0
    return size


# ------------------------------------------------------------------------------------- 1. reference and bounds
@pytest.mark.parametrize('scaled', [False, True])
def test_reference_is_the_plain_float64_formulas_on_the_edge_grid(scaled):
    """``ll`` against log(pi NB0 + (1 - pi) NB) written out with scipy's negative binomial and logaddexp in float64 (no autograd,
    none of the reference's branches); rows / rec are the negative binomial's whatever the logit"""
    import scipy.special as sp
    import scipy.stats as st
    x, mu, th, a, _ = Z.edge_grid(X=256)
    size = _grid_size(x) if scaled else None
    ref = EZ.reference(x, mu, th, a, size)
    xn, tn, an = x.double().numpy(), th.double().numpy(), a.double().numpy()
    r = mu.double().numpy() * (ref['s'].astype(np.float64)[:, None] if scaled else 1.0)
    assert np.array_equal(ref['rec'].numpy(), r)
    # the negative binomial with three lgammas subtracted (scipy's nbinom.logpmf loses whole units at theta = 1e6): float64
    # holds each of them to a few eps of its own size, which is the tolerance -- the point is the formula, not the last digits
    g = (sp.gammaln(xn + tn), sp.gammaln(tn), sp.gammaln(xn + 1))
    tl, xl = -tn * np.log1p(r / tn), np.where(xn > 0, -xn * np.log1p(tn / r), 0.0)
    nb = g[0] - g[1] - g[2] + tl + xl
    lpi, lq = -np.logaddexp(0.0, -an), -np.logaddexp(0.0, an)          # log sigmoid(a), log sigmoid(-a)
    plain = np.where(xn > 0, lq + nb, np.logaddexp(lpi, lq + nb))
    # (logaddexp adds log pi and a log1p that may cancel it: |log pi| counts; the row sum of 256 terms: 8 more on |plain|)
    tol = 8 * np.finfo(np.float64).eps * (sum(np.abs(t) for t in g) + np.abs(tl) + np.abs(xl) + np.abs(lq) + np.abs(lpi)
                                          + 2 * np.abs(plain))
    err = np.abs(ref['ll'].numpy() - plain.sum(1))
    print('reference against the plain formulas: worst %.3g of the float64 tolerance' % float((err / (tol.sum(1) + 1e-300)).max()))
    assert np.all(err <= tol.sum(1)), float((err / (tol.sum(1) + 1e-300)).max())
    assert st is not None
    nbref = ER.reference('nb', x, mu, th, size)
    other = EZ.reference(x, mu, th, torch.zeros_like(a), size)
    for k in ('rows', 'rows_bound', 'rec', 'rec_bound'):
        assert torch.equal(ref[k], nbref[k]) and torch.equal(ref[k], other[k]), k
    assert bool((ref['ll_bound'] > 0).all()) and bool(torch.isfinite(ref['ll']).all())
    assert sp is not None


def test_the_cases_are_zero_heavy_and_cover_the_logits():
    for M, X in SHAPES[1:]:
        for scaled, other in ((False, False), (True, False), (True, True)):
            x, mu, th, a, size = EZ.case(M, X, seed=1, scaled=scaled, other=other)
            assert float((x == 0).double().mean()) >= 1 / 3 and bool((x[0] == 0).all())
            assert set(np.unique(a.numpy())) <= set(np.float32(Z.LOGITS))
            assert (size is x) == (scaled and not other) and (size is None) == (not scaled)
            if M * X >= 64:
                assert len(np.unique(a.numpy())) == len(Z.LOGITS)


@pytest.mark.parametrize('scaled', [False, True])
def test_careful_emulation_is_inside_the_bounds(scaled):
    worst = {}
    for M, X in SHAPES:
        for other in ((False, True) if scaled else (False,)):
            for counts in ('mixed', 'thousands'):
                x, mu, th, a, size = EZ.case(M, X, seed=1, scaled=scaled, other=other, counts=counts)
                ref, em = EZ.reference(x, mu, th, a, size), EZ.emulate(x, mu, th, a, size)
                for key in ('rows', 'll', 'rec'):
                    w = _worst(em[key], ref[key], ref[key + '_bound'])
                    worst[key] = max(worst.get(key, 0.0), w)
                    assert w <= 1.0, (scaled, other, counts, M, X, key, w)
    x, mu, th, a, _ = Z.edge_grid(X=256)
    size = _grid_size(x) if scaled else None
    ref, em = EZ.reference(x, mu, th, a, size), EZ.emulate(x, mu, th, a, size)
    for key in ('rows', 'll', 'rec'):
        w = _worst(em[key], ref[key], ref[key + '_bound'])
        worst['grid ' + key] = w
        assert w <= 1.0, ('grid', scaled, key, w)
    print('zinb%s: careful emulation, worst fraction of the bound %s' % (' scaled' if scaled else '', worst))


def _named_case(name):
    if name == 'grid':
        x, mu, th, a, _ = Z.edge_grid(X=256)
        return x, mu, th, a, None
    if name == 'grid-scaled':
        x, mu, th, a, _ = Z.edge_grid(X=256)
        return x, mu, th, a, _grid_size(x)
    assert name == 'deep'          # (six rows of 257 genes, the size source another matrix ten times as deep as the target)
    return EZ.case(6, 257, seed=2, scaled=True, other=True)


# (fault, the named case, the output it shows in).  'naive_zero' needs the vanishing addend: mu = 1e-6 with theta = 1e6 next
# to a logit of -30 -- the edge grid; the faults that need a depth take the deep size source
FAULT_CASES = [('nb_ll', 'deep', 'll'), ('mixture_mean', 'deep', 'rows'), ('mixture_mean', 'deep', 'rec'),
               ('logit_scaled', 'deep', 'll'), ('swapped', 'deep', 'll'), ('naive_zero', 'grid', 'll'),
               ('ll_unscaled', 'deep', 'll')]


@pytest.mark.parametrize('fault,name,key', FAULT_CASES)
def test_faulty_emulations_are_outside(fault, name, key):
    x, mu, th, a, size = _named_case(name)
    ref = EZ.reference(x, mu, th, a, size)
    good, bad = EZ.emulate(x, mu, th, a, size), EZ.emulate(x, mu, th, a, size, fault=fault)
    for k in ('rows', 'll', 'rec'):
        assert _worst(good[k], ref[k], ref[k + '_bound']) <= 1.0, k
    ex = ref64.excess(torch.from_numpy(np.asarray(bad[key], np.float64)), ref[key], ref[key + '_bound'])
    print('%s on %s: %s outside by %.3g x its bound at worst (%d of %d rows outside)' % (
        fault, name, key, float(ex.max()), int((ex.reshape(len(ex), -1).max(1)[0] > 1).sum()), len(ex)))
    assert float(ex.max()) > 1.0, (fault, name, key, float(ex.max()))


# --------------------------------------------------------------------------------------------- 2. refusals
@pytest.fixture(scope='module')
def lib():
    from drvae_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_point_refusals_without_gpu(lib):
    """kind 4 returns its code before anything is launched (a: an address that is looked at and never dereferenced; M = 0 where
    the call is valid: the checked arguments alone decide)"""
    from drvae_amd import _lib
    a = 0x1000
    call = lambda **kw: lib.dv_recon_rows(C.byref(_lib.ReconRows(**kw)), None)
    ops = dict(x=a, ldx=8, mu=a, ldp=16, rows=a, X=8)
    k = _lib.RECON_ZINB
    # valid forms (no rows: no launch)
    assert call(M=0, kind=k, sd=a, ldt=16, **ops) == 0 and call(M=0, kind=k, sd=a, ldt=24, **ops) == 0
    assert call(M=0, kind=k, sd=a, ldt=16, size_x=a, size_ld=8, rec_out=a, rec_ld=16, **ops) == 0
    assert call(M=0, kind=k, sd=a, ldt=8192, X=4096, x=a, ldx=4096, mu=a, ldp=4096, rows=a) == 0          # (no width limit)
    # [theta | logit] needs 2X columns, at M = 0 too
    assert call(M=0, kind=k, sd=a, ldt=15, **ops) == -1 and call(M=0, kind=k, sd=a, ldt=8, **ops) == -1
    assert call(M=0, kind=k, sd=a, **ops) == -1 and call(M=0, kind=k, **ops) == -1
    assert call(M=4, kind=k, sd=a, ldt=15, **ops) == -1
    # no sd with rows to do
    assert call(M=4, kind=k, ldt=16, **ops) == -1
    # raw-head biases
    assert call(M=0, kind=k, sd=a, ldt=16, bias_mu=a, **ops) == -1
    assert call(M=0, kind=k, sd=a, ldt=16, bias_sd=a, **ops) == -1
    assert call(M=0, kind=k, sd=a, ldt=16, bias_mu=a, bias_sd=a, **ops) == -1
    # rec_out without a size source
    assert call(M=0, kind=k, sd=a, ldt=16, rec_out=a, rec_ld=16, **ops) == -1
    # kind 3's other refusals: missing operands, strides below the width
    assert call(M=4, kind=k, sd=a, ldt=16, X=8) == -1
    assert call(M=4, kind=k, sd=a, ldt=16, X=8, x=a, ldx=4, mu=a, ldp=16, rows=a) == -1
    assert call(M=4, kind=k, sd=a, ldt=16, size_x=a, size_ld=4, **ops) == -1
    assert call(M=4, kind=k, sd=a, ldt=16, size_x=a, size_ld=8, rec_out=a, rec_ld=4, **ops) == -1
    # the unknown kinds from now on
    assert call(M=0, kind=5, sd=a, ldt=16, **ops) == -1 and call(M=0, kind=-1, sd=a, ldt=16, **ops) == -1
    # kinds 1 .. 3 as they were
    for kind in (1, 2, 3):
        assert call(M=0, kind=kind, sd=a, ldt=16, **ops) == 0
    assert call(M=0, kind=3, sd=a, ldt=8, **ops) == 0 and call(M=0, kind=3, sd=a, ldt=7, **ops) == -1


def test_the_kind_has_a_name_of_its_own_beside_the_table():
    from drvae_amd import _lib
    from drvae_amd import engine as E
    assert _lib.RECON_ZINB == 4 and _lib.RECON_KIND == {None: 0, 'binary': 1, 'poisson': 2, 'nb': 3} and _lib.ABI_VERSION == 13
    fam = E.REC_FAMILIES['zinb']
    assert fam.recon_kind == 4 and fam.eval_ll is True and len(fam.heads) == 3
    assert all(f.recon_kind is not None for f in E.REC_FAMILIES.values())
    assert len({f.recon_kind for f in E.REC_FAMILIES.values()}) == len(E.REC_FAMILIES)


def test_the_launcher_keeps_its_parameter_list():
    import drvae_amd.kernels as K
    sig = inspect.signature(K.recon_rows)
    assert list(sig.parameters) == ['rows', 'll', 'x', 'mu', 'sd', 'bias', 'sd_shift', 'kind', 'size_from', 'rec_out']
    kinds = {n: p.kind for n, p in sig.parameters.items()}
    assert all(kinds[n] == inspect.Parameter.POSITIONAL_OR_KEYWORD for n in ('rows', 'll', 'x', 'mu', 'sd'))
    assert all(kinds[n] == inspect.Parameter.KEYWORD_ONLY for n in ('bias', 'sd_shift', 'kind', 'size_from', 'rec_out'))
    assert inspect.signature(kernel_ref.recon_rows) == sig


def test_launcher_refuses_host_tensors_and_wrong_shapes():
    import drvae_amd.kernels as K
    x, mu, th, a, size = EZ.case(3, 8, scaled=True)
    sd = torch.cat([th, a], 1)
    with pytest.raises(RuntimeError, match='no CPU'):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, sd, kind='zinb')
    with pytest.raises(AssertionError):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, th, kind='zinb')              # (theta alone: no logit block)
    with pytest.raises(AssertionError):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, None, kind='zinb')
    with pytest.raises(AssertionError):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, sd, kind='nb')                # ('nb' keeps its (M, X) theta)


# ------------------------------------------------------------------------------------ 3. _EvalGraph.get (host)
@pytest.mark.parametrize('sw', [{}, dict(x_transform='log1p', library_size=True)])
def test_a_host_dataset_keeps_the_step_by_step_path(sw, monkeypatch):
    from drvae_amd import fit as F
    from tests.test_fit import _tiny_model
    kernel_ref.install(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = _tiny_model('drvae', device='cpu', type_rec='zinb', add_noise_var=0.0, **sw)
    ds = Z.zi_dataset('drvae', 24, 2, 'cpu')
    assert F._EvalGraph.get(model, ds) is None
    perf, txt = model.evaluate_performance_on_dataset(ds)
    assert np.isfinite(perf['x1_rmse']) and txt.count('RMSE') == 2 and np.isfinite(perf['x1_ll'])
    assert 'recon_kind is None' not in inspect.getsource(F)
    # the graphs of a kind outside the table ``RECON_KIND`` are kept under a key of their own, and both keys are dropped together
    assert F._EvalGraph.cache(model) is model.__dict__['_eval_graphs_own_kind'] and '_eval_graphs' not in model.__dict__
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        nb = _tiny_model('drvae', device='cpu', type_rec='nb', add_noise_var=0.0)
    assert F._EvalGraph.cache(nb) is nb.__dict__['_eval_graphs'] and '_eval_graphs_own_kind' not in nb.__dict__
    model._create_optimizer()
    assert not any(k in model.__dict__ for k in F._EvalGraph.CACHE_KEYS)
