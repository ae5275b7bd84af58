"""CPU checks of the count kinds of ``dv_recon_rows`` (the whole-set evaluation of the count decoders in one graph replay):
the float64 reference and its bounds (``tests/eval_counts_ref.py``) hold a careful fp32 emulation and catch five faulty
ones by at least 10 x; the C entry point's refusals through ctypes on the cross-compiled library (no launch: no GPU here);
the CPU stand-in of the new keywords; ``_EvalGraph.get``'s decision for a host dataset."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import eval_counts_ref as ER
from tests import kernel_ref
from tests import ref64

SHAPES = ((1, 1), (5, 13), (3, 16), (4, 257), (2, 1028))


def _worst(got, ref, bnd):
    return float(ref64.excess(torch.from_numpy(np.asarray(got, np.float64)), ref, bnd).max())


def _sources(scaled):
    return (False, True) if scaled else (False,)


# ------------------------------------------------------------------------------------- 1. reference and bounds
def test_reference_is_the_plain_float64_formulas():
    """the reference against scipy's distributions and numpy's moments on a small case; the size factor of an all-zero row
    is 1 / X and ``rec`` = s * v"""
    import scipy.stats as st
    x, mu, th, size = ER.case('nb', 5, 13, scaled=True, other=True)
    ref = ER.reference('nb', x, mu, th, size)
    s = np.maximum(size.double().numpy().sum(1), 1.0) / 13
    assert s[0] == 1.0 / 13 and np.allclose(ref['s'], s, rtol=1e-7)
    r = ref['s'].astype(np.float64)[:, None] * mu.double().numpy()      # (the fp32 quotient is data of the reference)
    assert np.array_equal(ref['rec'].numpy(), r)
    xn, tn = x.double().numpy(), th.double().numpy()
    ll = st.nbinom.logpmf(xn, tn, tn / (tn + r)).sum(1)
    assert np.allclose(ref['ll'].numpy(), ll, rtol=1e-9, atol=1e-9)
    rows = ref['rows'].numpy()
    assert np.allclose(rows[:, 0], ((xn - r) ** 2).sum(1), rtol=1e-12)
    assert np.allclose(rows[:, 1], xn.mean(1)) and np.allclose(rows[:, 2], r.mean(1), rtol=1e-12)
    assert np.allclose(rows[:, 3], xn.var(1) * 13, rtol=1e-10, atol=1e-9) and np.allclose(rows[:, 4], r.var(1) * 13, rtol=1e-10)
    assert np.allclose(rows[:, 5], ((xn - xn.mean(1, keepdims=True)) * (r - r.mean(1, keepdims=True))).sum(1), rtol=1e-10)
    x, mu, _, size = ER.case('poisson', 4, 16, scaled=True)
    ref = ER.reference('poisson', x, mu, None, size)
    assert np.allclose(ref['ll'].numpy(), st.poisson.logpmf(x.double().numpy(), ref['rec'].numpy()).sum(1), rtol=1e-9, atol=1e-9)
    x, mu, _, _ = ER.case('binary', 4, 16)
    ref = ER.reference('binary', x, mu)
    assert np.allclose(ref['ll'].numpy(), st.bernoulli.logpmf(x.double().numpy(), mu.double().numpy()).sum(1), rtol=1e-9)
    assert ER.C_STAT <= ref64.C_MAX and ER.C_POIS <= ref64.C_MAX


@pytest.mark.parametrize('kind,scaled', ER.COMBOS)
def test_careful_emulation_is_inside_the_bounds(kind, scaled):
    worst = {}
    for M, X in SHAPES:
        for other in _sources(scaled):
            for counts in ('mixed', 'thousands') if kind != 'binary' else ('mixed',):
                x, mu, th, size = ER.case(kind, M, X, seed=1, scaled=scaled, other=other, counts=counts)
                ref, em = ER.reference(kind, x, mu, th, size), ER.emulate(kind, x, mu, th, size)
                for key in ('rows', 'll', 'rec'):
                    w = _worst(em[key], ref[key], ref[key + '_bound'])
                    worst[key] = max(worst.get(key, 0.0), w)
                    assert w <= 1.0, (kind, scaled, other, counts, M, X, key, w)
    print('%s%s: careful emulation, worst fraction of the bound %s' % (kind, ' scaled' if scaled else '', worst))


def _fault_case(fault):
    kind = 'nb' if fault == 'theta_scaled' else 'poisson'
    counts = 'thousands' if fault == 'raw_moments' else 'mixed'
    return (kind,) + ER.case(kind, 6, 257, seed=2, scaled=True, other=True, counts=counts)


@pytest.mark.parametrize('fault,key,cols', [('raw_moments', 'rows', (3, 4, 5)), ('size_target', 'rows', (0, 2, 4, 5)),
                                            ('size_target', 'll', None), ('size_target', 'rec', None),
                                            ('stats_unscaled', 'rows', (0, 2, 4, 5)), ('ll_unscaled', 'll', None),
                                            ('theta_scaled', 'll', None)])
def test_faulty_emulations_are_at_least_ten_times_outside(fault, key, cols):
    kind, x, mu, th, size = _fault_case(fault)
    ref = ER.reference(kind, x, mu, th, size)
    good, bad = ER.emulate(kind, x, mu, th, size), ER.emulate(kind, x, mu, th, size, fault=fault)
    for k in ('rows', 'll', 'rec'):
        assert _worst(good[k], ref[k], ref[k + '_bound']) <= 1.0, k
    ex = ref64.excess(torch.from_numpy(np.asarray(bad[key], np.float64)), ref[key], ref[key + '_bound'])
    ex = ex[2:]         # (row 0 is all zero, row 1's source equals its target: the faults that need a depth do not show there)
    if cols is not None:
        for c in cols:
            print(fault, key, 'column', c, 'worst', float(ex[:, c].max()))
            assert float(ex[:, c].max()) >= 10.0, (fault, key, c, float(ex[:, c].max()))
    else:
        print(fault, key, 'worst', float(ex.max()), 'least', float(ex.reshape(len(ex), -1).max(1)[0].min()))
        assert float(ex.reshape(len(ex), -1).max(1)[0].min()) >= 10.0, (fault, key)


@pytest.mark.parametrize('kind', ['poisson', 'nb'])
def test_raw_moments_without_a_size_source_are_outside_in_every_centred_sum(kind):
    """the same fault on the plain kinds (r = v ~ 3000, no scaling): variance sums and the covariance, each >= 10 x"""
    x, mu, th, _ = ER.case(kind, 6, 257, seed=2, counts='thousands')
    ref = ER.reference(kind, x, mu, th)
    good, bad = ER.emulate(kind, x, mu, th), ER.emulate(kind, x, mu, th, fault='raw_moments')
    assert _worst(good['rows'], ref['rows'], ref['rows_bound']) <= 1.0
    ex = ref64.excess(torch.from_numpy(np.asarray(bad['rows'], np.float64)), ref['rows'], ref['rows_bound'])[1:]
    for c in (3, 4, 5):
        print(kind, 'raw_moments (plain) column', c, 'worst', float(ex[:, c].max()), 'least', float(ex[:, c].min()))
        assert float(ex[:, c].max()) >= 10.0, (c, float(ex[:, c].max()))


# ------------------------------------------------------------------------------------------ 2. the stand-in
def test_the_stand_in_wraps_kernel_ref_and_states_the_count_kinds(monkeypatch):
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    assert K.recon_rows is kernel_ref.recon_rows and K.recon_finalize is kernel_ref.recon_finalize
    x, mu, sd = torch.randn(4, 13), torch.randn(4, 13), torch.rand(4, 13) + 0.5
    a, b, la, lb = torch.zeros(4, 6), torch.zeros(4, 6), torch.zeros(4), torch.zeros(4)
    K.recon_rows(a, la, x, mu, sd)
    kernel_ref.recon_rows(b, lb, x, mu, sd)
    assert torch.equal(a, b) and torch.equal(la, lb)
    x, mu, th, size = ER.case('nb', 5, 13, scaled=True, other=True)
    ref = ER.reference('nb', x, mu, th, size)
    rows, ll, rec = torch.zeros(5, 6), torch.zeros(5), mu.clone()
    K.recon_rows(rows, ll, x, rec, th, kind='nb', size_from=size, rec_out=rec)         # (aliased: the mean head becomes the mean)
    assert torch.equal(rows, ref['rows'].float()) and torch.equal(ll, ref['ll'].float()) and torch.equal(rec, ref['rec'].float())
    K.recon_rows(rows, None, x, mu, None, kind='poisson')
    assert torch.equal(rows, ER.reference('poisson', x, mu)['rows'].float())
    with pytest.raises(AssertionError):
        K.recon_rows(rows, None, x, mu, None, kind='binary', size_from=size)
    with pytest.raises(AssertionError):
        K.recon_rows(rows, None, x, mu, None, kind='poisson', rec_out=rec)


# --------------------------------------------------------------------------------------------- 3. refusals
@pytest.fixture(scope='module')
def lib():
    from drvae_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_point_refusals_without_gpu(lib):
    """every refusal of the count kinds returns its code before anything is launched; a descriptor whose new fields are zero
    returns what it always did.  (a, odd: addresses that are looked at and never dereferenced; M = 0 where the call is valid:
    the checked arguments alone decide and nothing is launched)"""
    from drvae_amd import _lib
    a = 0x1000
    RR = _lib.ReconRows
    call = lambda **kw: lib.dv_recon_rows(C.byref(RR(**kw)), None)
    ops = dict(x=a, ldx=8, mu=a, ldp=16, rows=a, X=8)
    # the Gaussian pass, as ever
    assert call(M=4, X=8) == -1 and call(M=4, X=4096) == -3 and call(M=-1, X=8) == -1 and call(M=4, X=0) == -1
    assert call(M=0, X=8) == 0
    assert call(M=0, X=8, size_x=a, size_ld=8) == -1 and call(M=0, X=8, rec_out=a, rec_ld=8) == -1     # (count operands)
    # the count kinds: valid forms (no rows: no launch)
    for kind in (1, 2, 3):
        assert call(M=0, kind=kind, sd=a, ldt=16, **ops) == 0
    assert call(M=0, kind=2, size_x=a, size_ld=8, rec_out=a, rec_ld=16, **ops) == 0
    assert call(M=0, kind=3, sd=a, ldt=16, size_x=a, size_ld=8, rec_out=a, rec_ld=16, **ops) == 0
    assert call(M=0, kind=2, X=4096, x=a, ldx=4096, mu=a, ldp=4096, rows=a) == 0        # (no width limit)
    # the refusals
    assert call(M=0, kind=4, **ops) == -1 and call(M=0, kind=-1, **ops) == -1           # unknown kind
    assert call(M=0, kind=1, size_x=a, size_ld=8, **ops) == -1                           # a size source with Bernoulli
    for kind in (1, 2, 3):                                                               # raw-head biases with a count kind
        assert call(M=0, kind=kind, sd=a, ldt=16, bias_mu=a, **ops) == -1
        assert call(M=0, kind=kind, sd=a, ldt=16, bias_sd=a, **ops) == -1
        assert call(M=0, kind=kind, sd=a, ldt=16, bias_mu=a, bias_sd=a, **ops) == -1
    assert call(M=0, kind=3, sd=a, **ops) == -1 and call(M=0, kind=3, sd=a, ldt=7, **ops) == -1     # theta's stride
    assert call(M=0, kind=2, rec_out=a, rec_ld=16, **ops) == -1                          # rec_out without a size source
    assert call(M=0, kind=3, sd=a, ldt=16, rec_out=a, rec_ld=16, **ops) == -1
    # rows to do: missing operands, strides below the width
    assert call(M=4, kind=2, X=8) == -1 and call(M=4, kind=3, ldt=16, **ops) == -1       # (no heads | no theta)
    assert call(M=4, kind=2, X=8, x=a, ldx=4, mu=a, ldp=16, rows=a) == -1
    assert call(M=4, kind=2, size_x=a, size_ld=4, **ops) == -1
    assert call(M=4, kind=2, size_x=a, size_ld=8, rec_out=a, rec_ld=4, **ops) == -1


def test_descriptor_mirrors_the_header_with_the_count_fields_last():
    from drvae_amd import _lib
    names = [f[0] for f in _lib.ReconRows._fields_]
    assert names[:12] == ['x', 'ldx', 'mu', 'sd', 'ldp', 'bias_mu', 'bias_sd', 'sd_shift', 'M', 'X', 'rows', 'll']
    assert names[12:] == ['kind', 'ldt', 'size_x', 'size_ld', 'rec_out', 'rec_ld']
    assert _lib.RECON_KIND == {None: 0, 'binary': 1, 'poisson': 2, 'nb': 3} and _lib.ABI_VERSION == 13


def test_launcher_refuses_host_tensors_and_mixed_forms():
    import drvae_amd.kernels as K
    x, mu, th, size = ER.case('nb', 3, 8, scaled=True)
    with pytest.raises(RuntimeError, match='no CPU'):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, th, kind='nb')
    with pytest.raises(AssertionError):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, th, size_from=size)           # (count operands with the Gaussian pass)
    with pytest.raises(AssertionError):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, th, kind='poisson')           # (a theta head the kind does not have)
    with pytest.raises(TypeError, match='size_form'):
        K.recon_rows(torch.zeros(3, 6), None, x, mu, th, kind='nb', size_form=size)       # (a misspelt keyword is not swallowed)
    import inspect
    assert [p for p in inspect.signature(K.recon_rows).parameters][:5] == ['rows', 'll', 'x', 'mu', 'sd']


# ------------------------------------------------------------------------------------ 4. _EvalGraph.get (host)
@pytest.mark.parametrize('type_rec,sw', [('binary', {}), ('poisson', dict(library_size=True)),
                                         ('nb', dict(x_transform='log1p', library_size=True))])
def test_a_host_dataset_keeps_the_step_by_step_path(type_rec, sw, monkeypatch):
    import warnings
    from drvae_amd import fit as F
    from tests.test_counts_cpu import _counts_dataset
    from tests.test_fit import _tiny_model
    kernel_ref.install(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = _tiny_model('drvae', device='cpu', type_rec=type_rec, add_noise_var=0.0, **sw)
    ds = _counts_dataset('drvae', 24, 2, 'cpu', 1.0, 0.0)
    if type_rec == 'binary':
        ds.x1, ds.x2 = (ds.x1 > 2).float(), (ds.x2 > 2).float()
    assert F._EvalGraph.get(model, ds) is None
    perf, txt = model.evaluate_performance_on_dataset(ds)
    assert np.isfinite(perf['x1_rmse']) and txt.count('RMSE') == 2
    assert np.isfinite(perf['x1_ll']) if type_rec == 'nb' else np.isnan(perf['x1_ll'])
