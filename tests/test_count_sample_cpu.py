"""CPU checks of the posterior-predictive sampler (the ``dv_draw_desc`` form of ``dv_fill_normal``): the float64 reference of
the header's specification (``tests/count_sample_ref.py``) samples the right law, faulty emulations of it are caught, the grid
of the GPU test leaves the reference at most 2 % undecided elements and no cap hit, and -- through the built library, without a
GPU -- every refusal, the descriptor's layout and the argument errors of the model-level interface."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import count_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LAW = 100000           # draws per cell
Z_MAX = 5.0              # standard errors

# name -> (mu, theta, logit or None, size factor or None)
CELLS = {
    'small theta': (3.0, 1e-2, None, None),
    'theta < 1': (0.5, 0.3, None, None),
    'moderate': (5.0, 2.0, None, None),
    'PTRS, theta < 1': (50.0, 0.7, None, None),
    'PTRS': (2000.0, 5.0, None, None),
    'Poisson limit': (30.0, 1e5, None, None),
    'ZINB, 60 % dropout': (5.0, 2.0, float(np.log(0.6 / 0.4)), None),
    'library-scaled': (0.05, 1.5, None, 100.0),
}


def cell_draws(name, n=N_LAW, seed=77, event=3, **kw):
    mu, theta, logit, s = CELLS[name]
    ops = dict(mu=np.full((1, n), mu, np.float32), theta=np.full((1, n), theta, np.float32))
    if logit is not None:
        ops['logit'] = np.full((1, n), logit, np.float32)
    if s is not None:
        ops['size'] = np.array([s], np.float32)
    return R.draw('nb' if logit is None else 'zinb', seed=seed, event=event, **ops, **kw)


def cell_law(name):
    mu, theta, logit, s = CELLS[name]
    mean = float(np.float32(mu)) if s is None else float(np.float32(s) * np.float32(mu))
    return R.law(mean, float(np.float32(theta)), 0.0 if logit is None else 1.0 / (1.0 + np.exp(-float(np.float32(logit)))))


def z_scores(values, law):
    """(mean, P(x = 0), P(x <= floor(mean))) of the draws ``values`` against the analytic ``law``, in standard errors: CLT
    for the mean, binomial for the two probabilities"""
    v = np.asarray(values, np.float64).reshape(-1)
    mean, sd, p0, pq = law
    se = lambda p: np.sqrt(p * (1 - p) / v.size)
    return ((v.mean() - mean) / (sd / np.sqrt(v.size)), ((v == 0).mean() - p0) / se(p0),
            ((v <= np.floor(mean)).mean() - pq) / se(pq))


@pytest.mark.parametrize('name', sorted(CELLS))
def test_the_specification_samples_the_right_law(name):
    r = cell_draws(name)
    assert not r['cap'].any()
    v = r['value']
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and np.all(v == np.floor(v))
    z = z_scores(v, cell_law(name))
    print('%s: mean %+.2f, P(0) %+.2f, P(x <= floor(mean)) %+.2f standard errors' % ((name,) + z))
    assert max(abs(t) for t in z) <= Z_MAX, z


def test_poisson_kind_samples_the_poisson_law():
    for lam, s in ((0.3, None), (4.0, 2.0), (700.0, None)):
        ops = dict(mu=np.full((1, N_LAW), lam, np.float32))
        if s is not None:
            ops['size'] = np.array([s], np.float32)
        r = R.draw('poisson', seed=5, event=1, **ops)
        z = z_scores(r['value'], R.law(float(np.float32(lam)) * (s or 1.0), np.inf))
        assert not r['cap'].any() and max(abs(t) for t in z) <= Z_MAX, (lam, z)


@pytest.mark.parametrize('fault,name', [('gamma_scale', 'moderate'), ('no_boost', 'theta < 1'), ('gate_flip', 'ZINB, 60 % dropout'),
                                        ('no_size', 'library-scaled')])
def test_a_faulty_emulation_misses_the_law(fault, name):
    z = z_scores(cell_draws(name, fault=fault)['value'], cell_law(name))
    print('%s at %s: %r' % (fault, name, z))
    assert max(abs(t) for t in z) > Z_MAX, z


@pytest.mark.parametrize('fault', ['swap_blocks', 'no_sample'])
def test_a_faulty_stream_fails_the_exact_comparison(fault):
    """a law-preserving fault -- other blocks, or every sample the same -- is caught element by element on the GPU test's grid"""
    wrong = total = 0
    for i in (2, 5, 7):
        case, ref = R.grid_reference('zinb', i)
        _, bad = R.grid_reference('zinb', i, fault=fault)
        w, _ = R.compare(bad['value'], ref)
        wrong, total = wrong + int(w.sum()), total + w.size
        if fault == 'no_sample' and case['S'] > 1:
            assert np.array_equal(bad['value'][0], bad['value'][1], equal_nan=True)
    assert wrong > 0.05 * total, (wrong, total)


def test_the_naive_accept_test_in_fp32_is_caught_at_a_large_theta():
    """d - d v + d ln v subtracts values of size d: in fp32 the Gamma accept decision is lost at a large theta.  At theta in
    1e7 .. 1e8 (>= 1e5) and means of 1e3 .. 1e4 the share of elements that are undecided or WRONG against the reference lies
    far above the cap, and the wrong ones -- decided by the reference, drawn otherwise -- alone do; the specified form, in
    the same fp32 arithmetic, has no wrong element at all.

    Figures of this test: naive form 18.6 % undecided-or-wrong, 10.3 % wrong; specified form 0 wrong (8.3 % of the elements
    are undecided by nature at these rates: floor(... + lam) with lam ~ 1e4 and a relative error of 1e-6).  Inside the grid's
    own range, theta in 1e5 .. 1e6, the naive form is wrong on 0.2 % .. 0.5 % of the elements only: the Poisson draw has blocks
    of its own (8 ..), so a lost Gamma decision moves the rate by a part in theta's root and no uniform of the Poisson draw."""
    rs = np.random.RandomState(3)
    n = 40000
    ops = dict(mu=np.exp(rs.uniform(np.log(1e3), np.log(1e4), (1, n))).astype(np.float32),
               theta=np.exp(rs.uniform(np.log(1e7), np.log(1e8), (1, n))).astype(np.float32))
    ref = R.draw('nb', seed=11, **ops)
    share, wrong_share = {}, {}
    for fault in (None, 'naive'):
        got = R.draw('nb', seed=11, ft=np.float32, fault=fault, **ops)
        wrong, und = R.compare(got['value'], ref)
        share[fault], wrong_share[fault] = float((wrong | und).mean()), float(wrong.mean())
    print('theta in 1e7 .. 1e8: undecided-or-wrong %r, wrong %r' % (share, wrong_share))
    assert wrong_share[None] == 0.0
    assert share['naive'] > R.UNDECIDED_CAP and wrong_share['naive'] > R.UNDECIDED_CAP, (share, wrong_share)


@pytest.mark.parametrize('kind', R.GRID_KINDS)
def test_the_grid_leaves_the_reference_decided(kind):
    """the condition of the GPU comparison: on its exact grid the reference alone has at most 2 % undecided elements and no
    cap hit; an fp32 emulation of the specification differs from it on undecided elements only"""
    n = und = flips = 0
    for i in range(len(R.GRID_SHAPES)):
        case, ref = R.grid_reference(kind, i)
        assert ref['value'].shape == (case['S'], case['M'], case['X'])
        assert not ref['cap'].any(), (kind, i)
        n, und = n + ref['value'].size, und + int((ref['margin'] < 1).sum())
        _, emu = R.grid_reference(kind, i, ft=np.float32)
        if kind == 'diag_gaussian':
            assert np.all(np.abs(emu['value'] - ref['value']) <= ref['tol'])
            continue
        wrong, _ = R.compare(emu['value'], ref)
        assert not wrong.any(), (kind, i, int(wrong.sum()))
        flips += int((emu['value'] != ref['value']).sum())
    print('%s: %d elements, %.4f %% undecided, fp32 emulation differs on %.4f %%' % (kind, n, 100.0 * und / n, 100.0 * flips / n))
    assert und <= R.UNDECIDED_CAP * n, (kind, und, n)


def test_defined_results_for_heads_outside_the_domain():
    nan, inf = np.nan, np.inf
    mu = np.array([[nan, 0.0, -3.0, inf, 2.0, 2.0, 2.0, 2.0, 1e8, 2.0]], np.float32)
    th = np.array([[1.0, 1.0, 1.0, 1.0, nan, 0.0, -1.0, inf, 1e9, 1.0]], np.float32)
    lg = np.array([[0.0, -30.0, -30.0, -30.0, 0.0, 0.0, 0.0, -30.0, -30.0, nan]], np.float32)
    v = R.draw('nb', mu=mu, theta=th, seed=1)['value'][0, 0]
    assert np.isnan(v[0]) and v[1] == 0 and v[2] == 0 and v[3] == R.FLT_MAX and np.isnan(v[4:7]).all()
    assert np.isfinite(v[7]) and v[7] >= 0 and v[8] >= 2.0 ** 24 and np.isfinite(v[9])
    # a denormal theta, whose quotient d / theta overflows fp32: the rate is 0
    tiny = R.draw('nb', mu=np.full((1, 64), 5.0, np.float32), theta=np.full((1, 64), 1e-40, np.float32), seed=1)
    assert np.all(tiny['value'] == 0) and not tiny['cap'].any()
    z = R.draw('zinb', mu=mu, theta=th, logit=lg, seed=1)['value'][0, 0]
    assert np.isnan(z[0]) and z[1] == 0 and z[3] == R.FLT_MAX and np.isnan(z[4:7]).all() and np.isnan(z[9])
    p = R.draw('poisson', mu=mu, seed=1)['value'][0, 0]
    assert np.isnan(p[0]) and p[1] == 0 and p[2] == 0 and p[3] == R.FLT_MAX and p[8] == 1e8
    assert not R.draw('poisson', mu=mu, seed=1)['cap'].any()


# ------------------------------------------------------------------------------------------- the built library
@pytest.fixture(scope='module')
def lib():
    from drvae_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_descriptor_mirrors_the_header():
    from drvae_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'drvae_hip.h')).read()
    body = re.search(r'typedef struct dv_draw_desc \{(.*?)\} dv_draw_desc;', src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for st in body.split(';'):
        st = st.strip()
        if not st:
            continue
        head = re.match(r'(?:const\s+)?\w+', st).group(0)
        for j, part in enumerate(st.split(',')):
            decl = part.strip() if j == 0 else head + ' ' + part.strip()
            kind = C.c_void_p if '*' in decl else {'int64_t': C.c_int64, 'int32_t': C.c_int32, 'float': C.c_float}[decl.split()[0]]
            fields.append((re.sub(r'.*[\s\*]', '', decl), kind))
    assert fields == list(_lib.DrawDesc._fields_)
    assert _lib.ABI_VERSION == 13
    assert _lib.SIGNATURES['dv_fill_normal'][-1] is C.POINTER(_lib.DrawDesc) and len(_lib.SIGNATURES['dv_fill_normal']) == 6
    m = re.search(r'#define DV_DRAW_MAX_SAMPLES (\d+)', src), re.search(r'#define DV_DRAW_MAX_ROW (\d+)', src)
    assert (int(m[0].group(1)), int(m[1].group(1))) == (_lib.DRAW_MAX_SAMPLES, _lib.DRAW_MAX_ROW)
    from drvae_amd import count_sample as CS
    assert CS.KIND == R.KIND
    enum = re.search(r'enum \{ DV_RECON_GAUSS = 0, DV_RECON_BERNOULLI = 1, DV_RECON_POISSON = 2, DV_RECON_NEGBIN = 3, DV_RECON_ZINB = 4 \}', src)
    assert enum is not None


def test_refusals_without_a_gpu(lib):
    """every refusal of the sampler comes before any launch, at M == 0 and S == 0 too: the arguments alone decide.  (a:
    an address that is looked at and never dereferenced)"""
    from drvae_amd import _lib
    a, X = 0x1000, 8
    # draw = NULL: dv_fill_normal as it always was
    assert lib.dv_fill_normal(a, 0, 1, None, None, None) == 0
    assert lib.dv_fill_normal(a, -1, 1, None, None, None) == -1
    assert lib.dv_fill_normal(None, 4, 1, None, None, None) == -1

    def call(**kw):
        base = dict(kind=4, M=0, X=X, S=0, mu=a, ldm=X, sd=a, lds=X, theta=a, ldt=X, logit=a, ldl=X, out=a, ldo=X, sso=0)
        base.update(kw)
        return lib.dv_fill_normal(None, 0, 1, None, None, C.byref(_lib.DrawDesc(**base)))
    for kind in range(5):
        assert call(kind=kind) == 0
        assert call(kind=kind, M=0, S=3) == 0 and call(kind=kind, M=4, S=0, sso=4 * X) == 0
    for empty in (dict(M=0, S=3), dict(M=4, S=0), dict(M=0, S=0)):
        bad = lambda **kw: call(**dict(empty, **kw))
        assert bad(kind=5) == -1 and bad(kind=-1) == -1                       # unknown kind
        assert bad(mu=None) == -1
        assert bad(kind=0, sd=None) == -1                                      # a missing operand for the kind
        assert bad(kind=3, theta=None) == -1 and bad(kind=4, theta=None) == -1
        assert bad(kind=4, logit=None) == -1
        assert bad(kind=3, logit=None, sd=None) == 0                           # (operands the kind does not read: ignored)
        assert bad(kind=0, size=a) == -1 and bad(kind=1, size=a) == -1         # a size vector with Gaussian / Bernoulli
        for kind in (2, 3, 4):
            assert bad(kind=kind, size=a) == 0
        assert bad(ldm=X - 1) == -1 and bad(ldo=X - 1) == -1 and bad(ldl=X - 1) == -1       # row strides below X
        assert bad(kind=0, lds=X - 1) == -1 and bad(kind=3, lds=0) == 0
        assert bad(ldt=X - 1) == -1 and bad(ldt=0) == 0 and bad(ldt=1) == -1   # (theta's 0: one shared row)
        assert bad(S=-1) == -1 and bad(M=-1) == -1 and bad(X=-1) == -1 and bad(k0=-1) == -1
        assert bad(S=_lib.DRAW_MAX_SAMPLES + 1) == -1                           # beyond the counter layout
        assert bad(k0=_lib.DRAW_MAX_SAMPLES) == (-1 if empty['S'] else 0)
        assert bad(row0=-1) == -1 and bad(row0=_lib.DRAW_MAX_ROW - empty['M'] + 1) == -1
        assert bad(row0=_lib.DRAW_MAX_ROW - empty['M']) == 0
        assert bad(grow=a, row0=1) == -1 and bad(grow=a) == 0
    assert call(M=4, S=3, sso=3 * X + X - 1) == -1                             # samples that overlap
    assert call(M=4, S=3, sso=4 * X, out=None) == -1                           # out NULL with rows to do
    assert call(M=4, S=3, sso=4 * X, X=0, ldm=0, ldo=0, ldt=0, ldl=0, out=None) == 0    # (nothing to write)


# ------------------------------------------------------------------------------------------- the model-level interface
def _quiet(kind, **kw):
    from tests.test_dropout_cpu import tiny_model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return tiny_model(kind, **kw)


def _host_dataset(kind, n=12, X=13):
    from tests.test_eval_chunks_cpu import _host_dataset as make
    return make(kind, n, X)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_argument_errors_of_the_model_interface(kind):
    model = _quiet(kind, type_rec='nb')
    x = torch.ones(4, 13)
    for bad in ('mode', None, 'Mean'):
        with pytest.raises(ValueError, match='latent'):
            model.sample_x(x, latent=bad)
        with pytest.raises(ValueError, match='latent'):
            model.posterior_predictive(_host_dataset(kind), latent=bad)
    for bad in (0, -1, 1.5, 2 ** 24 + 1, None, '3', True):
        with pytest.raises(ValueError, match='n_samples'):
            model.sample_x(x, n_samples=bad)
    with pytest.raises(ValueError, match='library_size'):       # size_factor= on a model whose means carry no size factor
        model.sample_x(x, size_factor=1.0)
    ds = _host_dataset(kind)
    with pytest.raises(ValueError, match='host'):                # a host-resident set: no silent other path
        model.posterior_predictive(ds, 2)
    with pytest.raises(ValueError, match='out must be'):         # a wrong shape, a wrong dtype
        model.posterior_predictive(ds, 2, out=torch.zeros(2, 12, 12))
    with pytest.raises(ValueError, match='out must be'):
        model.posterior_predictive(ds, 2, out=torch.zeros(3, 12, 13))
    with pytest.raises(ValueError, match='float32'):
        model.posterior_predictive(ds, 2, out=torch.zeros(2, 12, 13, dtype=torch.float64))
    with pytest.raises(ValueError, match='pinned'):              # (a pageable host tensor cannot be filled from the device)
        model.posterior_predictive(ds, 2, out=torch.zeros(2, 12, 13))
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='chunk_rows'):
            model.posterior_predictive(ds, chunk_rows=bad)
    model._dp = (0, 2)
    with pytest.raises(NotImplementedError, match='data parallelism'):
        model.posterior_predictive(ds)
    model._dp = None


def test_the_default_seed_is_not_the_train_steps():
    from drvae_amd import count_sample as CS
    seeds = {CS.default_seed(s) for s in range(64)}
    assert len(seeds) == 64 and not seeds & set(range(64))
    assert all(0 <= s < 2 ** 64 for s in seeds)
    assert len({CS.default_seed(5), CS.default_seed(5) ^ CS.X2_SEED_XOR, CS.default_seed(5) ^ CS.LATENT_SEED_XOR}) == 3
