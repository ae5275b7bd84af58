"""CPU: the effect reduction's float64 reference and bounds (tests/effect_ref.py) held against a careful fp32 emulation and
against faulty ones, the refusals of the launch at the C level (no GPU is touched), the ctypes mirror of the header, and the
argument errors of ``perturbation_effect``.  The kernel and the model-level numbers: tests/test_gpu_effect.py."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import effect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = len(R.CASES)


# ------------------------------------------------------------------------------------------- the grid and its reference
def test_the_grid_meets_every_value_of_every_axis():
    seen = lambda k: {cs[k] for cs in R.CASES}
    assert seen('X') == set(R.XS) and seen('M') == set(R.MS)
    assert seen('layout') == set(R.LAYOUTS) and seen('view') == set(R.VIEWS)
    assert seen('mode') == {0, 1} and seen('delta') == {0.25, 1.0}
    assert {cs['c'] for cs in R.CASES if cs['mode'] == 0} == {0.0, 1.0} and all(cs['c'] == 0 for cs in R.CASES if cs['mode'] == 1)
    assert {1, 2, 3} <= seen('row_blocks')
    shapes = [R.blocks_of(cs['M'], cs['row_blocks']) for cs in R.CASES]
    assert any(b[-1][0] == b[-1][1] for b in shapes), 'no case with an empty last block'
    assert any(0 < b[-1][1] - b[-1][0] < b[0][1] - b[0][0] for b in shapes), 'no case with a short last block'
    assert any(cs['row_blocks'] > cs['M'] / 2 and cs['M'] >= 8 for cs in R.CASES)
    assert all(1 <= cs['row_blocks'] <= cs['M'] for cs in R.CASES)
    # both access paths at a 1024-gene seam, the scalar path by X and by alignment
    assert any(cs['X'] % 4 == 0 and cs['view'] != 'odd_offset' and cs['X'] > 1024 for cs in R.CASES)
    assert any(cs['X'] % 4 == 0 and cs['view'] == 'odd_offset' for cs in R.CASES)


@pytest.mark.parametrize('i', range(N_CASES))
def test_the_reference_alone_decides_all_but_one_percent(i):
    cs, ref = R.grid_case(i)
    decisions = 2 * ref['elements']
    assert ref['undecided'] <= R.UNDECIDED_CAP * decisions, (cs['i'], ref['undecided'], decisions)
    assert np.all(ref['bound'] >= 0) and np.all(np.isfinite(ref['value']))
    if cs.get('ties'):
        assert ref['undecided'] == 0        # mode 1 on a quarter grid: exact elements, strict comparisons


@pytest.mark.parametrize('i', range(N_CASES))
def test_a_careful_fp32_emulation_stays_inside_every_bound(i):
    cs, ref = R.grid_case(i)
    R.hold(R.emulate(cs['a'], cs['b'], **R.launch_kw(cs)), ref, 'case %d' % i)


def _special_heads():
    """heads that make invalid elements at c == 0: NaN, +-inf, 0 and negative values among ordinary ones"""
    rs = np.random.RandomState(7)
    a, b = R.heads(12, 20, 0, rs)
    a, b = a.copy(), b.copy()
    nan, inf = np.float32('nan'), np.float32('inf')
    a[0, :6] = [nan, inf, 0.0, -1.0, 2.0, 0.0]
    b[0, :6] = [1.0, 1.0, 1.0, 1.0, nan, 0.0]
    a[5, 3], b[7, 3], b[9, 4] = 0.0, inf, -0.0
    return a, b


def test_invalid_elements_reduce_n_only():
    a, b = _special_heads()
    ref = R.reference(a, b, mode=0, c=0.0, delta=0.25)
    assert list(ref['value'][0, 0, 0, :6]) == [11, 11, 11, 9, 10, 11] and np.all(ref['value'][0, 0, 0, 6:] == 12)
    R.hold(R.emulate(a, b, mode=0, c=0.0, delta=0.25), ref, 'special heads')
    # with a pseudocount the zeros are valid again
    ref1 = R.reference(a, b, mode=0, c=1.0, delta=0.25)
    assert list(ref1['value'][0, 0, 0, :6]) == [11, 11, 12, 10, 11, 12]
    R.hold(R.emulate(a, b, mode=0, c=1.0, delta=0.25), ref1, 'special heads, c = 1')


def _first(pred):
    return next(i for i, cs in enumerate(R.CASES) if pred(cs))


FAULT_CASES = {
    'ge': lambda: _first(lambda cs: cs.get('ties') and cs['M'] == 67),
    'c_one_side': lambda: _first(lambda cs: cs['mode'] == 0 and cs['c'] == 1.0 and cs['M'] >= 5),
    'ln': lambda: _first(lambda cs: cs['mode'] == 0 and cs['M'] >= 5),
    'seam_group': lambda: _first(lambda cs: cs['layout'] == 'alternating' and cs['row_blocks'] == 5),
    'short_block_dropped': lambda: _first(lambda cs: cs['M'] == 67 and cs['row_blocks'] == 34),
    'left_out_counted': lambda: _first(lambda cs: cs['layout'] in ('negative', 'too_big') and cs['M'] >= 5),
}


@pytest.mark.parametrize('fault', R.FAULTS)
def test_a_faulty_emulation_leaves_the_bounds(fault):
    """each fault lands at least ten times outside a bound or breaks a count interval"""
    if fault == 'invalid_counted':
        a, b = _special_heads()
        kw = dict(mode=0, c=0.0, delta=0.25)
        ref = R.reference(a, b, **kw)
    else:
        cs, ref = R.grid_case(FAULT_CASES[fault]())
        a, b, kw = cs['a'], cs['b'], R.launch_kw(cs)
    assert R.excess(R.emulate(a, b, **kw), ref) <= (1.0, 0)
    worst, bad = R.excess(R.emulate(a, b, fault=fault, **kw), ref)
    print('%s: %.3g of a bound, %d counts outside' % (fault, worst, bad))
    assert worst >= 10.0 or bad > 0, fault
    if fault == 'ge':
        assert bad > 0          # (the sums are untouched: only the strict inequality tells)


def test_the_other_group_layouts_are_caught_too():
    for layout in ('negative', 'too_big'):
        cs, ref = R.grid_case(_first(lambda c: c['layout'] == layout and c['M'] >= 5))
        worst, bad = R.excess(R.emulate(cs['a'], cs['b'], fault='left_out_counted', **R.launch_kw(cs)), ref)
        assert worst >= 10.0 or bad > 0, layout


# ------------------------------------------------------------------------------------------- the built library
@pytest.fixture(scope='module')
def lib():
    from drvae_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _struct_fields(src, cname):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), src, flags=re.S).group(1)
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
    return fields


def test_the_descriptors_mirror_the_header():
    from drvae_amd import _lib, effect
    src = open(os.path.join(ROOT, 'include', 'drvae_hip.h')).read()
    assert _struct_fields(src, 'dv_effect_desc') == list(_lib.EffectDesc._fields_)
    assert [n for n, _ in _lib.EffectDesc._fields_] == ['a', 'lda', 'b', 'ldb', 'mode', 'delta', 'pseudo', 'out', 'row_blocks',
                                                        'n_grp', 'grp']
    draw = _struct_fields(src, 'dv_draw_desc')
    assert draw == list(_lib.DrawDesc._fields_) and draw[-1] == ('fx', C.c_void_p)
    assert 'const dv_effect_desc* fx;' in src
    assert src.index('} dv_effect_desc;') < src.index('typedef struct dv_draw_desc {')
    assert _lib.ABI_VERSION == 13 and len(_lib.SIGNATURES) == 84 and len(_lib.SIGNATURES['dv_fill_normal']) == 6
    assert effect.STATS == R.STATS and (_lib.EFFECT_LFC, _lib.EFFECT_DIFF) == (0, 1)
    assert effect.MODE == {'diag_gaussian': 1, 'poisson': 0, 'nb': 0, 'zinb': 0}


def test_refusals_without_a_gpu(lib):
    """every refusal comes before any launch, at M == 0 too: the arguments alone decide (a: an address that is looked at and
    never dereferenced)"""
    from drvae_amd import _lib
    a, X = 0x1000, 8

    def call(M=0, outer=None, args=None, **kw):
        base = dict(a=a, lda=X, b=a, ldb=X, mode=0, delta=0.25, pseudo=0.0, out=a, row_blocks=1, n_grp=1, grp=None)
        base.update(kw)
        fx = _lib.EffectDesc(**base)
        d = _lib.DrawDesc(**dict(dict(M=M, X=X, fx=C.addressof(fx)), **(outer or {})))
        return lib.dv_fill_normal(*(args or (None, 0, 0, None)), None, C.byref(d))

    assert call() == 0 and call(grp=a, n_grp=65535) == 0 and call(mode=1) == 0 and call(pseudo=1.0, delta=0.0) == 0
    assert call(a=None, b=None, out=None) == 0                      # (M == 0: no operand is needed)
    for M in (0, 4):
        bad = lambda **kw: call(M=M, **kw)
        assert bad(n_grp=0) == -1 and bad(n_grp=-1) == -1 and bad(n_grp=65536) == -1
        assert bad(row_blocks=0) == -1 and bad(row_blocks=-1) == -1 and bad(row_blocks=max(M, 1) + 1) == -1
        assert bad(lda=X - 1) == -1 and bad(ldb=X - 1) == -1 and bad(lda=0) == -1
        assert bad(mode=2) == -1 and bad(mode=-1) == -1
        assert bad(delta=-0.5) == -1 and bad(delta=float('nan')) == -1
        assert bad(pseudo=-1.0) == -1 and bad(pseudo=float('inf')) == -1 and bad(pseudo=float('nan')) == -1
        assert bad(mode=1, pseudo=1.0) == -1
        # every other outer field, and dv_fill_normal's own arguments, must be zero / NULL
        for outer in (dict(kind=3), dict(S=1), dict(mu=a), dict(ldm=X), dict(sd=a), dict(lds=X), dict(theta=a), dict(ldt=X),
                      dict(logit=a), dict(ldl=X), dict(size=a), dict(out=a), dict(ldo=X), dict(sso=X), dict(row0=1), dict(grow=a),
                      dict(k0=1), dict(M=-1), dict(X=0), dict(X=-1)):
            assert bad(outer=outer) == -1, outer
        for args in ((a, 0, 0, None), (None, 4, 0, None), (None, 0, 1, None), (None, 0, 0, a)):
            assert bad(args=args) == -1, args
    assert call(M=70000, row_blocks=65536) == -1
    assert call(M=4, a=None) == -1 and call(M=4, b=None) == -1 and call(M=4, out=None) == -1
    # fx == NULL: the sampler as it was (its own refusals are held by tests/test_count_sample_cpu.py)
    assert lib.dv_fill_normal(None, 0, 1, None, None, C.byref(_lib.DrawDesc(kind=2, M=0, X=X, S=0, mu=a, ldm=X, out=a, ldo=X))) == 0


# ------------------------------------------------------------------------------------------- host side
def test_the_row_block_rule():
    from drvae_amd import effect as E
    for M, X, G in ((1, 1, 1), (37, 20, 3), (900, 978, 1), (900, 978, 8), (2048, 20000, 1), (2048, 20000, 8), (10 ** 6, 978, 1)):
        rb = E.row_blocks_for(M, X, G)
        assert 1 <= rb <= max(M, 1) and rb <= 65535
        assert rb == 1 or (M // rb >= E.MIN_ROWS and rb * G * -(-X // E.CHUNK) <= E.TARGET_WORKGROUPS)
    assert E.row_blocks_for(900, 978, 1) == 28 and E.row_blocks_for(2048, 20000, 1) == 3 and E.row_blocks_for(2048, 20000, 8) == 1


def test_fold_and_summarize():
    from drvae_amd import effect as E
    rs = np.random.RandomState(3)
    part = torch.from_numpy(rs.rand(5, 2, 7, 6))
    acc = torch.zeros(2, 7, 6, dtype=torch.float64)
    assert E.fold(acc, part) is acc and torch.allclose(acc, part.sum(0), rtol=0, atol=1e-15)
    E.fold(acc, part)
    assert torch.allclose(acc, 2 * part.sum(0), rtol=0, atol=1e-14)
    raw = torch.zeros(2, 7, 3, dtype=torch.float64)
    #            n, sum e, sum e^2, up, down, sum a, sum b
    raw[0, :, 0] = torch.tensor([4.0, 2.0, 3.0, 1.0, 0.0, 8.0, 12.0], dtype=torch.float64)
    raw[0, :, 1] = torch.tensor([2.0, 2.0, 2.0 - 1e-17, 2.0, 0.0, 1.0, 1.0], dtype=torch.float64)      # (variance rounds below 0)
    res = E.summarize(raw)
    assert list(res) == ['n', 'lfc_mean', 'lfc_sd', 'p_up', 'p_down', 'mean_base', 'mean_pert', 'raw'] and res['raw'] is raw
    assert res['lfc_mean'][0, 0] == 0.5 and abs(float(res['lfc_sd'][0, 0]) - 0.5 ** 0.5) < 1e-15 and res['p_up'][0, 0] == 0.25
    assert res['mean_base'][0, 0] == 2.0 and res['mean_pert'][0, 0] == 3.0 and res['lfc_sd'][0, 1] == 0.0
    for k in ('lfc_mean', 'lfc_sd', 'p_up', 'p_down', 'mean_base', 'mean_pert'):
        assert torch.isnan(res[k][0, 2]) and torch.isnan(res[k][1]).all(), k
        assert res[k].dtype == torch.float64 and tuple(res[k].shape) == (2, 3)
    assert (res['n'][1] == 0).all()


def test_the_launcher_refuses_host_tensors_and_wrong_shapes():
    from drvae_amd import effect as E
    a = torch.zeros(4, 6)
    with pytest.raises(ValueError, match='float64 device tensor'):
        E.effect_cols(torch.zeros(1, 1, 7, 6, dtype=torch.float64), a, a, mode=0, delta=0.25)


def _quiet(kind, **kw):
    from tests.test_dropout_cpu import tiny_model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return tiny_model(kind, **kw)


def _host_dataset(kind, n=12, X=13):
    from tests.test_eval_chunks_cpu import _host_dataset as make
    return make(kind, n, X)


def test_vfae_has_no_perturbation_effect():
    with pytest.raises(AttributeError, match='no perturbation path'):
        _quiet('vfae', type_rec='nb').perturbation_effect(_host_dataset('vfae'))


@pytest.mark.parametrize('kind', ['drvae', 'pvae'])
def test_argument_errors_of_the_model_interface(kind):
    model, ds = _quiet(kind, type_rec='nb'), _host_dataset(kind)
    with pytest.raises(ValueError, match='host'):                # a host-resident set: no silent other path
        model.perturbation_effect(ds)
    for bad in ('mode', None, 'Mean'):
        with pytest.raises(ValueError, match='latent'):
            model.perturbation_effect(ds, latent=bad)
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match='n_samples'):
            model.perturbation_effect(ds, n_samples=bad, latent='sample')
    with pytest.raises(ValueError, match="n_samples must be 1 with latent='mean'"):
        model.perturbation_effect(ds, n_samples=2)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='chunk_rows'):
            model.perturbation_effect(ds, chunk_rows=bad)
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='pseudocount'):
            model.perturbation_effect(ds, pseudocount=bad)
    with pytest.raises(ValueError, match='delta'):
        model.perturbation_effect(ds, delta=-0.1)
    with pytest.raises(ValueError, match='binary'):
        _quiet(kind, type_rec='binary').perturbation_effect(ds)
    with pytest.raises(ValueError, match='pseudocount'):         # a Gaussian model's effect is a difference
        _quiet(kind).perturbation_effect(ds, pseudocount=1.0)
    model._dp = (0, 2)
    with pytest.raises(NotImplementedError, match='data parallelism'):
        model.perturbation_effect(ds)
    model._dp = None
