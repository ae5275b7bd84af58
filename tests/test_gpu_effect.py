"""-m gpu: the effect reduction (``effect.effect_cols``: the ``dv_draw_desc.fx`` form of ``dv_fill_normal``) against the float64
reference of the header's specification (``tests/effect_ref.py``), and ``perturbation_effect`` on top.

The rule of every comparison (``effect_ref.hold``): the five sums lie within the bound the reference derives per output element
from the roundings of one element and of the float64 accumulation, ``n`` is exact, and each of the two counts lies in [sure,
sure + undecided].  The reference's undecided share stays under 1 % on every grid case (asserted on the CPU,
``tests/test_effect_cpu.py``)."""
import warnings

import numpy as np
import pytest
import torch

from tests import csr_feed_ref as CF
from tests import effect_ref as R
from tests.test_dropout_cpu import tiny_model
from tests.test_effect_cpu import _special_heads

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 5            # float64 guard elements in front of and behind ``out``


@pytest.fixture(scope='module')
def E(dev):
    from drvae_amd import _lib, effect
    _lib.load()
    return effect


def _operands(a, b, view, dev):
    """the (M, X) arrays on the device: ``contiguous`` -- a tensor each; ``columns`` -- the two halves of ONE (M, 2 X) buffer
    (row stride 2 X); ``odd_offset`` -- rows of stride X + 3 that start one float behind a 16-byte boundary (the scalar path)"""
    a, b = torch.from_numpy(np.array(a, np.float32)), torch.from_numpy(np.array(b, np.float32))      # (copies: the grid is read-only)
    M, X = a.shape
    if view == 'contiguous':
        return a.to(dev), b.to(dev)
    if view == 'columns':
        buf = torch.full((M, 2 * X), SENTINEL, device=dev)
        buf[:, :X], buf[:, X:] = a.to(dev), b.to(dev)
        return buf[:, :X], buf[:, X:]
    out = []
    for t in (a, b):
        ld = X + 3
        buf = torch.full((M * ld + 8,), SENTINEL, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:1 + M * ld].view(M, ld)[:, :X]
        v.copy_(t.to(dev))
        out.append(v)
    return tuple(out)


def _launch(E, dev, a, b, *, mode, c, delta, grp, G, row_blocks, fill=SENTINEL):
    """one launch into a buffer with guard bands: the guards are intact -> out (row_blocks, G, 7, X), numpy"""
    M, X = a.shape
    n = row_blocks * G * 7 * X
    buf = torch.full((n + 2 * PAD,), fill, dtype=torch.float64, device=dev)
    out = buf[PAD:PAD + n].view(row_blocks, G, 7, X)
    g = None if grp is None else torch.from_numpy(np.ascontiguousarray(grp, np.int32)).to(dev)
    E.effect_cols(out, a, b, grp=g, n_groups=G, mode=mode, delta=delta, pseudocount=c)
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all()), 'a guard element was written'
    return out.cpu().numpy()


@pytest.mark.parametrize('i', range(len(R.CASES)))
def test_kernel_holds_the_reference(i, E, dev):
    """every grid case: inside the reference's bounds, the operands untouched, the guard bands intact, every element written
    and two launches equal bit for bit (the second starts from another fill)"""
    cs, ref = R.grid_case(i)
    a, b = _operands(cs['a'], cs['b'], cs['view'], dev)
    keep = a.clone(), b.clone()
    kw = R.launch_kw(cs)
    got = _launch(E, dev, a, b, **kw)
    R.hold(got, ref, 'case %d: X %d M %d blocks %d %s %s mode %d c %g' % (i, cs['X'], cs['M'], cs['row_blocks'], cs['layout'],
                                                                          cs['view'], cs['mode'], cs['c']))
    assert torch.equal(a, keep[0]) and torch.equal(b, keep[1]), 'an operand was modified'
    again = _launch(E, dev, a, b, fill=123.5, **kw)
    assert np.array_equal(got, again), 'two launches differ, or an element was left unwritten'
    if cs['view'] != 'contiguous':         # the access path does not change a bit: the same numbers in the same order
        a2, b2 = _operands(cs['a'], cs['b'], 'contiguous', dev)
        assert np.array_equal(got, _launch(E, dev, a2, b2, **kw)), 'the access paths disagree'


@pytest.mark.parametrize('mode,c', [(0, 0.0), (0, 1.0), (1, 0.0)])
@pytest.mark.parametrize('X', [3, 1028])
def test_aliased_operands_with_delta_zero_count_nothing(mode, c, X, E, dev):
    """a is b: e == 0 exactly in every element, and the STRICT inequalities at delta = 0 count none of them"""
    rs = np.random.RandomState(X)
    a_np, _ = R.heads(9, X, mode, rs)
    a = torch.from_numpy(a_np).to(dev)
    got = _launch(E, dev, a, a, mode=mode, c=c, delta=0.0, grp=None, G=1, row_blocks=2)
    tot = got.sum(0)[0]
    assert np.all(tot[0] == 9), 'every element is valid'
    assert np.all(tot[3] == 0) and np.all(tot[4] == 0), 'e == 0 was counted as above or below delta = 0'
    assert np.all(got[:, 0, 1] == 0) and np.all(got[:, 0, 2] == 0)
    assert np.array_equal(tot[5], tot[6]) and np.allclose(tot[5], a_np.astype(np.float64).sum(0), rtol=1e-14, atol=0)


@pytest.mark.parametrize('view', ['contiguous', 'odd_offset'])
def test_nan_inf_and_zero_heads_are_invalid_and_reduce_n_only(view, E, dev):
    a_np, b_np = _special_heads()
    for c in (0.0, 1.0):
        ref = R.reference(a_np, b_np, mode=0, c=c, delta=0.25)
        a, b = _operands(a_np, b_np, view, dev)
        got = _launch(E, dev, a, b, mode=0, c=c, delta=0.25, grp=None, G=1, row_blocks=1)
        assert np.all(np.isfinite(got))
        assert np.array_equal(got[0, 0, 0], ref['value'][0, 0, 0])
        R.hold(got, ref, 'special heads, c = %g, %s' % (c, view))
    assert list(ref['value'][0, 0, 0, :6]) == [11, 11, 12, 10, 11, 12]


def test_the_launcher_checks_shapes_and_strides(E, dev):
    a = torch.ones(4, 8, device=dev)
    out = torch.zeros(1, 2, 7, 8, dtype=torch.float64, device=dev)
    g = torch.zeros(4, dtype=torch.int32, device=dev)
    kw = dict(mode=0, delta=0.25, n_groups=2)
    E.effect_cols(out, a, a, grp=g, **kw)
    with pytest.raises(ValueError, match='out must be'):
        E.effect_cols(out[:, :1], a, a, grp=g, **kw)
    with pytest.raises(ValueError, match='out must be'):
        E.effect_cols(out.float(), a, a, grp=g, **kw)
    with pytest.raises(ValueError, match='b must be'):
        E.effect_cols(out, a, a[:3], grp=g, **kw)
    with pytest.raises(ValueError, match='one group per row'):
        E.effect_cols(out, a, a, grp=g[:3], **kw)
    with pytest.raises(ValueError, match='overlap'):           # a row expanded over the rows
        E.effect_cols(out, a, a[:1].expand(4, 8), grp=g, **kw)
    with pytest.raises(RuntimeError, match='int32'):
        E.effect_cols(out, a, a, grp=g.long(), **kw)
    with pytest.raises(RuntimeError, match='invalid argument'):     # the library's own refusal reaches the caller
        E.effect_cols(out, a, a, grp=g, mode=1, delta=0.25, n_groups=2, pseudocount=1.0)
    # no rows: zeros, without a launch
    z = torch.full((1, 2, 7, 8), SENTINEL, dtype=torch.float64, device=dev)
    E.effect_cols(z, a[:0], a[:0], grp=g[:0], **kw)
    assert bool((z == 0).all())


# --------------------------------------------------------------------------------------- the model-level interface
MODELS = {
    'drvae-nb-lib': ('drvae', dict(type_rec='nb', library_size=True, x_transform='log1p_norm')),
    'pvae-zinb-gene': ('pvae', dict(type_rec='zinb', dispersion='gene')),
    'pvae-gauss': ('pvae', dict()),
}
NROWS, DIM_X, G = 37, 20, 3
SEED, EVENT = 24681357911, 2 ** 32 + 5


def _model(name, dev, **more):
    kind, kw = MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return tiny_model(kind, device=dev, dim_x=DIM_X, **dict(kw, **more))


def _dataset(name, dev):
    return CF.counts_dataset(MODELS[name][0], NROWS, DIM_X, 4, dev)       # (rows with mixed has_x2 / has_y flags)


def _groups(dev):
    r = np.arange(NROWS)
    return torch.from_numpy(np.where(r % 5 == 4, -1 - r % 2, r % G)).to(dev)      # three groups, every fifth row left out


@torch.no_grad()
def _reference(model, ds, latent, S, groups, delta, c):
    """the float64 reference on the heads decoded from ``sample_x(latent='sample')``'s latents (from ``forward()``'s heads for
    ``'mean'``), samples stacked along the rows -> (the (G, 7, X) reference, sum |a|, sum |b| per group)"""
    x1, s = ds.x1, ds.s
    if latent == 'mean':
        kw = dict(size_factor=1.0) if getattr(model, 'library_size', False) else {}      # (the UNSCALED heads: times 1.0)
        fw = model.forward(x1, s, **kw)
        heads = [(fw['px1'][0], fw['px2'][0])]
    else:
        lat = model.sample_x(x1, s, n_samples=S, latent='sample', seed=SEED, event=EVENT)
        cond = model._s_inputs(s, x1)
        heads = [(model.decoder_x([lat['z1_samp'][k]] + cond)[0], model.decoder_x([lat['z2_samp'][k]] + cond)[0]) for k in range(S)]
    A = np.concatenate([h[0].cpu().numpy() for h in heads])
    B = np.concatenate([h[1].cpu().numpy() for h in heads])
    g = np.tile(groups.cpu().numpy(), len(heads))
    mode = 1 if model.type_rec == 'diag_gaussian' else 0
    ref = R.fold_blocks(R.reference(A, B, mode=mode, c=c, delta=delta, grp=g, G=G, row_blocks=1))
    absum = lambda H: np.stack([np.abs(H[g == k].astype(np.float64)).sum(0) for k in range(G)])
    return ref, absum(A), absum(B)


@pytest.mark.parametrize('latent,S', [('mean', 1), ('sample', 3)])
@pytest.mark.parametrize('name', list(MODELS))
def test_perturbation_effect_is_the_reference_on_the_models_heads(name, latent, S, dev, E):
    model, ds, groups = _model(name, dev), _dataset(name, dev), _groups(dev)
    c = 0.0 if name == 'pvae-gauss' else 0.5
    ref, _, _ = _reference(model, ds, latent, S, groups, 0.25, c)
    assert ref['undecided'] <= R.UNDECIDED_CAP * 2 * ref['elements']
    res = model.perturbation_effect(ds, n_samples=S, latent=latent, groups=groups, n_groups=G, delta=0.25, pseudocount=c,
                                    seed=SEED, event=EVENT)
    assert list(res) == ['n', 'lfc_mean', 'lfc_sd', 'p_up', 'p_down', 'mean_base', 'mean_pert', 'raw']
    raw = res['raw']
    assert raw.dtype == torch.float64 and raw.is_cuda and tuple(raw.shape) == (G, 7, DIM_X)
    R.hold(raw.cpu().numpy(), ref, '%s latent %s' % (name, latent))
    kept = int((groups >= 0).sum())
    assert float(res['n'].sum()) == S * kept * DIM_X                       # (a pseudocount or a difference: all valid)
    n = raw[:, 0]
    for key, want in (('lfc_mean', raw[:, 1] / n), ('p_up', raw[:, 3] / n), ('p_down', raw[:, 4] / n),
                      ('mean_base', raw[:, 5] / n), ('mean_pert', raw[:, 6] / n),
                      ('lfc_sd', (raw[:, 2] / n - (raw[:, 1] / n) ** 2).clamp_min(0).sqrt())):
        assert tuple(res[key].shape) == (G, DIM_X) and torch.equal(res[key], want), key
    # one group, no groups argument: the whole set
    one = model.perturbation_effect(ds, n_samples=S, latent=latent, delta=0.25, pseudocount=c, seed=SEED, event=EVENT)
    assert tuple(one['raw'].shape) == (1, 7, DIM_X) and float(one['n'][0, 0]) == S * NROWS


@pytest.mark.parametrize('name', list(MODELS))
def test_perturbation_effect_is_independent_of_chunks_and_storage(name, dev, E):
    """counts are equal for every ``chunk_rows`` and for a ``CsrRows`` set; the sums are two float64 folds of the same at
    most T = n_samples x rows terms per element and lie within T 2^-52 sum |term| of each other (``effect_ref.fold_bound``:
    each fold is within (T - 1) 2^-53 sum |term| of the exact sum).  The Philox counter does not move."""
    model, ds, groups = _model(name, dev), _dataset(name, dev), _groups(dev)
    eng = model.engine()
    ctr = eng.rng_ctr.clone()
    c = 0.0 if name == 'pvae-gauss' else 1.0
    S = 2
    _, abs_a, abs_b = _reference(model, ds, 'sample', S, groups, 1.0, c)
    kw = dict(n_samples=S, latent='sample', groups=groups, n_groups=G, delta=1.0, pseudocount=c, seed=SEED, event=EVENT)
    whole = model.perturbation_effect(ds, **kw)['raw'].cpu().numpy()
    bound = R.fold_bound(whole, S * NROWS, abs_a, abs_b)
    sp = CF.to_csr_dataset(ds, ('x1',))
    runs = [('chunk_rows %r' % C, model.perturbation_effect(ds, chunk_rows=C, **kw)) for C in (1, 5, 37, 64, None)]
    runs += [('csr, chunk_rows %r' % C, model.perturbation_effect(sp, chunk_rows=C, **kw)) for C in (5, None)]
    for what, res in runs:
        raw = res['raw'].cpu().numpy()
        assert np.array_equal(raw[:, [0, 3, 4]], whole[:, [0, 3, 4]]), what + ': the counts differ'
        err = np.abs(raw - whole)
        print('%s: worst sum difference %.3g of the fold bound' % (what, float(np.max(np.where(err == 0, 0, err / np.maximum(bound, 1e-300))))))
        assert np.all(err <= bound), what
    assert torch.equal(eng.rng_ctr, ctr), 'the training counter moved'


def test_group_arguments(dev, E):
    model, ds = _model('pvae-zinb-gene', dev), _dataset('pvae-zinb-gene', dev)
    groups = _groups(dev)
    with pytest.raises(ValueError, match='n_groups'):
        model.perturbation_effect(ds, groups=groups)
    with pytest.raises(ValueError, match='>= n_groups'):
        model.perturbation_effect(ds, groups=groups, n_groups=2)
    with pytest.raises(ValueError, match='integer tensor of shape'):
        model.perturbation_effect(ds, groups=groups[:5], n_groups=G)
    with pytest.raises(ValueError, match='integer tensor of shape'):
        model.perturbation_effect(ds, groups=groups.float(), n_groups=G)
    # a group without rows: n == 0 and NaN ratios; zero means without a pseudocount are invalid, not -inf
    res = model.perturbation_effect(ds, groups=groups, n_groups=G + 1)
    assert bool((res['n'][G] == 0).all()) and bool(res['lfc_mean'][G].isnan().all()) and bool(res['p_up'][G].isnan().all())
    assert bool(res['lfc_mean'][:G].isfinite().all())


def test_perturbation_effect_leaves_training_untouched(dev):
    """the same model trained one step with and without a summary in front of it: the same parameters, optimizer state
    (through the step's result) and Philox counter"""
    from tests.test_anneal_cpu import _model_batch
    name = 'drvae-nb-lib'
    ds = _dataset(name, dev)
    states = []
    for first in (False, True):
        model = _model(name, dev)
        batch = {k: v.to(dev) for k, v in _model_batch(model).items()}
        batch['x1'], batch['x2'] = batch['x1'].abs().round(), batch['x2'].abs().round()      # (counts)
        model.engine()
        if first:
            before = {k: v.clone() for k, v in model.state_dict().items()}
            model.perturbation_effect(ds, n_samples=2, latent='sample', chunk_rows=8, groups=_groups(dev), n_groups=G)
            model.perturbation_effect(ds)
            after = model.state_dict()
            assert all(torch.equal(before[k], after[k]) for k in before), 'a parameter moved'
        for _ in range(2):
            model.run_on_batch(train_mode=True, **batch)
        torch.cuda.synchronize()
        states.append(({k: v.clone() for k, v in model.state_dict().items()}, model.engine().rng_ctr.clone()))
    (a, ca), (b, cb) = states
    assert torch.equal(ca, cb)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
