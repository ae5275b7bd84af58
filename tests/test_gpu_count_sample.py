"""-m gpu: the posterior-predictive sampler (``count_sample.draw``: the ``dv_draw_desc`` form of ``dv_fill_normal``) against the
float64 reference of the header's specification (``tests/count_sample_ref.py``), and the model-level interface on top.

The rule of every comparison (``count_sample_ref.compare``): an element the reference DECIDES -- every decision it took stands
further from its threshold than fp32 rounding of the specified arithmetic can move it -- must be EQUAL (the Gaussian kind:
within the normal's bound times sd); an undecided one must be finite, non-negative and integral; the undecided share of the
reference stays under 2 % (asserted for the grid on the CPU, ``tests/test_count_sample_cpu.py``, and here per model)."""
import warnings

import numpy as np
import pytest
import torch

from tests import count_sample_ref as R
from tests import csr_feed_ref as CF
from tests import philox_ref as P
from tests.test_count_sample_cpu import Z_MAX, z_scores
from tests.test_dropout_cpu import tiny_model

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 3            # guard columns behind every row of ``out``, guard rows around it


@pytest.fixture(scope='module')
def CS(dev):
    from drvae_amd import _lib, count_sample
    _lib.load()
    return count_sample


def _view(a, dev, misalign, pad=0):
    """the (M, X) array ``a`` on the device as rows of stride X + pad in a buffer of its own; ``misalign``: the first row starts
    one float behind a 16-byte boundary (the scalar path); else X + pad is rounded up to a multiple of 4 (the quad path,
    where X % 4 == 0)"""
    a = np.asarray(a, np.float32)
    M, X = a.shape
    ld = X + pad
    if not misalign:
        ld = (ld + 3) // 4 * 4
    buf = torch.full((M * ld + 8,), SENTINEL, device=dev)
    off = 1 if misalign else 0
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + M * ld].view(M, ld)[:, :X]
    v.copy_(torch.from_numpy(a))
    return v


def _launch(CS, dev, case, misalign, S=None, sample0=0, rows=None, row0=None, grow=None):
    """one launch of a grid case (all of its rows or the rows ``rows``) into a sentinel-filled buffer with guard rows and
    columns: the guards are intact, the operands unmodified -> out (S, M, X), numpy"""
    ops, X = case['ops'], case['X']
    sel = np.arange(case['M']) if rows is None else np.asarray(rows)
    M = sel.size
    S = case['S'] if S is None else S
    dops, keep = {}, {}
    for k, v in ops.items():
        if k == 'size':
            dops[k] = torch.from_numpy(np.ascontiguousarray(v[sel])).to(dev)
        elif k == 'theta' and v.ndim == 1:
            dops[k] = _view(v[None], dev, misalign).expand(M, X)          # ONE shared row: stride 0
        else:
            dops[k] = _view(v[sel], dev, misalign)
        keep[k] = dops[k].clone()
    ld = X + PAD if misalign else (X + PAD + 3) // 4 * 4
    per = (M + 2) * ld                                   # a guard row in front of and behind every sample
    buf = torch.full((S * per + 8,), SENTINEL, device=dev)
    off = 1 if misalign else 0
    whole = buf[off:off + S * per].view(S, M + 2, ld)
    out = whole[:, 1:M + 1, :X]
    CS.draw(out, dops['mu'], kind=case['kind'], seed=case['seed'], event=case['event'],
            row0=(case['row0'] if row0 is None else row0) if grow is None else 0, grow=grow, sample0=sample0,
            **{k: v for k, v in dops.items() if k != 'mu'})
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert bool(((dops[k] == v) | (dops[k].isnan() & v.isnan())).all()), 'operand %s was modified' % k
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[off:off + S * per].view(S, M + 2, ld)[:, 1:M + 1, :X] = True
    assert bool((buf[~mask] == SENTINEL).all()), 'an element outside the described ones was written'
    return out.cpu().numpy()


def _hold(got, ref, what):
    wrong, und = R.compare(got, ref)
    print('%s: %d elements, %d undecided, %d differ from the reference, %d wrong' % (
        what, got.size, int(und.sum()), int((got != ref['value']).sum()), int(wrong.sum())))
    if wrong.any():
        i = np.argwhere(wrong)[0]
        raise AssertionError('%s: element %r: got %r, reference %r (margin %g, tol %g); %d wrong in all' % (
            what, tuple(i), got[tuple(i)], ref['value'][tuple(i)], ref['margin'][tuple(i)], ref['tol'][tuple(i)], int(wrong.sum())))


# --------------------------------------------------------------------------------------- the kernel against the reference
@pytest.mark.parametrize('i', range(len(R.GRID_SHAPES)))
@pytest.mark.parametrize('kind', R.GRID_KINDS)
def test_kernel_equals_the_reference_on_both_access_paths(kind, i, CS, dev):
    case, ref = R.grid_reference(kind, i)
    outs = {}
    for misalign in (False, True):
        outs[misalign] = _launch(CS, dev, case, misalign)
        _hold(outs[misalign], ref, '%s X %d M %d S %d %s' % (kind, case['X'], case['M'], case['S'],
                                                             'scalar path' if misalign or case['X'] % 4 else 'quad path'))
    assert np.array_equal(outs[False], outs[True], equal_nan=True), 'the two access paths disagree'


# --------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize('kind', ['diag_gaussian', 'poisson', 'zinb'])
def test_an_element_depends_on_its_coordinates_only(kind, CS, dev):
    case = R.grid_case(kind, 2)                                    # X 4 (quad), M 9, S 3, per-element theta, a size vector
    M = case['M']
    full = _launch(CS, dev, case, False)
    assert np.array_equal(full, _launch(CS, dev, case, False), equal_nan=True), 'two launches differ'
    # rows in pieces with their row0, and shuffled with a ``grow`` array
    for lo, hi in ((0, 4), (4, 5), (5, 9)):
        part = _launch(CS, dev, case, True, rows=np.arange(lo, hi), row0=case['row0'] + lo)
        assert np.array_equal(part, full[:, lo:hi], equal_nan=True), (lo, hi)
    perm = np.random.RandomState(0).permutation(M)
    grow = torch.from_numpy((case['row0'] + perm).astype(np.int32)).to(dev)
    shuffled = _launch(CS, dev, case, False, rows=perm, grow=grow)
    assert np.array_equal(shuffled, full[:, perm], equal_nan=True)
    # sample k of the S = 3 launch is the S = 1 launch at that sample index
    for k in range(case['S']):
        one = _launch(CS, dev, case, False, S=1, sample0=k)
        assert np.array_equal(one[0], full[k], equal_nan=True), k
    assert not np.array_equal(full[0], full[1]) and not np.array_equal(full[1], full[2])
    # another seed, another event: other draws
    for change in (dict(seed=case['seed'] + 1), dict(event=case['event'] + 1), dict(event=case['event'] + 2 ** 32)):
        assert not np.array_equal(full, _launch(CS, dev, dict(case, **change), False), equal_nan=True), change


# --------------------------------------------------------------------------------------- the law, on the device
@pytest.mark.parametrize('kind', ['nb', 'zinb'])
def test_device_draws_have_the_law(kind, CS, dev):
    """one (row, gene) operand repeated over 2^17 elements: mean and zero fraction within 5 standard errors of the analytic
    values (the reference passes first: tests/test_count_sample_cpu.py)"""
    n, mu, theta, logit = 2 ** 17, 6.0, 1.7, float(np.log(0.6 / 0.4))
    out = torch.empty(1, 1, n, device=dev)
    full = lambda v: torch.full((1, n), v, device=dev)
    CS.draw(out, full(mu), kind=kind, theta=full(theta), logit=full(logit) if kind == 'zinb' else None, seed=2024, event=9)
    v = out.cpu().numpy().reshape(-1)
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and np.all(v == np.floor(v))
    pi = 1.0 / (1.0 + np.exp(-float(np.float32(logit)))) if kind == 'zinb' else 0.0
    law = R.law(float(np.float32(mu)), float(np.float32(theta)), pi)
    host = lambda t: None if t is None else np.full((1, n), t, np.float32)
    ref = R.draw(kind, mu=host(mu), theta=host(theta), logit=host(logit) if kind == 'zinb' else None, seed=2024, event=9)
    assert max(abs(t) for t in z_scores(ref['value'], law)) <= Z_MAX, 'the reference itself misses the law at this seed'
    _hold(out.cpu().numpy(), ref, kind + ' 2^17 draws of one operand')
    z = z_scores(v, law)
    print('%s: mean %+.2f, P(0) %+.2f, P(x <= floor(mean)) %+.2f standard errors' % ((kind,) + z))
    assert max(abs(t) for t in z) <= Z_MAX, z


# --------------------------------------------------------------------------------------- defined behaviour
def test_heads_outside_the_domain_give_the_stated_results(CS, dev):
    """NaN, inf, 0, negative heads and rates beyond 2^24: the launch returns (every loop is bounded) and writes what the header
    states -- the reference's values, NaN for NaN"""
    nan, inf = np.nan, np.inf
    fmax = float(np.finfo(np.float32).max)
    mu = np.array([[nan, 0.0, -3.0, inf, 2.0, 2.0, 2.0, 2.0, 1e8, 2.0, 3e7, 1e-30, 5.0, -inf, 1e38, 2.0, 5.0, 5.0, fmax]], np.float32)
    th = np.array([[1.0, 1.0, 1.0, 1.0, nan, 0.0, -1.0, inf, 1e9, 1.0, inf, 1e-3, 1e-30, 1.0, 1e38, -inf, 1e-40, 1e-45, 1e30]], np.float32)
    lg = np.array([[0.0, -30.0, -30.0, -30.0, 0.0, 0.0, 0.0, -30.0, -30.0, nan, -inf, inf, -200.0, 0.0, -90.0, 1.0, -30.0, -30.0, -30.0]],
                  np.float32)
    mu, th, lg = (np.repeat(a, 3, 0) for a in (mu, th, lg))
    size = np.array([1.0, 1e30, 0.0], np.float32)
    for kind in ('poisson', 'nb', 'zinb', 'binary'):
        ops = dict(mu=mu)
        if kind in ('nb', 'zinb'):
            ops['theta'] = th
        if kind == 'zinb':
            ops['logit'] = lg
        if kind != 'binary':
            ops['size'] = size
        case = dict(kind=kind, X=mu.shape[1], M=3, S=2, seed=99, event=0, row0=0, ops=ops)
        ref = R.draw(kind, S=2, seed=99, **ops)
        assert not ref['cap'].any()
        got = _launch(CS, dev, case, False)
        _hold(got, ref, kind + ' outside the domain')
        assert np.array_equal(np.isnan(got), np.isnan(ref['value']))
    # the Gaussian kind is plain IEEE arithmetic: NaN and inf propagate
    ops = dict(mu=np.array([[nan, 0.0, -3.0, inf, 2.0, 2.0, -inf, 1.0]], np.float32),
               sd=np.array([[1.0, 0.0, nan, 1.0, inf, -1.0, 2.0, 1e-30]], np.float32))
    ref = R.draw('diag_gaussian', S=2, seed=99, **ops)
    got = _launch(CS, dev, dict(kind='diag_gaussian', X=8, M=1, S=2, seed=99, event=0, row0=0, ops=ops), False)
    fin = np.isfinite(ref['value'])
    assert np.array_equal(np.isnan(got), np.isnan(ref['value'])) and np.array_equal(got[~fin], ref['value'][~fin], equal_nan=True)
    assert np.all(np.abs(got[fin] - ref['value'][fin]) <= ref['tol'][fin])


# --------------------------------------------------------------------------------------- the model-level interface
MODELS = {
    'drvae-poisson': ('drvae', dict(type_rec='poisson')),
    'pvae-nb-lib-norm': ('pvae', dict(type_rec='nb', library_size=True, x_transform='log1p_norm')),
    'vfae-zinb-use_s-gene-batch': ('vfae', dict(type_rec='zinb', use_s=True, dim_s=2, dispersion='gene-batch')),
    'drvae-nb-gene': ('drvae', dict(type_rec='nb', dispersion='gene')),
    'pvae-gauss': ('pvae', dict()),
}
NROWS, DIM_X = 37, 20


def _model(name, dev, **more):
    kind, kw = MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return tiny_model(kind, device=dev, dim_x=DIM_X, **dict(kw, **more))


def _dataset(name, dev):
    kind, kw = MODELS[name]
    return CF.counts_dataset(kind, NROWS, DIM_X, 4, dev, n_s=kw.get('dim_s', 1))


def _ref_of_heads(model, px, S, seed, event, row0, sample0=0, size=None):
    """the reference on finished heads ``px`` (device tensors, as ``forward`` returns them)"""
    n = lambda t: t.detach().cpu().numpy()
    tr = model.type_rec
    ops = dict(mu=n(px[0]))
    if tr == 'diag_gaussian':
        ops['sd'] = n(px[1])
    if tr in ('nb', 'zinb'):
        ops['theta'] = n(px[1])
    if tr == 'zinb':
        ops['logit'] = n(px[2])
    if size is not None:
        ops['size'] = n(size)
    return R.draw(tr, S=S, seed=seed, event=event, row0=row0, sample0=sample0, **ops)


def _hold_model(got, ref, what):
    _hold(got.cpu().numpy(), ref, what)
    assert (ref['margin'] < 1).mean() <= R.UNDECIDED_CAP, what


@pytest.mark.parametrize('name', list(MODELS))
def test_sample_x_at_the_posterior_mean_is_the_reference_on_forwards_heads(name, dev, CS):
    model, ds = _model(name, dev), _dataset(name, dev)
    x1, s = ds.x1[:9], ds.s[:9]
    kw = dict(size_factor=0.7) if getattr(model, 'library_size', False) else {}
    fw = model.forward(x1, s, **kw)
    seed, event, row0 = 123456789123, 2 ** 32 + 7, 11
    got = model.sample_x(x1, s, n_samples=3, seed=seed, event=event, row0=row0, **kw)
    assert list(got) == (['x1_samp', 'x2_samp'] if model.kind != 'vfae' else ['x1_samp'])
    assert tuple(got['x1_samp'].shape) == (3, 9, DIM_X)
    # forward()'s means carry the size factor already (ONE fp32 product, the kernel's): the reference takes them as they are
    _hold_model(got['x1_samp'], _ref_of_heads(model, fw['px1'], 3, seed, event, row0), name + ' x1_samp')
    if model.kind != 'vfae':
        _hold_model(got['x2_samp'], _ref_of_heads(model, fw['px2'], 3, seed ^ CS.X2_SEED_XOR, event, row0), name + ' x2_samp')
    # the default seed; rows sampled as a piece with its row0 are those rows' draws
    a = model.sample_x(x1, s, n_samples=2, **kw)
    _hold_model(a['x1_samp'], _ref_of_heads(model, fw['px1'], 2, CS.default_seed(model.random_seed), 0, 0), name + ' default seed')
    b = model.sample_x(x1[4:], s[4:], n_samples=2, row0=4, **kw)
    _hold_model(b['x1_samp'], _ref_of_heads(model, [h[4:] for h in fw['px1']], 2, CS.default_seed(model.random_seed), 0, 4),
                name + ' rows 4 .. 8 with row0 = 4')


def test_sample_x_inside_averaged_parameters(dev, CS):
    model = _model('drvae-poisson', dev, ema_decay=0.9)
    ds = _dataset('drvae-poisson', dev)
    model.engine()
    with model.averaged_parameters():
        fw = model.forward(ds.x1[:5], ds.s[:5])
        got = model.sample_x(ds.x1[:5], ds.s[:5], seed=5)
    _hold_model(got['x1_samp'], _ref_of_heads(model, fw['px1'], 1, 5, 0, 0), 'averaged parameters')


@pytest.mark.parametrize('name', list(MODELS))
@torch.no_grad()
def test_sample_x_with_sampled_latents(name, dev, CS):
    """``latent='sample'``: z1 / z2 are the specified row-keyed draws (draw ids 2k / 2k + 1 under seed ^ LATENT_SEED_XOR), and
    the counts are the reference on the heads decoded from them"""
    model, ds = _model(name, dev), _dataset(name, dev)
    x1, s = ds.x1[:9], ds.s[:9]
    seed, event, row0, S = 987654321, 3, 5, 2
    got = model.sample_x(x1, s, n_samples=S, latent='sample', seed=seed, event=event, row0=row0)
    cond = model._s_inputs(s, x1)
    qz1 = model.encoder_z1([model._enc_x(x1)] + cond)
    size = model.size_factor(x1) if getattr(model, 'library_size', False) else None
    Z = model.dim_z1
    U = 2.0 ** -24
    for k in range(S):
        z, r, a = P.row_draws(row0 + np.arange(9), Z, 2 * k, seed ^ CS.LATENT_SEED_XOR, event)
        mu, sd = qz1[0].double().cpu().numpy(), np.exp(0.5 * qz1[1].double().cpu().numpy())
        z1 = got['z1_samp'][k]
        assert np.all(np.abs(z1.double().cpu().numpy() - (mu + sd * z)) <= sd * 4 * U * (r + r * a) + 8 * U * (np.abs(mu) + np.abs(sd * z)))
        px = model.decoder_x([z1] + cond)
        _hold_model(got['x1_samp'][k:k + 1], _ref_of_heads(model, px, 1, seed, event, row0, sample0=k, size=size),
                    '%s latent sample %d' % (name, k))
        if model.kind != 'vfae':
            pz2 = model.decoder_z2Fz1([z1])
            z, r, a = P.row_draws(row0 + np.arange(9), Z, 2 * k + 1, seed ^ CS.LATENT_SEED_XOR, event)
            mu, sd = pz2[0].double().cpu().numpy(), np.exp(0.5 * pz2[1].double().cpu().numpy())
            z2 = got['z2_samp'][k]
            assert np.all(np.abs(z2.double().cpu().numpy() - (mu + sd * z)) <= sd * 4 * U * (r + r * a) + 8 * U * (np.abs(mu) + np.abs(sd * z)))
            px = model.decoder_x([z2] + cond)
            # x2_samp is drawn at x1's size factor
            _hold_model(got['x2_samp'][k:k + 1], _ref_of_heads(model, px, 1, seed ^ CS.X2_SEED_XOR, event, row0, sample0=k, size=size),
                        '%s latent sample %d, x2' % (name, k))
    assert not torch.equal(got['x1_samp'][0], got['x1_samp'][1])


@pytest.mark.parametrize('name', ['pvae-nb-lib-norm', 'vfae-zinb-use_s-gene-batch', 'drvae-nb-gene'])
def test_posterior_predictive_is_independent_of_chunks_and_storage(name, dev, CS):
    model, ds = _model(name, dev), _dataset(name, dev)
    eng = model.engine()
    ctr = eng.rng_ctr.clone()
    for latent in ('mean', 'sample'):
        whole = model.posterior_predictive(ds, 2, latent=latent, seed=31, event=4)
        assert tuple(whole.shape) == (2, NROWS, DIM_X) and whole.is_cuda
        for C in (1, 5, 37, 64):
            assert torch.equal(model.posterior_predictive(ds, 2, chunk_rows=C, latent=latent, seed=31, event=4), whole), (latent, C)
        sp = CF.to_csr_dataset(ds, ('x1',))
        assert torch.equal(model.posterior_predictive(sp, 2, chunk_rows=5, latent=latent, seed=31, event=4), whole), latent
        host = torch.empty(2, NROWS, DIM_X).pin_memory()
        assert model.posterior_predictive(ds, 2, chunk_rows=16, out=host, latent=latent, seed=31, event=4) is host
        assert torch.equal(host, whole.cpu())
        on_dev = torch.full((2, NROWS, DIM_X), SENTINEL, device=dev)
        model.posterior_predictive(sp, 2, chunk_rows=8, out=on_dev, latent=latent, seed=31, event=4)
        assert torch.equal(on_dev, whole)
    # x1_samp of sample_x on the whole set is the same draw
    assert torch.equal(model.sample_x(ds.x1, ds.s, n_samples=2, seed=31, event=4)['x1_samp'],
                       model.posterior_predictive(ds, 2, chunk_rows=5, seed=31, event=4))
    assert torch.equal(eng.rng_ctr, ctr), 'the training counter moved'


def test_posterior_predictive_leaves_training_untouched(dev):
    """the same model trained one step with and without a draw in front of it: the same bits, the same counter"""
    from tests.test_anneal_cpu import _model_batch
    name = 'pvae-nb-lib-norm'
    ds = _dataset(name, dev)
    states = []
    for sample_first in (False, True):
        model = _model(name, dev)
        batch = {k: v.to(dev) for k, v in _model_batch(model).items()}
        batch['x1'], batch['x2'] = batch['x1'].abs().round(), batch['x2'].abs().round()      # (counts)
        model.engine()
        if sample_first:
            model.posterior_predictive(ds, 2, chunk_rows=8, latent='sample')
            model.sample_x(ds.x1[:4], ds.s[:4])
        model.run_on_batch(train_mode=True, **batch)
        torch.cuda.synchronize()
        states.append(({k: v.clone() for k, v in model.state_dict().items()}, model.engine().rng_ctr.clone()))
    (a, ca), (b, cb) = states
    assert torch.equal(ca, cb)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
