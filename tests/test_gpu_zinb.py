"""GPU: the zero-inflated negative-binomial data decoder (``type_rec='zinb'``) on the real kernels -- ``dv_rec_nll_rows`` kinds
``DV_REC_ZINB`` / ``DV_REC_ZINB_LIB`` against float64 within the bound of ``tests/zinb_ref.py`` (shapes, gather, memory contract,
both paths, the edge grid), the block, the fused step against the model-level float64 reference (eager == captured, host-fed ==
feed, the riders together), the model class and ``fit`` against the negative-binomial model."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import ref64
from tests import zinb_ref as Z
from tests.test_nb_cpu import make_engine, set_batch
from tests.test_zinb_cpu import SWITCHES, _case, combined_against_reference, host_fed_equals_feed

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GPU_TOL = ((1e-4, 2e-5), None, (2e-4, 5e-5))      # losses / (gradients: not compared) / parameters: tests/test_gpu_counts.py's


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert _lib.REC_KIND['zinb'] == 5 and _lib.REC_KIND['zinb_lib'] == 6
    return K


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


# --------------------------------------------------------------------------------- 1. shapes, memory contract
def _random_case(Mr, X, n_src=7, seed=1):
    """integer counts (a third zeros, a few at 1500), heads from random pre-activations, logits over +-8, a gather that repeats
    and permutes"""
    g = torch.Generator().manual_seed(seed + 131 * X + Mr)
    mu = F.softplus(torch.randn(Mr, X, generator=g) * 3) + Z.MU_SHIFT
    th = F.softplus(torch.randn(Mr, X, generator=g) * 3) + Z.THETA_SHIFT
    a = torch.randn(Mr, X, generator=g) * 4
    xs = torch.poisson(torch.rand(n_src, X, generator=g) * 6)
    xs[torch.rand(n_src, X, generator=g) < 0.33] = 0.0
    xs[torch.rand(n_src, X, generator=g) < 0.05] = 1500.0
    xi = torch.tensor([3, 0, 3, 6, 1], dtype=torch.int32)[:Mr]
    coef = torch.randn(Mr, generator=g)
    return xs, mu, th, a, xi, coef


def _launch(K, dev, xs, mu, th, a, xi, coef, library, pad, misalign=False):
    """operands as strided views inside sentinel-filled buffers; returns (rows, gradients, the buffers for the guard check)"""
    Mr, X = mu.shape
    ld = 3 * X + pad
    vbuf = torch.full((Mr + 2, ld), SENTINEL)
    vbuf[:Mr, :X], vbuf[:Mr, X:2 * X], vbuf[:Mr, 2 * X:3 * X] = mu, th, a
    vbuf = vbuf.to(dev)
    dbuf = torch.full((Mr + 2, ld), SENTINEL, device=dev)
    obuf = torch.full((Mr + 2,), SENTINEL, device=dev)
    v, d, o = vbuf[:Mr, :3 * X], dbuf[:Mr, :3 * X], obuf[:Mr]
    assert v.stride(0) > 3 * X and (v.stride(0) % 4 != 0) == misalign
    K.rec_nll_rows(o, xs.to(dev), v, kind='zinb', shift=Z.MU_SHIFT, xidx=xi.to(dev), coef=None if coef is None else coef.to(dev),
                   dpre=d if coef is not None else None, library=library)
    ob, db, vb = host(obuf), host(dbuf), host(vbuf)
    assert bool((ob[Mr:] == SENTINEL).all()) and bool((db[Mr:] == SENTINEL).all()) and bool((db[:, 3 * X:] == SENTINEL).all())
    assert bool((vb[:, 3 * X:] == SENTINEL).all()) and bool((vb[Mr:] == SENTINEL).all())
    if coef is None:
        assert bool((db == SENTINEL).all())
    return ob[:Mr], db[:Mr, :3 * X]


def _check(tag, rows, grads, ref, X, frac=None):
    w = [ref64.check(tag + ' rows', rows, ref['rows'], ref['rows_bound'])]
    if grads is not None:
        for i, k in enumerate(('gm', 'gt', 'gd')):
            w.append(ref64.check('%s %s' % (tag, k), grads[:, i * X:(i + 1) * X], ref[k], ref[k + '_bound']))
    if frac is not None:
        frac.append((tag, w))
    return w


@pytest.mark.parametrize('library', [False, True], ids=['zinb', 'zinb_lib'])
@pytest.mark.parametrize('X', [1, 3, 4, 13, 260, 1028])
def test_kernel_against_the_reference_and_its_memory_contract(K, dev, X, library):
    """5 rows through a gather that repeats and permutes 7 source rows, with and without ``coef``; X = 1, 3, 13: the scalar
    path, 4: one 16-byte quad, 260: the scalar loop's second trip (row stride no multiple of 4), 1028: the 16-byte loop's
    second trip.  On 4 | X both paths run (aligned and misaligned row stride) and agree within the bound; repeats are bit-equal"""
    xs, mu, th, a, xi, coef = _random_case(5, X)
    ref = Z.reference(xs[xi.long()], mu, th, a, coef=coef, library=library)
    pads = [8, 5] if X % 4 == 0 else [5]      # (pad 5 on 4 | X: a misaligned row stride, the dispatcher takes the scalar path)
    got = {}
    for pad in pads:
        mis = (3 * X + pad) % 4 != 0
        rows, grads = _launch(K, dev, xs, mu, th, a, xi, coef, library, pad, misalign=mis)
        _check('X=%d pad=%d' % (X, pad), rows, grads, ref, X)
        again = _launch(K, dev, xs, mu, th, a, xi, coef, library, pad, misalign=mis)
        assert torch.equal(again[0], rows) and torch.equal(again[1], grads)
        rows_only, _ = _launch(K, dev, xs, mu, th, a, xi, None, library, pad, misalign=mis)
        _check('X=%d pad=%d, no coef' % (X, pad), rows_only, None, ref, X)
        got[pad] = (rows, grads)
    if len(got) == 2:      # 16-byte path against the scalar path: both inside the bound of the same reference
        (r8, g8), (r5, g5) = got[8], got[5]
        assert torch.all((r8.double() - r5.double()).abs() <= 2 * ref['rows_bound'])
        for i, k in enumerate(('gm', 'gt', 'gd')):
            assert torch.all((g8[:, i * X:(i + 1) * X].double() - g5[:, i * X:(i + 1) * X].double()).abs() <= 2 * ref[k + '_bound'])


def test_refusals_and_no_rows(K, dev):
    X = 4
    x, v = torch.zeros(4, X, device=dev), torch.ones(4, 3 * X, device=dev)
    out, d = torch.full((4,), SENTINEL, device=dev), torch.full((4, 3 * X), SENTINEL, device=dev)
    coef = torch.ones(4, device=dev)
    from drvae_amd import _lib
    lib = _lib.load()
    f, st = K._f32, K._stream()
    for kind in (5, 6):
        call = lambda ldv, ldd, vv=v, cc=coef, dd=d, Mr=4: lib.dv_rec_nll_rows(kind, 1e-6, f(cc), f(x), X, None, f(vv), ldv, Mr, X,
                                                                              f(out), f(dd), ldd, st)
        assert call(3 * X - 1, 3 * X) != 0 and call(3 * X, 3 * X - 1) != 0        # ldv / ldd below 3X
        assert call(3 * X, 3 * X, vv=None) != 0 and call(3 * X, 3 * X, dd=None) != 0     # a missing operand with M > 0
        assert call(3 * X, 3 * X, vv=None, cc=None, dd=None, Mr=0) == 0           # M == 0: a no-op
    assert lib.dv_rec_nll_rows(7, 1e-6, None, f(x), X, None, f(v), 3 * X, 4, X, f(out), None, 0, st) != 0
    K.rec_nll_rows(out[:0], x, v[:0], kind='zinb', shift=Z.MU_SHIFT, coef=coef[:0], dpre=d[:0])
    assert bool((host(out) == SENTINEL).all()) and bool((host(d) == SENTINEL).all())


# ------------------------------------------------------------------------------------------- 2. edge grid
@pytest.mark.parametrize('library', [False, True], ids=['zinb', 'zinb_lib'])
def test_edge_grid_within_the_bound(K, dev, library):
    """``nb_ref``'s edge grid crossed with logits -30 .. 30, more than half of it zeros: rows and the three gradient blocks
    within the bound, on the 16-byte path (X = 256) and on the scalar path (its first 255 columns)"""
    x, mu, th, a, coef = Z.edge_grid()
    for Xs in (256, 255):
        xs, ms, ts, as_ = (t[:, :Xs].contiguous() for t in (x, mu, th, a))
        if library:      # integer counts: the rows' own totals are the size factors (0.004 .. 3e4 over the grid)
            ref = Z.reference(xs, ms, ts, as_, coef=coef, library=True)
        else:
            ref = Z.reference(xs, ms, ts, as_, coef=coef)
        Mr = xs.shape[0]
        out, dpre = torch.full((Mr,), SENTINEL, device=dev), torch.full((Mr, 3 * Xs), SENTINEL, device=dev)
        K.rec_nll_rows(out, xs.to(dev), torch.cat([ms, ts, as_], 1).to(dev), kind='zinb', shift=Z.MU_SHIFT, coef=coef.to(dev),
                       dpre=dpre, library=library)
        rows, g = host(out), host(dpre)
        worst = [float(ref64.excess(rows, ref['rows'], ref['rows_bound']).max())] + \
            [float(ref64.excess(g[:, i * Xs:(i + 1) * Xs], ref[k], ref[k + '_bound']).max()) for i, k in enumerate(('gm', 'gt', 'gd'))]
        print('edge grid (%s, X = %d), worst |err| / bound: rows %.3g  d/da_m %.3g  d/da_t %.3g  d/da_d %.3g'
              % (('zinb_lib' if library else 'zinb', Xs) + tuple(worst)))
        _check('edge grid X=%d' % Xs, rows, g, ref, Xs)


def test_a_row_whose_total_is_X_equals_the_unscaled_kind_bit_for_bit(K, dev):
    for X in (12, 13):
        xs, mu, th, a, _, coef = _random_case(5, X, n_src=5)
        xs[:] = 1.0
        xs[0, :2] = torch.tensor([0.0, 2.0])          # (still a total of X, with a zero in it)
        xs[3, :4] = torch.tensor([0.0, 0.0, 3.0, 1.0])
        assert bool((xs.sum(1) == X).all())
        res = []
        for library in (False, True):
            out, d = torch.zeros(5, device=dev), torch.zeros(5, 3 * X, device=dev)
            K.rec_nll_rows(out, xs.to(dev), torch.cat([mu, th, a], 1).to(dev), kind='zinb', shift=Z.MU_SHIFT, coef=coef.to(dev),
                           dpre=d, library=library)
            res.append((host(out), host(d)))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ 3. block
def test_block_forward_and_logp_match_float64(dev):
    from drvae_amd import blocks as blk
    g = torch.Generator().manual_seed(5)
    z = torch.randn(16, 5, generator=g)
    x = torch.poisson(torch.rand(16, 13, generator=g) * 8) * (torch.rand(16, 13, generator=g) > 0.4)
    x[0, 3] = 2500.0
    for wn in (False, True):
        torch.manual_seed(3)
        dec = blk.ZeroInflatedNegativeBinomialDecoder([5], [8], 13, nonlin='elu', weight_norm=wn).to(dev)
        if wn:
            dec([z.to(dev)])                      # (WeightNorm's data-dependent initialisation happens on first use)
        p64 = {k: v.detach().cpu().double() for k, v in dec.named_parameters()}

        def lin(h, q):
            w, b = p64[q + '.weight'], p64[q + '.bias']
            if q + '.g' in p64:
                w = w * (p64[q + '.g'] / w.norm(dim=1))[:, None]
            return h @ w.t() + b
        h = F.elu(lin(z.double(), 'nnet.model.linear1'))
        mu64 = F.softplus(lin(h, 'decoder_m.linear_m')) + Z.MU_SHIFT
        th64 = F.softplus(lin(h, 'decoder_t.linear_t')) + Z.THETA_SHIFT
        lg64 = lin(h, 'decoder_d.linear_d')
        lp64 = Z.logp64(x.double(), mu64, th64, lg64).sum(1)
        with torch.no_grad():
            mu, th, lg = dec([z.to(dev)])
            lp = dec.logp_perx(x.to(dev), mu, th, lg)
        np.testing.assert_allclose(host(mu).numpy(), mu64.numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(host(th).numpy(), th64.numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(host(lg).numpy(), lg64.numpy(), rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(host(lp).numpy(), lp64.numpy(), rtol=2e-5, atol=1e-4)
        s = dec.sample(mu, th, lg)
        assert tuple(s.shape) == (16, 13) and bool((s >= 0).all()) and bool((s == s.floor()).all())


# ----------------------------------------------------------------------------------------- 4. fused step
@pytest.mark.parametrize('sw', ['off', 'both'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_matches_float64_and_eager_equals_captured(kind, sw, dev):
    """16 rows at the tiny sizes of ``tests/test_gpu_nb.py``: a train-mode pass and three Adam steps against the model-level
    float64 reference; then three steps eager and captured (Philox noise): equal bit for bit"""
    from tests.test_zinb_cpu import run_against_reference
    run_against_reference(kind, 'plain', sw, dev, tol=GPU_TOL)
    spec, batch = _case(kind, add_noise_var=0.01 if SWITCHES[sw] else 0.0)
    params = Z.ModelRef(spec, seed=9).engine_params()
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, params, dev, type_rec='zinb', **SWITCHES[sw])
        set_batch(eng, batch, dev)
        eng.train_step()
        losses = [eng.losses()]
        for _ in range(2):
            if captured:
                if eng._graph_key is None:
                    eng.capture()
                eng.replay()
            else:
                eng.train_step()
            losses.append(eng.losses())
        torch.cuda.synchronize()
        out.append(([getattr(arena, w).clone() for w in ('param', 'exp_avg', 'exp_avg_sq')], losses))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0])) and out[0][1] == out[1][1]
    assert all(np.isfinite(v) for l in out[0][1] for v in l.values())


@pytest.mark.parametrize('variant', ['weight_norm', 'universal'])
def test_fused_step_variants_match_float64(variant, dev):
    from tests.test_zinb_cpu import run_against_reference
    run_against_reference('drvae', variant, 'both', dev, tol=GPU_TOL)


@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
def test_host_fed_step_equals_feed_step_bit_for_bit(captured, dev):
    host_fed_equals_feed('drvae', dev, captured=captured)


def test_combined_riders_match_the_float64_model_reference(dev):
    combined_against_reference(dev, tol=GPU_TOL)


# -------------------------------------------------------------------------------------------- 5. model class
def _model(kind, type_rec, dev, **kw):
    from tests.test_fit import _tiny_model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return _tiny_model(kind, device=dev, type_rec=type_rec, add_noise_var=0.0, x_transform='log1p', **kw)


def _batch_kw(kind, ds, n=16):
    kw = dict(x1=ds.x1[:n], s=ds.s[:n], y=ds.y[:n], has_y=ds.has_y[:n])
    if kind != 'vfae':
        kw.update(x2=ds.x2[:n], has_x2=ds.has_x2[:n])
    return kw


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_model_class_trains_predicts_and_round_trips(kind, dev, tmp_path):
    from drvae_amd import blocks as blk
    model = _model(kind, 'zinb', dev)
    assert type(model.decoder_x) is blk.ZeroInflatedNegativeBinomialDecoder
    ds = Z.zi_dataset(kind, 16, 1, dev)
    kw = _batch_kw(kind, ds)
    l0 = float(model.run_on_batch(train_mode=True, **kw)['CMPL'])
    for _ in range(40):
        l1 = float(model.run_on_batch(train_mode=True, **kw)['CMPL'])
    assert np.isfinite(l1) and l1 < l0
    res = model.forward(ds.x1)
    assert len(res['px1']) == 3 and all(tuple(t.shape) == (16, 13) for t in res['px1'])
    assert torch.equal(res['x1_rec'], res['px1'][0]) and bool((res['px1'][0] > 0).all()) and bool((res['px1'][1] > 0).all())
    if kind == 'drvae':
        assert len(res['px2']) == 3 and torch.equal(res['x2_pert'], res['px2'][0])
    lp = model.decoder_x.logp_perx(ds.x1, *res['px1'])
    assert tuple(lp.shape) == (16,) and bool(torch.isfinite(lp).all())
    fn = str(tmp_path / 'zinb.pth')
    model.save_to_file(fn)
    other = _model(kind, 'zinb', dev, random_seed=11)
    assert not torch.equal(other.decoder_x.decoder_d.linear_d.weight, model.decoder_x.decoder_d.linear_d.weight)
    other.load_params_from_file(fn)
    for (k, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(torch.equal(p, q) for p, q in zip(other.forward(ds.x1)['px1'], res['px1']))
    # the whole training state: parameters, both moments (the third head's with them) and the iteration count
    st = str(tmp_path / 'zinb_state.pth')
    model.save_training_state(st)
    twin = _model(kind, 'zinb', dev, random_seed=12)
    twin.load_training_state(st)
    assert twin.finished_training_iters == model.finished_training_iters == 41
    a, b = model.engine().arena, twin.engine().arena
    for name in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(b.exp_avg_sq[b.offsets['decoder_x.decoder_d.linear_d.weight']:].abs().max()) > 0


FIT = dict(n_train=1024, depth=50.0, learning_rate=5e-2, batch=16)


def test_fit_on_zero_inflated_counts_beats_the_negative_binomial(dev, tmp_path):
    """``fit`` for 3 epochs on zero-inflated Gamma-Poisson counts (theta = 2, gene means 50 .. 360, structural zeros 0.1 .. 0.6 by
    gene; ``x_transform='log1p'``): the held-out mean log-likelihood per row of the zero-inflated model exceeds that of a
    negative-binomial model trained the same way, the evaluation runs step by step without a warning and reports that
    log-likelihood.  The settings were chosen on the CPU stand-ins (three seeds; figures in ``profiles/r24_zinb.md``); only the
    sign is asserted"""
    from tests.test_fit import _loader
    tr, va = Z.zi_dataset('drvae', FIT['n_train'], 1, dev, depth=FIT['depth']), Z.zi_dataset('drvae', 64, 101, dev, depth=FIT['depth'])
    ll = {}
    for type_rec in ('zinb', 'nb'):
        model = _model('drvae', type_rec, dev, epochs=3, learning_rate=FIT['learning_rate'], random_seed=5)
        model.w2log = lambda *a: None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            model.fit(_loader(tr, FIT['batch']), _loader(va, 8), add_noise=False, verbose=False, early_stop=False,
                      model_filename=str(tmp_path / 'b.pth'))
            perf, _ = model.evaluate_performance_on_dataset(va)
        assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
        assert model.finished_training_iters == 3 * (FIT['n_train'] // FIT['batch'])
        assert np.isfinite(float(perf['losses']['ELBO']))
        res = model.forward(va.x1)
        with torch.no_grad():
            ll[type_rec] = float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean())
        assert perf['x1_ll'] == pytest.approx(ll[type_rec], rel=1e-5)
        if type_rec == 'zinb':
            assert model.__dict__.get('_eval_graphs', {}) == {}      # (declined up front: no graph was tried)
    print('held-out mean log-likelihood per row: zinb %.4f  nb %.4f' % (ll['zinb'], ll['nb']))
    assert np.isfinite(ll['zinb']) and np.isfinite(ll['nb']) and ll['zinb'] > ll['nb']
