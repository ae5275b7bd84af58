"""GPU: the negative-binomial data decoder (``type_rec='nb'``) on the real kernels -- ``dv_rec_nll_rows`` kind
``DV_REC_NEGBIN`` against float64 within the bound of ``tests/nb_ref.py`` on the edge grid, its memory contract, the kernel
against its CPU stand-in, the block, the fused step against the model-level float64 reference (eager, captured, the
batch-independent plan; dropout, clipping, AdamW with the average, annealing) and the model class through ``run_on_batch`` /
``forward`` / ``fit``."""
import warnings

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests.golden import cases as C
from tests.test_nb_cpu import LR, make_engine, set_batch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert _lib.REC_KIND['nb'] == 2
    return K


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------- 1. edge grid
@pytest.fixture(scope='module')
def grid():
    x, mu, th, coef = R.edge_grid()
    return x, mu, th, coef, R.reference(x, mu, th, coef=coef)


def test_edge_grid_within_the_bound(K, dev, grid):
    """means from softplus(-30) + 1e-6 to 1e4, theta from its shift to 1e6, counts 0 .. 30000: rows and both gradient halves
    against float64 within C U sum|components| (C and the components: ``tests/nb_ref.py``)"""
    x, mu, th, coef, ref = grid
    Mr, X = x.shape
    v = torch.cat([mu, th], 1).to(dev)
    out, dpre = torch.full((Mr,), SENTINEL, device=dev), torch.full((Mr, 2 * X), SENTINEL, device=dev)
    K.rec_nll_rows(out, x.to(dev), v, kind='nb', shift=R.MU_SHIFT, coef=coef.to(dev), dpre=dpre)
    got, gd = host(out), host(dpre)
    worst = [float(ref64.excess(got, ref['rows'], ref['rows_bound']).max()),
             float(ref64.excess(gd[:, :X], ref['gm'], ref['gm_bound']).max()),
             float(ref64.excess(gd[:, X:], ref['gt'], ref['gt_bound']).max())]
    print('edge grid, worst |err| / bound: rows %.3g  d/da_m %.3g  d/da_t %.3g' % tuple(worst))
    ref64.check('rec_nll_rows (nb) rows', got, ref['rows'], ref['rows_bound'])
    ref64.check('rec_nll_rows (nb) d/da_m', gd[:, :X], ref['gm'], ref['gm_bound'], x=x, mu=mu, theta=th)
    ref64.check('rec_nll_rows (nb) d/da_t', gd[:, X:], ref['gt'], ref['gt_bound'], x=x, mu=mu, theta=th)
    # the same through the scalar kernel (X = 255 is no multiple of 4) on the grid's first 255 columns
    Xs = X - 1
    xs, ms, ts = (t[:, :Xs].contiguous() for t in (x, mu, th))
    rs = R.reference(xs, ms, ts, coef=coef)
    out2, dpre2 = torch.full((Mr,), SENTINEL, device=dev), torch.full((Mr, 2 * Xs), SENTINEL, device=dev)
    K.rec_nll_rows(out2, xs.to(dev), torch.cat([ms, ts], 1).to(dev), kind='nb', shift=R.MU_SHIFT, coef=coef.to(dev), dpre=dpre2)
    g2 = host(dpre2)
    ref64.check('rec_nll_rows (nb, scalar kernel) rows', host(out2), rs['rows'], rs['rows_bound'])
    ref64.check('rec_nll_rows (nb, scalar kernel) d/da_m', g2[:, :Xs], rs['gm'], rs['gm_bound'], x=xs, mu=ms, theta=ts)
    ref64.check('rec_nll_rows (nb, scalar kernel) d/da_t', g2[:, Xs:], rs['gt'], rs['gt_bound'], x=xs, mu=ms, theta=ts)


def test_zero_count_rows_have_an_exactly_zero_lgamma_pair(K, dev):
    """x = 0, one gene per row, mu at its floor: log p = theta log(theta/(theta+mu)) -- the lgamma pair and lgamma(1)
    contribute exactly 0, so the row equals that ONE term to the term's own few roundings (quotient, log1p, product: 5 U),
    whatever theta is (two lgammas subtracted would leave up to an ulp of lgamma(1e6) = 1 here)"""
    th = torch.tensor(R.THETAS, dtype=torch.float32)
    n = th.numel()
    mu = torch.full((n,), float(np.float32(np.log1p(np.exp(-30.0)) + R.MU_SHIFT)))
    v = torch.stack([mu, th], 1).to(dev)
    x = torch.zeros(n, 1, device=dev)
    out = torch.full((n,), SENTINEL, device=dev)
    K.rec_nll_rows(out, x, v, kind='nb', shift=R.MU_SHIFT)
    got = host(out).double()
    want = -th.double() * torch.log1p(mu.double() / th.double())
    assert torch.all(want < 0) and torch.all((got - want).abs() <= 5 * ref64.U * want.abs()), (got, want)
    # exactly the fp32 product of theta and the rounded log ratio: nothing else was added
    lt = (-torch.log1p(mu.double() / th.double()))
    assert torch.all((got / th.double() - lt).abs() <= 4 * ref64.U * lt.abs())


# ------------------------------------------------------------------------------ 2. shapes, memory contract
def _random_case(Mr, X, n_src=20, seed=1):
    g = torch.Generator().manual_seed(seed + 131 * X + Mr)
    am, at = torch.randn(Mr, X, generator=g) * 3, torch.randn(Mr, X, generator=g) * 3
    mu = torch.nn.functional.softplus(am) + R.MU_SHIFT
    th = torch.nn.functional.softplus(at) + R.THETA_SHIFT
    xs = torch.poisson(torch.rand(n_src, X, generator=g) * 6)
    xs[torch.rand(n_src, X, generator=g) < 0.05] = 1500.0
    xi = torch.randint(0, n_src, (Mr,), generator=g).to(torch.int32)
    coef = torch.randn(Mr, generator=g)
    return xs, mu, th, xi, coef


@pytest.mark.parametrize('X', [1, 101, 257, 104])
def test_shapes_gather_and_memory_contract(K, dev, X):
    """37 rows gathered from 20 source rows; heads and gradients are views into wider sentinel-filled buffers (row strides
    larger than 2X, rows beyond M): nothing outside the views moves; ``coef=None`` writes no gradient; a second call gives
    the same bits; the stand-in agrees at the Poisson check's tolerances.  X = 104: the 16-byte kernel on strided rows"""
    Mr = 37
    xs, mu, th, xi, coef = _random_case(Mr, X)
    pad = 8 if X % 4 == 0 else 5
    vbuf = torch.full((Mr + 3, 2 * X + pad), SENTINEL)
    vbuf[:Mr, :X], vbuf[:Mr, X:2 * X] = mu, th
    vbuf, xs_d, xi_d, coef_d = vbuf.to(dev), xs.to(dev), xi.to(dev), coef.to(dev)
    v = vbuf[:Mr, :2 * X]
    dbuf = torch.full((Mr + 3, 2 * X + pad), SENTINEL, device=dev)
    obuf = torch.full((Mr + 3,), SENTINEL, device=dev)
    d, o = dbuf[:Mr, :2 * X], obuf[:Mr]
    assert v.stride(0) > 2 * X and d.stride(0) > 2 * X
    K.rec_nll_rows(o, xs_d, v, kind='nb', shift=R.MU_SHIFT, xidx=xi_d, coef=coef_d, dpre=d)
    first = (host(obuf).clone(), host(dbuf).clone())
    assert bool((first[1][:, 2 * X:] == SENTINEL).all()) and bool((first[1][Mr:] == SENTINEL).all())
    assert bool((first[0][Mr:] == SENTINEL).all()) and bool((host(vbuf)[:, 2 * X:] == SENTINEL).all())
    assert bool(torch.isfinite(first[0][:Mr]).all()) and bool(torch.isfinite(first[1][:Mr, :2 * X]).all())
    # float64 within the bound
    ref = R.reference(xs[xi.long()], mu, th, coef=coef)
    ref64.check('rows', first[0][:Mr], ref['rows'], ref['rows_bound'])
    ref64.check('d/da_m', first[1][:Mr, :X], ref['gm'], ref['gm_bound'])
    ref64.check('d/da_t', first[1][:Mr, X:2 * X], ref['gt'], ref['gt_bound'])
    # the CPU stand-in
    o_ref, d_ref = torch.zeros(Mr), torch.zeros(Mr, 2 * X)
    kernel_ref.rec_nll_rows(o_ref, xs, torch.cat([mu, th], 1), kind='nb', shift=R.MU_SHIFT, xidx=xi, coef=coef, dpre=d_ref)
    np.testing.assert_allclose(first[0][:Mr].numpy(), o_ref.numpy(), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(first[1][:Mr, :2 * X].numpy(), d_ref.numpy(), rtol=2e-4, atol=1e-5)
    # second call: the same bits
    K.rec_nll_rows(o, xs_d, v, kind='nb', shift=R.MU_SHIFT, xidx=xi_d, coef=coef_d, dpre=d)
    assert torch.equal(host(obuf), first[0]) and torch.equal(host(dbuf), first[1])
    # coef=None: rows only, the gradient buffer is not touched
    d2 = torch.full((Mr, 2 * X), SENTINEL, device=dev)
    o2 = torch.full((Mr,), SENTINEL, device=dev)
    K.rec_nll_rows(o2, xs_d, v, kind='nb', shift=R.MU_SHIFT, xidx=xi_d, coef=None, dpre=d2)
    assert torch.equal(host(o2), first[0][:Mr]) and bool((host(d2) == SENTINEL).all())
    K.rec_nll_rows(o2, xs_d, v, kind='nb', shift=R.MU_SHIFT, xidx=xi_d)
    assert torch.equal(host(o2), first[0][:Mr])


def test_no_rows_is_a_no_op(K, dev):
    out, d = torch.full((4,), SENTINEL, device=dev), torch.full((4, 26), SENTINEL, device=dev)
    x, v = torch.zeros(4, 13, device=dev), torch.ones(4, 26, device=dev)
    K.rec_nll_rows(out[:0], x, v[:0], kind='nb', shift=R.MU_SHIFT, coef=torch.ones(4, device=dev)[:0], dpre=d[:0])
    assert bool((host(out) == SENTINEL).all()) and bool((host(d) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3. block
def test_block_forward_logp_and_backward_match_float64(dev):
    """``NegativeBinomialDecoder`` on 16 x 13 (plain and WeightNorm heads): heads, ``logp_perx`` and the autograd gradients
    of every parameter against the same block in float64 torch"""
    from drvae_amd import blocks as blk
    g = torch.Generator().manual_seed(5)
    z = torch.randn(16, 5, generator=g)
    x = torch.poisson(torch.rand(16, 13, generator=g) * 8)
    x[0, 3], x[7, 11] = 2500.0, 9000.0
    for wn in (False, True):
        torch.manual_seed(3)
        dec = blk.NegativeBinomialDecoder([5], [8], 13, nonlin='elu', weight_norm=wn).to(dev)
        if wn:
            dec(([z.to(dev)]))                      # (WeightNorm's data-dependent initialisation happens on first use)
        p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in dec.named_parameters()}

        def lin(h, q):
            w, b = p64[q + '.weight'], p64[q + '.bias']
            if q + '.g' in p64:
                w = w * (p64[q + '.g'] / w.norm(dim=1))[:, None]
            return h @ w.t() + b
        h = torch.nn.functional.elu(lin(z.double(), 'nnet.model.linear1'))
        mu64 = torch.nn.functional.softplus(lin(h, 'decoder_m.linear_m')) + R.MU_SHIFT
        th64 = torch.nn.functional.softplus(lin(h, 'decoder_t.linear_t')) + R.THETA_SHIFT
        lp64 = R.logp64(x.double(), mu64, th64).sum(1)
        lp64.sum().backward()
        mu, th = dec([z.to(dev)])
        lp = dec.logp_perx(x.to(dev), mu, th)
        dec.logp(x.to(dev), mu, th).backward()
        assert tuple(mu.shape) == tuple(th.shape) == (16, 13) and tuple(lp.shape) == (16,)
        # fp32 products of 5 / 8 terms behind two activations; log p terms up to 1e5 per row (the raised counts)
        np.testing.assert_allclose(host(mu).numpy(), mu64.detach().numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(host(th).numpy(), th64.detach().numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(host(lp).numpy(), lp64.detach().numpy(), rtol=2e-5, atol=1e-4)
        for k, prm in dec.named_parameters():
            ref = p64[k].grad.numpy()
            np.testing.assert_allclose(host(prm.grad).numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=k)
        s = dec.sample(mu.detach(), th.detach())
        assert tuple(s.shape) == (16, 13) and bool((s >= 0).all()) and bool((s == s.floor()).all())


# ----------------------------------------------------------------------------------------- 4. fused step
@pytest.mark.parametrize('universal', [False, True], ids=['structure', 'universal'])
@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_fused_step_matches_the_float64_model_reference(kind, universal, dev):
    """16 rows of counts (a few at 1e3 .. 1e4), three Adam steps against the model-level float64 reference; then the same three
    steps eager and captured (Philox noise): equal bit for bit"""
    spec = C.tiny_spec(kind, add_noise_var=0.0, learning_rate=LR)
    batch = R.count_batch(spec, 16, seed=3)
    ref = R.ModelRef(spec, seed=9)
    eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb')
    eng.universal = universal
    set_batch(eng, batch, dev)
    assert eng.plan.universal == universal and eng._route().nll == 'rec'
    for step in range(3):
        nz = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nz)
        eng.train_step(nz)
        for k, val in eng.losses().items():
            np.testing.assert_allclose(val, float(want[k].detach()), rtol=1e-4, atol=2e-5, err_msg='step %d %s' % (step, k))
    for k, prm in ref.params().items():
        np.testing.assert_allclose(arena.p(k).cpu().numpy(), prm, rtol=2e-4, atol=5e-5, err_msg=k)
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb')
        eng.universal = universal
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


def _overdispersed(n, seed, X=13, theta=2.0):
    """Gamma-Poisson counts with known inverse dispersion ``theta``: gene means 1 .. 4, shifted by the class (raw counts are the
    encoder's input too: kept at the size of the Poisson cases' so that a freshly initialised encoder stays in range)"""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    mean = (1.0 + (np.arange(X) % 4))[None, :] * np.where((np.arange(X) % 3 == 0)[None, :], 1.0 + 0.8 * y[:, None], 1.0)
    x1 = rs.poisson(rs.gamma(theta, mean / theta)).astype(np.float32)
    x2 = rs.poisson(rs.gamma(theta, 1.3 * mean / theta)).astype(np.float32)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    return x1, (x2 * hx[:, None]).astype(np.float32), y, hx, hy


def _dataset(kind, n, seed, dev):
    from drvae_amd import data as D
    x1, x2, y, hx, hy = _overdispersed(n, seed)
    t = lambda a: torch.from_numpy(a).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(np.zeros(n, np.int64)), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2), t(np.zeros(n, np.int64)), t(y), t(hx), t(hy))


def _model(kind, type_rec, dev, **kw):
    from tests.test_fit import _tiny_model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return _tiny_model(kind, device=dev, type_rec=type_rec, add_noise_var=0.0, **kw)


def _batch_kw(kind, ds, n=16):
    kw = dict(x1=ds.x1[:n], s=ds.s[:n], y=ds.y[:n], has_y=ds.has_y[:n])
    if kind != 'vfae':
        kw.update(x2=ds.x2[:n], has_x2=ds.has_x2[:n])
    return kw


@pytest.mark.parametrize('extra', [dict(dropout_rate=0.25), dict(max_grad_norm=1.0), dict(optim_alg='adamw', ema_decay=0.9),
                                   dict(anneal_kl=True, anneal_kl_itermax=10, anneal_learning_rate=True, anneal_lr_itermax=100)],
                         ids=['dropout', 'clipped', 'adamw+ema', 'annealed'])
def test_the_steps_riders_train_finite_and_decreasing(extra, dev):
    """nothing new is needed for hidden-layer dropout (one shared keep mask in front of both heads), gradient-norm clipping,
    AdamW with the parameter average, or the annealing schedules: 40 steps on one batch of overdispersed counts stay finite
    and lower the loss (first five against last five steps; under KL annealing the loss's own weights move, so there the
    reconstruction term is what must improve)"""
    model = _model('drvae', 'nb', dev, **extra)
    kw = _batch_kw('drvae', _dataset('drvae', 16, 1, dev))
    key, sign = ('RECL', -1.0) if 'anneal_kl' in extra else ('CMPL', 1.0)
    cm = [sign * float(model.run_on_batch(train_mode=True, **kw)[key]) for _ in range(40)]
    assert np.isfinite(cm).all() and np.mean(cm[-5:]) < np.mean(cm[:5]), cm
    if 'ema_decay' in extra:
        with model.averaged_parameters():
            assert bool(torch.isfinite(model.engine().arena.param).all())
    assert bool(torch.isfinite(model.engine().arena.param).all())
    if 'max_grad_norm' in extra:
        import drvae_amd.kernels as K
        rec = K.clip_record_values(model.engine().clip_rec)
        assert np.isfinite(rec['norm']) and rec['n_skipped'] == 0 and rec['coef'] <= 1.0


# -------------------------------------------------------------------------------------------- 5. model class
@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_model_class_trains_predicts_and_round_trips(kind, dev, tmp_path):
    from drvae_amd import blocks as blk
    model = _model(kind, 'nb', dev)
    assert type(model.decoder_x) is blk.NegativeBinomialDecoder
    ds = _dataset(kind, 16, 1, dev)
    kw = _batch_kw(kind, ds)
    l0 = float(model.run_on_batch(train_mode=True, **kw)['CMPL'])
    for _ in range(40):
        l1 = float(model.run_on_batch(train_mode=True, **kw)['CMPL'])
    assert np.isfinite(l1) and l1 < l0
    res = model.forward(ds.x1)
    assert len(res['px1']) == 2 and all(tuple(t.shape) == (16, 13) for t in res['px1'])
    assert torch.equal(res['x1_rec'], res['px1'][0]) and bool((res['px1'][0] > 0).all()) and bool((res['px1'][1] > 0).all())
    if kind == 'drvae':
        assert len(res['px2']) == 2 and torch.equal(res['x2_pert'], res['px2'][0])
    lp = model.decoder_x.logp_perx(ds.x1, *res['px1'])
    assert tuple(lp.shape) == (16,) and bool(torch.isfinite(lp).all())
    fn = str(tmp_path / 'nb.pth')
    model.save_to_file(fn)
    other = _model(kind, 'nb', dev, random_seed=11)
    assert not torch.equal(other.decoder_x.decoder_t.linear_t.weight, model.decoder_x.decoder_t.linear_t.weight)
    other.load_params_from_file(fn)
    for (k, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    res2 = other.forward(ds.x1)
    assert torch.equal(res2['px1'][0], res['px1'][0]) and torch.equal(res2['px1'][1], res['px1'][1])


@pytest.mark.parametrize('mode', ['stratified', 'sampler'])
def test_fit_on_overdispersed_counts_beats_the_poisson_decoder(mode, dev, tmp_path):
    """``fit`` with a ``DeviceBatcher`` for 3 epochs on 64 rows of Gamma-Poisson counts (theta = 2): the held-out mean
    log-likelihood of the negative-binomial model exceeds that of a Poisson model trained the same way on the same data"""
    from drvae_amd import data as D
    from tests.test_fit import _loader
    tr, va = _dataset('drvae', 64, 1, dev), _dataset('drvae', 32, 2, dev)
    w = D.compute_balanced_weights(np.arange(64) % 5)
    ll = {}
    for type_rec in ('nb', 'poisson'):
        model = _model('drvae', type_rec, dev, epochs=3)
        bat = D.DeviceBatcher(tr, w, 16, seed=3, **(dict(mode='sampler') if mode == 'sampler' else {}))
        model.fit(bat, _loader(va, 8), add_noise=False, verbose=False, early_stop=False, model_filename=str(tmp_path / 'b.pth'))
        assert model.finished_training_iters == 3 * 4 and model.engine().universal == (mode == 'sampler')
        perf, _ = model.evaluate_performance_on_dataset(va)
        assert np.isfinite(float(perf['losses']['ELBO']))
        res = model.forward(va.x1)
        ll[type_rec] = float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean())
        if type_rec == 'nb':
            assert perf['x1_ll'] == pytest.approx(ll['nb'], rel=1e-5)      # (the step-by-step evaluation reports it)
    print('held-out mean log-likelihood per row: nb %.4f  poisson %.4f' % (ll['nb'], ll['poisson']))
    assert np.isfinite(ll['nb']) and np.isfinite(ll['poisson']) and ll['nb'] > ll['poisson']
