"""CPU: raw-count inputs (``x_transform='log1p'``, ``library_size=True``) -- the float64 reference itself (scipy, autograd,
s = 1), its bound against fp32 emulations (a careful one inside, three faulty ones caught), construction and refusals, the
switches-off step as it was, the fused step on the plain-PyTorch stand-ins against the model-level float64 reference, the
host-fed step against the feed step, and inference.  The kernels themselves: ``tests/test_gpu_counts.py``."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests.golden import cases as C
from tests.test_dropout_cpu import tiny_model
from tests.test_nb_cpu import LR, close, make_engine, set_batch

SWITCHES = {'log1p': dict(x_transform='log1p'), 'lib': dict(library_size=True),
            'both': dict(x_transform='log1p', library_size=True)}


# ----------------------------------------------------------------------------------------- 1. the reference
def _small(seed=0, Mr=6, X=8):
    rs = np.random.RandomState(seed)
    x = rs.poisson(rs.gamma(2.0, 3.0, (Mr, X))).astype(np.float32)
    x[0] = 0                                      # an all-zero row: s = 1 / X
    x[1] = 1                                      # a row whose total is X: s = 1
    a_m, a_t = rs.uniform(-3, 3, (Mr, X)), rs.uniform(-3, 3, (Mr, X))
    v = (F.softplus(torch.from_numpy(a_m)) + R.MU_SHIFT).float()
    th = (F.softplus(torch.from_numpy(a_t)) + R.THETA_SHIFT).float()
    return torch.from_numpy(x), v, th


def test_library_reference_equals_scipy_autograd_and_the_unscaled_reference_at_s_1():
    import scipy.stats as st
    x, v, th = _small()
    X = x.shape[1]
    coef = torch.ones(x.shape[0])
    ref = CR.reference('nb', x, v, th, coef=coef)
    s = CR.size_factor32(x)
    assert s[0] == np.float32(1.0 / X) and s[1] == 1.0
    mu = s.astype(np.float64)[:, None] * v.double().numpy()
    T = th.double().numpy()
    want = st.nbinom.logpmf(x.double().numpy(), T, T / (T + mu))
    np.testing.assert_allclose(ref['ll'].numpy(), want, rtol=1e-12, atol=1e-12)
    # gradients == float64 autograd through s * (softplus(a) + shift), at pre-activations whose heads are the fp32 values
    inv = lambda y: torch.where(y > 30, y, torch.log(torch.expm1(torch.clamp(y, max=30.0))))
    a_m, a_t = inv(v.double() - R.MU_SHIFT), inv(th.double() - R.THETA_SHIFT)
    S = torch.from_numpy(s.astype(np.float64))
    gm, gt = CR.grads_autograd('nb', x.double(), a_m, a_t, S)
    np.testing.assert_allclose(ref['gm'].numpy(), gm.numpy(), rtol=1e-6, atol=1e-9)      # (softplus^-1 of an fp32 head: 1e-7)
    np.testing.assert_allclose(ref['gt'].numpy(), gt.numpy(), rtol=1e-6, atol=1e-9)
    pm, _ = CR.grads_autograd('poisson', x.double(), a_m, None, S)
    pref = CR.reference('poisson', x, v, coef=coef)
    np.testing.assert_allclose(pref['gm'].numpy(), pm.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pref['ll'].numpy(), st.poisson.logpmf(x.double().numpy(), mu), rtol=1e-12, atol=1e-12)
    # s = 1: the unscaled reference, exactly
    plain = R.reference(x[1:2], v[1:2], th[1:2], coef=coef[1:2])
    for k in ('ll', 'rows', 'gm', 'gt'):
        assert torch.equal(ref[k][1:2], plain[k]), k


# -------------------------------------------------------------------------------------------- 2. the bound
SIZES = (1.0 / 256, 0.1, 1.0, 37.5, 1e3)


@pytest.fixture(scope='module')
def grid():
    x, mu, th, coef = R.edge_grid()
    s = np.asarray(SIZES, np.float32)[np.arange(x.shape[0]) % len(SIZES)]
    ref = CR.reference('nb', x, mu, th, coef=coef, s=s)
    ref['coef'] = coef
    return x.numpy(), mu.numpy(), th.numpy(), s, ref


def _excess(emu, ref):
    ll, gm, gt = (torch.from_numpy(a.astype(np.float64)) for a in emu)
    c = ref64.f64(ref['coef'])[:, None]
    return (ref64.excess(ll, ref['ll'], ref['ll_bound']), ref64.excess(c * gm, ref['gm'], ref['gm_bound']),
            ref64.excess(c * gt, ref['gt'], ref['gt_bound']))


def test_careful_fp32_emulation_stays_inside_the_bound(grid):
    x, v, th, s, ref = grid
    assert set(np.unique(s)) == set(np.asarray(SIZES, np.float32))
    e = [float(t.max()) for t in _excess(CR.emulate_fp32(x, v, th, s), ref)]
    print('careful emulation x size factors, worst |err| / bound: rows %.3g  d/da_m %.3g  d/da_t %.3g' % tuple(e))
    assert max(e) <= 1


def test_three_faulty_emulations_are_caught(grid):
    x, v, th, s, ref = grid
    big = torch.from_numpy(np.broadcast_to((s >= 37.5)[:, None], x.shape).copy())
    _, e_gm, _ = _excess(CR.emulate_fp32(x, v, th, s, slope='scaled'), ref)
    assert float(e_gm[big].max()) >= 10, 'slope(m - shift): %.3g' % float(e_gm[big].max())
    _, e_gm, _ = _excess(CR.emulate_fp32(x, v, th, s, factor_s=False), ref)
    assert float(e_gm[big].max()) >= 10, 'g_m without s: %.3g' % float(e_gm[big].max())
    # the training noise added to the TARGETS: the rows evaluated on x + sigma * eps (in float64: the error is the noise's own)
    xs, vs, ts = _small(seed=2, Mr=8, X=16)
    clean = CR.reference('nb', xs, vs, ts)
    eps = torch.from_numpy(np.random.RandomState(5).randn(*xs.shape))
    noisy = torch.clamp(xs.double() + 0.01 * eps, min=0.0)
    rows = R.logp64(noisy, clean['m'], ts.double()).sum(1)
    e = ref64.excess(rows, clean['rows'], clean['rows_bound'])
    assert float(e.max()) >= 10, 'noise on the targets: %.3g' % float(e.max())
    xt, xin, bnd = CR.feed_reference(xs, noise=eps.float(), sigma=0.01)
    assert torch.equal(xt, xs) and float(ref64.excess(torch.log1p(noisy), xin, bnd).max()) >= 10


# --------------------------------------------------------------------------- 3. construction and refusals
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_construction_and_refusals(kind):
    from drvae_amd import engine as E
    m = tiny_model(kind, type_rec='nb', x_transform='log1p', library_size=True)
    cfg = m._step_config()
    assert cfg.x_transform == 'log1p' and cfg.library_size is True and cfg.split_x
    assert list(m.state_dict()) == list(tiny_model(kind, type_rec='nb').state_dict())
    off = tiny_model(kind, type_rec='poisson')._step_config()
    assert off.x_transform is None and off.library_size is False and not off.split_x
    for type_rec in ('diag_gaussian', 'binary'):
        for sw in SWITCHES.values():
            with pytest.raises(ValueError, match='count decoders'):
                tiny_model(kind, type_rec=type_rec, **sw)
    with pytest.raises(ValueError, match='x_transform'):
        tiny_model(kind, type_rec='nb', x_transform='sqrt')
    with pytest.raises(ValueError, match='x_transform'):
        E.StepConfig(type_rec='poisson', x_transform='log')
    with pytest.raises(ValueError, match='library_size'):
        E.StepConfig(type_rec='diag_gaussian', library_size=True)
    # attributes until the engine is built; a later change raises
    late = tiny_model(kind, type_rec='poisson')
    late.library_size = True
    assert late.engine().cfg.library_size is True
    late.x_transform = 'log1p'
    with pytest.raises(RuntimeError, match='x_transform'):
        late.engine()


def test_fit_and_bind_refuse_negative_data():
    from drvae_amd import data as D
    m = tiny_model('vfae', type_rec='nb', x_transform='log1p')
    x = torch.ones(16, 13)
    x[3, 2] = -1.0
    ds = D.VFAEDataset(x, torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.int64), torch.ones(16, dtype=torch.int64))
    loader = types.SimpleNamespace(dataset=ds)
    with pytest.raises(ValueError, match='x >= 0'):
        m.fit(loader, loader)
    with pytest.raises(ValueError, match='x >= 0'):
        D.DeviceBatcher(ds, torch.ones(16), 8, seed=1).bind(m.engine())


# ------------------------------------------------------------------------ 4. switches off: the step as it was
def _launch_log(mp_ctx, names):
    import drvae_amd.kernels as K
    log = []
    for fn in names:
        real = getattr(K, fn)
        mp_ctx.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append((_n, sorted(k))), _f(*a, **k))[1])
    return log


@pytest.mark.parametrize('type_rec', ['nb', 'poisson'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_switches_off_is_the_step_as_it_was(kind, type_rec):
    """what is checked: with both switches off the plan has no ``XT`` and no identity table, the explicit path launches
    ``rows_gather`` and never ``batch_feed``, the row launch carries exactly its five keywords and no ``library``; and the launch
    list (names and keyword names), the plan's buffers and every bit of three train steps are the same whether the stand-ins of
    the earlier rounds or this feature's are installed (the engine code is this tree's both times: the explicit assertions, not a
    recorded list of the parent's, carry the comparison with the step as it was)"""
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR)
    if type_rec == 'nb':
        batch, params = R.count_batch(spec, 16, seed=3), R.ModelRef(spec, seed=9).engine_params()
    else:       # (the oracle's own Poisson case: small counts, a freshly initialised encoder reads them raw)
        pspec = C.tiny_spec(kind, type_rec='poisson', add_noise_var=0.01)
        batch, params = M.make_batch(pspec, 16, seed=3), M.init_params(pspec, 9, as_numpy=True)
    noises = [M.make_noise(spec, 16, seed=10 + i) for i in range(3)]
    names = sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel', 'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles'})
    out = {}
    for tag, install in (('before', kernel_ref.install), ('after', kernel_ref.install)):
        with pytest.MonkeyPatch.context() as mp:
            install(mp)
            eng, arena = make_engine(spec, params, type_rec=type_rec)
            set_batch(eng, batch)
            with pytest.MonkeyPatch.context() as mpc:
                log = _launch_log(mpc, names)
                for nz in noises:
                    eng.train_step(nz)
            bufs = sorted(k for k, v in vars(eng.plan).items() if torch.is_tensor(v))
            assert bool(torch.isfinite(arena.param).all())
            out[tag] = (log, bufs, arena.param.clone(), arena.exp_avg.clone(), arena.loss.clone())
    a, b = out['before'], out['after']
    assert a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))
    assert 'XT' not in b[1] and 'id_table' not in b[1]
    assert not [n for n, _ in b[0] if n == 'batch_feed'] and [n for n, _ in b[0] if n == 'rows_gather']
    rec = [kw for n, kw in b[0] if n == 'rec_nll_rows']
    assert len(rec) == 3 and all(kw == ['coef', 'dpre', 'kind', 'shift', 'xidx'] for kw in rec)
    assert kernel_ref.CALLS['split_feed'] == 0 and kernel_ref.CALLS['lib_rows'] == 0 and kernel_ref.CALLS['plain_rows'] == 3


# ----------------------------------------------------------------------- 5. the fused step on the stand-ins
def _case(kind, **over):
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR, **over)
    batch = CR.count_batch(spec, 16, seed=3)
    s = CR.size_factor32(batch['x1'])
    assert s.max() / s.min() > 3 and np.all(batch['x1'] == np.floor(batch['x1']))
    return spec, batch


def _use_s_case(kind):
    for sd in range(3, 60):
        spec, _ = _case(kind, use_s=True, dim_s=2)
        batch = CR.count_batch(spec, 16, seed=sd)
        hx, hy, s = batch['has_x2'].astype(bool), batch['has_y'].astype(bool), batch['s'].reshape(-1)
        groups = {'drvae': [hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx], 'pvae': [~hx, hx], 'vfae': [hy, ~hy]}[kind]
        if all(len(set(s[g])) == 2 for g in groups):
            return spec, batch
    raise AssertionError('no suitable batch')


CASES = [('plain', 'log1p'), ('plain', 'lib'), ('plain', 'both'), ('weight_norm', 'both'), ('use_s', 'both'),
         ('universal', 'both')]


def run_against_reference(kind, variant, sw, dev='cpu', tol=((2e-5, 2e-6), (3e-4, 2e-6), (1e-4, 2e-5))):
    """losses and gradients of a train-mode pass WITH input noise, then three Adam steps at 16 rows, against the model-level
    float64 reference; returns the engine"""
    spec, batch = _use_s_case(kind) if variant == 'use_s' else _case(kind, weight_norm=variant == 'weight_norm')
    ref = CR.ModelRef(spec, seed=9, **SWITCHES[sw])
    eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb', **SWITCHES[sw])
    eng.universal = variant == 'universal'
    set_batch(eng, batch, dev)
    p = eng.plan
    assert p.universal == (variant == 'universal') and p.XT.shape == p.XIN.shape and p.XT.data_ptr() != p.XIN.data_ptr()
    noise = M.make_noise(spec, 16, seed=4)
    want, _ = ref.loss(batch, noise, True)
    with ref.context():
        want['CMPL'].backward()
    eng.training = True
    eng.set_noise(noise)
    eng.forward()
    eng.backward()
    for k, v in eng.losses().items():
        close(v, float(want[k].detach()), *tol[0])
    if tol[1] is not None:
        for k, g in ref.grads().items():
            close(arena.g(k), g, *tol[1])
    # the targets are the raw rows, the encoder's rows carry transform and noise
    rows = np.concatenate([batch['x1'][p.rows], batch['x2'][p.rows][p.pair_host]])
    assert np.array_equal(p.XT.cpu().numpy(), rows)
    nz = np.concatenate([noise['nx1'][p.rows], noise['nx2'][p.rows][p.pair_host]])
    t = np.log1p(rows.astype(np.float64)) if SWITCHES[sw].get('x_transform') else rows.astype(np.float64)
    np.testing.assert_allclose(p.XIN.cpu().numpy(), t + np.float32(spec.add_noise_var) * nz.astype(np.float64), rtol=1e-6, atol=1e-7)
    for prm in ref.tr.params.values():
        prm.grad = None
    for step in range(3):
        nzs = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nzs)
        eng.train_step(nzs)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), *tol[0])
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    return eng


@pytest.mark.parametrize('variant,sw', CASES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_matches_the_float64_model_reference(kind, variant, sw, monkeypatch):
    kernel_ref.install(monkeypatch)
    run_against_reference(kind, variant, sw)
    lib = bool(SWITCHES[sw].get('library_size'))
    assert kernel_ref.CALLS['split_feed'] > 0 and kernel_ref.CALLS['plain_feed'] == 0
    assert (kernel_ref.CALLS['lib_rows'] > 0) == lib and (kernel_ref.CALLS['plain_rows'] > 0) == (not lib)


def _counts_dataset(kind, n, seed, dev='cpu', decades=2.0, lo=0.0):
    """Gamma-Poisson counts (theta = 2, gene means 1 .. 4 at depth 1) whose per-row depths are log-uniform over ``decades``
    from 10^lo"""
    from drvae_amd import data as D
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    rs = np.random.RandomState(seed + 77)
    d = 10 ** rs.uniform(lo, lo + decades, n)
    mean = (1.0 + (np.arange(13) % 4))[None, :] * np.where((np.arange(13) % 3 == 0)[None, :], 1.0 + 0.8 * y[:, None], 1.0)
    x1 = rs.poisson(rs.gamma(2.0, d[:, None] * mean / 2.0)).astype(np.float32)
    x2 = (rs.poisson(rs.gamma(2.0, d[:, None] * 1.3 * mean / 2.0)) * hx[:, None]).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(np.zeros(n, np.int64)), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2), t(np.zeros(n, np.int64)), t(y), t(hx), t(hy))


def host_fed_equals_feed(kind, dev, extra=None, steps=3, captured=False, use_s=False):
    """two engines from one set of weights: one trains on the graph-resident feed's batches, the other on the same rows through
    ``set_batch``; same seed, same Philox draws -- parameters, moments and losses must agree bit for bit.  Returns the losses"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR, **(dict(use_s=True, dim_s=2) if use_s else {}))
    ds = _counts_dataset(kind, 48, 4, dev)
    if use_s:       # (nuisance classes carried on the device: the masked sampler feed)
        ds.s = torch.from_numpy(np.random.RandomState(8).randint(0, 2, 48)).to(dev)
    ref = R.ModelRef(spec, seed=9)
    kw = dict(type_rec='nb', x_transform='log1p', library_size=True, **(extra or {}))
    fed, a1 = make_engine(spec, ref.engine_params(), dev, **kw)
    twin, a0 = make_engine(spec, ref.engine_params(), dev, **kw)
    bat = D.DeviceBatcher(ds, torch.ones(48), 16, seed=5, mode='sampler', **(dict(carry_s='masked') if use_s else {}))
    bat.bind(fed)
    bat.begin_epoch()
    twin.universal = True
    if use_s:
        twin.carry_s = 'masked'
    table = fed.plan.live_feed.table.cpu().numpy()
    losses = []
    for b in range(steps):
        if captured:
            if fed._graph_key is None:
                fed.capture()
                bat.rebase()
            fed.replay()
        else:
            fed.train_step()
        i = torch.from_numpy(table[b].astype(np.int64)).to(dev)
        g = lambda name: getattr(ds, name)[i] if hasattr(ds, name) else None
        twin.set_batch(ds.x1[i], g('x2'), ds.y[i], g('has_x2').cpu() if kind != 'vfae' else np.zeros(16, np.int64),
                       ds.has_y[i].cpu() if kind != 'pvae' else np.zeros(16, np.int64), **(dict(s=ds.s[i]) if use_s else {}))
        assert twin.plan.universal and twin.plan.live_feed is None
        twin.train_step()
        assert torch.equal(fed.plan.XT, twin.plan.XT) and torch.equal(fed.plan.XIN, twin.plan.XIN)
        assert fed.losses() == twin.losses()
        losses.append(fed.losses())
    assert all(torch.equal(getattr(a1, w), getattr(a0, w)) for w in ('param', 'exp_avg', 'exp_avg_sq'))
    assert all(np.isfinite(v) for l in losses for v in l.values())
    return losses


@pytest.mark.parametrize('kind,use_s', [('drvae', False), ('pvae', False), ('vfae', False), ('vfae', True)])
def test_host_fed_step_equals_feed_step_bit_for_bit(kind, use_s, monkeypatch):
    """(the sampler feed binds the batch-independent plan: every case here runs on it)"""
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed(kind, 'cpu', use_s=use_s)
    assert kernel_ref.CALLS['split_feed'] >= 6 and kernel_ref.CALLS['plain_feed'] == 0


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_two_shards_sum_to_the_whole_batch(kind, monkeypatch):
    """row-sharded data parallelism needs nothing new (transform and size factor are row-local): two engines on rows [0, 8) and
    [8, 16) with the global counts and their rows of the noise hold loss scalars and gradients that SUM to the whole batch's"""
    kernel_ref.install(monkeypatch)
    spec, batch = _case(kind)
    ref = R.ModelRef(spec, seed=9)
    noise = M.make_noise(spec, 16, seed=4)
    hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
    counts = (16, int(hx.sum()), int(hy.sum()))

    def xchg(lo, hi):
        eng, arena = make_engine(spec, ref.engine_params(), type_rec='nb', **SWITCHES['both'])
        b = {k: v[lo:hi] for k, v in batch.items()}
        t = lambda k: torch.from_numpy(b[k].copy())
        eng.set_batch(t('x1'), t('x2'), b['y'], b['has_x2'], b['has_y'], counts=counts)
        eng.training = True
        eng.set_noise(M.slice_noise(noise, lo, hi))
        eng.forward()
        eng.backward()
        eng.losses()
        return arena.xchg.clone().double().numpy()
    whole, parts = xchg(0, 16), xchg(0, 8) + xchg(8, 16)
    np.testing.assert_allclose(parts, whole, rtol=2e-5, atol=2e-6 * np.abs(whole).max())
    assert np.abs(whole).max() > 1 and kernel_ref.CALLS['lib_rows'] > 0


COMBINED = dict(dropout_rate=0.25, max_grad_norm=1.0, anneal_kl=True, anneal_kl_itermax=10, ema_decay=0.9)


def combined_against_reference(dev='cpu', tol=((2e-5, 2e-6), None, (1e-4, 2e-5)), steps=3):
    """dropout (column masks), clipping at a norm the gradients exceed, KL annealing and the parameter average TOGETHER with both
    switches, DrVAE: losses of every step, the parameters and the averaged parameters against ``counts_ref.RidersRef``"""
    from tests.test_dropout_cpu import column_masks
    spec, batch = _case('drvae')
    rid = {k: v for k, v in COMBINED.items() if k not in ('dropout_rate',)}
    eng, arena = make_engine(spec, R.ModelRef(spec, seed=9).engine_params(), dev, type_rec='nb', **SWITCHES['both'], **COMBINED)
    set_batch(eng, batch, dev)
    sites = eng.dropout_sites()
    assert eng.plan.universal and len(sites) == 4 and all(s['layer'] == 1 for s in sites)
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (sites[i]['M'], 1)) for i, m in cols.items()})
    ref = CR.RidersRef(spec, seed=9, **SWITCHES['both'], sched=dict(anneal_kl=True, anneal_kl_itermax=rid['anneal_kl_itermax']),
                       max_grad_norm=rid['max_grad_norm'], ema_decay=rid['ema_decay'], keep=1.0 - COMBINED['dropout_rate'],
                       cols={CR.chain_block(spec, s['chain']): cols[i] for i, s in enumerate(sites)})
    clipped = 0
    for step in range(steps):
        nz = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nz)
        eng.train_step(nz)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), *tol[0])
        st = eng.clip_stats()
        assert st['n_skipped'] == 0
        clipped += st['coef'] < 1.0
    assert clipped == steps, 'the threshold is one the gradients exceed'
    assert eng.schedule_record()['beta_kl'] == pytest.approx(0.01 + (steps - 1) / 10.0)
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    for k, e in ref.averaged().items():
        close(arena.e(k), e, *tol[2])
    assert not torch.equal(arena.avg, arena.param)
    return eng


def test_combined_riders_match_the_float64_model_reference(monkeypatch):
    kernel_ref.install(monkeypatch)
    combined_against_reference()
    assert kernel_ref.CALLS['split_feed'] > 0 and kernel_ref.CALLS['lib_rows'] > 0


def test_combined_riders_host_fed_equals_feed(monkeypatch):
    """dropout, clipping, KL annealing and the parameter average together with both switches: both pieces are row-local, so
    the riders need nothing new -- the host-fed and the feed step stay bit-identical and finite"""
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed('drvae', 'cpu', extra=COMBINED)


# ----------------------------------------------------------------------------------------------- 6. inference
def test_inference_scales_by_the_right_rows_factor(monkeypatch):
    kernel_ref.install(monkeypatch)
    ds = _counts_dataset('drvae', 16, 3)
    m = tiny_model('drvae', type_rec='nb', x_transform='log1p', library_size=True)
    plain = tiny_model('drvae', type_rec='nb')
    plain.load_state_dict(m.state_dict())
    res = m.forward(ds.x1)
    s1, s2 = m.size_factor(ds.x1), m.size_factor(ds.x2)
    np.testing.assert_array_equal(s1.numpy(), CR.size_factor32(ds.x1))
    assert float(s1.max() / s1.min()) > 3
    # the block's own means at the encoder's view of the rows
    z1 = m.encoder_z1([torch.log1p(ds.x1)])[0]
    mu1, th1 = m.decoder_x([z1])
    assert torch.equal(res['z1'], z1) and torch.equal(res['x1_rec'], s1[:, None] * mu1) and torch.equal(res['px1'][1], th1)
    mu2, _ = m.decoder_x([res['z2']])
    assert torch.equal(res['x2_pert'], s1[:, None] * mu2)                     # x1's factor: x2's depth is unknown
    assert not torch.equal(plain.forward(ds.x1)['z1'], z1)
    r2 = m.forward_w_pert_identity(ds.x1, ds.x2)
    z2 = m.encoder_z1([torch.log1p(ds.x2)])[0]
    assert torch.equal(r2['z2'], z2) and torch.equal(r2['x2_rec'], s2[:, None] * m.decoder_x([z2])[0])
    assert torch.equal(r2['x2_pert'], s1[:, None] * mu1)
    # block level: size= scales the mean in front of the existing formula
    lp = m.decoder_x.logp_perx(ds.x1, mu1, th1, size=s1)
    assert torch.equal(lp, m.decoder_x.logp_perx(ds.x1, s1[:, None] * mu1, th1))
    ref = CR.reference('nb', ds.x1, mu1.detach(), th1.detach())
    np.testing.assert_allclose(lp.detach().numpy(), ref['rows'].numpy(), rtol=1e-4, atol=1e-4)
    pois = tiny_model('pvae', type_rec='poisson', library_size=True)
    rate = pois.decoder_x([torch.zeros(16, 5)])[0]
    assert torch.equal(pois.decoder_x.logp_perx(ds.x1, rate, size=s1), pois.decoder_x.logp_perx(ds.x1, s1[:, None] * rate))
    torch.manual_seed(0)
    a = m.decoder_x.sample(mu1, th1, size=s1)
    torch.manual_seed(0)
    assert torch.equal(a, m.decoder_x.sample(s1[:, None] * mu1, th1))
