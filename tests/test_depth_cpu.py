"""CPU: the depth-normalised encoder input (``x_transform='log1p_norm'``) and the ``size_factor=`` keyword of inference -- the
bound of ``tests/depth_ref.py`` against fp32 emulations (a careful one inside on every element, five faulty ones caught),
construction and refusals, the fused step on the plain-PyTorch stand-ins against the model-level float64 reference, the
host-fed step against the feed step, the launch lists of the steps that existed before (pinned from the parent commit), depth
invariance of ``z1`` and the decoder's output at a chosen depth.  The kernel itself: ``tests/test_gpu_depth.py``."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import depth_ref as DR
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests.golden import cases as C
from tests.test_counts_cpu import COMBINED, _case, _counts_dataset, _launch_log, _use_s_case
from tests.test_dropout_cpu import tiny_model
from tests.test_nb_cpu import LR, close, make_engine, set_batch

NORM = 'log1p_norm'
SIGMA = 0.01


# -------------------------------------------------------------------------------------------- 1. the bound
@pytest.fixture(scope='module')
def grid():
    """the edge rows (x1), a second set of rows with other totals (the x2 rows of the same slots), noise, the float64 references
    with and without noise"""
    from drvae_amd import kernels as K
    assert K.FEED_TRANSFORM[NORM] == 3, 'the launch these emulations stand for'
    x = DR.edge_rows(16)
    other = np.roll(x, 1, axis=0)
    noise = np.random.RandomState(3).randn(*x.shape).astype(np.float32)
    src = torch.from_numpy(x)
    return x, other, noise, DR.feed_reference(src), DR.feed_reference(src, torch.from_numpy(noise), SIGMA)


def _worst(got, ref):
    return float(ref64.excess(torch.from_numpy(got), ref[1], ref[2]).max())


def test_careful_fp32_emulation_stays_inside_the_bound_on_every_element(grid):
    x, _, noise, plain, noisy = grid
    xt, xin = DR.emulate_fp32(x)
    xtn, xinn = DR.emulate_fp32(x, noise, SIGMA)
    e = _worst(xin, plain), _worst(xinn, noisy)
    print('careful emulation, worst |err| / bound: no noise %.3g  noise %.3g  (C = %d)' % (e + (DR.C_NORM,)))
    assert np.array_equal(xt, x) and np.array_equal(xtn, x) and max(e) <= 1
    # an all-zero row gives T = 0 exactly; a row whose total is X gives the bits of the 'log1p' feed
    assert np.all(xin[0] == 0) and torch.all(plain[1][0] == 0)
    assert np.array_equal(xin[2], np.log1p(x[2])) and torch.equal(plain[1][2], CR.feed_reference(torch.from_numpy(x[2:3]))[1][0])
    assert float(plain[1][3, 0]) < 1e-4 and x[4].astype(np.float64).sum() == 2 ** 24 - 1 and x[5].max() == 30000


@pytest.mark.parametrize('fault', DR.FAULTS)
def test_faulty_fp32_emulations_are_caught(grid, fault):
    x, other, noise, plain, noisy = grid
    if fault == 'targets_too':
        xt, _ = DR.emulate_fp32(x, fault=fault)
        e = float(ref64.excess(torch.from_numpy(xt), ref64.f64(x), ref64.bound(1, np.abs(x))).max())
    elif fault == 'noisy_sum':
        e = _worst(DR.emulate_fp32(x, noise, SIGMA, fault=fault)[1], noisy)
    else:
        e = _worst(DR.emulate_fp32(x, fault=fault, other=other)[1], plain)
    print('%s: worst |err| / bound %.3g' % (fault, e))
    assert e >= 10          # (a non-finite value counts as inf)


# --------------------------------------------------------------------------- 2. construction and refusals
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_construction_and_refusals(kind):
    from drvae_amd import engine as E
    from drvae_amd import kernels as K
    assert NORM in E.X_TRANSFORMS and K.FEED_TRANSFORM[NORM] == 3 and 2 not in K.FEED_TRANSFORM.values()
    for lib in (False, True):
        m = tiny_model(kind, type_rec='nb', x_transform=NORM, library_size=lib)
        cfg = m._step_config()
        assert cfg.x_transform == NORM and cfg.library_size is lib and cfg.split_x
        assert list(m.state_dict()) == list(tiny_model(kind, type_rec='nb').state_dict())
        assert [n for n, _ in m.named_parameters()] == [n for n, _ in tiny_model(kind, type_rec='nb').named_parameters()]
    for type_rec in ('diag_gaussian', 'binary'):
        with pytest.raises(ValueError, match='count decoders'):
            tiny_model(kind, type_rec=type_rec, x_transform=NORM)
        with pytest.raises(ValueError, match='count decoders'):
            E.StepConfig(type_rec=type_rec, x_transform=NORM)
    for type_rec in ('poisson', 'nb', 'zinb'):
        assert E.StepConfig(type_rec=type_rec, x_transform=NORM).split_x
        assert E.check_counts_config(NORM, False, type_rec) == dict(x_transform=NORM, library_size=False)
    with pytest.raises(ValueError, match='x_transform'):
        E.StepConfig(type_rec='nb', x_transform='log1p_normed')
    # an attribute until the engine is built; a later change raises
    late = tiny_model(kind, type_rec='nb', x_transform='log1p')
    late.x_transform = NORM
    assert late.engine().cfg.x_transform == NORM
    late.x_transform = 'log1p'
    with pytest.raises(RuntimeError, match='x_transform'):
        late.engine()


def test_fit_and_bind_refuse_negative_data():
    import types
    from drvae_amd import data as D
    m = tiny_model('vfae', type_rec='nb', x_transform=NORM)
    x = torch.ones(16, 13)
    x[3, 2] = -1.0
    ds = D.VFAEDataset(x, torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.int64), torch.ones(16, dtype=torch.int64))
    loader = types.SimpleNamespace(dataset=ds)
    with pytest.raises(ValueError, match='x >= 0'):
        m.fit(loader, loader)
    with pytest.raises(ValueError, match='x >= 0'):
        D.DeviceBatcher(ds, torch.ones(16), 8, seed=1).bind(m.engine())


# ----------------------------------------------------------------------- 3. the fused step on the stand-ins
CASES = [('plain', False), ('plain', True), ('weight_norm', True), ('use_s', True), ('universal', False), ('universal', True)]


def run_against_reference(kind, variant, lib, dev='cpu', tol=((2e-5, 2e-6), (3e-4, 2e-6), (1e-4, 2e-5))):
    """losses and gradients of a train-mode pass WITH input noise, then three Adam steps at 16 rows whose depths differ, against
    the model-level float64 reference (``tests/test_counts_cpu.run_against_reference`` with the new transform); returns the engine"""
    spec, batch = _use_s_case(kind) if variant == 'use_s' else _case(kind, weight_norm=variant == 'weight_norm')
    ref = DR.ModelRef(spec, seed=9, library_size=lib)
    eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb', x_transform=NORM, library_size=lib)
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
    # the targets are the raw rows; the encoder's rows are the normalised ones plus noise, each row by its OWN total
    rows = np.concatenate([batch['x1'][p.rows], batch['x2'][p.rows][p.pair_host]])
    nz = np.concatenate([noise['nx1'][p.rows], noise['nx2'][p.rows][p.pair_host]])
    assert np.array_equal(p.XT.cpu().numpy(), rows)
    _, xin64, bnd = DR.feed_reference(torch.from_numpy(rows), torch.from_numpy(nz), spec.add_noise_var)
    ref64.check('encoder rows of the step', p.XIN.cpu(), xin64, bnd)
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


@pytest.mark.parametrize('variant,lib', CASES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_matches_the_float64_model_reference(kind, variant, lib, monkeypatch):
    kernel_ref.install(monkeypatch)
    run_against_reference(kind, variant, lib)
    assert kernel_ref.CALLS['norm_feed'] > 0 and kernel_ref.CALLS['plain_feed'] == 0
    assert (kernel_ref.CALLS['lib_rows'] > 0) == lib and (kernel_ref.CALLS['plain_rows'] > 0) == (not lib)


def host_fed_equals_feed(kind, dev, extra=None, steps=3, captured=False, use_s=False, x_transform=NORM, library_size=True):
    """``tests/test_counts_cpu.host_fed_equals_feed`` with the transform as an argument: two engines from one set of weights, one
    on the graph-resident feed's batches, the other on the same rows through ``set_batch``; same seed, same Philox draws --
    targets, encoder rows, parameters, moments and losses agree bit for bit.  Returns the losses"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR, **(dict(use_s=True, dim_s=2) if use_s else {}))
    ds = _counts_dataset(kind, 48, 4, dev)
    if use_s:       # (nuisance classes carried on the device: the masked sampler feed)
        ds.s = torch.from_numpy(np.random.RandomState(8).randint(0, 2, 48)).to(dev)
    ref = R.ModelRef(spec, seed=9)
    kw = dict(type_rec='nb', x_transform=x_transform, library_size=library_size, **(extra or {}))
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
        assert torch.equal(fed.plan.XT[:16], ds.x1[i])
        assert fed.losses() == twin.losses()
        losses.append(fed.losses())
    assert all(torch.equal(getattr(a1, w), getattr(a0, w)) for w in ('param', 'exp_avg', 'exp_avg_sq'))
    assert all(np.isfinite(v) for l in losses for v in l.values())
    return losses


@pytest.mark.parametrize('kind,use_s,lib', [('drvae', False, True), ('pvae', False, False), ('vfae', False, True), ('vfae', True, True)])
def test_host_fed_step_equals_feed_step_bit_for_bit(kind, use_s, lib, monkeypatch):
    """(the sampler feed binds the batch-independent plan: every case here runs on it)"""
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed(kind, 'cpu', use_s=use_s, library_size=lib)
    assert kernel_ref.CALLS['norm_feed'] >= 6 and kernel_ref.CALLS['plain_feed'] == 0


def combined_against_reference(dev='cpu', tol=((2e-5, 2e-6), None, (1e-4, 2e-5)), steps=3):
    """dropout (column masks), clipping at a norm the gradients exceed, KL annealing and the parameter average TOGETHER with the
    normalised feed and ``library_size``, DrVAE: losses of every step, parameters and averaged parameters against the reference"""
    from tests.test_dropout_cpu import column_masks
    spec, batch = _case('drvae')
    rid = {k: v for k, v in COMBINED.items() if k != 'dropout_rate'}
    eng, arena = make_engine(spec, R.ModelRef(spec, seed=9).engine_params(), dev, type_rec='nb', x_transform=NORM,
                             library_size=True, **COMBINED)
    set_batch(eng, batch, dev)
    sites = eng.dropout_sites()
    assert eng.plan.universal and len(sites) == 4 and all(s['layer'] == 1 for s in sites)
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (sites[i]['M'], 1)) for i, m in cols.items()})
    ref = DR.ModelRef(spec, seed=9, library_size=True, sched=dict(anneal_kl=True, anneal_kl_itermax=rid['anneal_kl_itermax']),
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
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    for k, e in ref.averaged().items():
        close(arena.e(k), e, *tol[2])
    return eng


def test_combined_riders_match_the_float64_model_reference(monkeypatch):
    kernel_ref.install(monkeypatch)
    combined_against_reference()
    assert kernel_ref.CALLS['norm_feed'] > 0 and kernel_ref.CALLS['lib_rows'] > 0


def test_combined_riders_host_fed_equals_feed(monkeypatch):
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed('drvae', 'cpu', extra=COMBINED)


def test_adamw_step_host_fed_equals_feed(monkeypatch):
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed('pvae', 'cpu', extra=dict(optim_alg='adamw', ema_decay=0.9))


# ---------------------------------------------------------------------- 4. the steps that existed: launch lists
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'depth_launches.json')
LAUNCH_CASES = {'log1p': dict(x_transform='log1p', library_size=True), 'off': {}}


def launch_record(kind, sw):
    """names and keyword names of every launcher call of ``set_batch`` + two train steps of an 'nb' model on the stand-ins of
    ``tests/kernel_ref.py`` (nothing of this feature is installed: the record can be taken on the parent commit)"""
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR)
    batch, params = CR.count_batch(spec, 16, seed=3), R.ModelRef(spec, seed=9).engine_params()
    names = sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel', 'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles'})
    with pytest.MonkeyPatch.context() as mp:
        kernel_ref.install(mp)
        eng, _ = make_engine(spec, params, type_rec='nb', **LAUNCH_CASES[sw])
        with pytest.MonkeyPatch.context() as mpc:
            log = _launch_log(mpc, names)
            set_batch(eng, batch)
            for i in range(2):
                eng.train_step(M.make_noise(spec, 16, seed=10 + i))
    return [[n, kw] for n, kw in log]


def digest(log):
    return hashlib.sha256(json.dumps(log, separators=(',', ':')).encode()).hexdigest()


def write_golden(path=GOLDEN):
    """(run on the parent commit: ``python -c "from tests import test_depth_cpu as T; T.write_golden()"``)"""
    out = {}
    for kind in ('drvae', 'pvae', 'vfae'):
        for sw in LAUNCH_CASES:
            log = launch_record(kind, sw)
            out['%s/%s' % (kind, sw)] = dict(digest=digest(log), launches=[n for n, _ in log])
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write('\n')


@pytest.mark.parametrize('sw', sorted(LAUNCH_CASES))
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_launch_lists_of_the_existing_steps_equal_the_parents(kind, sw):
    with open(GOLDEN) as fh:
        want = json.load(fh)['%s/%s' % (kind, sw)]
    log = launch_record(kind, sw)
    assert [n for n, _ in log] == want['launches']
    assert digest(log) == want['digest'], 'a keyword of a launch changed'
    feeds = [kw for n, kw in log if n == 'batch_feed']
    assert (len(feeds) == 2 and all('transform' in kw and 'xt' in kw for kw in feeds)) if sw == 'log1p' else not feeds


# ------------------------------------------------------------------------------------ 5. depth invariance
def _int_rows(n=12, X=13, seed=0):
    rs = np.random.RandomState(seed)
    d = 10 ** rs.uniform(0, 2, n)
    x = rs.poisson(d[:, None] * (1.0 + np.arange(X) % 4)[None, :]).astype(np.float32)
    x[0] = 0
    x[0, 4] = 1                                     # total 1: the guard's edge
    assert x.sum(1).min() >= 1 and x.sum(1).max() * 4 < 2 ** 24
    return torch.from_numpy(x)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_z1_does_not_move_with_depth(kind, monkeypatch):
    """integer counts, totals >= 1: 4x / (4s) == x / s exactly (a power of two), so z1 is the same BITS at four times the depth;
    under 'log1p' it moves"""
    kernel_ref.install(monkeypatch)
    x = _int_rows()
    m = tiny_model(kind, type_rec='nb', x_transform=NORM, library_size=True)
    a, b = m.forward(x), m.forward(4 * x)
    assert torch.equal(a['z1'], b['z1']) and torch.equal(a['qz1'][1], b['qz1'][1])
    assert torch.equal(m._enc_x(x), torch.log1p(x / m.size_factor(x)[:, None])) and torch.equal(m._enc_x(x), m._enc_x(4 * x))
    np.testing.assert_array_equal(m.size_factor(x).numpy(), CR.size_factor32(x))
    assert torch.equal(b['x1_rec'], 4 * a['x1_rec'])               # (the decoder's depth comes back through library_size)
    plain = tiny_model(kind, type_rec='nb', x_transform='log1p', library_size=True)
    plain.load_state_dict(m.state_dict())
    assert not torch.equal(plain.forward(x)['z1'], plain.forward(4 * x)['z1'])
    one = torch.ones(3, 13)                          # s = 1: what 'log1p' reads
    assert torch.equal(m.forward(one)['z1'], plain.forward(one)['z1'])
    if kind != 'vfae':
        x2 = _int_rows(seed=1)
        r, r4 = m.forward_w_pert_identity(x, x2), m.forward_w_pert_identity(4 * x, 4 * x2)
        assert torch.equal(r['z1'], r4['z1']) and torch.equal(r['z2'], r4['z2'])
        assert torch.equal(r['z2'], m.encoder_z1([torch.log1p(x2 / m.size_factor(x2)[:, None])])[0])      # x2's OWN total


# ------------------------------------------------------------------------------------- 6. size_factor=
@pytest.mark.parametrize('type_rec', ['nb', 'zinb', 'poisson'])
def test_size_factor_keyword(type_rec, monkeypatch):
    kernel_ref.install(monkeypatch)
    ds = _counts_dataset('drvae', 16, 3)
    x1, x2 = ds.x1, ds.x2
    m = tiny_model('drvae', type_rec=type_rec, x_transform=NORM, library_size=True)
    z1 = m.encoder_z1([m._enc_x(x1)])[0]
    raw1 = m.decoder_x([z1])
    obs = m.forward(x1)
    s1, s2 = m.size_factor(x1), m.size_factor(x2)
    assert float(s1.max() / s1.min()) > 3
    # 1.0: the unscaled heads -- the denoised expression at a common depth of dim_x counts per cell
    at1 = m.forward(x1, size_factor=1.0)
    assert torch.equal(at1['x1_rec'], raw1[0]) and torch.equal(at1['px1'][0], raw1[0])
    assert torch.equal(at1['x2_pert'], m.decoder_x([obs['z2']])[0]) and torch.equal(at1['z1'], obs['z1'])
    # a tensor; the observed factors passed in == None
    t = torch.linspace(0.5, 3.0, 16)
    att = m.forward(x1, size_factor=t)
    assert torch.equal(att['x1_rec'], t[:, None] * raw1[0]) and torch.equal(att['x2_pert'], t[:, None] * at1['x2_pert'])
    same = m.forward(x1, size_factor=s1)
    for k in ('x1_rec', 'x2_pert'):
        assert torch.equal(same[k], obs[k])
    # theta and the dropout logit are never scaled
    for px in ('px1', 'px2'):
        for i in range(1, len(obs[px])):
            assert torch.equal(att[px][i], obs[px][i]) and torch.equal(at1[px][i], obs[px][i])
    assert len(obs['px1']) == {'poisson': 1, 'nb': 2, 'zinb': 3}[type_rec]
    # the identity form: px2 AND px2_rec
    idn, idt = m.forward_w_pert_identity(x1, x2), m.forward_w_pert_identity(x1, x2, size_factor=t)
    assert torch.equal(idn['x2_pert'], s1[:, None] * raw1[0]) and torch.equal(idt['x2_pert'], t[:, None] * raw1[0])
    rec = m.decoder_x([idn['z2']])[0]
    assert torch.equal(idn['x2_rec'], s2[:, None] * rec) and torch.equal(idt['x2_rec'], t[:, None] * rec)
    assert torch.equal(idt['px2_rec'][0], idt['x2_rec'])
    # through reconstruct(**kwargs)
    got = m.reconstruct(x1=x1, size_factor=1.0)
    np.testing.assert_array_equal(got[0], raw1[0].detach().numpy())
    np.testing.assert_array_equal(got[2], at1['x2_pert'].numpy())
    # refusals
    off = tiny_model('drvae', type_rec=type_rec, x_transform=NORM)
    assert off.forward(x1, size_factor=None)['x1_rec'].shape == x1.shape
    with pytest.raises(ValueError, match='library_size'):
        off.forward(x1, size_factor=1.0)
    with pytest.raises(ValueError, match='library_size'):
        off.forward_w_pert_identity(x1, x2, size_factor=t)
    with pytest.raises(ValueError, match='size_factor'):
        m.forward(x1, size_factor=torch.ones(5))
    v = tiny_model('vfae', type_rec=type_rec, library_size=True)
    assert torch.equal(v.forward(x1, size_factor=2.0)['x1_rec'], 2.0 * v.forward(x1, size_factor=1.0)['x1_rec'])


# ---------------------------------------------------------------------------- 7. fit and evaluation on the stand-ins
def test_fit_and_evaluation_on_the_stand_ins(monkeypatch, tmp_path):
    """``fit`` with the normalised feed and ``library_size`` through host loaders (``DeviceBatcher``'s epoch mode needs a device:
    ``tests/test_gpu_depth.py``): finite losses, the evaluation's likelihood at the scaled mean, z1 free of depth afterwards"""
    from tests.test_fit import _loader
    kernel_ref.install(monkeypatch)
    tr, va = _counts_dataset('drvae', 48, 1), _counts_dataset('drvae', 16, 2)
    model = tiny_model('drvae', type_rec='nb', x_transform=NORM, library_size=True, epochs=2)
    model.w2log = lambda *a: None
    model.fit(_loader(tr, 16), _loader(va, 8), add_noise=True, verbose=False, early_stop=False,
              model_filename=str(tmp_path / 'm.pth'))
    assert model.finished_training_iters == 2 * 3 and kernel_ref.CALLS['norm_feed'] > 0
    perf, _ = model.evaluate_performance_on_dataset(va)
    assert all(np.isfinite(float(v)) for v in perf['losses'].values())
    res = model.forward(va.x1)
    assert perf['x1_ll'] == pytest.approx(float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean()), rel=1e-5)
    assert torch.equal(res['z1'], model.forward(4 * va.x1)['z1'])
