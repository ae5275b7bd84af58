"""CPU: the annealing schedules of the fused train step (anneal_kl / anneal_yloss / anneal_learning_rate) -- the device
record's values against the float64 formula (and a faulty emulation the check must catch), construction and refusals, the
annealed step against ``tests/anneal_ref.py`` on the three models, the schedules-off step bit for bit, resuming, data
parallelism and the dual-graph ordering -- with the HIP launchers replaced by their plain-PyTorch references
(tests/kernel_ref.py).  The kernels themselves are checked on the GPU
(tests/test_gpu_anneal.py)."""
import dataclasses
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests import anneal_ref as R
from tests import kernel_ref

# ramps of 3 iterations, crossed and saturated within the 6 steps of a test; the y-loss ramp with and without an offset
SCHEDULES = {
    'kl': R.settings(anneal_kl=True, anneal_kl_itermax=3),
    'yloss': R.settings(anneal_yloss=True, anneal_yloss_itermax=3),
    'yloss_offset': R.settings(anneal_yloss=True, anneal_yloss_itermax=3, anneal_yloss_offset=2),
    'lr': R.settings(anneal_learning_rate=True, anneal_lr_itermax=3),
    'all': R.settings(anneal_kl=True, anneal_kl_itermax=3, anneal_yloss=True, anneal_yloss_itermax=3, anneal_yloss_offset=2,
                      anneal_learning_rate=True, anneal_lr_itermax=3),
}
N_STEPS = 6
# the tolerances tests/test_engine_cpu.py holds the unannealed step to (losses; parameters), unchanged
LOSS_TOL, PARAM_TOL = dict(rtol=2e-5, atol=2e-6), dict(rtol=1e-4, atol=2e-5)


def make_engine(spec, params, sched=None, device='cpu', **kw):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    cfg_kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    cfg_kw.update(sched or {})
    cfg_kw.update(kw)
    cfg = E.StepConfig(**cfg_kw)
    arena = ParamArena(E.param_shapes(cfg), device, frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena), arena


def set_batch(eng, batch, dev='cpu', counts=None):
    t = lambda k: torch.from_numpy(batch[k].copy()).to(dev)
    return eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'], counts=counts)


def case(kind, n=12, **over):
    spec = R.small_spec(kind, **over)
    return spec, R.small_batch(spec, n), [M.make_noise(spec, n, seed=40 + i) for i in range(N_STEPS + 1)]


def run_engine(spec, sched, batch, noises, params_seed=9, **kw):
    """(per-step loss dicts, final parameters by name, engine) of ``len(noises)`` eager train steps"""
    eng, arena = make_engine(spec, M.init_params(spec, params_seed, as_numpy=True), sched, **kw)
    set_batch(eng, batch)
    losses = []
    for noise in noises:
        eng.train_step(noise)
        losses.append(dict(eng.losses()))
    return losses, {k: arena.p(k).detach().clone().numpy() for k in arena.shapes}, eng


def run_reference(spec, sched, batch, noises, params_seed=9):
    tr = R.AnnealTrainer(spec, M.init_params(spec, params_seed), sched)
    losses = []
    for noise in noises:
        out, _ = tr.step(batch, noise)
        losses.append({k: float(v.detach()) for k, v in out.items()})
    return losses, {k: v.detach().numpy() for k, v in tr.params.items()}


# ------------------------------------------------------------------------------------------------ 1. the record
GRID = [(itermax, offset) for itermax in (1, 3, 100) for offset in (0, 2)]


def _records(fn):
    """{(schedule, itermax, offset, it): fp32 record} from the emulation ``fn`` over the whole grid"""
    out = {}
    for itermax, offset in GRID:
        for it in range(itermax + offset + 3):
            out[(itermax, offset, it)] = fn(it, (itermax, offset), itermax, (itermax, offset), itermax)
    return out


def _reference_records():
    out = {}
    for itermax, offset in GRID:
        s = R.settings(anneal_kl=True, anneal_kl_itermax=itermax, anneal_yloss=True, anneal_yloss_itermax=itermax,
                       anneal_yloss_offset=offset, anneal_learning_rate=True, anneal_lr_itermax=itermax)
        for it in range(itermax + offset + 3):
            out[(itermax, offset, it)] = R.record32(it, s, pert_itermax=itermax, pert_offset=offset)
    return out


def test_stand_in_record_equals_fp32_of_the_float64_formula():
    want, got = _reference_records(), _records(kernel_ref.record)
    assert set(want) == set(got) and len(want) == sum(m + o + 3 for m, o in GRID)
    for key in want:
        assert got[key].dtype == np.float32 and got[key].tobytes() == want[key].tobytes(), (key, got[key], want[key])
    # the ramp's ends: 0.01 up to the offset, 1 from itermax + offset on; the rate falls to its floor of 0.01
    assert want[(3, 2, 2)][2] == np.float32(0.01) and want[(3, 2, 5)][2] == np.float32(1.0)
    assert want[(3, 0, 0)][3] == np.float32(0.99) and want[(3, 0, 3)][3] == np.float32(0.01)


def test_record_check_catches_an_fp32_evaluation():
    want, bad = _reference_records(), _records(kernel_ref.record_fp32)
    off = [k for k in want if bad[k].tobytes() != want[k].tobytes()]
    print('fp32-evaluated schedule: %d of %d records differ from fp32(float64 formula), e.g. %s' % (len(off), len(want), off[:3]))
    assert off, 'the faulty emulation went unnoticed'
    # ... by a few fp32 roundings of values <= 1 (3 ulp(1) = 3.6e-7) on results >= 0.01: a relative tolerance of 1e-4 -- any
    # tolerance a loss comparison uses -- would have let every one of them through
    worst = max(float(np.max(np.abs(bad[k].astype(np.float64) - want[k]) / np.abs(want[k]))) for k in off)
    assert 0 < worst < 1e-4


def test_off_switches_leave_ones_in_the_record():
    r = kernel_ref.record(5, (0, 0), 0, (0, 7), 0)
    assert r.tobytes() == np.ones(4, np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ 2. construction
def tiny_model(kind, **kw):
    from tests.test_dropout_cpu import tiny_model as base
    return base(kind, **kw)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_construct_with_and_without_schedules(kind):
    from drvae_amd import engine as E
    plain = tiny_model(kind)
    cfg = plain._step_config()
    want = dict(R.DEFAULTS)
    assert {k: getattr(cfg, k) for k in want} == want and not cfg.annealed
    assert {k: getattr(plain, k) for k in want} == want
    named = {f.name for f in dataclasses.fields(E.StepConfig)}
    assert set(want) <= named
    assert E.StepConfig(**{k: getattr(cfg, k) for k in named if k not in want}) == cfg
    on = tiny_model(kind, anneal_kl=True, anneal_kl_itermax=7, anneal_learning_rate=True, anneal_lr_itermax=11)
    c = on._step_config()
    assert (c.anneal_kl, c.anneal_kl_itermax, c.anneal_learning_rate, c.anneal_lr_itermax, c.annealed) == (True, 7, True, 11, True)
    assert list(on.state_dict()) == list(plain.state_dict())
    for sw, mx in (('anneal_kl', 'anneal_kl_itermax'), ('anneal_yloss', 'anneal_yloss_itermax'),
                   ('anneal_learning_rate', 'anneal_lr_itermax')):
        for bad in (0, -3):
            with pytest.raises(ValueError):
                tiny_model(kind, **{sw: True, mx: bad})
            with pytest.raises(ValueError):
                E.StepConfig(**{sw: True, mx: bad})
            tiny_model(kind, **{sw: False, mx: bad})           # (off: its itermax is not looked at)
    if kind != 'pvae':
        m = tiny_model(kind, anneal_yloss=True, anneal_yloss_itermax=4, anneal_yloss_offset=2)
        c = m._step_config()
        assert (c.anneal_yloss, c.anneal_yloss_itermax, c.anneal_yloss_offset) == (True, 4, 2)


def _model_batch(model, n=8, seed=1):
    rs = np.random.RandomState(seed)
    x1 = torch.from_numpy(rs.standard_normal((n, model.dim_x)).astype(np.float32))
    i = np.arange(n)
    hy, hx = torch.from_numpy((i % 2 == 0).astype(np.int64)), torch.from_numpy(((i // 2) % 2 == 1).astype(np.int64))
    x2 = (x1 + 0.1 * torch.from_numpy(rs.standard_normal((n, model.dim_x)).astype(np.float32))) * hx[:, None].float()
    y, s = torch.from_numpy(rs.randint(0, 2, (n, 1)).astype(np.int64)), torch.zeros(n, 1, dtype=torch.int64)
    if model.kind == 'vfae':
        return dict(x1=x1, s=s, y=y, has_y=hy)
    if model.kind == 'pvae':
        return dict(x1=x1, x2=x2, s=s, has_x2=hx)
    return dict(x1=x1, x2=x2, s=s, y=y, has_x2=hx, has_y=hy)


def test_configurations_without_a_universal_plan_are_refused(monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd.VFAE import VFAE
    sup = VFAE(dim_x=13, dim_s=1, dim_y=2, dim_h_en_z1=[7], dim_h_de_z1=[6], dim_h_en_z2=[6], dim_h_de_x=[8], dim_h_clf=[],
               dim_z1=5, dim_z2=4, type_rec='diag_gaussian', nonlinearity='elu', semi_supervised=False, use_MMD=False,
               device='cpu', anneal_kl=True)
    with pytest.raises(NotImplementedError, match='supervised-only VFAE'):
        sup.run_on_batch(train_mode=True, **_model_batch(sup))
    cont = tiny_model('drvae', type_y='cont', anneal_learning_rate=True)
    kw = _model_batch(cont)
    kw['y'] = kw['y'].float()
    with pytest.raises(NotImplementedError, match="type_y='cont'"):
        cont.run_on_batch(train_mode=True, **kw)
    spec = R.small_spec('drvae', use_s=True, dim_s=2)
    eng, _ = make_engine(spec, M.init_params(spec, 1, as_numpy=True), SCHEDULES['kl'])
    with pytest.raises(NotImplementedError, match='use_s'):
        b = R.small_batch(spec)
        eng.set_batch(torch.from_numpy(b['x1']), torch.from_numpy(b['x2']), b['y'], b['has_x2'], b['has_y'], s=b['s'])
    # ... and the same models train unannealed
    tiny_model('drvae', type_y='cont').run_on_batch(train_mode=True, **kw)


def test_the_stratified_feed_is_refused_and_points_at_the_sampler(monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd import data as D
    from tests.test_fit import _tiny_dataset
    ds = _tiny_dataset('drvae', 32, 1)
    w = D.compute_balanced_weights(np.arange(len(ds)) % 5)
    model = tiny_model('drvae', anneal_yloss=True, anneal_yloss_itermax=3)
    with pytest.raises(NotImplementedError, match="mode='sampler'"):
        D.DeviceBatcher(ds, w, 8, seed=3).bind(model.engine())
    plan = D.DeviceBatcher(ds, w, 8, seed=3, mode='sampler').bind(model.engine())
    assert plan.universal and plan.annealed
    tiny_model('drvae')                                         # (unannealed: the stratified feed binds as ever)
    D.DeviceBatcher(ds, w, 8, seed=3).bind(tiny_model('drvae').engine())


def test_a_structure_plan_cannot_run_an_annealed_train_step(monkeypatch):
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae')
    eng, _ = make_engine(spec, M.init_params(spec, 1, as_numpy=True), SCHEDULES['kl'])
    eng.set_structure(batch['has_x2'], batch['has_y'])
    with pytest.raises(NotImplementedError, match='batch-independent plan'):
        eng.train_step(noises[0])


# ------------------------------------------------------------------------------------------------ 3. after the engine exists
def test_attribute_idiom_works_until_the_engine_is_built_then_raises(monkeypatch):
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae')
    model.anneal_kl, model.anneal_kl_itermax = True, 3            # the reference's idiom (src/DrVAE.py:92-97 are attributes)
    kw = _model_batch(model)
    model.run_on_batch(train_mode=True, **kw)
    eng = model.engine()
    assert eng.cfg.anneal_kl and eng.cfg.anneal_kl_itermax == 3 and eng.plan.universal and eng.plan.annealed
    assert eng.schedule_record()['beta_kl'] == float(np.float32(0.01))
    model.run_on_batch(train_mode=True, **kw)
    assert eng.schedule_record()['beta_kl'] == float(np.float32(0.01 + 1 / 3.))
    model.anneal_kl_itermax = 50                                  # too late to take effect: it must not be ignored
    with pytest.raises(RuntimeError, match='anneal_kl_itermax'):
        model.run_on_batch(train_mode=True, **kw)
    with pytest.raises(RuntimeError, match='anneal_kl_itermax'):
        model.engine()
    model.anneal_kl_itermax = 3
    model.run_on_batch(train_mode=True, **kw)                     # (put back: the run goes on)
    with pytest.raises(ValueError):
        model.anneal_kl_itermax = 0
        model.engine()
    plain = tiny_model('drvae')
    plain.run_on_batch(train_mode=True, **kw)
    plain.anneal_learning_rate = True
    with pytest.raises(RuntimeError, match='anneal_learning_rate'):
        plain.run_on_batch(train_mode=True, **kw)


# ------------------------------------------------------------------------------------------------ 4. the step
STEP_CASES = [(kind, name) for kind in ('drvae', 'pvae', 'vfae') for name in SCHEDULES
              if not (kind == 'pvae' and name.startswith('yloss'))]


@pytest.mark.parametrize('kind,name', STEP_CASES)
def test_annealed_step_against_the_reference(kind, name, monkeypatch):
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case(kind)
    sched = SCHEDULES[name]
    got, prm, eng = run_engine(spec, sched, batch, noises[:N_STEPS])
    want, wprm = run_reference(spec, sched, batch, noises[:N_STEPS])
    assert eng.plan.universal and eng.plan.annealed and eng.iters == N_STEPS
    for step in range(N_STEPS):
        for k, v in got[step].items():
            np.testing.assert_allclose(v, want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
    for k in prm:
        np.testing.assert_allclose(prm[k], wprm[k], err_msg=k, **PARAM_TOL)
    # the record the last step ran with, bit for bit
    rec = R.record32(N_STEPS - 1, sched, spec.anneal_perturb_rate_itermax, spec.anneal_perturb_rate_offset)
    assert eng.sched_rec.numpy().tobytes() == rec.tobytes()
    assert kernel_ref.CALLS['lr_scaled_sweeps'] == (N_STEPS if sched['anneal_learning_rate'] else 0)


def test_bucketed_universal_plans_anneal_too(monkeypatch):
    """the plans of the bucketed sampler feed (pair slots for the first rows only, a labeled range with one fprop row): the
    schedule rides on their masks launch as on the plain universal plan's"""
    kernel_ref.install(monkeypatch)
    spec = R.small_spec('drvae')
    batch = M.make_batch(spec, 8, seed=3)
    fl = {'a': (1, 0), 'b': (0, 0), 'c': (1, 1), 'd': (0, 1)}        # (labeled, pair); pairs first, labeled rows one run
    batch['has_y'] = np.array([fl[c][0] for c in 'dccaabbb'], np.int64)
    batch['has_x2'] = np.array([fl[c][1] for c in 'dccaabbb'], np.int64)
    batch['x2'] = batch['x2'] * batch['has_x2'][:, None].astype(np.float32)
    noises = [M.make_noise(spec, 8, seed=50 + i) for i in range(N_STEPS)]
    eng, arena = make_engine(spec, M.init_params(spec, 9, as_numpy=True), SCHEDULES['all'])
    eng.universal_pair_slots, eng.universal_labeled_range = 4, (1, 5)
    set_batch(eng, batch)
    assert eng.plan.universal and eng.plan.annealed and eng.plan.Np == 4 and eng.plan.one_slot is not None
    want, wprm = run_reference(spec, SCHEDULES['all'], batch, noises)
    for step, noise in enumerate(noises):
        eng.train_step(noise)
        for k, v in eng.losses().items():
            np.testing.assert_allclose(v, want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
    for k in arena.shapes:
        np.testing.assert_allclose(arena.p(k).numpy(), wprm[k], err_msg=k, **PARAM_TOL)


def test_clipped_annealed_step_against_the_reference(monkeypatch):
    """a threshold no gradient reaches: the clipped sweeps honour lr_scale and the step is the unclipped one's"""
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae')
    got, prm, eng = run_engine(spec, SCHEDULES['all'], batch, noises[:N_STEPS], max_grad_norm=1e6)
    want, wprm = run_reference(spec, SCHEDULES['all'], batch, noises[:N_STEPS])
    assert kernel_ref.CALLS['adam_l2_clip'] == N_STEPS and kernel_ref.CALLS['lr_scaled_sweeps'] == N_STEPS
    for step in range(N_STEPS):
        for k, v in got[step].items():
            np.testing.assert_allclose(v, want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
    for k in prm:
        np.testing.assert_allclose(prm[k], wprm[k], err_msg=k, **PARAM_TOL)


def test_adamax_annealed_learning_rate_against_the_reference(monkeypatch):
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae', optim_alg='adamax')
    got, prm, _ = run_engine(spec, SCHEDULES['lr'], batch, noises[:N_STEPS])
    want, wprm = run_reference(spec, SCHEDULES['lr'], batch, noises[:N_STEPS])
    for step in range(N_STEPS):
        for k, v in got[step].items():
            np.testing.assert_allclose(v, want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
    for k in prm:
        np.testing.assert_allclose(prm[k], wprm[k], err_msg=k, **PARAM_TOL)


def test_reported_scalars_stay_unscaled_in_training_and_evaluation(monkeypatch):
    """RECL / KLD / PERT / YL are the oracle's own (unannealed) scalars; ELBO / CMPL carry the betas -- in an evaluation
    pass mid-ramp too (the reference's loss_function applies them there), on the universal plan and on a structure plan"""
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae')
    sched = SCHEDULES['all']
    eng, arena = make_engine(spec, M.init_params(spec, 9, as_numpy=True), sched)
    set_batch(eng, batch)
    for noise in noises[:2]:
        eng.train_step(noise)                      # two iterations in: beta_kl = 0.01 + 2/3, beta_yr = 0.01 (offset 2)
    params = {k: torch.from_numpy(arena.p(k).detach().clone().numpy()) for k in arena.shapes}
    plain, _ = M.loss_function(spec, params, batch, noises[2], iters=2, training=False)
    want, _ = R.loss_function(spec, sched, params, batch, noises[2], iters=2, training=False)
    assert abs(float(want['CMPL']) - float(plain['CMPL'])) > 1e3 * (2e-5 * abs(float(plain['CMPL'])) + 2e-6)
    for how in ('universal', 'structure'):
        if how == 'structure':
            eng.set_structure(batch['has_x2'], batch['has_y'])
            p = eng.plan
            p.XSRC[:p.B].copy_(torch.from_numpy(batch['x1']))
            p.XSRC[p.B:].copy_(torch.from_numpy(batch['x2']))
            p.set_labels_host(batch['y'].reshape(-1))
            assert not p.universal
        else:
            set_batch(eng, batch)
        eng.training = False
        eng.set_noise(noises[2])
        eng.forward()
        got = eng.losses()
        for k in ('RECL', 'KLD', 'PERT', 'YL'):
            np.testing.assert_allclose(got[k], float(plain[k]), err_msg=how + ' ' + k, **LOSS_TOL)
        for k in ('ELBO', 'CMPL'):
            np.testing.assert_allclose(got[k], float(want[k]), err_msg=how + ' ' + k, **LOSS_TOL)
    assert eng.iters == 2


# ------------------------------------------------------------------------------------------------ 5. fails without the feature
def test_kl_warm_up_is_far_from_the_unannealed_run(monkeypatch):
    """the check the parent commit fails: with anneal_kl on, steps 0-2 (beta_kl = 0.01, 0.343, 0.677) are nowhere near a
    run with beta_kl = 1 -- the silently ignored switch of the code before this feature"""
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae')
    on, _, _ = run_engine(spec, SCHEDULES['kl'], batch, noises[:3])
    off, _, _ = run_engine(spec, None, batch, noises[:3])
    want, _ = run_reference(spec, SCHEDULES['kl'], batch, noises[:3])
    for step in range(3):
        for k in ('ELBO', 'CMPL'):
            tol = LOSS_TOL['rtol'] * abs(off[step][k]) + LOSS_TOL['atol']
            gap = abs(on[step][k] - off[step][k])
            print('step %d %s: annealed %.6f unannealed %.6f (%.0f tolerances apart)' % (step, k, on[step][k], off[step][k], gap / tol))
            assert gap > 1000 * tol
            np.testing.assert_allclose(on[step][k], want[step][k], **LOSS_TOL)


def test_the_reference_idiom_trains_with_the_ramp_not_with_beta_one(monkeypatch):
    """``model.anneal_kl = True`` after construction, the way the reference's users flip it: the model's losses over steps
    0-2 are the annealed reference's -- before this feature they were the unannealed ones, silently (this comparison fails
    there by value, not by a refused argument)"""
    kernel_ref.install(monkeypatch)
    spec = M.ModelSpec(kind='drvae', dim_x=13, dim_y=2, dim_z1=5, dim_z3=4, h_en_z1=[7], h_de_z1=[6], h_en_z3=[6], h_de_x=[8],
                       h_clf=[], L=2, learning_rate=5e-3, weight_decay=0.01, add_noise_var=0.01, pertloss_rate=0.05)
    model = tiny_model('drvae')
    params = M.init_params(spec, 4, as_numpy=True)
    assert list(model.state_dict()) == list(params)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    model.add_noise = True
    model.anneal_kl, model.anneal_kl_itermax = True, 3
    batch = M.make_batch(spec, 8, seed=2)
    noises = [M.make_noise(spec, 8, seed=60 + i) for i in range(3)]
    kw = {k: torch.from_numpy(batch[k].copy()) for k in ('x1', 'x2', 's', 'y', 'has_x2', 'has_y')}
    want, _ = run_reference(spec, SCHEDULES['kl'], batch, noises, params_seed=4)
    plain, _ = run_reference(spec, R.settings(), batch, noises, params_seed=4)
    for step, noise in enumerate(noises):
        got = model.run_on_batch(train_mode=True, noise=noise, **kw)
        for k, v in got.items():
            np.testing.assert_allclose(float(v), want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
        tol = LOSS_TOL['rtol'] * abs(plain[step]['CMPL']) + LOSS_TOL['atol']
        assert abs(float(got['CMPL']) - plain[step]['CMPL']) > 1000 * tol
    assert model.finished_training_iters == 3


# ------------------------------------------------------------------------------------------------ 6. schedules off
def _launch_log(mp_ctx, names):
    import drvae_amd.kernels as K
    log = []
    for fn in names:
        real = getattr(K, fn)
        mp_ctx.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append((_n, sorted(k))), _f(*a, **k))[1])
    return log


@pytest.mark.parametrize('universal', [False, True], ids=['structure', 'universal'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_schedules_off_is_the_step_as_it_was(kind, universal, monkeypatch):
    """the launch list (names and keyword names), the plan keys, the buffers and every bit of the result: an engine built
    without the arguments == one built with every switch spelled out as off (whatever their itermax)"""
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case(kind)
    params = M.init_params(spec, 9, as_numpy=True)
    off = R.settings(anneal_kl_itermax=3, anneal_yloss_itermax=3, anneal_yloss_offset=2, anneal_lr_itermax=3)
    out = {}
    for tag, sched in (('absent', None), ('off', off)):
        eng, arena = make_engine(spec, params, sched)
        eng.universal = universal
        set_batch(eng, batch)
        with pytest.MonkeyPatch.context() as mpc:
            log = _launch_log(mpc, sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel',
                              'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles'}))
            for noise in noises[:3]:
                eng.train_step(noise)
        assert eng.sched_rec is None and not eng.plan.annealed
        assert not hasattr(eng.plan, 'w_klz2') and not hasattr(eng.plan, 'w_klp')
        out[tag] = (log, list(eng._plans), sorted(k for k, v in vars(eng.plan).items() if torch.is_tensor(v)),
                    arena.param.clone(), arena.exp_avg.clone(), arena.exp_avg_sq.clone(), arena.loss.clone())
    a, b = out['absent'], out['off']
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert not any('lr_scale' in kw or 'anneal' in kw for _, kw in a[0])
    for x, y in zip(a[3:], b[3:]):
        assert torch.equal(x, y)
    assert (a[1][0][0] == 'universal') == universal


# ------------------------------------------------------------------------------------------------ 7. resume
def test_training_state_round_trip_continues_the_ramps_bitwise(monkeypatch, tmp_path):
    """``save_to_file`` is the reference's snapshot -- parameters only: a run resumed from it restarts its ramps (shown).
    ``save_training_state`` at step 2 into a fresh model: step 3 equals the uninterrupted run's, bit for bit"""
    kernel_ref.install(monkeypatch)
    kw = dict(anneal_kl=True, anneal_kl_itermax=3, anneal_yloss=True, anneal_yloss_itermax=3, anneal_learning_rate=True,
              anneal_lr_itermax=3)
    spec_noise = M.ModelSpec(kind='drvae', dim_x=13, dim_y=2, dim_z1=5, dim_z3=4, L=2)
    noises = [M.make_noise(spec_noise, 8, seed=70 + i) for i in range(3)]
    one = tiny_model('drvae', **kw)
    batch = _model_batch(one)
    for noise in noises[:2]:
        one.run_on_batch(train_mode=True, noise=noise, **batch)
    f, g = str(tmp_path / 'state.pth'), str(tmp_path / 'params.pth')
    one.save_training_state(f)
    one.save_to_file(g)
    one.run_on_batch(train_mode=True, noise=noises[2], **batch)
    want = one.engine().arena
    two = tiny_model('drvae', random_seed=77, **kw)
    two.load_training_state(f)
    assert two.finished_training_iters == 2 and int(two.engine().step_dev[0]) == 2
    two.run_on_batch(train_mode=True, noise=noises[2], **batch)
    got = two.engine().arena
    for name in ('param', 'exp_avg', 'exp_avg_sq', 'loss'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert two.engine().schedule_record() == one.engine().schedule_record()
    assert two.engine().schedule_record()['beta_kl'] == float(np.float32(0.01 + 2 / 3.))
    # the parameters-only snapshot: the ramps start over (iteration 0), as in a resumed reference run
    three = tiny_model('drvae', random_seed=78, **kw)
    three.load_params_from_file(g)
    three.run_on_batch(train_mode=True, noise=noises[2], **batch)
    assert three.finished_training_iters == 1 and three.engine().schedule_record()['beta_kl'] == float(np.float32(0.01))


# ------------------------------------------------------------------------------------------------ 8. data parallelism
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_steps(spec, batch, noises, counts, allreduce, lo=None, hi=None):
    if lo is not None:
        batch = {k: v[lo:hi] for k, v in batch.items()}
        noises = [M.slice_noise(n, lo, hi) for n in noises]
    eng, arena = make_engine(spec, M.init_params(spec, 9, as_numpy=True), SCHEDULES['all'])
    set_batch(eng, batch, counts=counts)
    out = []
    for noise in noises:
        eng.train_step(noise, allreduce=allreduce)
        out.append(arena.loss.clone().numpy())
    return np.stack(out), arena.param.clone().numpy(), eng.sched_rec.clone().numpy()


def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        import drvae_amd.kernels as K
        for name in kernel_ref.FUNCTIONS:
            setattr(K, name, getattr(kernel_ref, name))
        from drvae_amd import dist as D
        D.init_from_env(backend='gloo')
        spec, batch, noises = case('drvae')
        n = batch['x1'].shape[0]
        lo, hi = D.shard_rows(n, rank, world)
        counts = D.global_counts(batch['has_x2'][lo:hi], batch['has_y'][lo:hi], 'drvae', spec.semi_supervised)
        q.put((rank,) + _dp_steps(spec, batch, noises[:N_STEPS], counts, D.allreduce_sum, lo, hi))
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_equal_one_rank_with_every_schedule_on(monkeypatch):
    kernel_ref.install(monkeypatch)
    spec, batch, noises = case('drvae')
    single = _dp_steps(spec, batch, noises[:N_STEPS], None, None)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for res in got:
        assert len(res) == 4, res[1]
        _, losses, prm, rec = res
        np.testing.assert_allclose(losses, single[0], rtol=1e-5, atol=1e-6)       # (the bounds of tests/test_dp_gloo.py)
        np.testing.assert_allclose(prm, single[1], rtol=1e-5, atol=1e-6)
        assert rec.tobytes() == single[2].tobytes()
    np.testing.assert_array_equal(got[0][2], got[1][2])                           # replicas stay bit-identical


# ------------------------------------------------------------------------------------------------ 9. the dual-graph ordering
def test_every_recorded_form_orders_the_next_head_behind_the_tail(monkeypatch):
    """cfg-2 shape (150 rows): whichever way the annealed step is recorded, the next step's first launch -- which rewrites
    the record and the ELBO / CMPL weights -- is ordered behind this step's tail (``_head_behind_tail``, asserted inside
    ``_step_tail``); the single-process form keeps its side-chain sweep and loss scalars, i.e. there IS something to order"""
    kernel_ref.install(monkeypatch)
    from drvae_amd.schedule import StepSchedule, Tail
    spec = M.ModelSpec(kind='drvae')
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    eng, _ = make_engine(spec, params, SCHEDULES['all'])
    set_batch(eng, batch)
    plain, _ = make_engine(spec, params)
    plain.universal = True
    set_batch(plain, batch)
    for split in (False, True, 'overlap', 'captured'):
        t = eng._step_tail(split, on_gpu=True)
        assert t.dual and StepSchedule._head_behind_tail(t, split)
        assert t == plain._step_tail(split, on_gpu=True)          # the schedules change nothing of how the step is recorded
    t = eng._step_tail(False, on_gpu=True)
    assert t.late and t.side_adam and t.side_loss and t.adam_gated and not t.tail_gated
    # forms that would NOT be ordered are told apart
    assert not StepSchedule._head_behind_tail(Tail(dual=True, late=True, side_adam=True, side_loss=True), False)
    assert not StepSchedule._head_behind_tail(Tail(dual=True, side_loss=True), False)
    assert StepSchedule._head_behind_tail(Tail(dual=True, late=True, side_adam=True, side_loss=True, tail_gated=True), False)


def test_dual_graph_annealed_steps_equal_eager_steps_bitwise(monkeypatch):
    """both chains of the dual-graph step recorded and run in an order the device flags allow (tests/fold_trace.py), six
    steps across the ramp on the engine's own Philox draws: parameters, moments, losses and the record equal the eager
    engine's, bit for bit, and no wait finds its flag unpublished"""
    from tests import fold_trace as FT
    import drvae_amd.tuning as T
    kernel_ref.install(monkeypatch)
    # (the unfolded forms on either side: the CPU stand-ins of the folded launches agree with them to rounding only --
    # tests/test_fold_rows_cpu.py --, the device's bit for bit -- tests/test_gpu_anneal.py runs the folded step)
    monkeypatch.setenv('DRVAE_TUNE', 'fold_rows=0')
    monkeypatch.setattr(T, '_VALUES', None)
    spec, batch, _ = case('drvae')
    params = M.init_params(spec, 9, as_numpy=True)
    eager, ea = make_engine(spec, params, SCHEDULES['all'])
    dual, da = make_engine(spec, params, SCHEDULES['all'])
    for e in (eager, dual):
        set_batch(e, batch)
        e.training = True
    functions = sorted(set(kernel_ref.FUNCTIONS))
    for step in range(N_STEPS):
        eager.train_step()
        tail = dual._step_tail(False, on_gpu=True)
        assert tail.dual and tail.side_adam and tail.side_loss and not tail.fold_rows
        rec = FT.step(dual, tail, functions)
        for name in ('param', 'exp_avg', 'exp_avg_sq', 'loss'):
            assert torch.equal(getattr(da, name), getattr(ea, name)), (step, name)
        assert torch.equal(dual.sched_rec, eager.sched_rec)
        assert int(dual.sync_err[0::2].abs().sum()) == 0, 'a wait of the step found its flag unpublished'
        # the side chain's half of the sweep read the record too
        assert [n for c, n in rec.order if n == 'adam_l2'] == ['adam_l2', 'adam_l2']
    assert dual.sched_rec.numpy().tobytes() == R.record32(N_STEPS - 1, SCHEDULES['all']).tobytes()
    monkeypatch.setattr(T, '_VALUES', None)
