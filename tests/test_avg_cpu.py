"""CPU: parameter averaging (``ema_decay``) and decoupled weight decay (``optim_alg='adamw'``) in the fused train step -- the
references of tests/avg_ref.py against their own bounds and the faulty emulations, construction and refusals, the step with
both switches off, AdamW against ``torch.optim.AdamW`` in float64, the average against its float64 recurrence, the
``averaged_parameters()`` context, ``fit``, resuming, data parallelism and the dual-graph schedule -- with the HIP launchers
replaced by their plain-PyTorch references (tests/kernel_ref.py).  The kernels themselves
are checked on the GPU (tests/test_gpu_avg.py)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests import avg_ref as AR
from tests import kernel_ref
from tests import optim_ref as R
from tests.test_anneal_cpu import _free_port, _launch_log, _model_batch, tiny_model
from tests.test_anneal_cpu import case as small_case
from tests.test_anneal_cpu import make_engine as engine_with
from tests.test_anneal_cpu import set_batch as set_small_batch
from tests.test_clip_cpu import case_of, compare_state, grad_norm64, gradients, live_names, make_engine
from tests.test_dropout_cpu import set_batch

MODEL_CASES = ['tiny_drvae', 'tiny_pvae', 'tiny_vfae', 'tiny_drvae_wn']
D = 0.9                       # the average's decay in the model-level tests: a short memory, every step is seen
N_STEPS = 3


# ------------------------------------------------------------------------------------------------ 1. the checks themselves
@pytest.mark.parametrize('cls', R.CLASSES)
def test_adamw_reference_holds_both_emulations_on_every_class(cls):
    arrays = R.case(cls)
    worst = 0.0
    for t, gs, wd in R.settings(cls):
        h = R.hyper32(weight_decay=wd, gscale=gs)
        for lr_scale, coef in ((None, None), (AR.LR_SCALE, AR.CLIP_COEF)):
            he = AR.effective(h, lr_scale, coef)
            for fused in (False, True):
                got = AR.emulate('adamw', *arrays, t, h, fused, lr_scale=lr_scale, coef=coef)
                failed, w = AR.verify('adamw', got, arrays, t, he, site=cls)
                assert not failed, (cls, t, gs, wd, lr_scale, fused, w)
                worst = max(worst, max(w.values()))
    print('adamw %s: worst excess of the host emulations %.3f' % (cls, worst))


@pytest.mark.parametrize('fault', AR.ADAMW_FAULTS)
def test_adamw_bound_catches(fault):
    """every faulty decay is outside the bound on the classes with parameters of order one and of order 1e-3, at the decayed
    settings (wd = 0.05; the annealed rate and the clip coefficient at work)"""
    for cls in ('normal', 'warm', 'tiny'):
        arrays = R.case(cls)
        for t in R.TS:
            h = R.hyper32(weight_decay=0.05, gscale=1.0)
            he = AR.effective(h, AR.LR_SCALE, AR.CLIP_COEF)
            got = AR.emulate_adamw(*arrays, t, h, True, fault=fault, lr_scale=AR.LR_SCALE, coef=AR.CLIP_COEF)
            failed, w = AR.verify('adamw', got, arrays, t, he)
            assert 'p' in failed, (fault, cls, t, w)


@pytest.mark.parametrize('cls', R.CLASSES)
def test_average_reference_holds_both_emulations_on_every_class(cls):
    p_old = R.case(cls)[0]
    e = AR.avg_start(cls)
    p_new = R.emulate('adam', *R.case(cls), 3, R.hyper32(weight_decay=0.0), True)['p']
    for d in AR.AVG_DECAYS:
        for fused in (False, True):
            bad, w = AR.verify_avg(AR.emulate_avg(e, p_old, p_new, d, fused), e, p_new, d)
            assert not bad, (cls, d, fused, w)
    bad, _ = AR.verify_avg(AR.emulate_avg(e, p_old, p_new, 0.9, taken=False), e, p_new, 0.9, taken=False)
    assert not bad


@pytest.mark.parametrize('fault', AR.AVG_FAULTS)
def test_average_bound_catches(fault):
    for cls in ('normal', 'warm'):
        p_old, g, m, v = R.case(cls)
        e = AR.avg_start(cls)
        p_new = R.emulate('adam', p_old, g, m, v, 1, R.hyper32(weight_decay=0.0), True)['p']
        for d in (0.9, 0.999):
            taken = fault != 'moved_on_skipped_step'
            got = AR.emulate_avg(e, p_old, p_new, d, True, fault=fault, taken=taken)
            bad, w = AR.verify_avg(got, e, p_new, d, taken=taken)
            assert bad, (fault, cls, d, w)


# ------------------------------------------------------------------------------------------------ 2. construction
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_construct_with_the_new_switches(kind):
    from drvae_amd import engine as E
    plain = tiny_model(kind)
    assert plain.ema_decay is None and plain._step_config().ema_decay is None and plain.ema_eval is True
    on = tiny_model(kind, ema_decay=0.99, optim_alg='adamw')
    cfg = on._step_config()
    assert cfg.ema_decay == 0.99 and cfg.optim_alg == 'adamw'
    assert list(on.state_dict()) == list(plain.state_dict())
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError):
            tiny_model(kind, ema_decay=bad)
        with pytest.raises(ValueError):
            E.StepConfig(ema_decay=bad)
    with pytest.raises(ValueError):
        tiny_model(kind, optim_alg='sgd')
    with pytest.raises(RuntimeError):
        plain.averaged_parameters()
    with pytest.raises(RuntimeError):
        plain.averaged_state_dict()


def test_adamax_launcher_refuses_decoupled_decay_and_a_bad_average(monkeypatch):
    kernel_ref.install(monkeypatch)
    import drvae_amd.kernels as K
    p, g, m, u = (torch.ones(8) for _ in range(4))
    step = torch.ones(1, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        K.adamax_l2(p, g, m, u, step, lr=1e-3, decoupled=True)
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(RuntimeError):
            K.adam_l2(p, g, m, u, step, lr=1e-3, avg=torch.ones(8), avg_decay=bad)
    with pytest.raises(ValueError):
        K.adam_l2(p, g, m, u, step, lr=1e-3, avg=torch.ones(8))


def test_the_ctypes_struct_carries_the_trailing_fields():
    """``kernels._hyper``: defaults leave the trailing fields zero / NULL (the sweep as it was); the fields sit behind lr_scale"""
    import ctypes as C
    from drvae_amd import _lib
    from drvae_amd import kernels as K
    names = [f[0] for f in _lib.AdamHyper._fields_]
    assert names[-4:] == ['lr_scale', 'decoupled', 'avg_decay', 'avg']
    h = K._hyper(1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, None)
    assert h.decoupled == 0 and h.avg_decay == 0.0 and not h.avg and not h.lr_scale
    h = K._hyper(1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, None, None, True)
    assert h.decoupled == 1 and not h.avg
    with pytest.raises(ValueError):
        K._hyper(1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, None, torch.zeros(8), False, torch.zeros(8), None)
    assert C.sizeof(_lib.AdamHyper) == 48 and _lib.AdamHyper.avg.offset == 40


def test_the_library_validates_the_trailing_fields_before_any_launch():
    """n == 0 and every other argument valid, so the tested field alone decides and nothing is launched (the pattern of
    tests/test_cabi.py; a, odd, off: addresses that are looked at and never dereferenced)"""
    import ctypes as C
    from drvae_amd import _lib
    lib = _lib.load()
    a, odd, off = 0x1000, 0x1004, 0x1002
    H = lambda **kw: C.byref(_lib.AdamHyper(lr=1e-3, **kw))
    adam = (lambda h: lib.dv_adam_l2(a, a, a, a, 0, h, a, None, 0, None),
            lambda h: lib.dv_adam_l2_clipped(a, a, a, a, 0, h, a, None, 0, None))
    adamax = (lambda h: lib.dv_adamax_l2(a, a, a, a, 0, h, a, None, 0, None),
              lambda h: lib.dv_adamax_l2_clipped(a, a, a, a, 0, h, a, None, 0, None))
    for fn in adam + adamax:
        assert fn(H()) == 0
        assert fn(H(avg=a, avg_decay=0.9)) == 0
        assert fn(H(avg=odd, avg_decay=0.9)) == 0                 # 4-byte aligned is enough (the scalar loop)
        assert fn(H(avg=off, avg_decay=0.9)) == -1
        for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
            assert fn(H(avg=a, avg_decay=bad)) == -1
            assert fn(H(avg_decay=bad)) == 0                      # read only when avg != NULL
    for fn in adam:
        assert fn(H(decoupled=1)) == 0 and fn(H(decoupled=1, avg=a, avg_decay=0.5)) == 0
    for fn in adamax:
        assert fn(H(decoupled=1)) == -1                           # torch has no decoupled Adamax


def test_a_late_change_of_ema_decay_raises(monkeypatch):
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae')
    model.ema_decay = 0.5                  # the attribute idiom works until the engine is built
    assert hasattr(model.engine().arena, 'avg')
    model.ema_decay = 0.75
    with pytest.raises(RuntimeError):
        model.engine()
    model.ema_decay = None
    with pytest.raises(RuntimeError):
        model.engine()
    model.ema_decay = 0.5
    model.engine()


# ------------------------------------------------------------------------------------------------ 3. off means untouched
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_pvae', 'tiny_vfae', 'tiny_drvae_adamax'])
def test_switches_off_is_the_step_as_it_was(name, monkeypatch):
    """the launch list with every launch's keyword names, and every bit of the result: the extended stand-ins with the
    switches off == the wrapped stand-ins (which know neither keyword); no average is allocated"""
    case, spec, params = case_of(name)
    functions = sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel', 'col_moment_blocks',
                                                                                   'nll_raw_cs_shape', 'heads_tiles'})
    out = {}
    for tag, install, kw in (('parent', kernel_ref.install, {}), ('off', kernel_ref.install, dict(ema_decay=None))):
        with pytest.MonkeyPatch.context() as outer:
            install(outer)
            eng, arena = make_engine(spec, params, **kw)
            set_batch(eng, case['batch'])
            with pytest.MonkeyPatch.context() as mpc:
                log = _launch_log(mpc, functions)
                for noise in case['noises'][:2]:
                    eng.train_step(noise)
            assert not hasattr(arena, 'avg') and eng.averaged is False
            out[tag] = (log, arena.param.clone(), arena.exp_avg.clone(), arena.exp_avg_sq.clone(), arena.loss.clone())
    a, b = out['parent'], out['off']
    assert a[0] == b[0]
    assert not any({'avg', 'avg_decay', 'decoupled'} & set(kw) for _, kw in b[0])
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert kernel_ref.CALLS['decoupled_sweeps'] == 0 and kernel_ref.CALLS['averaged_sweeps'] == 0


# ------------------------------------------------------------------------------------------------ 4. AdamW against torch
class AdamW64:
    """torch.optim.AdamW in float64 on float64 copies of the parameters, stepped on the ORACLE's gradients (its fp32 autograd
    pass at the float64 route's current parameters, rounded to fp32), with torch's own clip and the annealed rate"""

    def __init__(self, spec, params, cfg, arena, max_norm=None, lr_itermax=0):
        self.spec, self.cfg = spec, cfg
        self.names = live_names(arena, cfg)
        self.oracle = M.init_params(spec, params)          # name -> fp32 leaf tensors
        self.p = {k: self.oracle[k].detach().double().clone().requires_grad_(True) for k in self.names}
        self.opt = torch.optim.AdamW(list(self.p.values()), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
        self.max_norm, self.lr_itermax, self.iters = max_norm, lr_itermax, 0
        self.traj = []

    def step(self, batch, noise):
        for k in self.names:
            self.oracle[k].data.copy_(self.p[k].detach().float())
            self.oracle[k].grad = None
        losses, _ = M.loss_function(self.spec, self.oracle, batch, noise, self.iters, True)
        losses['CMPL'].backward()
        for k in self.names:
            self.p[k].grad = self.oracle[k].grad.detach().double().clone()
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(self.p.values()), self.max_norm, norm_type=2)
        if self.lr_itermax:
            scale = float(kernel_ref.record(self.iters, (0, 0), 0, (0, 0), self.lr_itermax)[3])
            for grp in self.opt.param_groups:
                grp['lr'] = kernel_ref.lr_effective(self.cfg.learning_rate, torch.tensor([scale]))
        self.opt.step()
        self.iters += 1

    def state(self, k, what):
        if what == 'param':
            return self.p[k].detach()
        return self.opt.state[self.p[k]][what]


@pytest.mark.parametrize('anneal', [False, True], ids=['fixed_lr', 'annealed_lr'])
@pytest.mark.parametrize('clip', [False, True], ids=['unclipped', 'clipped'])
@pytest.mark.parametrize('name', MODEL_CASES)
def test_adamw_steps_against_torch_in_float64(name, clip, anneal, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    kw = dict(optim_alg='adamw')
    if anneal:
        kw.update(anneal_learning_rate=True, anneal_lr_itermax=3)
    thr = None
    if clip:
        probe, parena = make_engine(spec, params)
        set_batch(probe, case['batch'])
        gradients(probe, case['noises'][0])
        thr = 0.5 * grad_norm64(parena, probe.cfg)
    eng, arena = make_engine(spec, params, max_grad_norm=thr, **kw)
    if anneal:
        eng.universal = True
    set_batch(eng, case['batch'])
    ref = AdamW64(spec, case['param_seed'], eng.cfg, arena, max_norm=thr, lr_itermax=3 if anneal else 0)
    noises = case['noises'][:N_STEPS]            # (the WeightNorm case has two)
    for i, noise in enumerate(noises):
        eng.train_step(noise)
        ref.step(case['batch'], noise)
        compare_state(arena, ref, '%s step %d' % (name, i))
    assert kernel_ref.CALLS['decoupled_sweeps'] >= len(noises)
    # ... and the coupled form is NOT within that tolerance of it (weight_decay is 0.05 in these cases): the check sees the switch
    coupled, carena = make_engine(spec, params, max_grad_norm=thr, **dict(kw, optim_alg='adam'))
    if anneal:
        coupled.universal = True
    set_batch(coupled, case['batch'])
    for noise in noises:
        coupled.train_step(noise)
    with pytest.raises(AssertionError):
        compare_state(carena, ref, name + ' (coupled)')


# ------------------------------------------------------------------------------------------------ 5. the average
@pytest.mark.parametrize('name', MODEL_CASES + ['tiny_drvae_adamax'])
def test_average_equals_the_float64_recurrence_over_the_trajectory(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    eng, arena = make_engine(spec, params, ema_decay=D)
    assert torch.equal(arena.avg, arena.param)                 # starts as the initial parameters
    set_batch(eng, case['batch'])
    e64 = arena.param.double().numpy().copy()
    bound = np.zeros_like(e64)
    w = 1.0 - float(np.float32(D))
    noises = case['noises'][:N_STEPS]
    for noise in noises:
        eng.train_step(noise)
        p_new = arena.param.double().numpy()
        _, b = AR.ref_avg(e64, p_new, D)
        e64 = e64 + w * (p_new - e64)
        bound = (1.0 - w) * bound + b                          # (an earlier step's error is carried with weight d < 1)
    # the sum of the per-step bounds, each carried on with weight d: at most T x the per-step bound
    got = arena.avg.double().numpy()
    n = arena.n_live
    excess = R.excess(got[:n], e64[:n], bound[:n])
    print('%s: worst excess of the average after %d steps %.3f' % (name, len(noises), float(excess.max())))
    assert (excess <= 1.0).all()
    assert not torch.equal(arena.avg[:n], arena.param[:n])
    # frozen parameters (behind n_live) keep their initial value in the average; pads stay zero
    assert torch.equal(arena.avg[n:], arena.param[n:])
    for pad in arena.pads(arena.avg):
        assert not pad.any()
    assert kernel_ref.CALLS['averaged_sweeps'] == len(noises)


@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_drvae_adamax'])
def test_a_skipped_step_leaves_the_average_alone(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    eng, arena = make_engine(spec, params, max_grad_norm=1e6, ema_decay=D)
    set_batch(eng, case['batch'])
    eng.train_step(case['noises'][0])
    before = arena.avg.clone()
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case['batch'].items()}
    bad['x1'] = bad['x1'].copy()
    bad['x1'][0, 0] = float('nan')
    set_batch(eng, bad)
    eng.train_step(case['noises'][1])
    assert eng.clip_stats()['skipped_last']
    assert torch.equal(arena.avg, before)
    # the faulty stand-in that moves it anyway is seen by the same comparison
    kernel_ref.FAULT['name'] = 'moved_on_skipped_step'
    eng.train_step(case['noises'][1])
    assert eng.clip_stats()['skipped_last'] and not torch.equal(arena.avg, before)


# ------------------------------------------------------------------------------------------------ 6. the context
def test_averaged_parameters_context(monkeypatch, tmp_path):
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae', ema_decay=D)
    batch = _model_batch(model)
    spec_noise = M.ModelSpec(kind='drvae', dim_x=13, dim_y=2, dim_z1=5, dim_z3=4, L=2)
    noises = [M.make_noise(spec_noise, 8, seed=70 + i) for i in range(4)]
    for noise in noises[:3]:
        model.run_on_batch(train_mode=True, noise=noise, **batch)
    eng, arena = model.engine(), model.engine().arena
    live, avg = arena.param.clone(), arena.avg.clone()
    assert not torch.equal(live, avg)
    sd = model.averaged_state_dict()
    assert list(sd) == list(model.state_dict())
    for k, v in sd.items():
        assert torch.equal(v, arena.e(k)) and not torch.equal(v, arena.p(k))
    assert torch.equal(arena.param, live) and torch.equal(arena.avg, avg)        # ... without disturbing the live ones
    second = tiny_model('drvae', random_seed=11)
    second.load_state_dict(sd)
    second.finished_training_iters = model.finished_training_iters      # (the perturbation coefficient hangs on it)
    want = {k: float(v) for k, v in second.run_on_batch(train_mode=False, noise=noises[3], **batch).items()}
    with model.averaged_parameters():
        assert eng.averaged and torch.equal(arena.param, avg) and torch.equal(arena.avg, live)
        got = {k: float(v) for k, v in model.run_on_batch(train_mode=False, noise=noises[3], **batch).items()}
        inside = model.averaged_state_dict()
        for bad in (lambda: model.run_on_batch(train_mode=True, noise=noises[3], **batch), lambda: eng.train_step(noises[3]),
                    lambda: eng.optimizer_step(), lambda: eng.replay()):
            with pytest.raises(RuntimeError):
                bad()
        model.save_to_file(str(tmp_path / 'avg.pth'))          # the reference's snapshot: whatever the arena holds
    assert got == want
    assert all(torch.equal(inside[k], sd[k]) for k in sd)
    assert not eng.averaged and torch.equal(arena.param, live) and torch.equal(arena.avg, avg)     # live bits restored
    saved = torch.load(str(tmp_path / 'avg.pth'))
    assert all(torch.equal(saved[k], sd[k]) for k in sd)
    live_loss = {k: float(v) for k, v in model.run_on_batch(train_mode=False, noise=noises[3], **batch).items()}
    assert live_loss != got
    # an exception inside the context puts the live parameters back too
    with pytest.raises(KeyError):
        with model.averaged_parameters():
            raise KeyError('x')
    assert not eng.averaged and torch.equal(arena.param, live)
    # loading parameters resets the average to the loaded values
    model.load_state_dict(second.state_dict())
    assert torch.equal(arena.avg, arena.param) and torch.equal(arena.p('encoder_z1.nnet.model.linear1.weight'),
                                                                sd['encoder_z1.nnet.model.linear1.weight'])
    model.run_on_batch(train_mode=True, noise=noises[3], **batch)
    assert not torch.equal(arena.avg, arena.param)
    f = str(tmp_path / 'p.pth')
    second.save_to_file(f)
    model.load_params_from_file(f)
    assert torch.equal(arena.avg, arena.param)


# ------------------------------------------------------------------------------------------------ 7. fit
def _fit_once(monkeypatch, tmp_path, tag, **kw):
    from tests.test_fit import _loader, _tiny_dataset, _tiny_model
    model = _tiny_model('drvae', device='cpu', **kw)
    logs = []
    model.w2log = lambda *a: logs.append(' '.join(str(e) for e in a))
    tr, va = _tiny_dataset('drvae', 40, 1), _tiny_dataset('drvae', 24, 2)
    fn = str(tmp_path / (tag + '.pth'))
    seen = []
    real = model.save_to_file

    def save(filename):
        a = model.engine().arena
        seen.append((model.engine().averaged, a.param.clone(), a.avg.clone() if hasattr(a, 'avg') else None))
        return real(filename)
    model.save_to_file = save
    return model, logs, fn, seen, (tr, va, _loader)


def test_fit_evaluates_and_snapshots_the_average(monkeypatch, tmp_path):
    import re
    kernel_ref.install(monkeypatch)
    runs = {}
    for tag, kw, ema_eval in (('off', {}, True), ('avg', dict(ema_decay=D), True), ('live', dict(ema_decay=D), False)):
        model, logs, fn, seen, (tr, va, _loader) = _fit_once(monkeypatch, tmp_path, tag, **kw)
        model.ema_eval = ema_eval
        model.fit(_loader(tr, 8), _loader(va, 8), add_noise=True, verbose=False, early_stop=True, model_filename=fn)
        assert seen and os.path.exists(fn)
        runs[tag] = (model, logs, torch.load(fn), seen)
    model, _, saved, seen = runs['avg']
    averaged, held, other = seen[-1]
    assert averaged and not model.engine().averaged
    names = dict(model.named_parameters())
    for k in names:           # the file holds the average as it stood at the snapshot epoch (then in the parameter arena)
        assert torch.equal(saved[k], model.engine().arena._view(held, k)), k
        assert not torch.equal(saved[k], model.engine().arena._view(other, k)), k
    model, _, saved, seen = runs['live']
    averaged, held, other = seen[-1]
    assert not averaged
    for k in names:
        assert torch.equal(saved[k], model.engine().arena._view(held, k)), k
    # training itself is the same run (the live trajectory does not depend on what is evaluated)
    assert torch.equal(runs['avg'][0].engine().arena.param, runs['live'][0].engine().arena.param)
    assert torch.equal(runs['avg'][0].engine().arena.param, runs['off'][0].engine().arena.param)
    # log lines: identical in format (numbers and times masked)
    mask = lambda lines: [re.sub(r'[-+]?(\d+\.\d*|\.\d+|\d+)([eE][-+]?\d+)?|nan|inf', '#', ln) for ln in lines
                          if not ln.startswith(('Starting training', 'Finished training'))]
    strip = lambda lines: [ln for ln in mask(lines) if not ln.startswith(('* Snapshotting', 'Early stopping', 'Continuing'))]
    assert strip(runs['off'][1]) == strip(runs['avg'][1]) == strip(runs['live'][1])


# ------------------------------------------------------------------------------------------------ 8. resume
def test_training_state_round_trip_carries_the_average_bitwise(monkeypatch, tmp_path):
    kernel_ref.install(monkeypatch)
    kw = dict(ema_decay=D, optim_alg='adamw')
    spec_noise = M.ModelSpec(kind='drvae', dim_x=13, dim_y=2, dim_z1=5, dim_z3=4, L=2)
    noises = [M.make_noise(spec_noise, 8, seed=70 + i) for i in range(3)]
    one = tiny_model('drvae', **kw)
    batch = _model_batch(one)
    for noise in noises[:2]:
        one.run_on_batch(train_mode=True, noise=noise, **batch)
    f = str(tmp_path / 'state.pth')
    one.save_training_state(f)
    avg_at_2 = one.engine().arena.avg.clone()
    one.run_on_batch(train_mode=True, noise=noises[2], **batch)
    want = one.engine().arena
    two = tiny_model('drvae', random_seed=77, **kw)
    two.load_training_state(f)
    assert torch.equal(two.engine().arena.avg, avg_at_2) and not torch.equal(avg_at_2, two.engine().arena.param)
    two.run_on_batch(train_mode=True, noise=noises[2], **batch)
    got = two.engine().arena
    for name in ('param', 'exp_avg', 'exp_avg_sq', 'loss', 'avg'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    # ``.to()`` re-adoption keeps the run going: the average travels with the moments
    one._stash_optimizer_state()
    assert torch.equal(one._opt_stash['avg'], want.avg)
    one._opt_stash = None


def test_a_pending_stash_does_not_leak_the_old_average_into_loaded_weights(monkeypatch):
    """``.to()`` retires the engine and stashes the state; parameters loaded before the next engine is built must not meet
    the stashed average of the OLD weights.  Inside ``averaged_parameters()`` the state is neither moved nor saved"""
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae', ema_decay=D)
    batch = _model_batch(model)
    spec_noise = M.ModelSpec(kind='drvae', dim_x=13, dim_y=2, dim_z1=5, dim_z3=4, L=2)
    for i in range(2):
        model.run_on_batch(train_mode=True, noise=M.make_noise(spec_noise, 8, seed=70 + i), **batch)
    old_avg = model.engine().arena.avg.clone()
    with model.averaged_parameters():
        with pytest.raises(RuntimeError):
            model._stash_optimizer_state()
        with pytest.raises(RuntimeError):
            model.save_training_state('unused.pth')
    # what ``_apply`` does when the parameters have left the arena (``.to()``): stash, retire
    model._stash_optimizer_state()
    assert torch.equal(model._opt_stash['avg'], old_avg)
    for prm in model.parameters():
        prm.data = prm.data.clone()
    model._engine = model._arena = None
    other = tiny_model('drvae', random_seed=23)
    model.load_state_dict(other.state_dict())
    assert 'avg' not in model._opt_stash
    arena = model.engine().arena
    assert torch.equal(arena.avg, arena.param) and not torch.equal(arena.avg, old_avg)
    assert int(model.engine().step_dev[0]) == 2                   # (the rest of the stash still travels)


# ------------------------------------------------------------------------------------------------ 9. data parallelism
def _dp_steps(spec, batch, noises, counts, allreduce, lo=None, hi=None):
    if lo is not None:
        batch = {k: v[lo:hi] for k, v in batch.items()}
        noises = [M.slice_noise(n, lo, hi) for n in noises]
    eng, arena = engine_with(spec, M.init_params(spec, 9, as_numpy=True), None, ema_decay=D, optim_alg='adamw')
    set_small_batch(eng, batch, counts=counts)
    for noise in noises:
        eng.train_step(noise, allreduce=allreduce)
    return arena.param.clone().numpy(), arena.avg.clone().numpy()


def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        import drvae_amd.kernels as K
        for name in kernel_ref.FUNCTIONS:
            setattr(K, name, getattr(kernel_ref, name))
        from drvae_amd import dist as DD
        DD.init_from_env(backend='gloo')
        spec, batch, noises = small_case('drvae')
        n = batch['x1'].shape[0]
        lo, hi = DD.shard_rows(n, rank, world)
        counts = DD.global_counts(batch['has_x2'][lo:hi], batch['has_y'][lo:hi], 'drvae', spec.semi_supervised)
        q.put((rank,) + _dp_steps(spec, batch, noises[:N_STEPS], counts, DD.allreduce_sum, lo, hi))
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_keep_bit_identical_averages_equal_to_one_rank(monkeypatch):
    kernel_ref.install(monkeypatch)
    spec, batch, noises = small_case('drvae')
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
        assert len(res) == 3, res[1]
        np.testing.assert_allclose(res[1], single[0], rtol=1e-5, atol=1e-6)       # (the bounds of tests/test_dp_gloo.py)
        np.testing.assert_allclose(res[2], single[1], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(got[0][1], got[1][1])                           # replicas stay bit-identical:
    np.testing.assert_array_equal(got[0][2], got[1][2])                           # ... the averages too
    assert not np.array_equal(got[0][1], got[0][2])


def test_the_broadcast_of_data_parallelism_carries_the_average(monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd import dist as DD
    sent = []
    monkeypatch.setattr(DD, 'broadcast', lambda t: sent.append(t.data_ptr()))
    monkeypatch.setattr(DD, 'broadcast_int', lambda v: v)
    monkeypatch.setattr(DD, 'force_dp', lambda: True)
    model = tiny_model('drvae', ema_decay=D)
    model.enable_data_parallel(rank=0, world=1)
    assert model.engine().arena.avg.data_ptr() in sent
    sent.clear()
    plain = tiny_model('drvae')
    plain.enable_data_parallel(rank=0, world=1)
    assert len(sent) == 5


# ------------------------------------------------------------------------------------------------ 10. the dual-graph schedule
def test_dual_graph_schedule_sweeps_the_average_on_both_halves(monkeypatch):
    """cfg-2 shape recorded as the dual-graph step: 'adamw' takes the schedule 'adam' takes, the main chain's gated sweep and
    the side chain's half carry the decoupled switch and the average's slices [0, hs) and [hs, n_live); the result equals
    the eager engine's bit for bit"""
    from tests import fold_trace as FT
    import drvae_amd.kernels as K
    import drvae_amd.tuning as T
    kernel_ref.install(monkeypatch)
    monkeypatch.setenv('DRVAE_TUNE', 'fold_rows=0')
    monkeypatch.setattr(T, '_VALUES', None)
    spec, batch, _ = small_case('drvae')
    params = M.init_params(spec, 9, as_numpy=True)
    kw = dict(ema_decay=D, optim_alg='adamw')
    eager, ea = engine_with(spec, params, None, **kw)
    dual, da = engine_with(spec, params, None, **kw)
    plain, _ = engine_with(spec, params, None)
    for e in (eager, dual, plain):
        set_small_batch(e, batch)
        e.training = True
    for split in (False, True, 'overlap', 'captured'):
        assert dual._step_tail(split, on_gpu=True) == plain._step_tail(split, on_gpu=True)
    calls = []
    real = K.adam_l2
    monkeypatch.setattr(K, 'adam_l2', lambda *a, **k: (calls.append((a[0], k)), real(*a, **k))[1])
    functions = sorted(set(kernel_ref.FUNCTIONS))
    for step in range(N_STEPS):
        eager.train_step()
        tail = dual._step_tail(False, on_gpu=True)
        assert tail.dual and tail.side_adam and tail.adam_gated
        calls.clear()
        FT.step(dual, tail, functions)
        for name in ('param', 'exp_avg', 'exp_avg_sq', 'loss', 'avg'):
            assert torch.equal(getattr(da, name), getattr(ea, name)), (step, name)
        assert int(dual.sync_err[0::2].abs().sum()) == 0
        swept = [(p, k) for p, k in calls if k.get('avg') is not None
                 and da.param.data_ptr() <= p.data_ptr() < da.param.data_ptr() + 4 * da.n_params]
        assert len(swept) == 2
        spans = []
        for p, k in swept:
            assert k['decoupled'] is True and k['avg_decay'] == D
            off = (p.data_ptr() - da.param.data_ptr()) // 4
            assert (k['avg'].data_ptr() - da.avg.data_ptr()) // 4 == off and k['avg'].numel() == p.numel()
            spans.append((off, off + p.numel()))
        assert sorted(spans) == [(0, tail.hs), (tail.hs, da.n_live)]
    assert not torch.equal(da.avg[:da.n_live], da.param[:da.n_live])
    monkeypatch.setattr(T, '_VALUES', None)
