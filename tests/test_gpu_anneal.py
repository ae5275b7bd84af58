"""-m gpu: the annealing schedules of the fused train step on the real kernels -- the device record (``dv_batch_masks`` as a
launch of its own and as the feed's extra workgroup) bit for bit against fp32 of the float64 formula, every coefficient vector
it writes against float64, the optimiser sweeps with ``dv_adam_hyper.lr_scale`` on every launch path against
tests/optim_ref.py, the annealed step against tests/anneal_ref.py, eager == captured bit for bit in the dual-graph schedule
(plain, clipped, on the sampler feed), evaluation mid-ramp, ``fit``, and the schedules-off launch list.  Nothing here races a
wait on purpose: the ordering of the next step's head behind the side chain's tail is tested by bitwise equality."""
import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import anneal_ref as R
from tests import optim_ref as OR
from tests.test_anneal_cpu import N_STEPS, SCHEDULES, case, make_engine, run_reference, set_batch
from tests.test_gpu_optim import LEADS, bits, guards_hold, hold_sample, place

pytestmark = pytest.mark.gpu

BIG = (16 << 20) + 5            # adam_stream_kernel
# the tolerances tests/test_gpu_models.py holds the unannealed step to (losses; parameters), unchanged
LOSS_TOL, PARAM_TOL = dict(rtol=1e-4, atol=1e-5), dict(rtol=2e-4, atol=5e-5)


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


# ------------------------------------------------------------------------------------------------ 1. record + coefficient vectors
def _mask_buffers(B, L, Np, dev):
    f = lambda n: torch.full((n,), 9.0, device=dev)
    return dict(c_nll=f(L * (B + 2 * Np)), c_klz2=f(L * Np), c_yl=f(L * B), w_recl=f(2 * L * B), w_pert=f(L * B), w_yl=f(L * B),
                label=torch.full((L * B,), 9, dtype=torch.int32, device=dev), c_klp=f(B + Np))


def _anneal_buffers(B, L, Np, dev, step, sched):
    f = lambda n: torch.full((n,), 9.0, device=dev)
    return dict(step=step, pert=(3, 2), kl=sched['anneal_kl_itermax'] if sched['anneal_kl'] else 0,
                yl=(sched['anneal_yloss_itermax'] if sched['anneal_yloss'] else 0, sched['anneal_yloss_offset']),
                lr=sched['anneal_lr_itermax'] if sched['anneal_learning_rate'] else 0, mmd_rate=0.7, sched=f(4), w_elbo=f(3),
                w_cmpl=f(8), c_kld=f(L * B), w_klz2=f(L * Np), w_klp=f(B + Np))


def _expected_vectors(c, px, py, B, L, Np, n_tot, kl_rate, pert_rate, yl_rate, mmd_rate):
    """float64: every vector of the annealed launch from the four coefficients ``c`` and the batch's flags"""
    n_pairs, n_lab = max(1.0, float(px.sum())), max(1.0, float(py.sum()))
    ct = 1.0 / (L * n_tot)
    pxs, pyr = np.tile(px[:Np], L), np.tile(py, L)
    w_klz2 = np.where(pxs, c['beta_pert'] * kl_rate * ct, 0.0)
    w_klp = np.concatenate([np.full(B, 1.0 / n_tot), np.where(px[:Np], 1.0 / n_tot, 0.0)])
    return dict(
        c_nll=np.concatenate([np.full(L * B, -ct), np.where(pxs, -ct, 0.0),
                              np.where(pxs, -c['beta_pert'] * pert_rate / (L * n_pairs), 0.0)]),
        w_recl=np.concatenate([np.full(L * B, ct), np.where(pxs, ct, 0.0)]), w_pert=np.where(pxs, 1.0 / (L * n_pairs), 0.0),
        w_klz2=w_klz2, c_klz2=w_klz2 * c['beta_kl'], w_klp=w_klp, c_klp=w_klp * c['beta_kl'],
        c_yl=np.where(pyr, -yl_rate / (L * n_lab), 0.0) * c['beta_yr'], w_yl=np.full(L * B, 1.0 / (L * n_lab)),
        c_kld=np.full(L * B, c['beta_kl'] * ct), w_elbo=np.array([1.0, -c['beta_kl'], c['beta_pert'] * pert_rate]),
        w_cmpl=np.array([0, 0, 0, -c['beta_yr'] * yl_rate, -mmd_rate, -1.0, 0, 0]))


@pytest.mark.parametrize('name', ['all', 'kl', 'yloss', 'lr'])
def test_record_and_coefficient_vectors_in_both_forms_of_the_launch(K, dev, name):
    """``it`` = 0 .. 6 across ramps of 3 iterations (the perturbation and y-loss ramps with an offset of 2): the record is
    np.float32 of the float64 formula bit for bit; every vector within the bound of the existing masks test (rtol 1e-6), the
    single-rounding ones exactly; the launch of its own (through the table, and on explicit flags) and the feed's extra
    workgroup write the same bits; nothing is written outside the vectors"""
    sched = SCHEDULES[name]
    B, L, Np, Y, X = 37, 3, 16, 3, 12
    g = torch.Generator().manual_seed(0)
    hx = (torch.rand(200, generator=g) < 0.4).to(torch.int32).to(dev)
    hy = (torch.rand(200, generator=g) < 0.6).to(torch.int32).to(dev)
    y = torch.randint(0, Y, (200,), generator=g).to(torch.int32).to(dev)
    table = torch.randint(0, 200, (7, B), generator=g).to(torch.int32).to(dev)
    x1, x2 = torch.randn(200, X, generator=g).to(dev), torch.randn(200, X, generator=g).to(dev)
    pair_rows = torch.arange(Np, dtype=torch.int32, device=dev)
    base = torch.zeros(1, dtype=torch.int32, device=dev)
    rates = dict(n_tot=float(B), kl_rate=0.7, pert_rate=0.05, yl_rate=1.3)
    for it in range(7):
        step = torch.tensor([it], dtype=torch.int32, device=dev)
        rows = table[it].long()
        got = {}
        for form in ('own', 'explicit', 'feed'):
            bufs, an = _mask_buffers(B, L, Np, dev), _anneal_buffers(B, L, Np, dev, step, sched)
            kw = dict(rates, beta=None, hx=hx, hy=hy, y=y, Np=Np, anneal=an, **bufs)
            if form == 'own':
                K.batch_masks(B, L, table=table, n_batches=7, ctr=step, base=base, **kw)
            elif form == 'explicit':
                kw.update(hx=hx[rows].contiguous(), hy=hy[rows].contiguous(), y=y[rows].contiguous())
                K.batch_masks(B, L, **kw)
            else:
                K.batch_feed(torch.zeros(B + Np, X, device=dev), x1, x2, y, table, 7, step, base, pair_rows=pair_rows, L=L, masks=kw)
            torch.cuda.synchronize()
            got[form] = dict(bufs, **{k: an[k] for k in ('sched', 'w_elbo', 'w_cmpl', 'c_kld', 'w_klz2', 'w_klp')})
        for k in got['own']:
            assert torch.equal(got['own'][k], got['feed'][k]) and torch.equal(got['own'][k], got['explicit'][k]), (it, k)
        want = R.record32(it, sched, pert_itermax=3, pert_offset=2)
        rec = got['own']['sched'].cpu().numpy()
        assert rec.tobytes() == want.tobytes(), (it, rec, want)
        c = R.coefficients(it, sched, pert_itermax=3, pert_offset=2)
        px, py = hx[rows].cpu().numpy() != 0, hy[rows].cpu().numpy() != 0
        exp = _expected_vectors(c, px, py, B, L, Np, float(B), 0.7, 0.05, 1.3, 0.7)
        for k, w in exp.items():
            a = got['own'][k].cpu().numpy()
            np.testing.assert_allclose(a[:w.size], w, rtol=1e-6, atol=1e-9, err_msg='it=%d %s' % (it, k))
            assert (a[w.size:] == 9.0).all(), (it, k, 'written past its end')
        # single roundings: exact
        assert got['own']['w_elbo'][:2].cpu().numpy().tobytes() == np.array([1.0, -want[1]], np.float32).tobytes()
        assert got['own']['w_cmpl'].cpu().numpy()[[0, 1, 2, 4, 5, 6, 7]].tobytes() == \
            np.array([0, 0, 0, -np.float32(0.7), -1, 0, 0], np.float32).tobytes()
        lab = got['own']['label'].cpu().numpy()
        assert ((lab <= -2) == np.tile(py, L)).all()


def test_a_zeroed_tail_is_the_launch_as_it_was(K, dev):
    """the descriptor's trailing fields left zero (no ``anneal``): the same bits as ever, ``beta`` is read; outputs of the
    schedule without its step counter are refused"""
    from drvae_amd import _lib
    B, L = 21, 2
    g = torch.Generator().manual_seed(1)
    hx = (torch.rand(B, generator=g) < 0.5).to(torch.int32).to(dev)
    hy = (torch.rand(B, generator=g) < 0.5).to(torch.int32).to(dev)
    y = torch.randint(0, 3, (B,), generator=g).to(torch.int32).to(dev)
    beta = torch.tensor([0.01], device=dev)
    rates = dict(n_tot=float(B), kl_rate=0.7, pert_rate=0.05, yl_rate=1.3)
    a, b = _mask_buffers(B, L, B, dev), _mask_buffers(B, L, B, dev)
    K.batch_masks(B, L, beta=beta, hx=hx, hy=hy, y=y, **rates, **a)
    # the same coefficients from a schedule whose record comes out {0.01, 1, 1, 1}
    an = _anneal_buffers(B, L, B, dev, torch.zeros(1, dtype=torch.int32, device=dev), R.settings())
    an['pert'] = (1, 0)
    K.batch_masks(B, L, beta=None, hx=hx, hy=hy, y=y, anneal=an, **rates, **b)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert an['sched'].cpu().numpy().tobytes() == np.array([0.01, 1, 1, 1], np.float32).tobytes()
    assert torch.equal(an['w_klz2'], a['c_klz2']) and torch.equal(an['w_klp'], a['c_klp'])
    md = K._masks_desc(dict(rates, beta=beta, hx=hx, hy=hy, y=y, **a), B)
    md.w_elbo = K._f32(an['w_elbo'])
    import ctypes as C
    assert _lib.load().dv_batch_masks(C.byref(md), None, 0, None, None, B, L, K._stream()) == -1      # (refused: no launch)


# ------------------------------------------------------------------------------------------------ 2. the sweeps
def _lr_eff(h, s):
    return float(np.float32(np.float64(np.float32(h['lr'])) * np.float64(np.float32(s))))


def _hk(h):
    return {k: h[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'gscale')}


def _run(fn, src, dev, lead, *args, **kw):
    placed = [place(x, dev, lead) for x in src]
    fn(*[v for _, v in placed], *args, **kw)
    torch.cuda.synchronize()
    assert all(guards_hold(b, lead, src[0].numel()) for b, _ in placed)
    return placed


@pytest.mark.parametrize('kind', OR.KINDS)
def test_scaled_sweeps_within_the_bound_of_the_reference_at_the_scaled_rate(K, dev, kind):
    """float4 and scalar loops, plain / gated / clipped, both optimisers: every stored element within tests/optim_ref.py's
    componentwise bound of one step at lr * lr_scale; and bit-equal to the sweep handed that rate by value"""
    from tests.test_gpu_clip import _state_with
    plain, clipped = (K.adam_l2, K.adam_l2_clip) if kind == 'adam' else (K.adamax_l2, K.adamax_l2_clip)
    for s in (0.34333333, 0.01, 0.99):
        scale = torch.tensor([s], dtype=torch.float32, device=dev)
        for t, wd, gs in ((1, 0.0, 1.0), (7, 0.05, 0.125)):
            arrays, h, _ = OR.case_ref(kind, 'normal', t, gs, wd)
            h2 = dict(h, lr=_lr_eff(h, s))
            src = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            for lead in LEADS:
                site = (kind, s, t, wd, gs, lead)
                forms = {'plain': lambda *v, **k: plain(*v, step, **k),
                         'clipped': lambda *v, **k: clipped(*v, _state_with(dev, t, 1.0), **k)}
                if kind == 'adam':
                    flag, err = step.clone(), torch.zeros(2, dtype=torch.int32, device=dev)     # (published already: no wait)
                    forms['gated'] = lambda *v, **k: plain(*v, step, gate=(flag, step, 0, err, 3, min(40, arrays[0].size)), **k)
                ref_bits = None
                for form, fn in forms.items():
                    a = _run(fn, src, dev, lead, lr_scale=scale, **_hk(h))
                    b = _run(fn, src, dev, lead, **_hk(h2))
                    for (ba, _), (bb, _) in zip(a, b):
                        assert torch.equal(bits(ba), bits(bb)), site + (form,)
                    got = {'p': a[0][1].cpu().numpy(), 'm': a[2][1].cpu().numpy(), OR.STORED[kind][2]: a[3][1].cpu().numpy()}
                    failed, worst, _ = OR.verify(kind, got, arrays, t, h2, site=str(site + (form,)))
                    assert failed == set(), (site, form, worst)
                    if ref_bits is None:
                        ref_bits = [bits(x).clone() for x, _ in a]
                    else:
                        assert all(torch.equal(x, bits(y)) for x, (y, _) in zip(ref_bits, a)), site + (form,)


@pytest.mark.parametrize('kind,n,lead', [('adam', 4099, 0), ('adam', 4099, 1), ('adam', BIG, 0), ('adamax', 4099, 0),
                                         ('adamax', 4099, 1)])
def test_lr_scale_of_one_gives_the_bits_of_the_null_sweep(K, dev, kind, n, lead):
    """... and the streaming sweep honours the pointer: its scaled result is the by-value sweep's, a sample within the bound"""
    from tests.test_gpu_clip import _state, _state_with
    plain, clipped = (K.adam_l2, K.adam_l2_clip) if kind == 'adam' else (K.adamax_l2, K.adamax_l2_clip)
    src = _state(n, dev)
    h = OR.hyper32(weight_decay=0.05, gscale=0.125)
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    for form, fn in (('plain', lambda *v, **k: plain(*v, step, **k)),
                     ('clipped', lambda *v, **k: clipped(*v, _state_with(dev, 7, 0.37, 0, 2), **k))):
        a = _run(fn, src, dev, lead, **_hk(h))
        b = _run(fn, src, dev, lead, lr_scale=one, **_hk(h))
        for (ba, _), (bb, _) in zip(a, b):
            assert torch.equal(bits(ba), bits(bb)), (kind, n, lead, form)
        assert not torch.equal(a[0][1], src[0])
        del a, b
    s = 0.34333333
    scale = torch.tensor([s], dtype=torch.float32, device=dev)
    h2 = dict(h, lr=_lr_eff(h, s))
    a = _run(lambda *v, **k: plain(*v, step, **k), src, dev, lead, lr_scale=scale, **_hk(h))
    b = _run(lambda *v, **k: plain(*v, step, **k), src, dev, lead, **_hk(h2))
    for (ba, _), (bb, _) in zip(a, b):
        assert torch.equal(bits(ba), bits(bb)), (kind, n, lead)
    hold_sample(kind, [v for _, v in a], src, 7, h2, '%s n=%d lead=%d scaled' % (kind, n, lead))


# ------------------------------------------------------------------------------------------------ 3. the step
STEP_CASES = [('drvae', 'kl'), ('drvae', 'yloss_offset'), ('drvae', 'lr'), ('drvae', 'all'), ('pvae', 'all'), ('vfae', 'all')]


@pytest.mark.parametrize('kind,name', STEP_CASES)
def test_annealed_step_against_the_reference(dev, kind, name):
    """7 eager steps: the losses of every step and the final parameters at the tolerances of tests/test_gpu_models.py; the
    device record read back after every step"""
    spec, batch, noises = case(kind)
    sched = SCHEDULES[name]
    eng, arena = make_engine(spec, M.init_params(spec, 9, as_numpy=True), sched, device=dev)
    set_batch(eng, batch, dev)
    want, wprm = run_reference(spec, sched, batch, noises)
    for step, noise in enumerate(noises):
        eng.train_step(noise)
        got = eng.losses()
        rec = np.array(list(eng.schedule_record().values()), np.float32)
        assert rec.tobytes() == R.record32(step, sched, spec.anneal_perturb_rate_itermax, spec.anneal_perturb_rate_offset).tobytes()
        for k, v in got.items():
            np.testing.assert_allclose(v, want[step][k], err_msg='step %d %s' % (step, k), **LOSS_TOL)
    assert eng.plan.universal and eng.plan.annealed and len(noises) == N_STEPS + 1
    for k in arena.shapes:
        np.testing.assert_allclose(arena.p(k).cpu().numpy(), wprm[k], err_msg=k, **PARAM_TOL)


@pytest.mark.parametrize('clip', [None, 0.05], ids=['plain', 'clipped'])
def test_eager_equals_captured_bitwise_across_the_ramp(dev, clip):
    """a DrVAE with its classifier under the default schedule (two flag-ordered graphs): an eager iteration 0, then five
    replays across ramps of 3 iterations == six eager steps, bit for bit (Philox noise) -- the side chain's half of the sweep
    and its loss scalars read the record and the weights the NEXT replay's head rewrites"""
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    out = []
    for captured in (True, False):
        eng, arena = make_engine(spec, params, SCHEDULES['all'], device=dev, max_grad_norm=clip)
        set_batch(eng, batch, dev)
        eng.train_step()
        losses = [eng.losses()]
        for _ in range(N_STEPS - 1):
            if captured:
                if eng._graph_key is None:
                    eng.capture()
                    assert eng._side_graph is not None, 'the default schedule of this model is two flag-ordered graphs'
                eng.replay()
            else:
                eng.train_step()
            losses.append(eng.losses())
        if captured:
            eng.check_sync()
        torch.cuda.synchronize()
        out.append(([getattr(arena, w).clone() for w in ('param', 'exp_avg', 'exp_avg_sq')], losses, eng.schedule_record()))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert np.array(list(out[0][2].values()), np.float32).tobytes() == R.record32(N_STEPS - 1, SCHEDULES['all']).tobytes()
    # the ramp was crossed: ELBO's KL weight moved from 0.01 to 1 while the reported scalars stayed comparable
    assert out[0][1][0]['ELBO'] != out[0][1][-1]['ELBO']


def test_sampler_feed_replays_equal_eager_steps_on_the_same_rows(dev):
    """the feed's extra workgroup writes the schedule inside ONE captured (tail-gated) step, its head parked on flag ``tail``:
    six replays over two epochs of the index table == eager steps handed the same rows explicitly (the launch of its own), bit
    for bit"""
    from drvae_amd import data as D
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    big = M.make_batch(spec, 640, seed=9)
    t = lambda k: torch.from_numpy(big[k].copy())
    ds = D.DrVAEDataset(t('x1'), t('x2'), t('s'), t('y'), t('has_x2'), t('has_y')).to(dev)
    w = D.compute_balanced_weights(np.arange(640) % 7)
    bat = D.DeviceBatcher(ds, w, 64, seed=5, mode='sampler')
    fed, a1 = make_engine(spec, params, SCHEDULES['all'], device=dev)
    eager, a0 = make_engine(spec, params, SCHEDULES['all'], device=dev)
    bat.bind(fed)
    tables, recs = [], []
    for epoch in range(2):
        tables.append(bat.begin_epoch(n_batches=3).clone())
        if epoch == 0:
            fed.capture()
            assert fed._side_graph is not None
        for _ in range(3):
            fed.replay()
            recs.append(fed.schedule_record())
    fed.check_sync()
    assert fed.plan.annealed and fed.iters == 6
    for tab in tables:
        for b in range(3):
            i = tab[b].long()
            eager.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), ds.has_x2[i].cpu().numpy(), ds.has_y[i].cpu().numpy())
            eager.train_step()
    torch.cuda.synchronize()
    assert eager.losses() == fed.losses()
    for name in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(a0, name), getattr(a1, name)), name
    for it, rec in enumerate(recs):
        assert np.array(list(rec.values()), np.float32).tobytes() == R.record32(it, SCHEDULES['all']).tobytes(), it


def test_evaluation_mid_ramp_reports_unscaled_pieces_and_annealed_totals(dev):
    spec, batch, noises = case('drvae')
    sched = SCHEDULES['all']
    eng, arena = make_engine(spec, M.init_params(spec, 9, as_numpy=True), sched, device=dev)
    set_batch(eng, batch, dev)
    for noise in noises[:2]:
        eng.train_step(noise)
    torch.cuda.synchronize()
    params = {k: arena.p(k).detach().cpu().clone() for k in arena.shapes}
    plain, _ = M.loss_function(spec, params, batch, noises[2], iters=2, training=False)
    want, _ = R.loss_function(spec, sched, params, batch, noises[2], iters=2, training=False)
    for how in ('universal', 'structure'):
        if how == 'structure':
            eng.set_structure(batch['has_x2'], batch['has_y'])
            p = eng.plan
            p.XSRC[:p.B].copy_(torch.from_numpy(batch['x1']))
            p.XSRC[p.B:].copy_(torch.from_numpy(batch['x2']))
            p.set_labels_host(batch['y'].reshape(-1))
        else:
            set_batch(eng, batch, dev)
        eng.training = False
        eng.set_noise(noises[2])
        eng.forward()
        got = eng.losses()
        for k in ('RECL', 'KLD', 'PERT', 'YL'):
            np.testing.assert_allclose(got[k], float(plain[k]), err_msg=how + ' ' + k, **LOSS_TOL)
        for k in ('ELBO', 'CMPL'):
            np.testing.assert_allclose(got[k], float(want[k]), err_msg=how + ' ' + k, **LOSS_TOL)
    assert abs(float(want['CMPL']) - float(plain['CMPL'])) > 100 * (LOSS_TOL['rtol'] * abs(float(plain['CMPL'])) + LOSS_TOL['atol'])


def test_one_fit_epoch_on_the_sampler_feed_equals_stepping_by_hand(dev, tmp_path):
    from drvae_amd import data as D
    from tests.test_dropout_cpu import tiny_model
    from tests.test_fit import _loader, _tiny_dataset
    kw = dict(anneal_kl=True, anneal_kl_itermax=3, anneal_yloss=True, anneal_yloss_itermax=3, anneal_learning_rate=True,
              anneal_lr_itermax=3, epochs=1, device=dev)
    tr, va = _tiny_dataset('drvae', 64, 1, dev), _tiny_dataset('drvae', 32, 2, dev)
    w = D.compute_balanced_weights(np.arange(64) % 5)
    fitted = tiny_model('drvae', **kw)
    fitted.w2log = lambda *a: None
    fitted.fit(D.DeviceBatcher(tr, w, 16, seed=3, mode='sampler'), _loader(va, 8), add_noise=True, verbose=False,
               early_stop=False, model_filename=str(tmp_path / 'b.pth'))
    assert fitted.finished_training_iters == 4 and fitted.engine().plan.annealed
    hand = tiny_model('drvae', **kw)
    eng = hand.engine()
    bat = D.DeviceBatcher(tr, w, 16, seed=3, mode='sampler')
    bat.bind(eng)
    eng.add_noise = True
    bat.begin_epoch()
    for _ in range(len(bat)):
        eng.train_step()
    torch.cuda.synchronize()
    eng.check_sync()
    for name in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(eng.arena, name), getattr(fitted.engine().arena, name)), name
    assert eng.schedule_record() == fitted.engine().schedule_record()
    assert eng.schedule_record()['beta_kl'] == 1.0 and eng.schedule_record()['lr_scale'] == float(np.float32(0.01))
    perf, _ = fitted.evaluate_performance_on_dataset(va)
    assert all(np.isfinite(float(v)) for v in perf['losses'].values())


# ------------------------------------------------------------------------------------------------ 4. schedules off
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_schedules_off_step_launches_what_it_always_did(dev, kind, monkeypatch):
    """the captured step at the benchmark's batch shape, default and one-graph schedule, structure and universal plan: built
    without the arguments or with every switch off, the launch list is the same and so is every bit of three steps; switched
    on, the universal step has the SAME launches (the schedule rides on them)"""
    from tests.test_dropout_cpu import make_engine as plain_engine
    from tests.test_gpu_dropout import _captured_launch_names
    from tests.test_gpu_x3 import tuned
    spec = M.ModelSpec(kind=kind, L=1 if kind == 'pvae' else 2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    off = R.settings(anneal_kl_itermax=3, anneal_yloss_itermax=3, anneal_yloss_offset=2, anneal_lr_itermax=3)
    lists, state = {}, {}
    combos = {'': [(False, 'absent'), (False, 'off'), (True, 'absent'), (True, 'off'), (True, 'on')],
              'sched=3': [(True, 'off'), (True, 'on')]}
    for tune in ('', 'sched=3'):
        with tuned(tune):
            for universal, tag in combos[tune]:
                if True:
                    if tag == 'absent':
                        eng, arena = plain_engine(spec, params, device=dev)
                    else:
                        eng, arena = make_engine(spec, params, off if tag == 'off' else SCHEDULES['all'], device=dev)
                    eng.universal = universal
                    set_batch(eng, batch, dev)
                    eng.train_step()
                    lists[(tune, universal, tag)] = _captured_launch_names(eng, monkeypatch)
                    eng.replay()
                    eng.replay()
                    torch.cuda.synchronize()
                    eng.check_sync()
                    state[(tune, universal, tag)] = ([getattr(arena, w).clone() for w in ('param', 'exp_avg', 'exp_avg_sq', 'loss')],
                                                     list(eng._plans), (eng.sched_rec is None))
    for universal in (False, True):
        a, b = ('', universal, 'absent'), ('', universal, 'off')
        assert lists[a] and lists[a] == lists[b]
        assert all(torch.equal(x, y) for x, y in zip(state[a][0], state[b][0]))
        assert state[a][1] == state[b][1] and state[a][2] and state[b][2]
    for tune in ('', 'sched=3'):
        assert lists[(tune, True, 'on')] == lists[(tune, True, 'off')]
        assert not state[(tune, True, 'on')][2] and state[(tune, True, 'off')][2]
