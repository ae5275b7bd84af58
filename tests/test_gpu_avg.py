"""-m gpu: the parameter average and decoupled weight decay riding on the optimiser sweeps (``dv_adam_hyper.avg`` /
``.decoupled``), below model level on every launch path -- the float4 and the scalar loop of ``adam_kernel``, its capped
grid, ``adam_stream_kernel``, ``adamax_kernel`` past its grid cap, the gated and the clipped forms -- against
tests/avg_ref.py, the memory contract with the average as the fifth array, path equality, the switches-off launch bit for
bit; then the step: eager == captured with parameters AND average (plain dual-graph, clipped, sampler feed), the arena
holding the averaged values and a whole-set evaluation under ``averaged_parameters()`` between replays, two ranks on one
GPU and the captured exchange in fresh child processes, ``fit`` epochs.  tests/test_avg_cpu.py proves the bounds against
faulty emulations.
With ``-s`` the module prints the worst excess per path."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import avg_ref as AR
from tests import optim_ref as R
from tests.test_anneal_cpu import make_engine, set_batch
from tests.test_gpu_optim import big_inputs, bits, guards_hold, parked_elements, place, sample_indices

pytestmark = pytest.mark.gpu

MI = 1 << 20
KINDS = ('adam', 'adamw', 'adamax')
D = 0.9
TS = (1, 1000)
PATHS = {'adam': 2 * MI + 5, 'adamw': 2 * MI + 5, 'adamax': 3 * MI + 5}       # past each kernel's grid cap
STREAM = 16 * MI + 5                                                          # adam_stream_kernel


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


@pytest.fixture(scope='module', autouse=True)
def table():
    worst = {}
    yield worst
    print('\nsweeps with the two options on the device: worst |got - float64| / bound per path')
    for key in sorted(worst):
        print('  %-44s %s' % (' '.join(str(k) for k in key), '   '.join('%s %.3g' % qv for qv in sorted(worst[key].items()))))


def note(table, key, vals):
    row = table.setdefault(key, {})
    for q, v in vals.items():
        row[q] = max(row.get(q, 0.0), v)


def clip_state(K, dev, n, t, coef=1.0, skip=0, n_skipped=0):
    st = K.clip_state(dev, n, 1.0)
    st[0] = t
    rec = K.clip_record(st)
    rec.view(torch.float32)[1] = float(np.float32(coef))
    rec[2], rec[3] = skip, n_skipped
    return st


def sweep(K, kind, views, t, h, dev, avg=None, d=None, clip=None, lr_scale=None, mention=True, **kw):
    """one launch: ``views`` = (p, g, m, v); ``clip`` = a clip state (the clipped entry points); ``mention`` False: the call
    never names the new keywords"""
    hk = dict(lr=h['lr'], beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'], weight_decay=h['weight_decay'], gscale=h['gscale'])
    if lr_scale is not None:
        hk['lr_scale'] = torch.tensor([lr_scale], dtype=torch.float32, device=dev)
    if mention:
        hk.update(decoupled=kind == 'adamw', avg=avg, avg_decay=d if avg is not None else None)
    else:
        assert kind != 'adamw' and avg is None
    if clip is not None:
        fn, second = (K.adamax_l2_clip if kind == 'adamax' else K.adam_l2_clip), clip
    else:
        fn, second = (K.adamax_l2 if kind == 'adamax' else K.adam_l2), torch.tensor([t], dtype=torch.int32, device=dev)
    fn(*views, second, **hk, **kw)


def host(kind, views):
    torch.cuda.synchronize()
    p, _, m, v = views
    return {'p': p.cpu().numpy(), 'm': m.cpu().numpy(), AR.stored(kind)[2]: v.cpu().numpy()}


def class_inputs(kind, cls):
    return dict(R.cases('adamax' if kind == 'adamax' else 'adam'))[cls]


# ------------------------------------------------------------------------------------------------ 1. the bound, every path
ALL = [(k, c) for k in KINDS for c, _ in R.cases('adamax' if k == 'adamax' else 'adam')]


@pytest.mark.parametrize('with_avg', [False, True], ids=['no_avg', 'avg'])
@pytest.mark.parametrize('kind,cls', ALL, ids=['%s-%s' % kc for kc in ALL])
def test_within_the_bound_on_both_loops(K, dev, table, kind, cls, with_avg):
    arrays = class_inputs(kind, cls)
    e0 = AR.avg_start(cls if cls in R.CLASSES else 'normal')
    for t, gs, wd in R.settings(cls):
        if t not in TS:
            continue
        h = R.hyper32(weight_decay=wd, gscale=gs)
        for lead in (0, 1):
            site = '%s %s t=%d gscale=%g wd=%g lead=%d avg=%d' % (kind, cls, t, gs, wd, lead, with_avg)
            placed = [place(a, dev, lead) for a in arrays + ((e0,) if with_avg else ())]
            views = [v for _, v in placed]
            sweep(K, kind, views[:4], t, h, dev, avg=views[4] if with_avg else None, d=D)
            got = host(kind, views[:4])
            failed, worst = AR.verify(kind, got, arrays, t, h, site=site)
            if with_avg:
                bad, worst['e'] = AR.verify_avg(views[4].cpu().numpy(), e0, got['p'], D)
                assert not bad, (site, worst)
            print(site, 'excess', worst)
            note(table, (kind, 'n=%d' % R.N_CASE, 'lead=%d' % lead, 'avg=%d' % with_avg), worst)
            assert failed == set(), (site, worst)
            assert all(guards_hold(b, lead, arrays[0].size) for b, _ in placed), site
            if cls == 'pads':
                for q in [got['p'], got['m']] + ([views[4].cpu().numpy()] if with_avg else []):
                    assert not R.bits(q).any(), (site, 'a pad must stay bit-zero')


def _big_e(p):
    """an old average every element of which moves in an update: at least 3 away from the parameter (a tenth of that per
    sweep, against an ulp of 1e-6)"""
    return p + 3.0 + (torch.arange(p.numel(), device=p.device) % 5).float()


def run_big(K, dev, kind, inputs, lead, t, h, with_avg, **kw):
    """one sweep over copies of ``inputs`` (+ an average) placed at ``lead``; the memory contract is checked on the device.
    Returns (views after the sweep, old average)"""
    n = inputs[0].numel()
    e0 = _big_e(inputs[0])
    placed = [place(a, dev, lead) for a in tuple(inputs) + ((e0,) if with_avg else ())]
    views = [v for _, v in placed]
    sweep(K, kind, views[:4], t, h, dev, avg=views[4] if with_avg else None, d=D, **kw)
    torch.cuda.synchronize()
    assert all(guards_hold(b, lead, n) for b, _ in placed), 'written outside a view'
    assert torch.equal(bits(views[1]), bits(inputs[1])), 'g was written'
    olds = (inputs[0], inputs[2], inputs[3]) + ((e0,) if with_avg else ())
    for q, a, b in zip('pmve', (views[0], views[2], views[3]) + tuple(views[4:]), olds):
        assert bool((bits(a) != bits(b)).all()), '%s: an element was not written' % q
    return views, e0


def hold_sample(kind, views, inputs, e0, t, h, site):
    idx = torch.from_numpy(sample_indices(inputs[0].numel())).to(inputs[0].device)
    got = {'p': views[0][idx].cpu().numpy(), 'm': views[2][idx].cpu().numpy(), AR.stored(kind)[2]: views[3][idx].cpu().numpy()}
    failed, worst = AR.verify(kind, got, [a[idx].cpu().numpy() for a in inputs], t, h, site=site)
    assert failed == set(), (site, worst)
    if len(views) > 4:
        bad, worst['e'] = AR.verify_avg(views[4][idx].cpu().numpy(), e0[idx].cpu().numpy(), got['p'], D)
        assert not bad, (site, worst)
    return worst


def adamax_inputs(n, dev):
    p, g, m, _ = big_inputs(n, dev)
    return p, g, m, 0.7 * g.abs().roll(1) + 1e-3        # a running max that decides on about half the elements


@pytest.mark.parametrize('with_avg', [False, True], ids=['no_avg', 'avg'])
@pytest.mark.parametrize('kind', KINDS)
def test_capped_grid_within_the_bound_and_both_loops_give_the_same_bits(K, dev, table, kind, with_avg):
    """past the grid cap of adam_kernel (2048 workgroups) / adamax_kernel (4096): a sample within the bound, and the float4
    and the scalar loop (views shifted by one element) agree bit for bit in every array -- path equality of the new forms"""
    n, t, h = PATHS[kind], 7, R.hyper32(weight_decay=0.05, gscale=0.125)
    inputs = adamax_inputs(n, dev) if kind == 'adamax' else big_inputs(n, dev)
    fast, e0 = run_big(K, dev, kind, inputs, 0, t, h, with_avg)
    note(table, (kind, 'n=%d' % n, 'capped grid', 'avg=%d' % with_avg), hold_sample(kind, fast, inputs, e0, t, h, 'n=%d' % n))
    fast = [a.clone() for a in fast]
    scalar, _ = run_big(K, dev, kind, inputs, 1, t, h, with_avg)
    for q, a, b in zip('pgmve', fast, scalar):
        same = bits(a) == bits(b)
        assert bool(same.all()), ('%s n=%d: %s differs between the loops on %d elements' % (kind, n, q, int((~same).sum())))


@pytest.mark.parametrize('kind,with_avg', [('adam', True), ('adamw', False), ('adamw', True)])
def test_streaming_kernel_within_the_bound_and_equal_to_the_scalar_loop(K, dev, table, kind, with_avg):
    n, t, h = STREAM, 7, R.hyper32(weight_decay=0.05, gscale=0.125)
    inputs = big_inputs(n, dev)
    fast, e0 = run_big(K, dev, kind, inputs, 0, t, h, with_avg)
    note(table, (kind, 'n=%d' % n, 'streaming', 'avg=%d' % with_avg), hold_sample(kind, fast, inputs, e0, t, h, 'n=%d' % n))
    fast = [a.clone() for a in fast]
    scalar, _ = run_big(K, dev, kind, inputs, 1, t, h, with_avg)
    for q, a, b in zip('pgmve', fast, scalar):
        assert torch.equal(bits(a), bits(b)), (kind, q)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('lead', [0, 1])
def test_clipped_forms(K, dev, table, kind, lead):
    """a coefficient < 1 with skipped steps behind it and an annealed rate: within the bound at the effective rate, scale and
    step count; coef == 1.0f: the bits of the plain sweep, average included"""
    n = R.N_CASE
    arrays = class_inputs(kind, 'warm')
    e0 = AR.avg_start('warm')
    h = R.hyper32(weight_decay=0.05, gscale=0.125)
    t, skipped = 9, 2
    views = [place(a, dev, lead)[1] for a in arrays + (e0,)]
    st = clip_state(K, dev, n, t, coef=AR.CLIP_COEF, n_skipped=skipped)
    sweep(K, kind, views[:4], t, h, dev, avg=views[4], d=D, clip=st, lr_scale=AR.LR_SCALE)
    got = host(kind, views[:4])
    he = AR.effective(h, AR.LR_SCALE, AR.CLIP_COEF)
    failed, worst = AR.verify(kind, got, arrays, t - skipped, he)
    bad, worst['e'] = AR.verify_avg(views[4].cpu().numpy(), e0, got['p'], D)
    note(table, (kind, 'n=%d' % n, 'clipped lead=%d' % lead, 'avg=1'), worst)
    assert failed == set() and not bad, worst
    if kind == 'adamw':       # the decay is untouched by the clip coefficient and uses the annealed rate: the faults are seen
        for fault in ('decay_scaled_by_clip', 'decay_with_unannealed_lr'):
            wrong = AR.emulate_adamw(*arrays, t - skipped, h, True, fault=fault, lr_scale=AR.LR_SCALE, coef=AR.CLIP_COEF)
            assert float(np.abs(got['p'].astype(np.float64) - wrong['p']).max()) > 0
    plain = [place(a, dev, lead)[1] for a in arrays + (e0,)]
    one = [place(a, dev, lead)[1] for a in arrays + (e0,)]
    sweep(K, kind, plain[:4], t, h, dev, avg=plain[4], d=D)
    sweep(K, kind, one[:4], t, h, dev, avg=one[4], d=D, clip=clip_state(K, dev, n, t, coef=1.0))
    torch.cuda.synchronize()
    for q, a, b in zip('pgmve', plain, one):
        assert torch.equal(bits(a), bits(b)), (kind, q)


def test_a_gated_sweep_updates_the_average_like_the_plain_one(K, dev):
    """a slice inside one workgroup's span, the flag published before the launch: the gated kernel's bits == the plain one's"""
    n, lo, hi = R.N_CASE, 1100, 1500
    h = R.hyper32(weight_decay=0.05)
    arrays = class_inputs('adam', 'warm')
    e0 = AR.avg_start('warm')
    for kind in ('adam', 'adamw'):
        for lead in (0, 1):
            want = [place(a, dev, lead)[1] for a in arrays + (e0,)]
            sweep(K, kind, want[:4], 1, h, dev, avg=want[4], d=D)
            views = [place(a, dev, lead)[1] for a in arrays + (e0,)]
            step = torch.ones(1, dtype=torch.int32, device=dev)
            flag = torch.ones(1, dtype=torch.int32, device=dev)
            err = torch.zeros(2, dtype=torch.int32, device=dev)
            K.adam_l2(*views[:4], step, lr=h['lr'], weight_decay=h['weight_decay'], gate=(flag, step, 0, err, lo, hi),
                      decoupled=kind == 'adamw', avg=views[4], avg_decay=D)
            torch.cuda.synchronize()
            assert int(err[0]) == 0
            for q, a, b in zip('pgmve', views, want):
                assert torch.equal(bits(a), bits(b)), (kind, lead, q)


# ------------------------------------------------------------------------------------------------ 2. the memory contract
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 1023, 1025])
def test_memory_contract_with_five_arrays(K, dev, kind, n):
    t, h = 1, R.hyper32(weight_decay=0.05)
    inputs = R.frame_inputs(n)
    e0 = (inputs[0] * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    for lead in (0, 1):
        placed = [place(a, dev, lead) for a in inputs + (e0,)]
        before = {k: b.cpu().numpy().copy() for k, (b, _) in zip('pgmve', placed)}
        views = [v for _, v in placed]
        sweep(K, kind, views[:4], t, h, dev, avg=views[4], d=D)
        torch.cuda.synchronize()
        after = {k: b.cpu().numpy() for k, (b, _) in zip('pgmve', placed)}
        sl = slice(lead + R.GUARD, lead + R.GUARD + n)
        assert R.memory_faults(before, after, sl) == set(), (kind, n, lead)
        bad, w = AR.verify_avg(after['e'][sl], e0, after['p'][sl], D)
        assert not bad, (kind, n, lead, w)
    # the average shifted against the other four: it joins the alignment test (all five decide the loop), same bits
    for lead_e in (0, 1):
        views = [place(a, dev, 0)[1] for a in inputs] + [place(e0, dev, lead_e)[1]]
        sweep(K, kind, views[:4], t, h, dev, avg=views[4], d=D)
        torch.cuda.synchronize()
        if lead_e == 0:
            want = [v.clone() for v in views]
        else:
            for q, a, b in zip('pgmve', views, want):
                assert torch.equal(bits(a), bits(b)), (kind, n, q)


@pytest.mark.parametrize('kind', KINDS)
def test_a_sweep_that_returns_early_touches_nothing_of_the_average(K, dev, kind):
    """a halt word set, a clipped step skipped: all five arrays keep their bits, frame included"""
    n, h = R.N_CASE, R.hyper32(weight_decay=0.05)
    inputs = R.frame_inputs(n)
    e0 = (inputs[0] * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    for lead in (0, 1):
        for how in ('halt', 'skip'):
            placed = [place(a, dev, lead) for a in inputs + (e0,)]
            before = [b.clone() for b, _ in placed]
            views = [v for _, v in placed]
            if how == 'halt':
                err = torch.tensor([1, 0], dtype=torch.int32, device=dev)
                sweep(K, kind, views[:4], 1, h, dev, avg=views[4], d=D, halt=err)
            else:
                sweep(K, kind, views[:4], 1, h, dev, avg=views[4], d=D, clip=clip_state(K, dev, n, 1, coef=0.0, skip=1, n_skipped=1))
            torch.cuda.synchronize()
            for q, (b, _), old in zip('pgmve', placed, before):
                assert torch.equal(bits(b), bits(old)), (kind, lead, how, q)


@pytest.mark.parametrize('n,lead,lo,hi', [(100003, 0, 5000, 5402), (100003, 1, 5000, 5402)])
def test_a_timed_out_gate_leaves_the_parked_workgroups_average_alone(K, dev, n, lead, lo, hi):
    """max_spins = 50 and a flag nobody publishes (tests/test_gpu_optim.py::test_a_gate_that_times_out, with the average): the
    elements of the parked workgroups keep p, m, v AND e, every other element moves in all four"""
    from drvae_amd import _lib
    h = R.hyper32(weight_decay=0.05)
    inputs = big_inputs(n, dev, seed=2)
    e0 = _big_e(inputs[0])
    views = [place(a, dev, lead)[1] for a in tuple(inputs) + (e0,)]
    step = torch.ones(1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)
    w = _lib.Wait()
    w.flag, w.ctr, w.err, w.add, w.max_spins = K._i32(flag), K._i32(step), K._i32(err), 0, 50
    hy = K._hyper(h['lr'], h['beta1'], h['beta2'], h['eps'], h['weight_decay'], h['gscale'], None, views[0], True, views[4], D)
    hp, hn = K._halt(err)
    p, g, m, v = views[:4]
    _lib.check(_lib.load().dv_adam_l2_gated(K._f32(p), K._f32(g), K._f32(m), K._f32(v), n, C.byref(hy), K._i32(step),
                                            C.byref(w), lo, hi, hp, hn, K._stream()), 'dv_adam_l2_gated')
    torch.cuda.synchronize()
    assert int(err[0]) == 1
    kept = [bits(a) == bits(b) for a, b in zip((views[0], views[2], views[3], views[4]), (inputs[0], inputs[2], inputs[3], e0))]
    assert bool(kept[3][lo:hi].all()), 'the average of the gated slice was touched'
    for k in kept[1:]:
        assert torch.equal(kept[0], k), 'an element was updated in part'
    assert np.array_equal(kept[0].cpu().numpy(), parked_elements(n, lead == 0, lo, hi))
    assert 0 < int(kept[0].sum()) < n


# ------------------------------------------------------------------------------------------------ 4. both options off
@pytest.mark.parametrize('kind,n,lead', [('adam', R.N_CASE, 0), ('adam', R.N_CASE, 1), ('adam', STREAM, 0),
                                         ('adamax', R.N_CASE, 0), ('adamax', 3 * MI + 5, 1)])
def test_switches_off_gives_the_bits_of_a_call_that_never_mentions_them(K, dev, kind, n, lead):
    t, h = 3, R.hyper32(weight_decay=0.05, gscale=0.125)
    inputs = adamax_inputs(n, dev) if kind == 'adamax' else big_inputs(n, dev)
    out = []
    for mention in (False, True):
        for clip in (False, True):
            views = [place(a, dev, lead)[1] for a in inputs]
            sweep(K, kind, views, t, h, dev, mention=mention,
                  clip=clip_state(K, dev, n, t, coef=AR.CLIP_COEF) if clip else None)
            torch.cuda.synchronize()
            out.append((clip, views))
    for clip in (False, True):
        a, b = [v for c, v in out if c == clip]
        for q, x, y in zip('pgmv', a, b):
            assert torch.equal(bits(x), bits(y)), (kind, n, lead, clip, q)


# ------------------------------------------------------------------------------------------------ 5. the step
KW = dict(ema_decay=D, optim_alg='adamw')
STATE = ('param', 'exp_avg', 'exp_avg_sq', 'avg')


def _cfg2(dev, steps, captured, evaluate_at=None, **kw):
    """the default DrVAE configuration at 150 rows (two flag-ordered graphs): an eager step, then ``steps`` - 1 more, replayed
    or eager; ``evaluate_at``: the arena holds the averaged parameters for a while before that step (``swap_average``, what
    ``averaged_parameters()`` does; the evaluation itself between replays: ``test_fit_epochs_on_the_device_batcher``)"""
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    eng, arena = make_engine(spec, params, None, device=dev, **kw)
    set_batch(eng, batch, dev)
    eng.train_step()
    seen = None
    for i in range(1, steps):
        if i == evaluate_at:
            torch.cuda.synchronize()
            live, avg = arena.param.clone(), arena.avg.clone()
            eng.swap_average()               # (the gradient arena is the scratch: the next backward pass must not care)
            with pytest.raises(RuntimeError):
                eng.replay() if captured else eng.train_step()
            torch.cuda.synchronize()
            assert torch.equal(arena.param, avg) and torch.equal(arena.avg, live)
            seen = float(arena.param.double().sum())
            eng.swap_average()
            torch.cuda.synchronize()
            assert torch.equal(arena.param, live) and torch.equal(arena.avg, avg)
        if captured:
            if eng._graph_key is None:
                eng.capture()
            eng.replay()
        else:
            eng.train_step()
    if captured:
        eng.check_sync()
    torch.cuda.synchronize()
    return eng, arena, seen


@pytest.mark.parametrize('clip', [None, 0.05], ids=['plain', 'clipped'])
def test_eager_equals_captured_bitwise_parameters_and_average(dev, clip):
    """plain: the dual-graph schedule, the side chain sweeps the decoder heads' half of the parameters and of the average"""
    out = []
    for captured in (True, False):
        eng, arena, _ = _cfg2(dev, 5, captured, max_grad_norm=clip, **KW)
        tail = eng._step_tail(False, on_gpu=True)
        if captured and clip is None:
            assert eng._side_graph is not None and tail.side_adam and tail.adam_gated, 'adamw takes the schedule adam takes'
        out.append([getattr(arena, w).clone() for w in STATE] + [eng.losses()])
    for a, b in zip(out[0][:-1], out[1][:-1]):
        assert torch.equal(a, b)
    assert out[0][-1] == out[1][-1]
    avg, prm = out[0][3], out[0][0]
    n = arena.n_live
    assert bool((avg[:n] != prm[:n]).any()) and torch.equal(avg[n:], prm[n:])
    # the side chain's half moved too
    hs = tail.hs if (clip is None and tail.side_adam) else 0
    assert bool((avg[hs:n] != prm[hs:n]).any())


def test_the_average_of_the_step_follows_its_recurrence(dev):
    """eager steps: after each, e == fma(w, p_new - e_old, e_old) within the bound of tests/avg_ref.py, at the device's own
    parameters"""
    spec = M.ModelSpec(kind='drvae', L=2)
    eng, arena = make_engine(spec, M.init_params(spec, 3, as_numpy=True), None, device=dev, **KW)
    set_batch(eng, M.make_batch(spec, 150, seed=5), dev)
    assert torch.equal(arena.avg, arena.param)
    for _ in range(3):
        e_old = arena.avg.cpu().numpy().copy()
        eng.train_step()
        torch.cuda.synchronize()
        bad, w = AR.verify_avg(arena.avg.cpu().numpy(), e_old, arena.param.cpu().numpy(), D)
        assert not bad, w


def test_sampler_feed_replays_equal_eager_steps_with_the_average(dev):
    from drvae_amd import data as DD
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    big = M.make_batch(spec, 640, seed=9)
    t = lambda k: torch.from_numpy(big[k].copy())
    ds = DD.DrVAEDataset(t('x1'), t('x2'), t('s'), t('y'), t('has_x2'), t('has_y')).to(dev)
    w = DD.compute_balanced_weights(np.arange(640) % 7)
    bat = DD.DeviceBatcher(ds, w, 64, seed=5, mode='sampler')
    fed, a1 = make_engine(spec, params, None, device=dev, **KW)
    eager, a0 = make_engine(spec, params, None, device=dev, **KW)
    eager.universal = True          # (the batch-independent plan the sampler feed runs on: the same sums in the same order)
    bat.bind(fed)
    tab = bat.begin_epoch(n_batches=3).clone()
    fed.capture()
    for _ in range(3):
        fed.replay()
    fed.check_sync()
    for b in range(3):
        i = tab[b].long()
        eager.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), ds.has_x2[i].cpu().numpy(), ds.has_y[i].cpu().numpy())
        eager.train_step()
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(a0, name), getattr(a1, name)), name


# ------------------------------------------------------------------------------------------------ 6. evaluation in between
def test_evaluation_under_the_average_between_replays_leaves_the_trajectory_alone(dev):
    want, wa, _ = _cfg2(dev, 6, True, **KW)
    got, ga, seen = _cfg2(dev, 6, True, evaluate_at=3, **KW)
    assert seen is not None and np.isfinite(seen)
    for name in ('param', 'exp_avg', 'exp_avg_sq', 'avg', 'loss'):
        assert torch.equal(getattr(ga, name), getattr(wa, name)), name
    assert not got.averaged


def test_evaluation_inside_the_context_between_replays(dev):
    """captured training on the sampler feed, ``evaluate_performance_on_dataset`` under ``averaged_parameters()`` in the middle,
    further replays.  The whole-set evaluation draws its noise from the engine's Philox counter, so the trajectory is compared
    with one that runs the SAME evaluation on the live weights at the same place: parameters, moments and average bit for
    bit, and the two evaluations report different losses.  Around the evaluation the model's parameters are
    ``averaged_state_dict()``'s values, bit for bit, and the live ones afterwards (the exact equality of an evaluation inside
    the context with one of a model loaded from ``averaged_state_dict()``: tests/test_avg_cpu.py)"""
    from drvae_amd import data as DD
    from tests.test_dropout_cpu import tiny_model
    from tests.test_fit import _tiny_dataset
    tr, va = _tiny_dataset('drvae', 64, 1, dev), _tiny_dataset('drvae', 32, 2, dev)
    w = DD.compute_balanced_weights(np.arange(64) % 5)
    out = {}
    for how in ('averaged', 'live'):
        model = tiny_model('drvae', device=dev, **KW)
        eng = model.engine()
        bat = DD.DeviceBatcher(tr, w, 16, seed=3, mode='sampler')
        bat.bind(eng)
        eng.add_noise = True
        bat.begin_epoch(n_batches=8)
        eng.train_step()
        eng.capture()
        for _ in range(3):
            eng.replay()
        model.finished_training_iters = eng.iters
        if how == 'averaged':
            sd = model.averaged_state_dict()
            live = {k: v.detach().clone() for k, v in model.state_dict().items()}
            with model.averaged_parameters():
                with pytest.raises(RuntimeError):
                    eng.replay()
                # what the evaluation reads: the model's parameters ARE the averaged values now
                assert all(torch.equal(v.cpu(), sd[k]) for k, v in model.state_dict().items())
                perf, _ = model.evaluate_performance_on_dataset(va)
                assert all(torch.equal(v.cpu(), sd[k]) for k, v in model.state_dict().items())
            assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())      # live bits back
        else:
            perf, _ = model.evaluate_performance_on_dataset(va)
        for _ in range(4):
            eng.replay()
        eng.check_sync()
        torch.cuda.synchronize()
        out[how] = ([getattr(eng.arena, name).clone() for name in STATE], {k: float(v) for k, v in perf['losses'].items()})
    for name, a, b in zip(STATE, out['averaged'][0], out['live'][0]):
        assert torch.equal(a, b), name
    assert out['averaged'][1] != out['live'][1]


# ------------------------------------------------------------------------------------------------ 7. data parallelism
def _dp_worker(rank, world, port, q):
    """two ranks share the one GPU and exchange through gloo (RCCL refuses two ranks on one device): the broadcast of
    ``enable_data_parallel``, then the split-graph step on 150 rows per rank against one process on the 300 rows"""
    try:
        import os
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
        import torch.distributed as dist
        from drvae_amd import dist as DD
        from tests.test_dropout_cpu import tiny_model
        DD.init_from_env(backend='gloo')
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(0)
        # the broadcast: ranks built from different seeds hold rank 0's parameters AND average afterwards
        model = tiny_model('drvae', device=dev, random_seed=5 + rank, **KW)
        arena = model.engine().arena
        arena.avg.mul_(1.0 + rank)                # (an average of its own on every rank)
        model.enable_data_parallel(rank=rank, world=world)
        sent = True
        for t in (arena.param, arena.avg):
            ref = t.clone()
            dist.broadcast(ref, src=0)
            sent = sent and torch.equal(ref, t)
        sent = sent and torch.equal(arena.avg, arena.param)
        # the step
        spec = M.ModelSpec(kind='drvae', L=2)
        params = M.init_params(spec, 3, as_numpy=True)
        full = M.make_batch(spec, 300, seed=6)
        lo, hi = DD.shard_rows(300, rank, world)
        shard = {k: v[lo:hi] for k, v in full.items()}
        counts = DD.global_counts(shard['has_x2'], shard['has_y'])
        eng, a2 = make_engine(spec, params, None, device=dev, **KW)
        eng.seed, eng.row0 = 4242, lo
        set_batch(eng, shard, dev, counts=counts)
        eng.train_step(allreduce=DD.allreduce_sum)
        eng.capture(split_for_allreduce=True)
        for _ in range(3):
            eng.replay(DD.allreduce_sum)
        torch.cuda.synchronize()
        eng.check_sync()
        one, a1 = make_engine(spec, params, None, device=dev, **KW)
        one.seed = 4242
        set_batch(one, full, dev)
        for _ in range(4):
            one.train_step()
        torch.cuda.synchronize()
        # (norm-wise, the bound of tests/test_gpu_dp.py: the shards' sums are added in another order)
        perr = float((a2.param - a1.param).norm() / a1.param.norm())
        eerr = float((a2.avg - a1.avg).norm() / a1.avg.norm())
        moved = float((a2.avg - a2.param).norm() / a2.param.norm())
        same = True
        for t in (a2.param, a2.avg):             # replicas: bit-identical, the average too
            ref = t.clone()
            dist.broadcast(ref, src=0)
            same = same and torch.equal(ref, t)
        q.put((rank, bool(sent), bool(same), perr, eerr, moved))
        dist.destroy_process_group()
    except Exception as e:       # surface the failure instead of a hung join
        import traceback
        q.put((rank, 'error', traceback.format_exc(), str(e)))


def test_two_ranks_on_one_gpu_equal_one_rank_with_bit_identical_averages(dev):
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29300 + os.getpid() % 200
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for o in out:
        assert o[1] != 'error', o[2]
        rank, sent, same, perr, eerr, moved = o
        print('rank %d: parameters %.3g, average %.3g off the one-rank run (norm-wise); average %.3g off the parameters'
              % (rank, perr, eerr, moved))
        assert sent, 'the broadcast of enable_data_parallel did not carry the average'
        assert same, 'replicas differ'
        assert perr < 1e-4 and eerr < 1e-4 and moved > 10 * eerr, o


def _captured_exchange_worker(port, q):
    """a one-rank RCCL communicator: the exchange captured INTO the step's graph (``Tail.cap_fork``: the sweep's first workgroup
    parks on the side chain's tail), with the average's slice on that branch"""
    try:
        import os
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), DRVAE_FORCE_DP='1')
        os.environ.pop('RANK', None)
        os.environ.pop('WORLD_SIZE', None)
        import torch.distributed as dist
        from drvae_amd import dist as DD
        DD.init_from_env(backend='nccl')
        dev = torch.device('cuda', 0)
        spec = M.ModelSpec(kind='drvae', L=2)
        params = M.init_params(spec, 3, as_numpy=True)
        batch = M.make_batch(spec, 150, seed=5)
        res = []
        for captured in (True, False):
            eng, arena = make_engine(spec, params, None, device=dev, **KW)
            set_batch(eng, batch, dev)
            eng.train_step(allreduce=DD.allreduce_sum)
            fork = None
            if captured:
                eng.capture(split_for_allreduce='captured', allreduce=DD.allreduce_sum)
                fork = bool(eng._step_tail('captured', on_gpu=True).cap_fork)
                for _ in range(3):
                    eng.replay()
                eng.check_sync()
            else:
                for _ in range(3):
                    eng.train_step(allreduce=DD.allreduce_sum)
            torch.cuda.synchronize()
            res.append(([getattr(arena, w).clone() for w in STATE], fork))
        equal = [bool(torch.equal(a, b)) for a, b in zip(res[0][0], res[1][0])]
        n = arena.n_live
        moved = bool((res[0][0][3][:n] != res[0][0][0][:n]).any())
        q.put(('ok', equal, res[0][1], moved))
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        q.put(('error', traceback.format_exc(), str(e)))


def test_the_captured_exchange_sweeps_the_average(dev):
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_captured_exchange_worker, args=(29520 + os.getpid() % 40, q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert out[0] == 'ok', out[1]
    _, equal, fork, moved = out
    assert fork, 'this configuration records the captured exchange with a fork (Tail.cap_fork)'
    assert all(equal), dict(zip(STATE, equal))
    assert moved


# ------------------------------------------------------------------------------------------------ 8. fit
def test_fit_epochs_on_the_device_batcher(dev, tmp_path):
    """two epochs of ``fit`` on captured replays.  One epoch == stepping by hand, bit for bit (parameters, moments, average).
    Two epochs with the evaluations and the snapshot under ``averaged_parameters()`` between them == two epochs that evaluate
    and snapshot the live weights (``ema_eval = False``; both draw the same evaluation noise): holding the averaged values in
    the arena between replays leaves the trajectory alone"""
    from drvae_amd import data as DD
    from tests.test_dropout_cpu import tiny_model
    from tests.test_fit import _loader, _tiny_dataset
    kw = dict(ema_decay=D, optim_alg='adamw', device=dev)
    tr, va = _tiny_dataset('drvae', 64, 1, dev), _tiny_dataset('drvae', 32, 2, dev)
    w = DD.compute_balanced_weights(np.arange(64) % 5)

    def fit(epochs, ema_eval, tag):
        model = tiny_model('drvae', epochs=epochs, **kw)
        model.w2log = lambda *a: None
        model.ema_eval = ema_eval
        model.fit(DD.DeviceBatcher(tr, w, 16, seed=3, mode='sampler'), _loader(va, 8), add_noise=True, verbose=False,
                  early_stop=False, model_filename=str(tmp_path / (tag + '.pth')))
        torch.cuda.synchronize()
        assert model.finished_training_iters == 4 * epochs and not model.engine().averaged
        return model

    one = fit(1, True, 'one')
    hand = tiny_model('drvae', epochs=1, **kw)
    eng = hand.engine()
    bat = DD.DeviceBatcher(tr, w, 16, seed=3, mode='sampler')
    bat.bind(eng)
    eng.add_noise = True
    bat.begin_epoch()
    for _ in range(len(bat)):
        eng.train_step()
    torch.cuda.synchronize()
    eng.check_sync()
    for name in STATE:
        assert torch.equal(getattr(eng.arena, name), getattr(one.engine().arena, name)), name
    averaged, live = fit(2, True, 'avg'), fit(2, False, 'live')
    for name in STATE:
        assert torch.equal(getattr(averaged.engine().arena, name), getattr(live.engine().arena, name)), name
    a = averaged.engine().arena
    assert not torch.equal(a.avg[:a.n_live], a.param[:a.n_live])
    with averaged.averaged_parameters():
        perf, _ = averaged.evaluate_performance_on_dataset(va)
    assert all(np.isfinite(float(v)) for v in perf['losses'].values())
    other, _ = averaged.evaluate_performance_on_dataset(va)
    assert other['losses'] != perf['losses']
