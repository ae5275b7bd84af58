"""-m gpu: gradient-norm clipping and the non-finite guard of the fused train step on the device -- the norm launch and its
finalisation against tests/clip_ref.py on every size class and alignment, their determinism, the clipped sweeps bit for bit
against the plain ones, the skipped sweep, the model step (eager, captured, under the real schedule, data-parallel, ``fit``)
against the float64 route of tests/test_clip_cpu.py, and the switch-off launch list."""
import gc
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests import clip_ref as R
from tests import optim_ref as OR
from tests.golden import cases as C
from tests.test_clip_cpu import (STATE, STEP_CASES, Torch64, case_of, compare_state, grad_norm64, gradients, make_engine)
from tests.test_dropout_cpu import set_batch, tiny_model
from tests.test_gpu_optim import LEADS, bits, guards_hold, place

pytestmark = pytest.mark.gpu

BIG = (16 << 20) + 5            # the streaming paths of the norm launch and of the Adam sweep
SENT = -1234567                 # integer sentinel of the guard bands around the record


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


@pytest.fixture(scope='module')
def cases():
    """the fp32 arrays and their float64 sums of squares, computed once per (class, n)"""
    cache = {}

    def get(cls, n):
        if (cls, n) not in cache:
            g = R.values(cls, n)
            cache[(cls, n)] = (g, R.sumsq64(g))
        return cache[(cls, n)]
    return get


class Frame:
    """a clip state (step, max_norm, record, workspace: ``kernels.clip_state``) between guard bands of 64 integer sentinels"""

    def __init__(self, K, n, dev, n_skipped=0, step=1):
        self.np_ = K.sumsq_partials(n)
        words = K.CLIP_STATE_WORDS + 2 * self.np_
        self.buf = torch.full((R.GUARD + words + R.GUARD,), SENT, dtype=torch.int32, device=dev)
        self.state = self.buf[R.GUARD:R.GUARD + words]
        self.state[:K.CLIP_STATE_WORDS].zero_()
        self.rec, self.part = K.clip_record(self.state), K.clip_partials(self.state)
        self.state[0] = step
        self.rec[3] = n_skipped

    def run(self, K, g, gscale, max_norm):
        K.clip_set_max_norm(self.state, max_norm)
        K.clip_norm(g, self.state, gscale=gscale)

    def intact(self):
        b = self.buf
        return bool((b[:R.GUARD] == SENT).all()) and bool((b[-R.GUARD:] == SENT).all())

    def values(self, K):
        v = K.clip_record_values(self.rec)
        return dict(norm=v['norm'], coef=v['coef'], skip=int(v['skipped_last']), n_skipped=v['n_skipped'])


def test_partials_are_a_function_of_n_alone(K):
    assert [K.sumsq_partials(n) for n in (0, 1, 8192, 8193, 4099, BIG, 1 << 31)] == [1, 1, 1, 2, 1, 1024, 1024]
    assert [K.sumsq_partials(n) for n in (1023 * 8192, 1023 * 8192 + 1, 1024 * 8192)] == [1023, 1024, 1024]


# ------------------------------------------------------------------------------------------------ 1. norm and coefficient
@pytest.mark.parametrize('n', R.SIZES)
@pytest.mark.parametrize('cls', R.CLASSES)
def test_norm_and_coefficient_against_the_reference(K, dev, cases, cls, n):
    g, s = cases(cls, n)
    worst = 0.0
    for lead in LEADS:
        buf, view = place(g, dev, lead)
        before = bits(buf).clone()
        for gscale in (1.0, 0.125):
            norm = R.record(s, gscale, float('inf'))['norm']
            for max_norm in (0.5 * norm if norm > 0 else 1.0, float('inf')):
                want = R.record(s, gscale, max_norm)
                f = Frame(K, n, dev)
                f.run(K, view, gscale, max_norm)
                torch.cuda.synchronize()
                got = f.values(K)
                worst = max(worst, R.check(got, want, (cls, n, lead, gscale, max_norm)))
                assert got['n_skipped'] == 0 and f.intact()
                if cls == 'zeros':
                    assert got['norm'] == 0.0 and got['coef'] == 1.0
                if max_norm == float('inf'):
                    assert got['coef'] == 1.0
        assert torch.equal(bits(buf), before), 'the gradient (and its guard bands) is only read'
        assert guards_hold(buf, lead, n)
    print('%s n=%d: worst |got - float64| / bound %.3g' % (cls, n, worst))


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize('n', R.SIZES)
@pytest.mark.parametrize('cls', R.CLASSES)
def test_the_record_is_bitwise_reproducible(K, dev, cases, cls, n):
    """every case of the test above, twice, from different workspace contents: identical bits in the record and the partials"""
    g, s = cases(cls, n)
    for lead in LEADS:
        _, view = place(g, dev, lead)
        for gscale in (1.0, 0.125):
            norm = R.record(s, gscale, float('inf'))['norm']
            for max_norm in (0.5 * norm if norm > 0 else 1.0, float('inf')):
                runs = []
                for fill in (0.0, 7.5):
                    f = Frame(K, n, dev)
                    f.part.fill_(fill)              # (whatever the workspace held: every partial is written)
                    f.state[0] = int(fill)          # (... and whatever the step counter says: the norm pass does not read it)
                    f.run(K, view, gscale, max_norm)
                    torch.cuda.synchronize()
                    runs.append((f.rec.clone(), f.part.clone().view(torch.int64)))
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (cls, n, lead, gscale, max_norm)


# ------------------------------------------------------------------------------------------------ 3. clipped = plain sweep
def _state(n, dev, seed=1):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(n, generator=gen, device=dev) * 0.3
    g = torch.randn(n, generator=gen, device=dev) * 0.02
    m = torch.randn(n, generator=gen, device=dev) * 0.01
    v = torch.rand(n, generator=gen, device=dev) * 1e-4 + 1e-8
    return p, g, m, v


def _state_with(dev, t, coef, skip=0, n_skipped=0):
    """a clip state written by hand: step ``t`` and the record {norm 1.5, coef, skip, n_skipped}; no workspace is needed"""
    f = np.array([1.5, coef], np.float32).view(np.int32)
    return torch.tensor([t, 0, 0, 0, int(f[0]), int(f[1]), skip, n_skipped], dtype=torch.int32, device=dev)


def _sweeps(K, kind):
    return (K.adam_l2, K.adam_l2_clip) if kind == 'adam' else (K.adamax_l2, K.adamax_l2_clip)


@pytest.mark.parametrize('n', [OR.N_CASE, BIG])
@pytest.mark.parametrize('kind', OR.KINDS)
def test_clipped_sweep_equals_the_plain_sweep_at_the_scaled_gradient(K, dev, kind, n):
    plain, clipped = _sweeps(K, kind)
    src = _state(n, dev)
    coef = float(np.float32(0.37))
    for lead in LEADS:
        for wd in OR.DECAYS:
            for gscale in ((1.0, 0.125) if n == OR.N_CASE else (0.125,)):
                for t, ns in ((1, 0), (1000, 0), (1000, 3), (4, 3)):
                    h = OR.hyper32(weight_decay=wd, gscale=gscale)
                    hk = dict(lr=h['lr'], beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'], weight_decay=h['weight_decay'])
                    a = [place(x, dev, lead) for x in src]
                    b = [place(x, dev, lead) for x in src]
                    halt = torch.zeros(4, dtype=torch.int32, device=dev)
                    step = torch.tensor([t], dtype=torch.int32, device=dev)
                    clipped(*[v for _, v in a], _state_with(dev, t, coef, 0, ns), gscale=h['gscale'], halt=halt, **hk)
                    gs = float(np.float32(h['gscale']) * np.float32(coef))
                    plain(*[v for _, v in b], step - ns, gscale=gs, halt=halt, **hk)
                    torch.cuda.synchronize()
                    site = (kind, n, lead, wd, gscale, t, ns)
                    for (ba, _), (bb, _) in zip(a, b):
                        assert torch.equal(bits(ba), bits(bb)), site           # views AND guard bands, g included
                    assert not torch.equal(a[0][1], src[0]), site
                    assert not bool(halt.any())
        # coef == 1.0f gives the plain sweep's bits at gscale itself
        h = OR.hyper32(weight_decay=0.05, gscale=0.125)
        hk = {k: h[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'gscale')}
        step = torch.tensor([7], dtype=torch.int32, device=dev)
        outs = []
        for how in ('plain', 'one'):
            a = [place(x, dev, lead) for x in src]
            views = [v for _, v in a]
            if how == 'plain':
                plain(*views, step, **hk)
            else:
                clipped(*views, _state_with(dev, 7, 1.0), **hk)
            torch.cuda.synchronize()
            outs.append([bits(bf).clone() for bf, _ in a])
        for other in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(outs[0], other)), (kind, n, lead)


# ------------------------------------------------------------------------------------------------ 4. non-finite gradients
@pytest.mark.parametrize('kind,n,lead', [('adam', OR.N_CASE, 0), ('adam', OR.N_CASE, 1), ('adam', BIG, 0), ('adamax', OR.N_CASE, 0),
                                         ('adamax', OR.N_CASE, 1)])
def test_a_non_finite_gradient_skips_the_sweep(K, dev, kind, n, lead):
    _, clipped = _sweeps(K, kind)
    src = _state(n, dev)
    placed = [place(x, dev, lead) for x in src]
    views = [v for _, v in placed]
    before = [bits(b).clone() for b, _ in placed]
    halt = torch.zeros(6, dtype=torch.int32, device=dev)
    halt[1::2] = torch.tensor([11, 22, 33], dtype=torch.int32, device=dev)      # (tick statistics: not error words)
    halt0 = halt.clone()
    f = Frame(K, n, dev, step=1)                                # (with the first launch skipped: t = 0 is never evaluated)
    step = f.state[0:1]
    hk = dict(lr=5e-4, weight_decay=0.05, gscale=1.0, halt=halt)
    count = 0
    for bad in (float('nan'), float('inf'), float('-inf')):
        for pos in (0, n // 2, n - 1):
            keep = views[1][pos].clone()
            views[1][pos] = bad
            before[1] = bits(placed[1][0]).clone()
            f.run(K, views[1], 1.0, 2.0)
            clipped(*views, f.state, **hk)
            torch.cuda.synchronize()
            count += 1
            got = f.values(K)
            assert got['skip'] == 1 and got['n_skipped'] == count and got['coef'] == 0.0 and not math.isfinite(got['norm'])
            for (b, _), b0 in zip(placed, before):
                assert torch.equal(bits(b), b0), (kind, n, lead, bad, pos)
            assert torch.equal(halt, halt0) and f.intact()
            views[1][pos] = keep
            step += 1
    # not sticky: the next clean launch is applied, with t = step - n_skipped = 1
    before[1] = bits(placed[1][0]).clone()
    f.run(K, views[1], 1.0, 2.0)
    clipped(*views, f.state, **hk)
    torch.cuda.synchronize()
    got = f.values(K)
    assert got['skip'] == 0 and got['n_skipped'] == count and int(step) - count == 1
    twin = [place(x, dev, lead) for x in src]
    plain, _ = _sweeps(K, kind)
    plain(*[v for _, v in twin], torch.ones(1, dtype=torch.int32, device=dev),
          **dict(hk, gscale=float(np.float32(1.0) * np.float32(got['coef']))))
    torch.cuda.synchronize()
    for (b, _), (tb, _) in zip(placed, twin):
        assert torch.equal(bits(b), bits(tb)), (kind, n, lead)
    assert torch.equal(halt, halt0)


# ------------------------------------------------------------------------------------------------ 5. the step
def _graph_of_the_step(e):
    """forward + backward + clipped optimiser step on the injected noise as ONE captured graph (not replayed yet)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e._launch_sequence(draw=False, optimizer=False)          # warm-up: loads code objects, updates nothing
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e.step_dev -= 1                     # (the warm-up's loss-scalar launch advanced the step counter: take that back)
    e._ctr_bumped = False
    g = torch.cuda.CUDAGraph()
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            e._launch_sequence(draw=False, optimizer=True)
    finally:
        if on:
            gc.enable()
    return g


@pytest.mark.parametrize('name', STEP_CASES)
def test_three_clipped_steps_against_the_float64_route(dev, name):
    case, spec, params = case_of(name)
    noises = case['noises']
    probe, parena = make_engine(spec, params, device=dev)
    set_batch(probe, case['batch'], dev)
    gradients(probe, noises[0])
    torch.cuda.synchronize()
    thr = 0.5 * grad_norm64(parena, probe.cfg)           # half of the first step's norm: clipping is active
    ref = Torch64(parena, probe.cfg, thr)
    eager, earena = make_engine(spec, params, max_grad_norm=thr, device=dev)
    cap, carena = make_engine(spec, params, max_grad_norm=thr, device=dev)
    for e in (eager, cap):
        set_batch(e, case['batch'], dev)
    cap.training = True
    cap.set_noise(noises[0])
    graph = None
    for k in range(3):
        noise = noises[k % len(noises)]
        # the float64 route: an unclipped engine's gradients at the route's own parameters -> torch clip -> torch optimiser
        for n_ in ref.names:
            parena.p(n_).copy_(ref.state(n_, 'param').float())
        probe.iters = k
        gradients(probe, noise)
        torch.cuda.synchronize()
        norm = grad_norm64(parena, probe.cfg)
        ref.step(parena)
        eager.train_step(noise)
        torch.cuda.synchronize()
        st = eager.clip_stats()
        # the padding check: the launch's norm over the whole live slice against the float64 norm of the parameter views
        # of ITS OWN gradient arena
        own = grad_norm64(earena, eager.cfg)
        R.check(dict(norm=st['norm'], coef=st['coef'], skip=int(st['skipped_last'])), R.record(own * own, 1.0, thr), (name, k))
        assert (st['coef'] < 1.0 if k == 0 else st['coef'] <= 1.0) and st['n_skipped'] == 0 and math.isfinite(norm)
        compare_state(earena, ref, '%s eager step %d' % (name, k + 1))
        # captured: the same step as one graph, replayed; equal to the eager step bit for bit
        cap.set_noise(noise)
        if graph is None:
            graph = _graph_of_the_step(cap)
        cap.plan.set_beta(cap.beta_pert())
        graph.replay()
        cap.iters += 1
        torch.cuda.synchronize()
        for w in STATE + ('grad',):
            assert torch.equal(getattr(carena, w), getattr(earena, w)), (name, k, w)
        assert torch.equal(cap.clip_rec, eager.clip_rec)
    assert all(not bool(x.any()) for x in earena.pads(earena.grad)), 'pad columns of the gradient arena'


@pytest.mark.parametrize('name', STEP_CASES)          # the four named cases and the Adamax one
def test_an_infinite_threshold_changes_no_bit(dev, name):
    case, spec, params = case_of(name)
    out = []
    for kw in ({}, dict(max_grad_norm=float('inf'))):
        eng, arena = make_engine(spec, params, device=dev, **kw)
        set_batch(eng, case['batch'], dev)
        for k in range(3):
            eng.train_step(case['noises'][k % len(case['noises'])])
        torch.cuda.synchronize()
        out.append([getattr(arena, w).clone() for w in STATE])
        if kw:
            st = eng.clip_stats()
            assert st['coef'] == 1.0 and st['n_skipped'] == 0 and st['norm'] > 0
    assert all(torch.equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_vfae', 'tiny_pvae'])
def test_captured_schedule_replays_like_the_eager_clipped_step(dev, name):
    """``capture()`` under the default schedule (two flag-ordered graphs where the model has a classifier): Philox noise,
    three replays behind an eager step equal four eager steps bit for bit"""
    case, spec, params = case_of(name)
    out = []
    for captured in (True, False):
        eng, arena = make_engine(spec, params, max_grad_norm=0.05, device=dev)
        set_batch(eng, case['batch'], dev)
        eng.train_step()
        if captured:
            eng.capture()
            assert not eng.noise_ahead
            for _ in range(3):
                eng.replay()
            eng.check_sync()
        else:
            for _ in range(3):
                eng.train_step()
        torch.cuda.synchronize()
        st = eng.clip_stats()
        assert st['coef'] < 1.0 and st['n_skipped'] == 0
        out.append(([getattr(arena, w).clone() for w in STATE], eng.losses(), st))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0])) and out[0][1] == out[1][1] and out[0][2] == out[1][2]


def test_padded_rows_and_the_tuned_partition_at_the_benchmark_shape(dev, monkeypatch):
    """the default DrVAE configuration, 150 rows (978-column weights: rows padded to 980 inside the arena).  The norm the launch
    takes over the whole live slice, pad columns included, is the float64 norm of the parameter views, and the pads are zero.
    ``tune_partition`` replays the captured step on the live state and puts the state back: the clip record with it -- a
    tuning replay that the guard skips (emulated: every tuning replay bumps ``n_skipped``) must not stay counted while the step
    counter goes back, or the first real step would run with t = step - n_skipped <= 0."""
    monkeypatch.delenv('DRVAE_SIDE_CUS', raising=False)
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    eager, a0 = make_engine(spec, params, max_grad_norm=1.0, device=dev)
    graph, a1 = make_engine(spec, params, max_grad_norm=1.0, device=dev)
    for e in (eager, graph):
        set_batch(e, batch, dev)
        e.train_step()
    torch.cuda.synchronize()
    pads = a1.pads(a1.grad)
    assert len(pads) > 0 and sum(x.numel() for x in pads) > 1000, 'no padded rows at this shape'
    assert all(not bool(x.any()) for x in pads), 'pad columns of the gradient arena'
    st, own = graph.clip_stats(), grad_norm64(a1, graph.cfg)
    R.check(dict(norm=st['norm'], coef=st['coef'], skip=int(st['skipped_last'])), R.record(own * own, 1.0, 1.0), 'cfg 2')
    assert st['coef'] < 1.0
    graph.capture()
    assert graph._side_graph is not None, 'the dual-graph schedule was not taken'
    saved = (graph.clip_state.clone(), int(graph.step_dev))
    real, calls = graph.replay, []

    def replay_and_skip(*a, **k):
        out = real(*a, **k)
        graph.clip_rec[3] += 1
        calls.append(1)
        return out
    monkeypatch.setattr(graph, 'replay', replay_and_skip)
    chosen = graph.tune_partition(candidates=(32, 64), steps=4)
    monkeypatch.undo()
    assert chosen in (32, 64) and len(calls) == 2 * (4 + 4), 'tune_partition did not replay'
    assert int(graph.step_dev) == saved[1] and graph.clip_stats()['n_skipped'] == 0
    assert torch.equal(graph.clip_rec, K_record(saved[0]))
    with graph.partition():
        for _ in range(4):
            graph.replay()
    for _ in range(4):
        eager.train_step()
    torch.cuda.synchronize()
    graph.check_sync()
    assert torch.equal(a0.param, a1.param) and torch.equal(a0.exp_avg, a1.exp_avg) and torch.equal(a0.exp_avg_sq, a1.exp_avg_sq)
    assert eager.clip_stats() == graph.clip_stats() and eager.losses() == graph.losses()
    assert all(not bool(x.any()) for x in a1.pads(a1.grad))


def K_record(state):
    import drvae_amd.kernels as K
    return K.clip_record(state)


# ------------------------------------------------------------------------------------------------ 6. skip inside a captured step
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_pvae'])
def test_a_nan_input_skips_one_replay_and_training_goes_on(dev, name):
    case, spec, params = case_of(name)
    eng, arena = make_engine(spec, params, max_grad_norm=1.0, device=dev)
    p = set_batch(eng, case['batch'], dev)
    eng.train_step()
    eng.capture()
    eng.replay()
    torch.cuda.synchronize()
    before = [getattr(arena, w).clone() for w in STATE]
    step = int(eng.step_dev)
    keep = p.XSRC[0, 0].clone()            # (the batch's input rows: the step gathers from here)
    p.XSRC[0, 0] = float('nan')
    eng.replay()
    p.XSRC[0, 0] = keep
    torch.cuda.synchronize()
    st = eng.clip_stats()
    assert st['skipped_last'] and st['n_skipped'] == 1
    assert all(torch.equal(a, getattr(arena, w)) for a, w in zip(before, STATE))
    assert int(eng.step_dev) == step + 1
    for _ in range(2):
        eng.replay()
    torch.cuda.synchronize()
    eng.check_sync()
    st = eng.clip_stats()
    assert not st['skipped_last'] and st['n_skipped'] == 1 and math.isfinite(st['norm'])
    assert not torch.equal(before[0], arena.param) and bool(torch.isfinite(arena.param).all())
    assert all(math.isfinite(v) for v in eng.losses().values())
    # ... exactly as an engine that never saw the skipped replay: same draws per step, t without the skipped one
    twin, tarena = make_engine(spec, params, max_grad_norm=1.0, device=dev)
    set_batch(twin, case['batch'], dev)
    for k in range(5):
        if k == 2:                      # the skipped step: its draw event, its count, nothing else
            twin.draw_noise()
            twin.step_dev += 1
            twin.clip_rec[3] += 1
            twin.sync_side_counters()
            continue
        twin.train_step()
    torch.cuda.synchronize()
    assert torch.equal(tarena.exp_avg, arena.exp_avg) and torch.equal(tarena.param, arena.param)


# ------------------------------------------------------------------------------------------------ 7. the launch list
CLIP_NAMES = ('dv_grad_norm_clip', 'dv_adam_l2_clipped', 'dv_adamax_l2_clipped')


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_switch_off_step_launches_what_it_always_did(dev, kind, monkeypatch):
    from tests.test_dropout_cpu import make_engine as plain_engine
    from tests.test_gpu_dropout import _captured_launch_names
    from tests.test_gpu_x3 import tuned
    spec = M.ModelSpec(kind=kind, L=1 if kind == 'pvae' else 2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    lists = {}
    for tune in ('', 'sched=3'):
        with tuned(tune):
            for tag in ('absent', 'none', 'set'):
                if tag == 'absent':
                    eng, _ = plain_engine(spec, params, device=dev)
                else:
                    eng, _ = make_engine(spec, params, max_grad_norm=None if tag == 'none' else 1.0, device=dev)
                set_batch(eng, batch, dev)
                eng.train_step()
                lists[(tune, tag)] = _captured_launch_names(eng, monkeypatch)
                eng.replay()
                torch.cuda.synchronize()
                eng.check_sync()
    for tune in ('', 'sched=3'):
        absent, none = lists[(tune, 'absent')], lists[(tune, 'none')]
        assert absent and not [w for w in none if w in CLIP_NAMES]
        assert len(none) == len(absent) and none == absent
        assert none.count('dv_fill_normal_rows') == absent.count('dv_fill_normal_rows')
    plain, clipped = lists[('sched=3', 'none')], lists[('sched=3', 'set')]
    i = plain.index('dv_adam_l2')
    assert plain.count('dv_adam_l2') == 1
    assert clipped == plain[:i] + list(CLIP_NAMES[:2]) + plain[i + 1:]
    dual = lists[('', 'set')]
    assert [w for w in dual if w in CLIP_NAMES] == list(CLIP_NAMES[:2])
    assert 'dv_adam_l2' not in dual and 'dv_adam_l2_gated' not in dual
    print('%s: %d launches unclipped, %d clipped (one graph); default schedule %d / %d'
          % (kind, len(plain), len(clipped), len(lists[('', 'none')]), len(dual)))


# ------------------------------------------------------------------------------------------------ 8. data parallelism
def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK='0')
        import torch.distributed as dist
        from drvae_amd import dist as D
        from tests.test_engine_cpu import set_batch
        D.init_from_env(backend='gloo')
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(0)
        spec = C.tiny_spec('drvae')
        params = M.init_params(spec, 3, as_numpy=True)
        full = M.make_batch(spec, 16, seed=6)
        full['has_y'], full['has_x2'] = C._flags('acbdabcdbdcaabcd')
        lo, hi = D.shard_rows(16, rank, world)
        shard = {k: v[lo:hi] for k, v in full.items()}
        counts = D.global_counts(shard['has_x2'], shard['has_y'])
        # one rank on the 16 rows: the threshold is half of its first gradient norm
        probe, parena = make_engine(spec, params, device=dev)
        probe.seed = 4242
        set_batch(probe, full, dev)
        probe.training = True
        probe.draw_noise(bump=False)
        probe._launch_sequence(draw=False, optimizer=False)
        torch.cuda.synchronize()
        thr = 0.5 * grad_norm64(parena, probe.cfg)
        one, a1 = make_engine(spec, params, max_grad_norm=thr, device=dev)
        one.seed = 4242
        set_batch(one, full, dev)
        for _ in range(3):
            one.train_step()
        torch.cuda.synchronize()
        res = {}
        for mode in ('eager', 'split', 'overlap'):
            eng, arena = make_engine(spec, params, max_grad_norm=thr, device=dev)
            eng.seed, eng.row0 = 4242, lo
            set_batch(eng, shard, dev, counts=counts)
            eng.train_step(allreduce=D.allreduce_sum)
            if mode == 'eager':
                for _ in range(2):
                    eng.train_step(allreduce=D.allreduce_sum)
            else:
                eng.capture(split_for_allreduce=True if mode == 'split' else 'overlap')
                ar = D.OverlappedAllReduce() if mode == 'overlap' else D.allreduce_sum
                for _ in range(2):
                    eng.replay(ar)
            torch.cuda.synchronize()
            eng.check_sync()
            st = eng.clip_stats()
            perr = float((arena.param - a1.param).norm() / a1.param.norm())
            merr = float((arena.exp_avg - a1.exp_avg).norm() / a1.exp_avg.norm())
            rec = eng.clip_rec.cpu()
            both = [torch.zeros_like(rec) for _ in range(world)]
            dist.all_gather(both, rec)
            res[mode] = dict(perr=perr, merr=merr, same=bool(all(torch.equal(b, both[0]) for b in both)), coef=st['coef'],
                             n_skipped=st['n_skipped'], norm=st['norm'])
        q.put((rank, 'ok', res, one.clip_stats()))
        dist.destroy_process_group()
    except Exception as e:       # surface the failure instead of a hung join
        import traceback
        q.put((rank, 'error', traceback.format_exc(), str(e)))


def test_two_ranks_clip_like_one(dev):
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
        one = o[3]
        assert one['coef'] < 1.0 and one['n_skipped'] == 0
        for mode, r in o[2].items():
            print('rank %d %s: %s' % (o[0], mode, r))
            assert r['same'], (mode, 'norm and coef differ between the ranks')
            assert r['perr'] < 1e-4 and r['merr'] < 1e-4, (mode, r)           # (the tolerance of tests/test_gpu_dp.py)
            assert r['coef'] < 1.0 and r['n_skipped'] == 0
            assert abs(r['norm'] - one['norm']) <= 1e-4 * one['norm']


# ------------------------------------------------------------------------------------------------ 9. fit
@pytest.mark.parametrize('kind', ['drvae', 'pvae'])
def test_fit_with_a_threshold_trains_on_the_device_feed(dev, kind, tmp_path):
    import warnings
    from drvae_amd import data as D
    from tests.test_fit import _loader, _tiny_dataset
    model = tiny_model(kind, max_grad_norm=0.5, device=dev)
    model.w2log = lambda *a: None
    tr, va = _tiny_dataset(kind, 64, 1, dev), _tiny_dataset(kind, 32, 2, dev)
    w = D.compute_balanced_weights(np.arange(64) % 5)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (no step is skipped: no warning)
        model.fit(D.DeviceBatcher(tr, w, 16, seed=3), _loader(va, 8), add_noise=True, verbose=False, early_stop=False,
                  model_filename=str(tmp_path / 'b.pth'))
    assert model.finished_training_iters == 2 * 4
    st = model.grad_clip_stats()
    assert set(st) == {'norm', 'coef', 'skipped_last', 'n_skipped'}
    assert st['n_skipped'] == 0 and 0.0 < st['coef'] <= 1.0 and math.isfinite(st['norm']) and st['norm'] > 0
    assert bool(torch.isfinite(model.engine().arena.param).all())
    perf, _ = model.evaluate_performance_on_dataset(va)
    assert all(np.isfinite(float(v)) for v in perf['losses'].values())
    # a skipped step in an epoch is named by one warning
    eng = model.engine()
    eng.clip_rec[3] += 2
    with pytest.warns(UserWarning, match='2 train step'):
        assert model._warn_skipped_steps(3, 0) == 2
