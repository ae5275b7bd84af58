"""-m gpu: the optimiser sweeps (``dv_adam_l2``, ``dv_adam_l2_gated``, ``dv_adamax_l2``) below model level, on every launch
path: the float4 and the scalar loop of ``adam_kernel`` (a view shifted by one element takes the scalar one), its grid at
the 2048-workgroup cap, ``adam_stream_kernel`` from its threshold on, the gate and its time-out, ``halt``.

Against tests/optim_ref.py: every stored element of p, m, v / u within the componentwise float64 bound of one step and
at most twice as far from float64 as the worse host emulation; pads bit-zero; nothing outside the views and nothing of
g written, every element inside written; all paths bit-equal on the same inputs; a gated launch bit-equal to the plain
one.  tests/test_optim_cpu.py proves the same checks against faulty emulations.  With ``-s`` the module prints the
worst ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.test_gpu_kernels import _other_queue_stream

pytestmark = pytest.mark.gpu

NANBITS = 0x7fc00000
LEADS = (0, 1)                  # elements a view is shifted by: 0 = 16-byte aligned (float4 loops), 1 = the scalar loop
MI = 1 << 20
STREAM_SPAN = 4 * 16384 * 256   # elements one slot of adam_stream_kernel's grid covers
CAP_SPAN = 4 * 2048 * 256       # elements one pass of adam_kernel's capped grid covers (float4 loop)
# the smallest size that reaches each branch
BIG = (16 * MI - 4,             # float4 adam_kernel at the 2048-workgroup cap, the grid-stride loop wraps
       16 * MI,                 # the threshold: adam_stream_kernel, n4 == its stride, no second slot is valid
       24 * MI + 3,             # second slot valid for part of the grid, and a scalar tail
       40 * MI + 1)             # second iteration of the two-slot loop


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
    print('\noptimiser sweeps on the device: worst |got - float64| / bound, and worst distance / emulations\' distance')
    for key in sorted(worst):
        print('  %-48s %s' % (' '.join(str(k) for k in key), '   '.join('%s %.3g' % qv for qv in sorted(worst[key].items()))))


def note(table, key, vals):
    row = table.setdefault(key, {})
    for q, v in vals.items():
        row[q] = max(row.get(q, 0.0), v)


def bits(t):
    return t.view(torch.int32)


def place(t, dev, lead):
    """``t`` as a view into a NaN-filled device buffer, R.GUARD elements on both sides, shifted by ``lead`` elements"""
    t = torch.as_tensor(t)
    n, o = t.numel(), lead + R.GUARD
    buf = torch.full((o + n + R.GUARD,), float('nan'), dtype=torch.float32, device=dev)
    view = buf[o:o + n]
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == (lead % 4 == 0)
    return buf, view


def guards_hold(buf, lead, n):
    o = lead + R.GUARD
    return bool((bits(buf[:o]) == NANBITS).all()) and bool((bits(buf[o + n:]) == NANBITS).all())


def sweep(K, kind, views, t, h, dev, **kw):
    step = torch.tensor([t], dtype=torch.int32, device=dev)
    (K.adam_l2 if kind == 'adam' else K.adamax_l2)(*views, step, lr=h['lr'], beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'],
                                                   weight_decay=h['weight_decay'], gscale=h['gscale'], **kw)


def host(kind, views):
    torch.cuda.synchronize()
    p, _, m, v = views
    return {'p': p.cpu().numpy(), 'm': m.cpu().numpy(), R.STORED[kind][2]: v.cpu().numpy()}


# ------------------------------------------------------------------------------------------------ 1. the bound
ALL = [(k, c) for k in R.KINDS for c, _ in R.cases(k)]


@pytest.mark.parametrize('kind,cls', ALL, ids=['%s-%s' % kc for kc in ALL])
def test_within_the_bound_on_both_loops(K, dev, table, kind, cls):
    for t, gs, wd in R.settings(cls):
        arrays, h, ref = R.case_ref(kind, cls, t, gs, wd)
        yard = R.yardstick(kind, cls, t, gs, wd)
        for lead in LEADS:
            site = '%s %s t=%d gscale=%g wd=%g lead=%d' % (kind, cls, t, gs, wd, lead)
            placed = [place(a, dev, lead) for a in arrays]
            views = [v for _, v in placed]
            sweep(K, kind, views, t, h, dev)
            got = host(kind, views)
            failed, worst, dist = R.verify(kind, got, arrays, t, h, site=site, ref=ref)
            print(site, 'excess', worst, 'distance', dist, 'emulations', yard)
            note(table, (kind, cls, 'lead=%d' % lead, 'excess'), worst)
            note(table, (kind, cls, 'lead=%d' % lead, 'distance/emulations'),
                 {q: dist[q] / yard[q] if yard[q] > 0 else (0.0 if dist[q] == 0 else float('inf')) for q in dist})
            assert failed == set(), (site, worst)
            assert all(np.isfinite(a).all() for a in got.values()), site
            for q in dist:
                assert dist[q] <= 2 * yard[q], (site, q, dist[q], yard[q])
            assert all(guards_hold(b, lead, arrays[0].size) for b, _ in placed), site
            if cls == 'pads':
                for q in ('p', 'm') + (('v',) if kind == 'adam' else ()):
                    assert not R.bits(got[q]).any(), (site, q, 'a pad must stay bit-zero')


# ------------------------------------------------------------------------------------------------ 2. the memory contract
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 1023, 1025])
def test_memory_contract(K, dev, kind, n):
    t, h = 1, R.hyper32(weight_decay=0.05)
    inputs = R.frame_inputs(n)
    for lead in LEADS:
        placed = [place(a, dev, lead) for a in inputs]
        before = {k: b.cpu().numpy().copy() for k, (b, _) in zip('pgmv', placed)}
        sweep(K, kind, [v for _, v in placed], t, h, dev)
        torch.cuda.synchronize()
        after = {k: b.cpu().numpy() for k, (b, _) in zip('pgmv', placed)}
        sl = slice(lead + R.GUARD, lead + R.GUARD + n)
        assert R.memory_faults(before, after, sl) == set(), (kind, n, lead)
        got = {'p': after['p'][sl], 'm': after['m'][sl], R.STORED[kind][2]: after['v'][sl]}
        failed, worst, _ = R.verify(kind, got, inputs, t, h)
        assert failed == set(), (kind, n, lead, worst)


def test_an_empty_sweep_returns_ok(K, dev):
    e = [torch.empty(0, device=dev) for _ in range(4)]
    h = R.hyper32()
    sweep(K, 'adam', e, 1, h, dev)
    sweep(K, 'adamax', e, 1, h, dev)
    z = torch.zeros(2, dtype=torch.int32, device=dev)
    sweep(K, 'adam', e, 1, h, dev, gate=(z[0:1], z[1:2], 0, z, 0, 0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. path equality
def big_inputs(n, dev, seed=0):
    """device inputs in which an update changes every element of p, m and v (as ``R.frame_inputs``)"""
    gen = torch.Generator(device=dev).manual_seed(100 + seed)
    i = torch.arange(n, dtype=torch.int32, device=dev)
    p = torch.randn(n, generator=gen, device=dev)
    g = torch.randn(n, generator=gen, device=dev)
    return p, g, 1000.0 + (i % 7).float(), 1000.0 + (i % 5).float()


def sample_indices(n):
    """at most 2^20 elements: the first and the last 4096, 4096 on either side of every multiple of the streaming grid's
    slot (slot and iteration boundaries of adam_stream_kernel) and 64 on either side of every pass of the capped grid"""
    parts = [np.arange(0, min(4096, n)), np.arange(max(n - 4096, 0), n)]
    parts += [np.arange(b - 4096, b + 4096) for b in range(STREAM_SPAN, n + 4096, STREAM_SPAN)]
    parts += [np.arange(b - 64, b + 64) for b in range(CAP_SPAN, n + 64, CAP_SPAN)]
    idx = np.unique(np.concatenate(parts))
    idx = idx[(idx >= 0) & (idx < n)]
    assert idx.size <= MI
    return idx


def run_big(K, dev, kind, inputs, lead, t, h):
    """one sweep over copies of ``inputs`` placed at ``lead``; the memory contract is checked on the device.
    Returns the views (p, g, m, v) after the sweep"""
    n = inputs[0].numel()
    placed = [place(a, dev, lead) for a in inputs]
    views = [v for _, v in placed]
    sweep(K, kind, views, t, h, dev)
    torch.cuda.synchronize()
    assert all(guards_hold(b, lead, n) for b, _ in placed), 'written outside a view'
    assert torch.equal(bits(views[1]), bits(inputs[1])), 'g was written'
    for q, a, b in zip('pmv', (views[0], views[2], views[3]), (inputs[0], inputs[2], inputs[3])):
        assert bool((bits(a) != bits(b)).all()), '%s: an element was not written' % q
    return views


def hold_sample(kind, views, inputs, t, h, site):
    idx = torch.from_numpy(sample_indices(inputs[0].numel())).to(inputs[0].device)
    got = {'p': views[0][idx].cpu().numpy(), 'm': views[2][idx].cpu().numpy(), R.STORED[kind][2]: views[3][idx].cpu().numpy()}
    failed, worst, _ = R.verify(kind, got, [a[idx].cpu().numpy() for a in inputs], t, h, site=site)
    assert failed == set(), (site, worst)
    return worst


@pytest.mark.parametrize('n', BIG)
def test_all_paths_give_the_same_bits(K, dev, table, n):
    """``adam_one`` is inlined into every loop: the scalar loop (views shifted by one element) and whichever path alignment
    and size select must agree bit for bit in all four arrays, and a sample of the result lies within the bound"""
    t, h = 7, R.hyper32(weight_decay=0.05, gscale=0.125)
    inputs = big_inputs(n, dev)
    fast = run_big(K, dev, 'adam', inputs, 0, t, h)
    worst = hold_sample('adam', fast, inputs, t, h, 'n=%d aligned' % n)
    note(table, ('adam', 'n=%d' % n, 'sample', 'excess'), worst)
    fast = [a.clone() for a in (fast[0], fast[2], fast[3])]
    scalar = run_big(K, dev, 'adam', inputs, 1, t, h)
    for q, a, b in zip('pmv', fast, (scalar[0], scalar[2], scalar[3])):
        same = bits(a) == bits(b)
        assert bool(same.all()), ('n=%d: %s differs between the paths on %d elements, first at %d'
                                  % (n, q, int((~same).sum()), int((~same).nonzero()[0])))


def test_a_permutation_of_the_inputs_permutes_the_outputs(K, dev):
    n, t, h = 24 * MI + 3, 7, R.hyper32(weight_decay=0.05, gscale=0.125)
    inputs = big_inputs(n, dev)
    out = run_big(K, dev, 'adam', inputs, 0, t, h)
    out = [a.clone() for a in (out[0], out[2], out[3])]
    perm = torch.randperm(n, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    moved = run_big(K, dev, 'adam', [a[perm] for a in inputs], 0, t, h)
    for q, a, b in zip('pmv', out, (moved[0], moved[2], moved[3])):
        assert torch.equal(bits(a[perm]), bits(b)), q


def test_adamax_past_its_grid_cap(K, dev, table):
    """adamax_kernel's grid is capped at 4096 workgroups: 3 * 2^20 + 5 elements wrap its grid-stride loop"""
    n, t, h = 3 * MI + 5, 7, R.hyper32(weight_decay=0.05, gscale=0.125)
    p, g, m, _ = big_inputs(n, dev)
    inputs = (p, g, m, 0.7 * g.abs().roll(1) + 1e-3)        # a running max that decides on about half the elements
    a = run_big(K, dev, 'adamax', inputs, 0, t, h)
    note(table, ('adamax', 'n=%d' % n, 'sample', 'excess'), hold_sample('adamax', a, inputs, t, h, 'adamax n=%d' % n))
    b = run_big(K, dev, 'adamax', inputs, 1, t, h)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------ 4. the gate
def gated_raw(K, views, t_dev, h, flag, ctr, add, err, max_spins, lo, hi, halt=None):
    """``dv_adam_l2_gated`` with a ``max_spins`` of the caller's (``K.adam_l2(gate=)`` always passes the default)"""
    from drvae_amd import _lib
    p, g, m, v = views
    w = _lib.Wait()
    w.flag, w.ctr, w.err, w.add, w.max_spins = K._i32(flag), K._i32(ctr), K._i32(err), add, max_spins
    hy = _lib.AdamHyper(lr=h['lr'], beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'], weight_decay=h['weight_decay'],
                        gscale=h['gscale'])
    hp, hn = K._halt(halt)
    _lib.check(_lib.load().dv_adam_l2_gated(K._f32(p), K._f32(g), K._f32(m), K._f32(v), p.numel(), C.byref(hy), K._i32(t_dev),
                                            C.byref(w), lo, hi, hp, hn, K._stream()), 'dv_adam_l2_gated')


GATES = [(3 * MI + 5, 0, 2 * MI + 100, 2 * MI + 700),     # float4 loop, capped grid: the slice lies in the wrapped span
         (100003, 1, 5000, 5402),                         # an unaligned view: the scalar loop
         (100003, 0, 100001, 100003)]                     # entirely in the float4 loop's scalar tail


@pytest.mark.parametrize('n,lead,lo,hi', GATES)
def test_a_gated_sweep_equals_the_plain_one(K, dev, n, lead, lo, hi):
    t, h = 1, R.hyper32(weight_decay=0.05)
    inputs = big_inputs(n, dev, seed=1)
    want = run_big(K, dev, 'adam', inputs, lead, t, h)
    views = [place(a, dev, lead)[1] for a in inputs]
    g_final = views[1].clone()
    views[1][lo:hi] = 777.0                                # not final yet
    step = torch.ones(1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)
    side = _other_queue_stream(K, dev)
    torch.cuda.synchronize()
    K.adam_l2(*views, step, lr=h['lr'], weight_decay=h['weight_decay'], gate=(flag, step, 0, err, lo, hi))
    with torch.cuda.stream(side):
        torch.cuda._sleep(2000000)                         # ~1 ms: the sweep is parked on the gated slice by now
        views[1][lo:hi] = g_final[lo:hi]
        K.flag_publish(flag, step, 0)
    torch.cuda.synchronize()
    assert int(err[0]) == 0 and int(err[1]) > 0
    for q, a, b in zip('pgmv', views, want):
        assert torch.equal(bits(a), bits(b)), q


def parked_elements(n, vec4, lo, hi):
    """mask of the elements swept by workgroups that park on the gate [lo, hi): what ``adam_kernel`` computes as ``need``.
    A workgroup of 256 threads sweeps spans of 256 units (a unit: 4 elements in the float4 loop, else 1) a grid apart, the
    grid being capped at 2048 workgroups, and thread i of the grid the tail elements body + i, body + i + grid threads, ..."""
    per = 4 if vec4 else 1
    units = n // per
    grid = min(max((units + 255) // 256, 1), 2048)
    body = units * per
    e = np.arange(n)
    wg = np.where(e < body, (e // per // 256) % grid, ((e - body) % (grid * 256)) // 256)
    starts = np.arange(0, n, 256 * per)        # the kernel walks span starts up to n (a span inside the tail included)
    hit = (starts < hi) & (starts + 256 * per > lo)
    need = np.zeros(grid, bool)
    need[np.unique((starts[hit] // (256 * per)) % grid)] = True
    if hi > body and lo < n:
        need[:] = True                         # the tail is swept by every workgroup
    return need[wg]


@pytest.mark.parametrize('n,lead,lo,hi', GATES[:2])
def test_a_gate_that_times_out(K, dev, n, lead, lo, hi):
    """max_spins = 50 and a flag nobody publishes: the sticky error word is set, the launch returns, the elements of the
    workgroups that parked (the gated slice among them) keep p, m and v, every other element is updated in all three, and a
    launch that is handed the error word as ``halt`` changes nothing -- Adam and Adamax alike.  (The parked workgroups
    look at ``halt`` again after their wait: the gate's own error word has to be among it, as it is in the engine.  A gate
    whose word is not is only reported when it times out, like ``dv_flag_wait``, and the slice is swept.)"""
    t, h = 1, R.hyper32(weight_decay=0.05)
    inputs = big_inputs(n, dev, seed=2)
    want = run_big(K, dev, 'adam', inputs, lead, t, h)
    views = [place(a, dev, lead)[1] for a in inputs]
    step = torch.ones(1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)
    gated_raw(K, views, step, h, flag, step, 0, err, 50, lo, hi, halt=err)    # (as the engine: the gate's word is among ``halt``)
    torch.cuda.synchronize()
    assert int(err[0]) == 1
    kept = [bits(a) == bits(b) for a, b in zip((views[0], views[2], views[3]), (inputs[0], inputs[2], inputs[3]))]
    assert bool(kept[0][lo:hi].all()), 'the gated slice was touched'
    assert torch.equal(kept[0], kept[1]) and torch.equal(kept[0], kept[2]), 'an element was updated in part'
    for q, a, b in zip('pmv', (views[0], views[2], views[3]), (want[0], want[2], want[3])):
        assert torch.equal(bits(a)[~kept[0]], bits(b)[~kept[0]]), q
    assert torch.equal(bits(views[1]), bits(inputs[1]))
    assert np.array_equal(kept[0].cpu().numpy(), parked_elements(n, lead == 0, lo, hi)), 'not the parked workgroups\' elements'
    assert 0 < int(kept[0].sum()) < n
    frozen = [a.clone() for a in views]
    sweep(K, 'adam', views, 2, h, dev, halt=err)
    gated_raw(K, views, step, h, flag, step, -1, err, 50, lo, hi, halt=err)      # (an open gate: only ``halt`` stops it)
    sweep(K, 'adamax', views, 2, h, dev, halt=err)
    torch.cuda.synchronize()
    for a, b in zip(views, frozen):
        assert torch.equal(bits(a), bits(b)), 'a halted launch wrote'
    err.zero_()
    sweep(K, 'adamax', views, 2, h, dev, halt=err)         # the same launch with the word cleared does sweep
    torch.cuda.synchronize()
    assert bool((bits(views[2]) != bits(frozen[2])).all())


# ------------------------------------------------------------------------------------------------ 5. torch.optim
@pytest.mark.parametrize('T', [3, R.T_LONG])
def test_adam_p_m_v_against_torch_optim(K, dev, table, T):
    """T steps of the device sweep against torch.optim.Adam on the host, p, m and v: within ``R.trajectory_bounds`` -- what the
    fp32 betas of dv_adam_hyper and the fp32 rounding of both sides can amount to (derived there, proven on the host
    emulation in tests/test_optim_cpu.py)"""
    rs = np.random.RandomState(4)
    p0, gamma = rs.randn(R.N_CASE).astype(np.float32), rs.randn(R.N_CASE).astype(np.float32)
    h = R.hyper32()
    both, _ = R.trajectory_bounds(T, h, gamma, pmax=float(np.abs(p0).max()) + 1.0)
    ref = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=R.HYPER['lr'])
    p, m, v = torch.from_numpy(p0).to(dev), torch.zeros(p0.size, device=dev), torch.zeros(p0.size, device=dev)
    gd = torch.from_numpy(gamma).to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for k in range(1, T + 1):
        K.counter_add(step, 1)
        K.adam_l2(p, gd * R.long_scale(k), m, v, step, lr=R.HYPER['lr'])
        ref.grad = torch.from_numpy(gamma * np.float32(R.long_scale(k)))
        opt.step()
    torch.cuda.synchronize()
    assert int(step.item()) == T
    st = opt.state[ref]
    for q, got, want in (('p', p, ref.detach()), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
        d = np.abs(got.cpu().numpy().astype(np.float64) - want.numpy().astype(np.float64))
        note(table, ('adam', 'T=%d' % T, 'against torch.optim', 'distance'), {q: float(d.max())})
        note(table, ('adam', 'T=%d' % T, 'against torch.optim', 'distance/bound'), {q: float((d / both[q]).max())})
        assert (d <= both[q]).all(), (q, float((d / both[q]).max()))
