"""-m gpu: the device's N(0,1) source against the independent reference of tests/philox_ref.py, EVERY element of every
table, and Philox-driven train steps against the CPU oracle fed the reference's draws of the event each step must use.

Bound (the rule of tests/ref64.py): |got - ref| <= C * U * (r + r * a), U = 2^-24; r = sqrt(-2 ln u) carries the roundings
of logf, sqrtf, the product and the sincosf result, r * a the fp32 rounding of the angle a = 2 pi u.  Where r == 0 (the
uniform is exactly 1) the value must be exactly 0.  C_BOUND below is the smallest power of two the device needs (see
there); a wrong word, constant, round count or counter position is off by ~1e7 U.
"""
import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import philox_ref as P
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine, set_batch
from tests.test_philox_ref import EDGE_POSITIONS, EDGE_SEED, philox_steps_vs_oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# C: the smallest power of two the device needs.  Measured on the MI355X over all 76 comparisons of this file (each
# prints its figure; 5.6 M elements): worst |got - ref| / (U (r + r a)) = 2.892 (a cfg-1 PVAE table; 2^20 + 3 flat values
# 2.77, 70 000 rows 2.66, packed widths 2.40, train-step arenas 2.73) -> C = 4.  An fp32 emulation of the transform in
# numpy needs 3.1; the rule's cap is 64.
C_BOUND = 4.0
SENTINEL = -777.25


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def check(got, z, r, a, what):
    """every element of ``got`` (fp32, any device) against the float64 reference; -> the worst error in units of the bound's
    U (r + r a)"""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == z.shape, what
    assert np.all(np.isfinite(got)), what
    zero = r == 0
    assert np.all(got[zero] == 0), '%s: a value with radius 0 is not exactly 0' % what
    scale = U * (r + r * a)
    ratio = np.abs(got - z)[~zero] / scale[~zero]
    worst = float(ratio.max()) if ratio.size else 0.0
    print('%s: %d elements (%d exact zeros), worst error %.3f U(r + ra)' % (what, got.size, int(zero.sum()), worst))
    i = int(np.argmax(ratio)) if ratio.size else 0
    assert worst <= C_BOUND, '%s: element %d: got %r, reference %r (r %g, a %g): %.3g > C = %g' % (
        what, np.flatnonzero(~zero)[i], got[~zero][i], z[~zero][i], r[~zero][i], a[~zero][i], worst, C_BOUND)
    return worst


def draw_and_check(K, dev, desc, n_arena, seed, event, what, ctr_dev='event', park=None):
    """launch dv_fill_normal_rows on a sentinel-filled arena: every described element against the reference, every other
    element still the sentinel.  -> the arena"""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    assert desc[:, 0].min() >= 0 and desc[:, 1].min() > 0 and (desc[:, 0] + desc[:, 1]).max() <= n_arena     # in bounds
    arena = torch.full((n_arena,), SENTINEL, device=dev)
    d = torch.as_tensor(desc, dtype=torch.int32, device=dev)
    if ctr_dev == 'event':
        lo, hi = event & 0xffffffff, event >> 32
        ctr_dev = torch.tensor([lo - (1 << 32) if lo >= 1 << 31 else lo, hi - (1 << 32) if hi >= 1 << 31 else hi],
                               dtype=torch.int32, device=dev)
    K.fill_normal_rows(arena, d, seed, ctr_dev, park=park)
    torch.cuda.synchronize()
    off, z, r, a = P.rows_table(desc, seed, event)
    assert np.unique(off).size == off.size
    got = arena.cpu().numpy()
    check(got[off], z, r, a, what)
    rest = np.ones(n_arena, bool)
    rest[off] = False
    assert np.all(got[rest] == np.float32(SENTINEL)), '%s: an element outside the described rows was written' % what
    return arena


# --------------------------------------------------------------------------------------- dv_fill_normal_rows
def _default_spec(kind):
    return M.ModelSpec(kind=kind)


@pytest.mark.parametrize('row0', [0, 450])
@pytest.mark.parametrize('kind', ['drvae', 'vfae', 'pvae'])
def test_rows_real_descriptor_tables(kind, row0, K, dev):
    """``plan.noise_desc`` of the cfg-2-sized plans (150 rows), first rank and fourth, whole arena"""
    spec = _default_spec(kind)
    eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True), dev)
    eng.row0 = row0
    p = set_batch(eng, M.make_batch(spec, 150, seed=5), dev)
    desc = p.noise_desc.cpu().numpy()
    assert desc[:, 3].min() == row0 and desc[:, 3].max() == row0 + 149
    draw_and_check(K, dev, desc, p.noise.numel(), 12345, 2, '%s plan, row0 %d' % (kind, row0))
    # ... and the launch as the engine makes it, into the plan's own arena
    p.noise.fill_(SENTINEL)
    eng.seed = 999
    eng.draw_noise()
    torch.cuda.synchronize()
    off, z, r, a = P.rows_table(desc, 999, 0)
    assert np.array_equal(np.sort(off), np.arange(p.noise.numel()))
    check(p.noise.cpu().numpy()[off], z, r, a, '%s draw_noise, row0 %d' % (kind, row0))
    assert eng.rng_ctr.tolist() == [1, 0]


def test_rows_every_alignment_and_width(K, dev):
    """widths 1 .. 20000 packed back to back, so that rows start on every alignment (the float4 store path and the scalar
    one), gaps between some rows: nothing outside a row is written"""
    widths = [1, 2, 3, 5, 7, 13, 978, 980, 20000]
    rows, off = [], 0
    for rep in range(4):
        for i, w in enumerate(widths):
            off += ((rep + i) - off) % 4        # (a gap of 0 .. 3 elements that must keep the sentinel)
            rows.append([off, w, 3 + rep, 1000 * rep + i])
            off += w
    desc = np.asarray(rows)
    for w in widths:
        assert set((desc[desc[:, 1] == w, 0] % 4).tolist()) == {0, 1, 2, 3}, w       # every alignment, every width
    assert np.any(desc[1:, 0] == desc[:-1, 0] + desc[:-1, 1]) and np.any(desc[1:, 0] > desc[:-1, 0] + desc[:-1, 1])
    draw_and_check(K, dev, desc, off + 5, 2024, 7, 'packed widths')
    # the same rows in another order and at other offsets hold the same values (a value is keyed, not placed)
    a1 = draw_and_check(K, dev, desc, off + 5, 2024, 7, 'packed widths again')
    d2 = desc[::-1].copy()
    d2[:, 0] = np.concatenate([[0], np.cumsum(d2[:-1, 1])]) + 2
    a2 = draw_and_check(K, dev, d2, off + 5, 2024, 7, 'packed widths, reversed')
    for (o1, w, _, _), (o2, _, _, _) in zip(desc.tolist(), d2[::-1].tolist()):
        assert torch.equal(a1[o1:o1 + w], a2[o2:o2 + w])


def test_rows_beyond_one_grid_pass_and_parked_grid(K, dev):
    """70 000 rows of width 8: more rows than one pass of the grid (4096 workgroups x 4 waves); then the parked launch's
    512-workgroup grid on the same table, its flag already published: the same values"""
    n = 70000
    r = np.arange(n)
    desc = np.stack([8 * r, np.full(n, 8), 5 + r % 3, r * 7], 1)
    a1 = draw_and_check(K, dev, desc, 8 * n, 31337, 11, '70 000 rows')
    flag = torch.tensor([10], dtype=torch.int32, device=dev)         # published: flag >= ctr + add
    ctr = torch.tensor([6], dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)
    a2 = draw_and_check(K, dev, desc, 8 * n, 31337, 11, '70 000 rows, parked grid', park=(flag, ctr, err, 1))
    assert int(err[0]) == 0
    assert torch.equal(a1, a2)


def test_rows_uniform_of_exactly_one(K, dev):
    """the three positions where a word is >= 2^32 - 128 (tests/test_philox_ref.py re-derives them): exact zeros there,
    everything finite, the rest within the bound"""
    desc = np.asarray([[i * 980 + i, 978, 0, g] for i, (g, _, _) in enumerate(EDGE_POSITIONS)])
    arena = draw_and_check(K, dev, desc, 3 * 981 + 3, EDGE_SEED, 0, 'edge rows').cpu().numpy()
    for i, (g, blk, word) in enumerate(EDGE_POSITIONS):
        row = arena[desc[i, 0]:desc[i, 0] + 978]
        assert np.flatnonzero(row == 0).tolist() == [4 * blk + word, 4 * blk + word + 1]
        assert np.all(np.abs(row) <= P.R_MAX)


@pytest.mark.parametrize('seed', [0, 12345, 2 ** 32 + 5, 2 ** 63 + 9])
def test_rows_counters_and_keys(seed, K, dev):
    """event low / high word (key), the carry of dv_counter_add into the high word, 64-bit seeds, draw ids and global rows
    up to 2^31 - 1, no counter at all"""
    big = 2 ** 31 - 1
    desc = np.asarray([[0, 40, 0, 0], [40, 37, big, 1], [80, 33, 1, big], [120, 50, big, big], [172, 4, big - 1, big - 1]])
    for event in (5, (1 << 32) | 5, 0xFFFFFFFF):
        draw_and_check(K, dev, desc, 180, seed, event, 'seed %d event %#x' % (seed, event))
    ctr = torch.tensor([-1, 0], dtype=torch.int32, device=dev)       # (0xFFFFFFFF, 0)
    K.counter_add(ctr, 1)
    torch.cuda.synchronize()
    assert ctr.tolist() == [0, 1]
    draw_and_check(K, dev, desc, 180, seed, 1 << 32, 'seed %d event 2^32 by dv_counter_add' % seed, ctr_dev=ctr)
    draw_and_check(K, dev, desc, 180, seed, 0, 'seed %d, no counter' % seed, ctr_dev=None)


# -------------------------------------------------------------------------------------------- dv_fill_normal
@pytest.mark.parametrize('n', [1, 3, 4, 5, 2 ** 20 + 3])
def test_flat(n, K, dev):
    out = torch.full((n + 8,), SENTINEL, device=dev)
    ctr = torch.tensor([1000, 2], dtype=torch.int32, device=dev)
    K.fill_normal(out[:n], 2 ** 40 + 17, ctr)
    torch.cuda.synchronize()
    check(out[:n], *P.flat(n, 2 ** 40 + 17, (2 << 32) + 1000), what='flat n = %d' % n)
    assert bool((out[n:] == SENTINEL).all())
    K.fill_normal(out[:n], 4321, None)
    torch.cuda.synchronize()
    check(out[:n], *P.flat(n, 4321, 0), what='flat n = %d, no counter' % n)
    assert bool((out[n:] == SENTINEL).all())


def test_flat_counter_carries_into_the_high_word(K, dev):
    out = torch.zeros(256, device=dev)
    ctr = torch.tensor([0xFFFFFFF0 - (1 << 32), 0], dtype=torch.int32, device=dev)
    K.fill_normal(out, 77, ctr)
    torch.cuda.synchronize()
    check(out, *P.flat(256, 77, 0xFFFFFFF0), what='flat, block index carries')
    # (blocks 16 .. 63 have counter (i - 16, 1, 0, 0))
    assert P.flat(256, 77, 0xFFFFFFF0)[0][64] == P.normals(P.philox4x32_10(0, 1, 0, 0, 77, 0))[0][0]


# ------------------------------------------------------------------------- Philox-driven steps against the oracle
def _eager(e, t):
    e.train_step()


def _captured(e, t):
    if t == 0:
        e.capture()
    e.replay()


def _eager_then_captured(e, t):
    if t < 2:
        e.train_step()
    else:
        if t == 2:
            e.capture()          # (the noise buffer holds event 1's draws and the warm-up's: the first replay draws event 2's)
        e.replay()


def _model(name):
    if name.startswith('default_'):
        spec = _default_spec(name[8:])
        return spec, M.make_batch(spec, 150, seed=5)
    case = C.model_case(name)
    return case['spec'], case['batch']


MODELS = ['default_drvae', 'default_vfae', 'default_pvae', 'tiny_drvae', 'tiny_vfae', 'tiny_pvae']


@pytest.mark.parametrize('mode', ['eager', 'captured', 'eager_then_captured', 'universal'])
@pytest.mark.parametrize('name', MODELS)
def test_philox_train_steps_match_oracle(name, mode, dev):
    """Four train steps on the device's own draws against ``RefTrainer`` fed ``philox_ref.step_noise(event = t)``: step t
    consumed event t's noise -- (a) eager, (b) captured in the schedule the engine picks, (c) two eager steps, then capture and
    replay (the replay must draw for its own counter first), (d) the universal plan (eager, then captured).  Afterwards the
    noise arena holds event 4's draws where the schedule draws ahead (the dual-graph step: its side chain draws step t + 1's
    noise during step t -- every model here once captured, their steps being latency-bound) and event 3's, the last
    step's own, where it does not (every eager step)."""
    spec, batch = _model(name)
    drive = {'eager': _eager, 'captured': _captured, 'eager_then_captured': _eager_then_captured,
             'universal': _eager_then_captured}[mode]
    eng = philox_steps_vs_oracle(spec, batch, dev, drive, universal=(mode == 'universal'))
    eng.join_side()
    torch.cuda.synchronize()
    eng.check_sync()
    assert eng.noise_ahead == (mode != 'eager') and (eng._side_graph is not None) == (mode != 'eager')
    event = 4 if eng.noise_ahead else 3
    off, z, r, a = P.rows_table(eng.plan.noise_desc.cpu().numpy(), eng.seed, event)
    assert np.array_equal(np.sort(off), np.arange(eng.plan.noise.numel()))
    check(eng.plan.noise.cpu().numpy()[off], z, r, a, '%s %s: arena after 4 steps = event %d' % (name, mode, event))


@pytest.mark.parametrize('kind', ['drvae', 'vfae', 'pvae'])
def test_philox_second_rank_matches_oracle(kind, dev):
    """one rank of two: rows 150 .. 299 of a 300-row batch (``row0`` = 150, global normalisers) draw what
    ``step_noise(n_rows=300)`` holds for those rows -- forward losses against the oracle's on that slice, two events"""
    spec = _default_spec(kind)
    n, lo = 300, 150
    full = M.make_batch(spec, n, seed=5)
    counts = (n, int(full['has_x2'].sum()), int(full['has_y'].sum()))
    shard = {k: v[lo:] for k, v in full.items()}
    params = M.init_params(spec, 3, as_numpy=True)
    eng, _ = make_engine(spec, params, dev)
    eng.seed, eng.row0 = 77, lo
    set_batch(eng, shard, dev, counts=counts)
    tr = M.RefTrainer(spec, M.init_params(spec, 3))
    for event in range(2):
        eng.training = True
        eng.draw_noise()
        eng.forward()
        ref, _ = tr.loss(shard, M.slice_noise(P.step_noise(spec, n, 77, event), lo, n), training=True, counts=counts)
        for k, v in eng.losses().items():
            np.testing.assert_allclose(v, float(ref[k].detach()), rtol=2e-4, atol=2e-5, err_msg='%s %s event %d' % (kind, k, event))
    assert eng.rng_ctr.tolist() == [2, 0]


@pytest.mark.parametrize('kind', ['drvae', 'vfae', 'pvae'])
def test_philox_evaluation_draws_the_same_latents(kind, dev):
    """evaluation draws only the latent rows of the table (``desc[B + Np:]``): the input-noise rows stay untouched, the rest
    are the reference's numbers, and the eval loss is the oracle's on the latent draws of ``step_noise``"""
    spec = _default_spec(kind)
    batch = M.make_batch(spec, 150, seed=5)
    params = M.init_params(spec, 3, as_numpy=True)
    eng, _ = make_engine(spec, params, dev)
    eng.seed = 31
    p = set_batch(eng, batch, dev)
    eng.rng_ctr.copy_(torch.tensor([6, 0], dtype=torch.int32))
    p.noise.fill_(SENTINEL)
    eng.training = False
    eng.draw_noise()
    eng.forward()
    got = eng.losses()
    torch.cuda.synchronize()
    tr = M.RefTrainer(spec, M.init_params(spec, 3))
    ref, _ = tr.loss(batch, P.step_noise(spec, 150, 31, 6), training=False)
    for k, v in got.items():
        np.testing.assert_allclose(v, float(ref[k].detach()), rtol=2e-4, atol=2e-5, err_msg='%s %s' % (kind, k))
    n_in = (p.B + p.Np) * spec.dim_x
    arena = p.noise.cpu().numpy()
    assert np.all(arena[:n_in] == np.float32(SENTINEL))
    off, z, r, a = P.rows_table(p.noise_desc.cpu().numpy()[p.B + p.Np:], 31, 6)
    assert np.array_equal(np.sort(off), np.arange(n_in, arena.size))
    check(arena[off], z, r, a, '%s evaluation draw' % kind)
    assert eng.rng_ctr.tolist() == [7, 0]
