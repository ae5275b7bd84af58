"""CPU: is tests/philox_ref.py Philox4x32-10, and is the SPECIFIED keying of the train step's noise sound?

The GPU test (tests/test_gpu_philox.py) ties dv_fill_normal / dv_fill_normal_rows to this reference element by element,
so the distribution and independence checks run here, on the reference: they test the design (counter layout and key).
Every statistical threshold is the statistic's own quantile at a false-alarm rate of 1e-6; nothing is tuned.
"""
import math

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests import philox_ref as P
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine, set_batch

# (global row, col // 4, word) of draw id 0, seed 77, event 0, width 978 where the word is >= 2^32 - 128: the uniform is
# exactly 1.0f there, the radius 0 and the pair of normals exactly zero (found by a search over 164 000 rows)
EDGE_POSITIONS = [(97701, 140, 0), (134338, 77, 2), (160003, 226, 2)]
EDGE_SEED = 77


# ------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_known_answers(ctr, key, want):
    """the published test vectors of Philox4x32-10 (Random123 kat_vectors)"""
    got = P.philox4x32_10(*ctr, *key)
    assert all(w.dtype == np.uint32 for w in got)
    assert ' '.join('%08x' % int(w) for w in got) == want
    # ... vectorised: the same answers inside an array of counters
    c = [np.array([1, v, 2], dtype=np.uint64) for v in ctr]
    got = P.philox4x32_10(*c, *key)
    assert ' '.join('%08x' % int(w[1]) for w in got) == want
    assert len({tuple(int(w[i]) for w in got) for i in range(3)}) == 3


def test_uniform_mapping_at_its_ends():
    """specified behaviour: u = (float32(x) + 0.5f) * 2^-32 in fp32 is never 0 and IS exactly 1 for the top 128 words"""
    assert P.u01(0).dtype == np.float32
    assert float(P.u01(0)) == 2.0 ** -33 > 0
    assert P.R_MAX == math.sqrt(-2 * math.log(2.0 ** -33)) and 6.7637 < P.R_MAX < 6.7638
    top = np.arange(2 ** 32 - 4096, 2 ** 32, dtype=np.uint64).astype(np.uint32)
    u = P.u01(top)
    assert np.array_equal(u == np.float32(1.0), top.astype(np.int64) >= 2 ** 32 - 128)
    assert float(u.max()) == 1.0 and float(P.u01(2 ** 32 - 129)) == 1.0 - 2.0 ** -24
    assert np.all(np.diff(P.u01(np.linspace(0, 2 ** 32 - 1, 100001).astype(np.uint32)).astype(np.float64)) >= 0)
    # the transform at both ends: the largest radius, and an exact zero pair where u == 1
    z, r, a = P.normals([np.uint32(0), np.uint32(0), np.uint32(2 ** 32 - 1), np.uint32(12345)])
    assert r[0] == r[1] == P.R_MAX and abs(z[0]) <= P.R_MAX
    assert r[2] == r[3] == 0.0 and z[2] == 0.0 and z[3] == 0.0
    assert np.all(np.isfinite(z))
    # lanes 0, 1 share radius and angle (words 0, 1); lanes 2, 3 those of words 2, 3
    assert a[0] == a[1] == 2 * math.pi * 2.0 ** -33 and a[2] == a[3]
    w = [np.uint32(v) for v in (0x12345678, 0x9abcdef0, 0x0fedcba9, 0x87654321)]
    u = [float(P.u01(v)) for v in w]
    z = P.normals(w)[0]
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    np.testing.assert_allclose(z, want, rtol=1e-14, atol=1e-15)


def test_edge_positions_of_the_gpu_test():
    """the three positions tests/test_gpu_philox.py uses for "u == 1 exactly", re-derived from the reference alone"""
    for grow, blk, word in EDGE_POSITIONS:
        w = P.philox4x32_10(blk, grow, 0, 0, EDGE_SEED, 0)
        assert int(w[word]) >= 2 ** 32 - 128
        z, r, _ = P.row_draws([grow], 978, 0, EDGE_SEED, 0)
        cols = 4 * blk + word + np.arange(2)
        assert np.all(r[0, cols] == 0) and np.all(z[0, cols] == 0)
        assert np.count_nonzero(z[0] == 0) == 2


def test_table_and_flat_layouts():
    """rows_table / flat against the scalar definition, element by element, at a few positions"""
    seed, event = (7 << 32) | 11, (3 << 32) | 5
    desc = np.array([[10, 7, 4, 1000], [0, 3, 2, 2 ** 31 - 1], [40, 9, 2 ** 31 - 1, 3]])
    off, z, r, a = P.rows_table(desc, seed, event)
    assert off.tolist() == list(range(10, 17)) + [0, 1, 2] + list(range(40, 49))
    i = 0
    for o, w, d, g in desc.tolist():
        for c in range(w):
            ws = P.philox4x32_10(c // 4, g, d, 5, 11, 7 ^ 3)
            zz, rr, aa = P.normals(ws)
            assert (z[i], r[i], a[i]) == (zz[c % 4], rr[c % 4], aa[c % 4])
            i += 1
    zf = P.flat(11, seed, 0xFFFFFFFE)[0]
    for i in range(11):
        ctr = 0xFFFFFFFE + i // 4
        assert zf[i] == P.normals(P.philox4x32_10(ctr & 0xffffffff, ctr >> 32, 0, 0, 11, 7))[0][i % 4]
    # the header's warning: dv_fill_normal(seed, ctr < 2^32) IS the row-keyed stream (row 0, draw 0, event 0)
    assert np.array_equal(P.flat(64, 99, 0)[0], P.row_draws([0], 64, 0, 99, 0)[0][0])


# ------------------------------------------------------------ distribution and independence of the specified stream
N_SIDE = 1024
N = N_SIDE * N_SIDE
SEED = 12345


def _table(seed=SEED, event=0, draw=0, row0=0):
    return P.row_draws(row0 + np.arange(N_SIDE), N_SIDE, draw, seed, event)[0]


def _corr(a, b):
    a, b = a.reshape(-1) - a.mean(), b.reshape(-1) - b.mean()
    return float(a @ b / math.sqrt((a @ a) * (b @ b)))


def _poisson_interval(mu, alpha=1e-6):
    """[lo, hi]: the smallest interval with P(X < lo) <= alpha / 2 and P(X > hi) <= alpha / 2"""
    pmf = [math.exp(-mu + k * math.log(mu) - math.lgamma(k + 1)) for k in range(int(mu + 20 * math.sqrt(mu) + 40))]
    cdf = np.cumsum(pmf)
    lo = int(np.searchsorted(cdf, alpha / 2, side='right'))          # first k with P(X <= k) > alpha / 2
    hi = int(np.searchsorted(cdf, 1 - alpha / 2, side='left'))       # first k with P(X <= k) >= 1 - alpha / 2
    return lo, hi


@pytest.fixture(scope='module')
def base_table():
    return _table()


def test_stream_is_standard_normal(base_table):
    z = np.sort(base_table.reshape(-1))
    cdf = 0.5 * (1 + torch.erf(torch.from_numpy(z) / math.sqrt(2))).numpy()
    i = np.arange(N)
    ks = max(float(np.max((i + 1) / N - cdf)), float(np.max(cdf - i / N)))
    bound = math.sqrt(math.log(2e6) / (2 * N))            # Dvoretzky-Kiefer-Wolfowitz: P(D > x) <= 2 exp(-2 n x^2) = 1e-6
    print('KS distance %.3g (bound %.3g)' % (ks, bound))
    assert ks < bound
    assert np.abs(z).max() <= P.R_MAX
    sf = lambda k: math.erfc(k / math.sqrt(2))           # P(|z| > k)
    for k, want in ((3, (2575, 3095)), (4, (31, 110)), (5, (0, 7))):
        lo, hi = _poisson_interval(N * sf(k))
        n = int(np.count_nonzero(np.abs(z) > k))
        print('|z| > %d: %d in [%d, %d]' % (k, n, lo, hi))
        assert (lo, hi) == want
        assert lo <= n <= hi


@pytest.mark.parametrize('what', ['event', 'draw', 'rank', 'seed', 'event_hi'])
def test_neighbouring_streams_are_independent(base_table, what):
    """the next event, the next draw id, the next rank's rows, the next seed, and the key's high word (event + 2^32)"""
    other = {'event': lambda: _table(event=1), 'draw': lambda: _table(draw=1), 'rank': lambda: _table(row0=N_SIDE),
             'seed': lambda: _table(seed=SEED + 1), 'event_hi': lambda: _table(event=1 << 32)}[what]()
    c = max(abs(_corr(base_table, other)), abs(_corr(base_table ** 2, other ** 2)))
    print('%s: |corr| %.3g (bound %.3g)' % (what, c, 5 / math.sqrt(N)))
    assert c < 5 / math.sqrt(N)
    assert not np.any(base_table == other)


def test_stream_is_independent_within_a_table(base_table):
    t = base_table
    lanes = t.reshape(N_SIDE, N_SIDE // 4, 4)
    bound4 = 5 / math.sqrt(N / 4)
    worst = 0.0
    for i in range(4):
        for j in range(i + 1, 4):       # (Box-Muller pairs share a radius: uncorrelated all the same, squares too)
            worst = max(worst, abs(_corr(lanes[..., i], lanes[..., j])), abs(_corr(lanes[..., i] ** 2, lanes[..., j] ** 2)))
    print('lanes: |corr| %.3g (bound %.3g)' % (worst, bound4))
    assert worst < bound4
    for name, a, b in (('rows', t[:-1], t[1:]), ('columns', t[:, :-1], t[:, 1:]), ('blocks', lanes[:, :-1], lanes[:, 1:])):
        c = max(abs(_corr(a, b)), abs(_corr(a ** 2, b ** 2)))
        bound = 5 / math.sqrt(a.size)
        print('adjacent %s: |corr| %.3g (bound %.3g)' % (name, c, bound))
        assert c < bound


# ------------------------------------------------------------------- no two draws of a step share a stream
def _universal_ok(spec):      # (``FusedStep.universal_ok``)
    return spec.type_y != 'cont' and not (spec.kind == 'vfae' and not spec.semi_supervised) and not spec.use_s


def _plan_cases():
    out = [(n, C.model_case(n)['spec'], C.model_case(n)['batch']) for n in C.SMALL_MODEL_CASES]
    for kind in ('drvae', 'vfae', 'pvae'):
        spec = M.ModelSpec(kind=kind)
        out.append(('default_' + kind, spec, M.make_batch(spec, 150, seed=5)))
    return [c + (u,) for c in out for u in (False, True) if not u or _universal_ok(c[1])]


@pytest.mark.parametrize('name,spec,batch,universal', _plan_cases(),
                         ids=[c[0] + ('-universal' if c[3] else '') for c in _plan_cases()])
def test_no_two_draws_of_a_step_share_a_stream(name, spec, batch, universal, monkeypatch):
    kernel_ref.install(monkeypatch)
    B = len(batch['has_y'])
    pairs = {}
    for row0 in (0, B):
        eng, _ = make_engine(spec, M.init_params(spec, 1, as_numpy=True))
        assert eng.universal_ok() == _universal_ok(spec)
        eng.universal, eng.row0 = universal, row0
        p = set_batch(eng, batch)
        assert p.universal == universal
        desc = p.noise_desc.numpy().astype(np.int64)
        assert desc.shape[0] > 0
        ids = list(zip(desc[:, 2].tolist(), desc[:, 3].tolist()))
        assert len(set(ids)) == len(ids), 'two rows of one step draw from the same (draw id, global row)'
        assert desc[:, 3].min() >= row0 and desc[:, 3].max() < row0 + B and desc[:, 2].min() >= 0
        cover = np.zeros(p.noise.numel() + 1, np.int64)        # every element of the arena is drawn exactly once
        np.add.at(cover, desc[:, 0], 1)
        np.add.at(cover, desc[:, 0] + desc[:, 1], -1)
        assert desc[:, 1].min() > 0 and desc[:, 0].min() >= 0 and (desc[:, 0] + desc[:, 1]).max() <= p.noise.numel()
        assert np.all(np.cumsum(cover)[:-1] == 1)
        pairs[row0] = set(ids)
    assert not (pairs[0] & pairs[B]), 'two ranks of one step draw from the same (draw id, global row)'


# ------------------------------------------------------------------- the event bookkeeping, without a GPU
def philox_steps_vs_oracle(spec, batch, dev, drive, n_steps=4, seed=4242, universal=False, param_seed=11):
    """``n_steps`` train steps on the engine's OWN draws against the oracle fed philox_ref.step_noise(event = t): the
    losses after every step (rtol 2e-4, atol 2e-5: those of the injected-noise comparisons), at the end the parameters
    norm-wise (2e-3) and the Philox counter == the number of steps.  ``drive(eng, t)`` runs step t.  -> engine"""
    B = len(batch['has_y'])
    params = M.init_params(spec, param_seed, as_numpy=True)
    tr = M.RefTrainer(spec, M.init_params(spec, param_seed))
    eng, arena = make_engine(spec, params, dev)
    eng.seed, eng.universal = seed, universal
    p = set_batch(eng, batch, dev)
    assert p.universal == universal
    true_slot = None
    if universal:
        true_slot = np.where(np.asarray(batch['has_y']).reshape(-1) != 0, np.asarray(batch['y']).reshape(-1), -1)
    for t in range(n_steps):
        ref, _ = tr.step(batch, P.step_noise(spec, B, seed, t, true_slot=true_slot))
        drive(eng, t)
        got = eng.losses()
        for k, v in got.items():
            np.testing.assert_allclose(v, float(ref[k].detach()), rtol=2e-4, atol=2e-5, err_msg='%s %s step %d' % (spec.kind, k, t))
    for k in arena.shapes:
        a, b = arena.p(k).cpu().numpy().ravel(), tr.params[k].detach().numpy().ravel()
        err = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)
        assert err < 2e-3, '%s param %s: %g' % (spec.kind, k, err)
    assert eng.rng_ctr.cpu().tolist() == [n_steps, 0]
    assert eng.iters == n_steps
    return eng


@pytest.mark.parametrize('name,universal', [('tiny_drvae', False), ('tiny_vfae', False), ('tiny_pvae', False),
                                            ('tiny_drvae_cont', False), ('tiny_drvae', True), ('tiny_vfae', True),
                                            ('tiny_pvae', True)])
def test_cpu_engine_philox_steps_match_oracle(name, universal, monkeypatch):
    """draw_noise / optimizer_step / _rng_pending: step t of the CPU engine trains on event t's draws"""
    kernel_ref.install(monkeypatch)
    case = C.model_case(name)
    eng = philox_steps_vs_oracle(case['spec'], case['batch'], 'cpu', lambda e, t: e.train_step(), universal=universal)
    # the arena still holds the last step's draws (event 3), every element
    off, z, _, _ = P.rows_table(eng.plan.noise_desc.numpy(), eng.seed, 3)
    want = np.zeros(eng.plan.noise.numel(), np.float32)
    want[off] = z.astype(np.float32)
    assert np.array_equal(eng.plan.noise.numpy(), want)
    # evaluation draws the latent rows only -- the same numbers: eval loss == the oracle's on step_noise(event 4)
    ts = None
    if universal:
        b = case['batch']
        ts = np.where(np.asarray(b['has_y']).reshape(-1) != 0, np.asarray(b['y']).reshape(-1), -1)
    tr = M.RefTrainer(case['spec'], {k: eng.arena.p(k).clone().requires_grad_() for k in eng.arena.shapes})
    tr.iters = eng.iters
    ref, _ = tr.loss(case['batch'], P.step_noise(case['spec'], len(case['batch']['has_y']), eng.seed, 4, true_slot=ts), training=False)
    eng.training = False
    eng.draw_noise()
    eng.forward()
    for k, v in eng.losses().items():
        np.testing.assert_allclose(v, float(ref[k].detach()), rtol=2e-4, atol=2e-5, err_msg=k)
    assert eng.rng_ctr.tolist() == [5, 0]
