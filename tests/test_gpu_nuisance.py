"""-m gpu: the nuisance variable carried on the device.  Kernel level: ``dv_nuisance_feed`` and the grouped MMD penalty
(``dv_mmd_grouped_fwd`` / ``_bwd``) against fp64 numpy written from the formulas of include/drvae_hip.h
(tests/nuisance_cases.py).  Engine level: an epoch of ``DeviceBatcher(carry_s=True)`` through ONE captured step against
host-fed steps, the random-feature path recomputed from the buffers it leaves behind, launch counts, ``fit``."""
import math

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import nuisance_cases as NC
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine

pytestmark = pytest.mark.gpu

VALUE_RTOL, GRAD_RTOL, GRAD_ATOL = 5e-4, 5e-3, 5e-6          # tests/test_gpu_kernels.py::test_mmd_rff


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('dim_s', [2, 3])
@pytest.mark.parametrize('kind', ['drvae', 'vfae'])          # with / without pairs
def test_nuisance_feed_kernel(kind, dim_s, dev):
    import drvae_amd.kernels as K
    spec, big, ds = NC.dataset(kind, dim_s, dev)
    eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True), dev)
    rs = np.random.RandomState(dim_s)
    tab = rs.randint(0, 400, (5, 24))
    hx, hy = big['has_x2'].reshape(-1)[tab[0]], big['has_y'].reshape(-1)[tab[0]]
    s = big['s'].reshape(-1)
    i0 = torch.from_numpy(tab[0]).to(dev)
    host = eng.set_batch(ds.x1[i0], ds.x2[i0], ds.y[i0], hx, hy, s=s[tab[0]])
    eng.carry_s = True
    p = eng.set_batch(ds.x1[i0], ds.x2[i0], ds.y[i0], hx, hy, s=ds.s[i0])
    assert p is not host and p.carry_s and not host.carry_s and (p.Np > 0) == (kind == 'drvae')
    pairs = p.pair_host
    B, L = 24, spec.L
    table = torch.from_numpy(tab).to(dev).to(torch.int32)
    s32 = ds.s.reshape(-1).to(torch.int32)
    ctr, base = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for step, b0 in ((7, 7), (9, 7), (40, 7), (3, 7)):          # batch 0, in the middle, clamped past the end, clamped below
        ctr.fill_(step)
        base.fill_(b0)
        for t in (p.SOHe, p.SOHd):
            t.fill_(-1.0)
        K.nuisance_feed(p.SOHe, p.SOHd, p.s_cls, s32, table=table, n_batches=5, ctr=ctr, base=base,
                        pair_rows=p.pair_idx if p.Np else None, L=L)
        b = min(max(step - b0, 0), 4)
        e, d, c = NC.feed_ref(s, tab, step - b0, pairs, B, L, dim_s)
        assert np.array_equal(p.SOHe.cpu().numpy(), e) and np.array_equal(p.SOHd.cpu().numpy(), d)
        assert np.array_equal(p.s_cls.cpu().numpy(), c)
        host.set_s_device(ds.s.reshape(-1)[torch.from_numpy(tab[b]).to(dev)])      # today's device route, same rows
        assert torch.equal(host.SOHe, p.SOHe) and torch.equal(host.SOHd, p.SOHd)
    # the batch's own class vector (explicit batches)
    p.set_s_device(ds.s.reshape(-1)[torch.from_numpy(tab[2]).to(dev)])
    e, d, c = NC.feed_ref(s[tab[2]], None, 0, pairs, B, L, dim_s)
    assert np.array_equal(p.SOHe.cpu().numpy(), e) and np.array_equal(p.SOHd.cpu().numpy(), d)
    assert np.array_equal(p.s_cls.cpu().numpy(), c)


def _layout(shape):
    """(kind of model, has_x2, has_y, L, Z, R) of the three shapes"""
    if shape == 'tiny':                   # Z = 5, 6 + 9 rows
        return 'vfae', np.zeros(15, int), np.r_[np.ones(6, int), np.zeros(9, int)], 1, 5, 500
    if shape == 'cfg4':                   # config 4: Z = 100, 150 rows, L = 2, two groups
        return 'vfae', np.zeros(150, int), (np.arange(150) % 2), 2, 100, 500
    pat = np.arange(90) % 4               # four DrVAE groups with z2 terms, Z = 128, R no multiple of the 32-column tile
    return 'drvae', (pat >= 2).astype(int), (pat % 2 == 0).astype(int), 2, 128, 333


def _problem(shape, kernel, S, dev, seed=0, cls=None, z=None):
    model, hx, hy, L, Z, R = _layout(shape)
    ptr, rows, src, _ = NC.term_groups(model, hx, hy, L)
    rs = np.random.RandomState(seed)
    B = len(hx)
    n_z = int(rows.max()) + 1
    assert sorted(rows.tolist()) == list(range(n_z))
    cls = rs.randint(0, S, B) if cls is None else cls
    z = rs.standard_normal((n_z, Z)) if z is None else z
    Kc = 1 if S == 2 else S
    T, E = (len(ptr) - 1) * Kc, int(ptr[-1])
    rff = kernel == 'rbf_fourier'
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    zpad = torch.zeros(n_z, (Z + 3) // 4 * 4, device=dev)[:, :Z]
    zpad.copy_(f(z))
    g = dict(z=zpad, dz=torch.full((n_z, Z), float('nan'), device=dev), kind=kernel, R=R if rff else 0, S=S, cls=i(cls),
             grp_ptr=i(ptr), rows=i(rows), src=i(src), max_rows=int(np.diff(ptr).max()), a=1.0 / math.sqrt(Z),
             c=math.sqrt(2.0 / R) if rff else 1.0, w=(1.0 if S == 2 else 1.0 / S) / L, fac=-1.0,
             diff=torch.full((T, R if rff else Z), float('nan'), device=dev),
             cnt=torch.zeros(len(ptr) - 1, S, dtype=torch.int32, device=dev), m2=torch.full((T,), float('nan'), device=dev),
             value=torch.full((1,), float('nan'), device=dev),
             W=f(rs.standard_normal((T, Z, R))) if rff else None, b=f(rs.rand(T, R)) if rff else None,
             theta=torch.zeros(Kc * E, R, device=dev) if rff else None)
    return g, (ptr, rows, src, cls)


def _reference(g, lay):
    ptr, rows, src, cls = lay
    n = lambda t: None if t is None else t.cpu().numpy()
    return NC.mmd_ref(n(g['z']), cls, ptr, rows, src, g['S'], g['kind'], g['w'], g['fac'], n(g['W']), n(g['b']), g['a'], g['c'])


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('kernel', ['rbf_fourier', 'identity'])
@pytest.mark.parametrize('shape', ['tiny', 'cfg4', 'drvae4'])
def test_grouped_mmd_kernels_against_fp64(shape, kernel, S, dev):
    import drvae_amd.kernels as K
    g, lay = _problem(shape, kernel, S, dev, seed=11)
    K.mmd_grouped_fwd(g)
    K.mmd_grouped_bwd(g)
    torch.cuda.synchronize()
    diff, m2, value, dz, theta, cnt = _reference(g, lay)
    got_v, got_dz = float(g['value']), g['dz'].cpu().numpy().astype(np.float64)
    print('grouped MMD %s %s S=%d: value rel err %.3g, gradient max abs err %.3g (max |g| %.3g), diff max abs err %.3g'
          % (shape, kernel, S, abs(got_v - value) / abs(value), np.abs(got_dz - dz).max(), np.abs(dz).max(),
             np.abs(g['diff'].cpu().numpy() - diff).max()))
    assert np.array_equal(g['cnt'].cpu().numpy(), cnt)
    assert value < 0
    np.testing.assert_allclose(got_v, value, rtol=VALUE_RTOL)
    np.testing.assert_allclose(g['m2'].cpu().numpy(), m2, rtol=2 * VALUE_RTOL)
    np.testing.assert_allclose(got_dz, dz, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # deterministic: one writer per element
    keep = (g['value'].clone(), g['dz'].clone(), g['diff'].clone())
    K.mmd_grouped_fwd(g)
    K.mmd_grouped_bwd(g)
    assert all(torch.equal(a, b) for a, b in zip(keep, (g['value'], g['dz'], g['diff'])))


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('kernel', ['rbf_fourier', 'identity'])
def test_grouped_mmd_edge_cases(kernel, S, dev):
    """a term group whose rows all share one class (an empty side) and a term whose difference is exactly zero (two rows
    with identical latent values, one in each class): value 0, gradient 0, everything finite, the other terms as before"""
    import drvae_amd.kernels as K
    model, hx, hy, L, Z, R = _layout('tiny')
    rs = np.random.RandomState(5)
    cls = rs.randint(0, S, 15)
    cls[:S] = np.arange(S)
    g0, lay0 = _problem('tiny', kernel, S, dev, seed=2, cls=cls.copy())
    K.mmd_grouped_fwd(g0)
    K.mmd_grouped_bwd(g0)
    base_dz = g0['dz'].clone()
    # (1) the second group (rows 6..14): one class only
    c1 = cls.copy()
    c1[6:] = 1
    g, lay = _problem('tiny', kernel, S, dev, seed=2, cls=c1)
    K.mmd_grouped_fwd(g)
    K.mmd_grouped_bwd(g)
    diff, m2, value, dz, _, cnt = _reference(g, lay)
    Kc = 1 if S == 2 else S
    assert bool(torch.isfinite(g['dz']).all()) and math.isfinite(float(g['value']))
    assert bool((g['dz'][6:] == 0).all()) and bool((g['m2'][Kc:] == 0).all()) and bool((g['diff'][Kc:] == 0).all())
    assert torch.equal(g['dz'][:6], base_dz[:6])          # the first group: unaffected
    np.testing.assert_allclose(float(g['value']), value, rtol=VALUE_RTOL)
    assert value < 0
    # (2) the first group: two rows, identical latent values, one in each class
    if S == 2:
        hy2 = np.r_[np.ones(2, int), np.zeros(13, int)]
        ptr, rows, src, _ = NC.term_groups('vfae', np.zeros(15, int), hy2, 1)
        c2 = cls.copy()
        c2[:2] = [0, 1]
        g, lay = _problem('tiny', kernel, S, dev, seed=2, cls=c2)
        i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        g.update(grp_ptr=i(ptr), rows=i(rows), src=i(src), max_rows=13)
        g['z'][1].copy_(g['z'][0])
        K.mmd_grouped_fwd(g)
        K.mmd_grouped_bwd(g)
        diff, m2, value, dz, _, cnt = NC.mmd_ref(g['z'].cpu().numpy(), c2, ptr, rows, src, S, kernel, g['w'], g['fac'],
                                                  None if g['W'] is None else g['W'].cpu().numpy(),
                                                  None if g['b'] is None else g['b'].cpu().numpy(), g['a'], g['c'])
        assert float(g['m2'][0]) == 0.0 and bool((g['diff'][0] == 0).all()) and bool((g['dz'][:2] == 0).all())
        assert bool(torch.isfinite(g['dz']).all()) and math.isfinite(float(g['value'])) and value < 0
        np.testing.assert_allclose(float(g['value']), value, rtol=VALUE_RTOL)
        np.testing.assert_allclose(g['dz'].cpu().numpy(), dz, rtol=GRAD_RTOL, atol=GRAD_ATOL)


# ------------------------------------------------------------------------------------------------- engine
def _engines(kind, dim_s, dev, kernel=None, L=2, **over):
    from drvae_amd import data as D
    if kernel is not None:
        over.update(use_MMD=True, mmd_rate=0.7, kernel_MMD=kernel)
    spec, big, ds = NC.dataset(kind, dim_s, dev, L=L, **over)
    params = M.init_params(spec, 3, as_numpy=True)
    bat = D.DeviceBatcher(ds, torch.ones(400), 24, group_counts=NC.group_counts(big), seed=5, carry_s=True)
    fed, a1 = make_engine(spec, params, dev)
    other, a0 = make_engine(spec, params, dev)
    return spec, big, ds, bat, fed, a1, other, a0


@pytest.mark.parametrize('use_mmd', [False, True])
@pytest.mark.parametrize('dim_s', [2, 3])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_epoch_through_one_captured_step_equals_host_fed_steps(kind, dim_s, use_mmd, dev):
    """an epoch of 6 batches through ``begin_epoch(table=...)`` + ONE captured step against a second engine fed the same
    rows and classes from the host (``set_batch(..., s=host)``: today's host-list penalty); every (group, class) side of
    every batch is non-empty, so both paths define the same number"""
    spec, big, ds, bat, fed, a1, host, a0 = _engines(kind, dim_s, dev, kernel='identity' if use_mmd else None)
    tab = NC.epoch_table(big, dim_s, 6)
    NC.assert_every_side_filled(kind, big, tab, dim_s, bat.has_x2 * (kind != 'vfae'), bat.has_y * (kind != 'pvae'))
    bat.bind(fed)
    bat.begin_epoch(n_batches=6, table=torch.from_numpy(tab).to(dev))
    fed.capture()
    for b in range(6):
        fed.replay()
        i = torch.from_numpy(tab[b]).to(dev)
        host.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), bat.has_x2, bat.has_y, s=ds.s[i].cpu())
        host.train_step()
        if use_mmd:
            fed.join_side()
            np.testing.assert_allclose(fed.plan.MMDval.cpu().numpy(), host.plan.MMDval.cpu().numpy(), rtol=2e-5)
            assert float((fed.plan.DZMMD - host.plan.DZMMD).norm() / host.plan.DZMMD.norm()) < 2e-5
            assert float((a1.grad - a0.grad).norm() / a0.grad.norm()) < 2e-5
            lf, lh = fed.losses(), host.losses()
            for k in lf:
                np.testing.assert_allclose(lf[k], lh[k], rtol=1e-4, atol=1e-6)
            assert lh['MMD'] < 0
    torch.cuda.synchronize()
    fed.check_sync()
    assert len(fed._plans) == 1 and fed.iters == 6 and fed.plan.live_feed is not None
    if use_mmd:
        assert float((a1.param - a0.param).norm() / a0.param.norm()) < 1e-4
    else:
        assert torch.equal(a1.param, a0.param)
        assert fed.losses() == host.losses()


def _recompute(p, spec, kind, bat):
    """value and DZMMD of the step just run, in fp64 from what it left behind: the sample rows, W, b, the class vector"""
    g = p.mmd_grouped
    ptr, rows, src, _ = NC.term_groups(kind, bat.has_x2, bat.has_y, spec.L)
    assert np.array_equal(g['grp_ptr'].cpu().numpy(), ptr) and np.array_equal(g['rows'].cpu().numpy(), rows)
    assert np.array_equal(g['src'].cpu().numpy(), src)
    S, L = spec.dim_s, spec.L
    n = lambda t: t.cpu().numpy()
    R, Z = g['W'].shape[2], spec.dim_z1
    assert R == 500
    out = NC.mmd_ref(n(p.ZDEC[:p.o3]), n(p.s_cls), ptr, rows, src, S, 'rbf_fourier', (1.0 if S == 2 else 1.0 / S) / L,
                     -spec.mmd_rate / p.n_tot, n(g['W']), n(g['b']), 1.0 / math.sqrt(Z), math.sqrt(2.0 / R))
    return out[2], out[3]


@pytest.mark.parametrize('kind,dim_s', [('drvae', 3), ('vfae', 2)])
def test_fourier_penalty_recomputed_from_its_buffers(kind, dim_s, dev):
    """rbf_fourier: after an eager step and after replays, value and gradient recomputed in fp64 from ZDEC, the stacked
    W / b and the class vector; consecutive steps draw fresh features with the right moments"""
    spec, big, ds, bat, fed, a1, _, _ = _engines(kind, dim_s, dev, kernel='rbf_fourier')
    tab = NC.epoch_table(big, dim_s, 4, vary=True, seed=3)
    bat.bind(fed)
    p = fed.plan
    bat.feed(torch.from_numpy(tab[0]).to(dev))
    fed.train_step()
    draws = []

    def check(tag):
        fed.join_side()
        torch.cuda.synchronize()
        value, dz = _recompute(p, spec, kind, bat)
        got = p.DZMMD.cpu().numpy().astype(np.float64)
        print('fourier penalty %s %s: value %.6g (fp64 %.6g), gradient max abs err %.3g (max |g| %.3g)'
              % (kind, tag, float(p.MMDval), value, np.abs(got - dz).max(), np.abs(dz).max()))
        assert value < 0
        np.testing.assert_allclose(float(p.MMDval), value, rtol=VALUE_RTOL)
        np.testing.assert_allclose(got, dz, rtol=GRAD_RTOL, atol=GRAD_ATOL)
        draws.append((p.mmd_grouped['W'].cpu().numpy().copy(), p.mmd_grouped['b'].cpu().numpy().copy()))
    check('eager')
    bat.begin_epoch(n_batches=4, table=torch.from_numpy(tab).to(dev))
    fed.capture()
    for b in range(3):
        fed.replay()
        check('replay %d' % b)
        assert np.array_equal(p.s_cls.cpu().numpy(), big['s'].reshape(-1)[tab[b]])
    assert not np.array_equal(draws[-1][0], draws[-2][0]) and not np.array_equal(draws[-1][1], draws[-2][1])
    w = np.concatenate([draws[-1][0].reshape(-1), draws[-2][0].reshape(-1)]).astype(np.float64)
    u = np.concatenate([draws[-1][1].reshape(-1), draws[-2][1].reshape(-1)]).astype(np.float64)
    assert abs(w.mean()) < 5 / math.sqrt(w.size) and abs(w.var() - 1) < 5 * math.sqrt(2.0 / w.size)
    assert abs(u.mean() - 0.5) < 5 * math.sqrt(1 / 12 / u.size) and abs(u.var() - 1 / 12) < 5 * math.sqrt(1 / 180 / u.size)
    assert u.min() >= 0 and u.max() <= 1


def test_one_capture_serves_every_composition(dev):
    """capture once, replay over an epoch whose batches have different compositions of classes (empty sides included),
    release the allocator's cache half-way: equal -- bitwise -- to eager steps on a twin fed the same batches explicitly"""
    spec, big, ds, bat, fed, a1, twin, a0 = _engines('drvae', 3, dev, kernel='identity')
    tab = NC.epoch_table(big, 3, 8, vary=True, seed=1)
    s = big['s'].reshape(-1)
    g0 = np.nonzero((big['has_y'].reshape(-1) == 1) & (big['has_x2'].reshape(-1) == 0) & (s == 0))[0]
    tab[5, :6] = g0[:6]                                  # batch 5: the first data group holds one class only
    assert len({tuple(np.bincount(s[tab[b]], minlength=3)) for b in range(8)}) > 2
    bat.bind(fed)
    twin.carry_s = True
    bat.begin_epoch(n_batches=8, table=torch.from_numpy(tab).to(dev))
    fed.capture()
    for b in range(8):
        if b == 4:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        fed.replay()                                      # (no 'capture again': the plan has no composition signature)
        i = torch.from_numpy(tab[b]).to(dev)
        twin.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), bat.has_x2, bat.has_y, s=ds.s[i])
        twin.train_step()
        assert fed.losses() == twin.losses()
        assert torch.equal(fed.plan.DZMMD, twin.plan.DZMMD)
    torch.cuda.synchronize()
    fed.check_sync()
    assert torch.equal(a1.param, a0.param) and all(np.isfinite(v) for v in fed.losses().values())
    assert not hasattr(fed.plan, 'mmd_sig') and fed._graph_mmd_sig is None and len(fed._plans) == 1


def _captured_launches(eng, monkeypatch):
    from drvae_amd import _lib
    counts = {'n': 0, 'on': False}
    real = _lib.check

    def counting(code, what):
        if counts['on'] and not what.startswith('dv_gemm_set_option'):
            counts['n'] += 1
        return real(code, what)
    monkeypatch.setattr(_lib, 'check', counting)
    real_capture_main = eng._capture_main

    def capture_main(*a, **k):
        counts['on'] = True
        return real_capture_main(*a, **k)
    monkeypatch.setattr(eng, '_capture_main', capture_main)
    eng.capture()
    counts['on'] = False
    monkeypatch.setattr(_lib, 'check', real)
    return counts['n']


def test_launch_count_of_the_penalty(dev, monkeypatch):
    """(captured step with the penalty on this path) - (same model without): one constant, two launches (the grouped
    forward and backward; the random features are two torch launches more), whatever L and the number of classes; a model
    without ``use_s`` has the same step on a batcher that carries s as on one that does not"""
    from drvae_amd import data as D
    MMD_LAUNCHES = 2
    for L, dim_s in ((1, 2), (2, 3)):
        n = {}
        for kernel in (None, 'rbf_fourier'):
            spec, big, ds, bat, fed, _, _, _ = _engines('drvae', dim_s, dev, kernel=kernel, L=L)
            bat.bind(fed)
            bat.begin_epoch(n_batches=2)
            n[kernel] = _captured_launches(fed, monkeypatch)
            fed.replay()
            torch.cuda.synchronize()
            fed.check_sync()
        print('captured launches, L=%d dim_s=%d: %d without, %d with the penalty' % (L, dim_s, n[None], n['rbf_fourier']))
        assert n['rbf_fourier'] - n[None] == MMD_LAUNCHES
    n = []
    for carry in (False, True):
        spec = C.tiny_spec('drvae')
        big = M.make_batch(spec, 400, seed=9)
        t = lambda k: torch.from_numpy(big[k].copy())
        ds = D.DrVAEDataset(t('x1'), t('x2'), t('s'), t('y'), t('has_x2'), t('has_y')).to(dev)
        eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True), dev)
        bat = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, carry_s=carry)
        bat.bind(eng)
        bat.begin_epoch(n_batches=2)
        n.append(_captured_launches(eng, monkeypatch))
    assert n[0] == n[1] > 0


def _s_dataset(kind, n, seed, dim_s, dev):
    from drvae_amd import data as D
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    s = rs.randint(0, dim_s, n)
    x1 = (rs.standard_normal((n, 13)) + 0.8 * (2 * y[:, None] - 1) * (np.arange(13) % 3 == 0) + 0.5 * s[:, None]).astype(np.float32)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    x2 = ((x1 * 0.7 + 0.2) * hx[:, None]).astype(np.float32)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(s), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2), t(s), t(y), t(hx), t(hy))


@pytest.mark.parametrize('kind,dim_s', [('vfae', 2), ('drvae', 3)])
def test_fit_on_a_batcher_that_carries_s(kind, dim_s, tmp_path, dev):
    from drvae_amd import data as D
    from tests.test_fit import _loader, _tiny_model
    kw = dict(device='cuda', dim_s=dim_s, use_s=True, use_MMD=True, kernel_MMD='rbf_fourier', mmd_rate=1.0, epochs=1)
    model = _tiny_model(kind, **kw)
    tr, va = _s_dataset(kind, 128, 1, dim_s, 'cuda'), _s_dataset(kind, 32, 2, dim_s, 'cuda')
    w = D.compute_balanced_weights(np.arange(128) % 5)
    fn = str(tmp_path / 'best.pth')
    batcher = D.DeviceBatcher(tr, w, 32, seed=3, carry_s=True)
    eng = model.engine()
    seen, real_replay = [], eng.replay

    def replay(*a, **k):
        seen.append(eng.plan.live_feed is not None and eng.plan.carry_s)
        return real_replay(*a, **k)
    eng.replay = replay
    cmpl = []
    for epoch in range(6):
        model.fit(batcher, _loader(va, 8), add_noise=True, verbose=False, early_stop=False, model_filename=fn)
        batcher.bind(eng)
        eng.join_side()
        sums = eng.loss_sum.cpu().numpy().astype(np.float64) / len(batcher)
        from drvae_amd.plan import LOSS_IDX
        assert np.isfinite(sums).all() and sums[LOSS_IDX['MMD']] < 0
        cmpl.append(sums[LOSS_IDX['CMPL']])
    assert model.finished_training_iters == 6 * 4 and len(seen) >= 6 * 4 and all(seen)
    assert cmpl[-1] < cmpl[0], cmpl
    assert len(eng._captures) == 0 and eng._graph_key == batcher._bound_plan.key
    # the default batcher keeps today's refusals; sampler mode is refused with carry_s too
    with pytest.raises(NotImplementedError):
        _tiny_model(kind, **kw).fit(D.DeviceBatcher(tr, w, 32, seed=3), _loader(va, 8), add_noise=True, verbose=False,
                                    early_stop=False, model_filename=fn)
    with pytest.raises(NotImplementedError):
        _tiny_model(kind, **kw).fit(D.DeviceBatcher(tr, w, 32, seed=3, mode='sampler', carry_s=True), _loader(va, 8),
                                    add_noise=True, verbose=False, early_stop=False, model_filename=fn)
