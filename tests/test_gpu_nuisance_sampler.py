"""-m gpu: the nuisance variable on sampler-mode device batches.  Kernel level: ``dv_mmd_masked_fwd`` / ``_bwd`` against the
fp64 numpy reference written from the header (tests/nuisance_masked_cases.py).  Engine level: an epoch of
``DeviceBatcher(mode='sampler', carry_s='masked')`` through ONE captured step against host-fed steps, the random-feature path
recomputed from the buffers a step leaves behind, launch counts, the bucketed feed, ``fit``."""
import collections
import math

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import nuisance_cases as NC
from tests import nuisance_masked_cases as MC
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine
from tests.test_gpu_nuisance import GRAD_ATOL, GRAD_RTOL, VALUE_RTOL

pytestmark = pytest.mark.gpu

GUARD = 7.0


# ------------------------------------------------------------------------------------------------ kernels
def _layout(shape):
    """(model, B, Np, L, Z, R) of the three shapes"""
    if shape == 'tiny':                   # Z no multiple of 4: the scalar load path
        return 'vfae', 15, 0, 1, 5, 500
    if shape == 'drvae4':                 # four groups, z2 lists over fewer pair slots than rows, R no multiple of the column tile
        return 'drvae', 90, 48, 2, 128, 333
    return 'vfae', 260, 0, 1, 8, 16       # a list longer than one 256-thread counting pass


def _guarded(rows, cols, dev, fill, pad=False, dtype=torch.float32):
    """a (rows, cols) view with a guard row in front and behind (and pad columns): (view, whole buffer)"""
    width = (cols + 3) // 4 * 4 + 4 if pad else cols
    big = torch.full((rows + 2, width), GUARD, device=dev, dtype=dtype)
    view = big[1:-1, :cols]
    view.fill_(fill)
    return view, big


def _guards_intact(view, big):
    rows, cols = view.shape
    ok = bool((big[0] == GUARD).all()) and bool((big[-1] == GUARD).all())
    return ok and (big.shape[1] == cols or bool((big[1:-1, cols:] == GUARD).all()))


def _problem(shape, kernel, S, dev, seed=0, n_ds=300):
    model, B, Np, L, Z, R = _layout(shape)
    rs = np.random.RandomState(seed)
    Kc, G = (1 if S == 2 else S), MC.GROUPS[model]
    n_lists = L * (2 if Np else 1)
    T, n_z = n_lists * G * Kc, L * (B + Np)
    rff = kernel == 'rbf_fourier'
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    nan = float('nan')
    zpad = torch.zeros(n_z, (Z + 3) // 4 * 4, device=dev)[:, :Z]
    zpad.copy_(f(rs.standard_normal((n_z, Z))))
    bufs = dict(dz=_guarded(n_z, Z, dev, nan, pad=True), diff=_guarded(T, R if rff else Z, dev, nan),
                m2=_guarded(T, 1, dev, nan), cnt=_guarded(n_lists * G, S + 1, dev, -1, dtype=torch.int32),
                members=_guarded(n_lists * G, B, dev, -1, dtype=torch.int32))
    if rff:
        bufs['theta'] = _guarded(Kc * n_z, R, dev, nan)
    g = dict(z=zpad, kind=kernel, model=model, R=R if rff else 0, S=S, cls=i(rs.randint(0, S, B)), Np=Np, L=L,
             a=1.0 / math.sqrt(Z), c=math.sqrt(2.0 / R) if rff else 1.0, w=(1.0 if S == 2 else 1.0 / S) / L, fac=-1.0,
             value=torch.full((1,), nan, device=dev), W=f(rs.standard_normal((T, Z, R))) if rff else None,
             b=f(rs.rand(T, R)) if rff else None, theta=None)
    g.update({k: v[0] for k, v in bufs.items()})
    g['m2'] = bufs['m2'][0].reshape(-1)
    hx = rs.randint(0, 2, n_ds) if model != 'vfae' else None
    hy = rs.randint(0, 2, n_ds) if model != 'pvae' else None
    tab = rs.randint(0, n_ds, (5, B))
    src = dict(hx=hx, hy=hy, tab=tab, hx_dev=None if hx is None else i(hx), hy_dev=None if hy is None else i(hy), tab_dev=i(tab),
               ctr=torch.zeros(1, dtype=torch.int32, device=dev), base=torch.zeros(1, dtype=torch.int32, device=dev))
    return g, bufs, src


def _with_flags(g, src, mode, dev):
    """the operands with the batch's flags: ``mode`` = (ctr, base) through the table | None: batch-local (batch 2's rows)"""
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    B = g['cls'].numel()
    if mode is None:
        fx, fy = MC.batch_flags(src['hx'], src['hy'], src['tab'], 2, B)
        return dict(g, hx=None if src['hx'] is None else i(fx), hy=None if src['hy'] is None else i(fy)), (fx, fy)
    src['ctr'].fill_(mode[0])
    src['base'].fill_(mode[1])
    return dict(g, hx=src['hx_dev'], hy=src['hy_dev'], table=src['tab_dev'], n_batches=5, ctr=src['ctr'], base=src['base']), \
        MC.batch_flags(src['hx'], src['hy'], src['tab'], mode[0] - mode[1], B)


def _reference(g, flags):
    n = lambda t: None if t is None else t.cpu().numpy()
    return MC.masked_ref(n(g['z']), n(g['cls']), flags[0], flags[1], g['model'], g['Np'], g['L'], g['S'], g['kind'], g['w'],
                         g['fac'], n(g['W']), n(g['b']), g['a'], g['c'])


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('kernel', ['rbf_fourier', 'identity'])
@pytest.mark.parametrize('shape', ['tiny', 'drvae4', 'long'])
def test_masked_mmd_kernels_against_fp64(shape, kernel, S, dev):
    import drvae_amd.kernels as K
    g0, bufs, src = _problem(shape, kernel, S, dev, seed=11)
    # batch 0, one in the middle, clamped past the end, clamped below, and batch-local flags
    for mode in ((7, 7), (9, 7), (40, 7), (3, 7), None):
        g, flags = _with_flags(g0, src, mode, dev)
        for k in ('dz', 'diff'):
            g[k].fill_(float('nan'))
        K.mmd_masked_fwd(g)
        K.mmd_masked_bwd(g)
        torch.cuda.synchronize()
        ref = _reference(g, flags)
        got_v, got_dz = float(g['value']), g['dz'].cpu().numpy().astype(np.float64)
        print('masked MMD %s %s S=%d flags %s: value rel err %.3g, gradient max abs err %.3g (max |g| %.3g), diff max abs err %.3g'
              % (shape, kernel, S, mode, abs(got_v - ref['value']) / abs(ref['value']), np.abs(got_dz - ref['dz']).max(),
                 np.abs(ref['dz']).max(), np.abs(g['diff'].cpu().numpy() - ref['diff']).max()))
        assert np.array_equal(g['cnt'].cpu().numpy(), ref['cnt'])
        mem = g['members'].cpu().numpy()
        for tg, m in enumerate(ref['members']):
            assert np.array_equal(mem[tg, :len(m)], m)
        assert ref['value'] < 0
        np.testing.assert_allclose(got_v, ref['value'], rtol=VALUE_RTOL)
        np.testing.assert_allclose(g['m2'].cpu().numpy(), ref['m2'], rtol=2 * VALUE_RTOL)
        np.testing.assert_allclose(got_dz, ref['dz'], rtol=GRAD_RTOL, atol=GRAD_ATOL)
        # deterministic: one writer per element
        keep = (g['value'].clone(), g['dz'].clone(), g['diff'].clone())
        K.mmd_masked_fwd(g)
        K.mmd_masked_bwd(g)
        assert all(torch.equal(a, b) for a, b in zip(keep, (g['value'], g['dz'], g['diff'])))
    assert all(_guards_intact(*v) for v in bufs.values())


def _edge_problem(kernel, S, dev, fx, fy, cls, z=None):
    """DrVAE, B = 20, 12 pair slots, Z = 5, L = 1, batch-local flags"""
    B, Np, L, Z, R = 20, 12, 1, 5, 40
    rs = np.random.RandomState(2)
    Kc, G = (1 if S == 2 else S), 4
    T, n_z = 2 * L * G * Kc, L * (B + Np)
    rff = kernel == 'rbf_fourier'
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    nan = float('nan')
    zv = rs.standard_normal((n_z, Z))
    zv = zv if z is None else z                    # (W / b: the same draws whatever z)
    W, b = rs.standard_normal((T, Z, R)), rs.rand(T, R)
    bufs = dict(dz=_guarded(n_z, Z, dev, nan, pad=True), diff=_guarded(T, R if rff else Z, dev, nan), m2=_guarded(T, 1, dev, nan))
    if rff:
        bufs['theta'] = _guarded(Kc * n_z, R, dev, nan)
    zpad = torch.zeros(n_z, 8, device=dev)[:, :Z]
    zpad.copy_(f(zv))
    g = dict(z=zpad, kind=kernel, model='drvae', R=R if rff else 0, S=S, cls=i(cls), Np=Np, L=L, a=1.0 / math.sqrt(Z),
             c=math.sqrt(2.0 / R) if rff else 1.0, w=(1.0 if S == 2 else 1.0 / S) / L, fac=-1.0,
             value=torch.full((1,), nan, device=dev), W=f(W) if rff else None, b=f(b) if rff else None, theta=None,
             cnt=torch.zeros(2 * L * G, S + 1, dtype=torch.int32, device=dev),
             members=torch.zeros(2 * L * G, B, dtype=torch.int32, device=dev), hx=i(fx), hy=i(fy))
    g.update({k: v[0] for k, v in bufs.items()})
    g['m2'] = bufs['m2'][0].reshape(-1)
    return g, bufs, zv


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('kernel', ['rbf_fourier', 'identity'])
def test_masked_mmd_edge_cases(kernel, S, dev):
    """outputs pre-filled with NaN; a data group absent from the batch, a group with one class only, pair slots whose row is no
    pair, two identical rows in opposite classes: defined as 0, everything finite, the untouched terms bit-equal to the run
    without the edge, nothing outside the views written, two launches bit-equal"""
    import drvae_amd.kernels as K
    B, Np, Kc = 20, 12, (1 if S == 2 else S)
    pat = np.arange(B) % 4                         # groups round-robin: 0 = labeled single ... 3 = unlabeled pair
    fx, fy = pat >= 2, (pat % 2) == 0
    rs = np.random.RandomState(5)
    cls = rs.randint(0, S, B)
    cls[:4 * S] = np.repeat(np.arange(S), 4)       # every (group, class) cell holds a row
    grp = MC.data_groups('drvae', fx, fy)

    def run(fx, fy, cls, z=None):
        g, bufs, zv = _edge_problem(kernel, S, dev, fx, fy, cls, z)
        K.mmd_masked_fwd(g)
        K.mmd_masked_bwd(g)
        keep = (g['value'].clone(), g['dz'].clone(), g['diff'].clone(), g['m2'].clone())
        K.mmd_masked_fwd(g)
        K.mmd_masked_bwd(g)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(keep, (g['value'], g['dz'], g['diff'], g['m2'])))
        assert all(_guards_intact(*v) for v in bufs.values())
        assert bool(torch.isfinite(g['dz']).all()) and bool(torch.isfinite(g['diff']).all()) and bool(torch.isfinite(g['m2']).all())
        ref = _reference(g, (fx, fy))
        assert math.isfinite(float(g['value'])) and ref['value'] < 0
        np.testing.assert_allclose(float(g['value']), ref['value'], rtol=VALUE_RTOL)
        np.testing.assert_allclose(g['dz'].cpu().numpy(), ref['dz'], rtol=GRAD_RTOL, atol=GRAD_ATOL)
        assert np.array_equal(g['cnt'].cpu().numpy(), ref['cnt'])
        # pair slots whose row is no pair in this batch: exact zeros
        idle = B + np.nonzero(~fx[:Np])[0]
        assert len(idle) and bool((g['dz'][torch.from_numpy(idle).to(dev)] == 0).all())
        return g, zv

    base, zv = run(fx, fy, cls)
    rows_of = lambda gs: np.concatenate([np.nonzero(np.isin(grp, gs))[0], B + np.nonzero(np.isin(grp[:Np], gs) & fx[:Np])[0]])
    terms_of = lambda gs: np.concatenate([np.arange((q * 4 + gi) * Kc, (q * 4 + gi + 1) * Kc) for q in range(2) for gi in gs])
    same = lambda g, gs: (torch.equal(g['dz'][rows_of(gs)], base['dz'][rows_of(gs)]) and
                          torch.equal(g['diff'][terms_of(gs)], base['diff'][terms_of(gs)]))
    # (1) a data group absent from the batch: the labeled singles become unlabeled singles -- the groups of pairs are untouched
    fy1 = fy & fx
    g, _ = run(fx, fy1, cls, zv)
    assert bool((g['cnt'][0] == 0).all()) and bool((g['m2'][:Kc] == 0).all()) and bool((g['diff'][:Kc] == 0).all())
    assert same(g, [2, 3])
    # (2) a group with one class only: value 0, gradient 0 for its rows, the other groups untouched
    c2 = cls.copy()
    c2[grp == 1] = 1
    g, _ = run(fx, fy, c2, zv)
    assert bool((g['dz'][np.nonzero(grp == 1)[0]] == 0).all()) and bool((g['m2'][Kc:2 * Kc] == 0).all())
    assert same(g, [0, 2, 3])
    # (3) two identical rows in opposite classes are ALL of a group: m2 == 0 exactly
    if S == 2:
        fx3, fy3 = fx.copy(), fy.copy()
        fx3[grp == 0], fy3[grp == 0] = False, False          # the labeled singles leave ...
        fx3[[0, 4]], fy3[[0, 4]] = False, True               # ... but for two rows
        c3, z3 = cls.copy(), zv.copy()
        c3[[0, 4]] = [0, 1]
        z3[4] = z3[0]
        g, _ = run(fx3, fy3, c3, z3)
        assert float(g['m2'][0]) == 0.0 and bool((g['diff'][0] == 0).all()) and bool((g['dz'][[0, 4]] == 0).all())
        assert same(g, [2, 3])


# ------------------------------------------------------------------------------------------------- engine
def _engines(kind, dim_s, dev, kernel=None, L=2, **bat_kw):
    from drvae_amd import data as D
    over = dict(use_MMD=True, mmd_rate=0.7, kernel_MMD=kernel) if kernel is not None else {}
    spec, big, ds = NC.dataset(kind, dim_s, dev, L=L, **over)
    params = M.init_params(spec, 3, as_numpy=True)
    bat = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, mode='sampler', carry_s='masked', **bat_kw)
    fed, a1 = make_engine(spec, params, dev)
    other, a0 = make_engine(spec, params, dev)
    return spec, big, ds, bat, fed, a1, other, a0


def _replay_with_its_noise(fed, hy, y):
    """one replay; returns the N(0,1) draws that step used, as ``set_noise`` takes them (``nuisance_masked_cases.step_noise``).
    Where the side chain draws the NEXT step's noise behind the join, the draws of this step are in the arena before the
    replay (the first one: drawn here, as ``replay`` would); else they are there after it."""
    import drvae_amd.kernels as K
    fed.join_side()
    torch.cuda.synchronize()
    if fed.noise_ahead:
        if fed._noise_stale:
            K.fill_normal_rows(fed.plan.noise, fed.plan.noise_desc, fed.seed, fed.rng_ctr)
            fed._noise_stale = False
            torch.cuda.synchronize()
        noise = MC.step_noise(fed.plan, fed.cfg, hy, y)
        fed.replay()
        fed.join_side()
        torch.cuda.synchronize()
        return noise
    fed.replay()
    fed.join_side()
    torch.cuda.synchronize()
    return MC.step_noise(fed.plan, fed.cfg, hy, y)


def _dzmmd_on_host_layout(fed_p, host_p, L):
    """the rows of the batch-independent plan's DZMMD that the structure plan has, in its order"""
    B, Np, pairs = fed_p.B, fed_p.Np, torch.as_tensor(host_p.pair_host, device=fed_p.DZMMD.device)
    parts = [fed_p.DZMMD[:L * B]] + [fed_p.DZMMD[L * B + l * Np + pairs] for l in range(L)]
    return torch.cat(parts)


@pytest.mark.parametrize('use_mmd', [False, True])
@pytest.mark.parametrize('dim_s', [2, 3])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_one_captured_step_equals_host_fed_steps(kind, dim_s, use_mmd, dev):
    """an epoch of 6 constructed batches -- another number of rows per data group in each, every (group, class) cell filled --
    through ``begin_epoch(table=...)`` + ONE captured step on ONE plan, against a second engine fed the same rows, classes and
    draws from the host (``set_batch(..., s=host)``: a plan per structure, today's host-list penalty).  Tolerances: those of
    ``test_epoch_through_one_captured_step_equals_host_fed_steps`` with the penalty"""
    spec, big, ds, bat, fed, a1, host, a0 = _engines(kind, dim_s, dev, kernel='identity' if use_mmd else None)
    tab = MC.varied_table(kind, big, dim_s, 6)
    MC.assert_cells_filled_and_counts_differ(kind, big, tab, dim_s)
    p = bat.bind(fed)
    assert p.universal and p.carry_s and (p.mmd_masked is not None) == use_mmd
    bat.begin_epoch(n_batches=6, table=torch.from_numpy(tab).to(dev))
    fed.capture()
    hx_all, hy_all, y_all = (big[k].reshape(-1) for k in ('has_x2', 'has_y', 'y'))
    for b in range(6):
        rows = tab[b]
        noise = _replay_with_its_noise(fed, hy_all[rows], y_all[rows])
        assert np.array_equal(fed.plan.s_cls.cpu().numpy(), big['s'].reshape(-1)[rows])
        i = torch.from_numpy(rows).to(dev)
        host.iters = fed.iters - 1               # (the same perturbation annealing coefficient)
        host.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), hx_all[rows], hy_all[rows], s=ds.s[i].cpu())
        assert not host.plan.universal and not host.plan.carry_s
        host.train_step(noise=noise)
        host.join_side()
        torch.cuda.synchronize()
        lf, lh = fed.losses(), host.losses()
        rel_g = float((a1.grad - a0.grad).norm() / a0.grad.norm())
        line = 'sampler step %s dim_s=%d batch %d: gradient rel %.3g' % (kind, dim_s, b, rel_g)
        if use_mmd:
            fz = _dzmmd_on_host_layout(fed.plan, host.plan, spec.L)
            rel_z = float((fz - host.plan.DZMMD).norm() / host.plan.DZMMD.norm())
            print(line + ', MMDval %.7g / %.7g, DZMMD rel %.3g' % (float(fed.plan.MMDval), float(host.plan.MMDval), rel_z))
            np.testing.assert_allclose(fed.plan.MMDval.cpu().numpy(), host.plan.MMDval.cpu().numpy(), rtol=2e-5)
            assert rel_z < 2e-5
            assert lh['MMD'] < 0
        else:
            print(line)
        assert rel_g < 2e-5
        for k in lf:
            np.testing.assert_allclose(lf[k], lh[k], rtol=1e-4, atol=1e-6)
    fed.check_sync()
    assert len(fed._plans) == 1 and fed.iters == 6 and fed.plan.live_feed is not None
    assert float((a1.param - a0.param).norm() / a0.param.norm()) < 1e-4


@pytest.mark.parametrize('kind,dim_s', [('drvae', 3), ('vfae', 2)])
def test_fourier_penalty_recomputed_from_its_buffers(kind, dim_s, dev):
    """rbf_fourier: after an eager step on an explicit batch and after replays, value and gradient recomputed in fp64 from what
    the step leaves behind -- the sample rows, the stacked W / b, the class vector -- and the batch's flags"""
    spec, big, ds, bat, fed, a1, _, _ = _engines(kind, dim_s, dev, kernel='rbf_fourier')
    tab = MC.varied_table(kind, big, dim_s, 4, seed=3)
    bat.bind(fed)
    p = fed.plan
    hx_all, hy_all = big['has_x2'].reshape(-1).astype(bool), big['has_y'].reshape(-1).astype(bool)
    draws = []

    def check(tag, rows):
        fed.join_side()
        torch.cuda.synchronize()
        g = p.mmd_masked
        n = lambda t: t.cpu().numpy()
        fx = hx_all[rows] if kind != 'vfae' else np.zeros(len(rows), bool)
        fy = hy_all[rows] if kind != 'pvae' else np.zeros(len(rows), bool)
        S, L, Z = spec.dim_s, spec.L, spec.dim_z1
        R = g['W'].shape[2]
        assert R == 500 and np.array_equal(n(p.s_cls), big['s'].reshape(-1)[rows])
        ref = MC.masked_ref(n(p.ZDEC[:p.o3]), n(p.s_cls), fx, fy, kind, p.Np, L, S, 'rbf_fourier', (1.0 if S == 2 else 1.0 / S) / L,
                            -spec.mmd_rate / p.n_tot, n(g['W']), n(g['b']), 1.0 / math.sqrt(Z), math.sqrt(2.0 / R))
        got = p.DZMMD.cpu().numpy().astype(np.float64)
        print('masked fourier penalty %s %s: value %.6g (fp64 %.6g), gradient max abs err %.3g (max |g| %.3g)'
              % (kind, tag, float(p.MMDval), ref['value'], np.abs(got - ref['dz']).max(), np.abs(ref['dz']).max()))
        assert ref['value'] < 0
        np.testing.assert_allclose(float(p.MMDval), ref['value'], rtol=VALUE_RTOL)
        np.testing.assert_allclose(got, ref['dz'], rtol=GRAD_RTOL, atol=GRAD_ATOL)
        draws.append((n(g['W']).copy(), n(g['b']).copy()))
    bat.feed(torch.from_numpy(tab[0]).to(dev))
    fed.train_step()
    check('eager', tab[0])
    bat.begin_epoch(n_batches=4, table=torch.from_numpy(tab).to(dev))
    fed.capture()
    for b in range(3):
        fed.replay()
        check('replay %d' % b, tab[b])
    assert not np.array_equal(draws[-1][0], draws[-2][0]) and not np.array_equal(draws[-1][1], draws[-2][1])


def _captured_launches(eng, monkeypatch):
    """launches of the captured step by name: the library's through ``_lib.check``, torch's in-place random draws"""
    from drvae_amd import _lib
    counts, on = collections.Counter(), [False]
    real = _lib.check

    def counting(code, what):
        if on[0] and not what.startswith('dv_gemm_set_option'):
            counts[what] += 1
        return real(code, what)
    monkeypatch.setattr(_lib, 'check', counting)
    for name in ('normal_', 'uniform_'):
        def draw(self, *a, _real=getattr(torch.Tensor, name), _name=name, **k):
            if on[0]:
                counts['torch.' + _name] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, draw)
    real_capture_main = eng._capture_main

    def capture_main(*a, **k):
        on[0] = True
        return real_capture_main(*a, **k)
    monkeypatch.setattr(eng, '_capture_main', capture_main)
    eng.capture()
    on[0] = False
    monkeypatch.undo()
    return counts


def _diff(a, b):
    return {k: a.get(k, 0) - b.get(k, 0) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}


def test_launch_count_of_the_masked_step(dev, monkeypatch):
    """the captured step on the masked plan counts the same whatever batch it is captured at.  What it adds, by name: the
    penalty is exactly four launches (the two feature draws, dv_mmd_masked_fwd, dv_mmd_masked_bwd) on top of the same model's
    step without it; that step holds exactly one dv_nuisance_feed, and differs from the batch-independent step of the model
    WITHOUT ``use_s`` by that launch and the products of the one-hot operand (``use_s`` itself: two-operand first layers) --
    the very same additions, name by name, a stratified carried plan makes to a stratified step"""
    from drvae_amd import data as D
    for L, dim_s in ((1, 2), (2, 3)):
        n = {}
        for mode in ('sampler', 'stratified'):
            for kernel in ('rbf_fourier', None):
                over = dict(use_MMD=True, mmd_rate=0.7, kernel_MMD=kernel) if kernel else {}
                spec, big, ds = NC.dataset('drvae', dim_s, dev, L=L, **over)
                fed, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True), dev)
                if mode == 'sampler':
                    bat = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, mode='sampler', carry_s='masked')
                    tab = MC.varied_table('drvae', big, dim_s, 3)
                else:
                    bat = D.DeviceBatcher(ds, torch.ones(400), 24, group_counts=NC.group_counts(big), seed=5, carry_s=True)
                    tab = NC.epoch_table(big, dim_s, 3, vary=True)
                bat.bind(fed)
                bat.begin_epoch(n_batches=3, table=torch.from_numpy(tab).to(dev))
                n[mode, kernel] = _captured_launches(fed, monkeypatch)
                fed.replay()
                fed.replay()
                fed.join_side()
                if mode == 'sampler' and kernel:
                    again = _captured_launches(fed, monkeypatch)     # captured again, two batches on: another composition
                    assert again == n[mode, kernel]
                fed.replay()
                torch.cuda.synchronize()
                fed.check_sync()
            # the same step of the model without use_s
            plain_spec = C.tiny_spec('drvae', L=L)
            eng, _ = make_engine(plain_spec, M.init_params(plain_spec, 3, as_numpy=True), dev)
            pb = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, mode='sampler') if mode == 'sampler' else \
                D.DeviceBatcher(ds, torch.ones(400), 24, group_counts=NC.group_counts(big), seed=5)
            pb.bind(eng)
            pb.begin_epoch(n_batches=3, table=torch.from_numpy(tab).to(dev))
            n[mode, 'plain'] = _captured_launches(eng, monkeypatch)
            eng.replay()
            torch.cuda.synchronize()
            eng.check_sync()
        pen = _diff(n['sampler', 'rbf_fourier'], n['sampler', None])
        carry = _diff(n['sampler', None], n['sampler', 'plain'])
        print('stratified: carrying s adds %s' % _diff(n['stratified', None], n['stratified', 'plain']))
        print('captured launches L=%d dim_s=%d: %d plain, %d with s, %d with the penalty; the penalty adds %s, carrying s adds %s'
              % (L, dim_s, sum(n['sampler', 'plain'].values()), sum(n['sampler', None].values()),
                 sum(n['sampler', 'rbf_fourier'].values()), pen, carry))
        assert pen == {'torch.normal_': 1, 'torch.uniform_': 1, 'dv_mmd_masked_fwd': 1, 'dv_mmd_masked_bwd': 1}
        assert n['sampler', None]['dv_nuisance_feed'] == 1 and carry['dv_nuisance_feed'] == 1
        # ... the same additions a stratified carried plan makes
        assert carry == _diff(n['stratified', None], n['stratified', 'plain'])
        assert _diff(n['stratified', 'rbf_fourier'], n['stratified', None]) == \
            {'torch.normal_': 1, 'torch.uniform_': 1, 'dv_mmd_grouped_fwd': 1, 'dv_mmd_grouped_bwd': 1}


def test_bucketed_feed_switches_plans_that_all_carry(dev):
    """``pair_bucket=8, label_bucket=4`` (DrVAE): the epoch's batches switch between captured plans, every plan carries the
    classes and the masked penalty, and the steps equal -- bitwise -- eager steps of the same plans handed the same rows"""
    spec, big, ds, bat, fed, a1, eager, a0 = _engines('drvae', 3, dev, kernel='identity', pair_bucket=8, label_bucket=4)
    eager.universal, eager.carry_s = True, 'masked'
    rs = np.random.RandomState(4)
    hx = big['has_x2'].reshape(-1).astype(bool)
    # drawn rows with a share of pairs that changes from batch to batch: the batches land in different buckets
    tab = np.stack([np.concatenate([rs.choice(np.nonzero(hx)[0], npair), rs.choice(np.nonzero(~hx)[0], 24 - npair)])
                    for npair in (3, 9, 14, 20, 9, 3)])
    bat.bind(fed)
    bat.begin_epoch(n_batches=6, table=torch.from_numpy(tab).to(dev))
    bat.prepare_epoch(lambda e: e.capture())
    used = set()
    for k in range(6):
        bat.select(k)
        q = fed.plan
        used.add(q.key)
        assert q.universal and q.carry_s and q.mmd_masked is not None and q.key[-1] == 'carry_s' and q.live_feed.s32 is not None
        fed.replay()
        i = bat._tab_sorted[k].long()
        eager.universal_pair_slots, eager.universal_labeled_range = q.Np, bat.batch_specs[k][1:]
        eager.set_batch(ds.x1[i], ds.x2[i], ds.y[i].cpu(), ds.has_x2[i].cpu().numpy(), ds.has_y[i].cpu().numpy(), s=ds.s[i])
        assert eager.plan.key == q.key
        eager.train_step()
        fed.join_side()
        torch.cuda.synchronize()
        assert torch.equal(fed.plan.DZMMD, eager.plan.DZMMD) and fed.losses() == eager.losses()
    assert len(used) > 1 and bat.n_switch > 0
    assert torch.equal(a1.param, a0.param)
    fed.check_sync()


@pytest.mark.parametrize('kind,dim_s', [('vfae', 2), ('drvae', 3)])
def test_fit_on_a_sampler_batcher_that_carries_s(kind, dim_s, tmp_path, dev):
    from drvae_amd import data as D
    from drvae_amd.fit import _EvalGraph
    from drvae_amd.plan import LOSS_IDX
    from tests.test_fit import _loader, _tiny_model
    from tests.test_gpu_nuisance import _s_dataset
    kw = dict(device='cuda', dim_s=dim_s, use_s=True, use_MMD=True, kernel_MMD='rbf_fourier', mmd_rate=1.0, epochs=1)
    model = _tiny_model(kind, **kw)
    tr, va = _s_dataset(kind, 128, 1, dim_s, 'cuda'), _s_dataset(kind, 32, 2, dim_s, 'cuda')
    w = D.compute_balanced_weights(np.arange(128) % 5)
    fn = str(tmp_path / 'best.pth')
    batcher = D.DeviceBatcher(tr, w, 32, seed=3, mode='sampler', carry_s='masked')
    eng = model.engine()
    seen, real_replay = [], eng.replay

    def replay(*a, **k):
        seen.append(eng.plan.live_feed is not None and eng.plan.carry_s and eng.plan.universal and eng.plan.mmd_masked is not None)
        return real_replay(*a, **k)
    eng.replay = replay
    cmpl = []
    for epoch in range(6):
        model.fit(batcher, _loader(va, 8), add_noise=True, verbose=False, early_stop=False, model_filename=fn)
        batcher.bind(eng)
        eng.join_side()
        sums = eng.loss_sum.cpu().numpy().astype(np.float64) / len(batcher)
        assert np.isfinite(sums).all() and sums[LOSS_IDX['MMD']] < 0
        cmpl.append(sums[LOSS_IDX['CMPL']])
    assert model.finished_training_iters == 6 * 4 and len(seen) >= 6 * 4 and all(seen)
    assert cmpl[-1] < cmpl[0], cmpl
    assert len(eng._captures) == 0 and eng._graph_key == batcher._bound_plan.key and eng.carry_s == 'masked'
    # the whole-set evaluation: still the carried STRUCTURE plan of the set, and green
    perf, _ = model.evaluate_performance_on_dataset(tr)
    assert np.isfinite(model._valid_objective(perf))
    ev = _EvalGraph.get(model, tr)
    assert ev is not None and ev.plan.carry_s and not ev.plan.universal and ev.plan.mmd_grouped is not None
    assert eng.carry_s == 'masked' and eng.universal
