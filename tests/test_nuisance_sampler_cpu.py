"""CPU: the nuisance variable on sampler-mode device batches -- the C-ABI declarations of ``dv_mmd_masked_*``, the
stand-ins of its two launchers against the fp64 reference written from the header, that reference against the structure
tables of tests/nuisance_cases.py, and the engine / ``DeviceBatcher(mode='sampler', carry_s='masked')`` orchestration on
the stand-ins (the kernels themselves: tests/test_gpu_nuisance_sampler.py)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests import nuisance_cases as NC
from tests import nuisance_masked_cases as MC
from tests.test_engine_cpu import make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'drvae_hip.h')).read()


def _struct_fields(src, cname):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return [re.sub(r'.*[\s\*]', '', part.strip()) for st in body.split(';') if st.strip() for part in st.split(',')]


def test_abi_grows_by_two_entry_points_and_the_descriptor_matches_the_header():
    from drvae_amd import _lib
    src = _header()
    assert _struct_fields(src, 'dv_mmd_masked_desc') == [f[0] for f in _lib.MmdMasked._fields_]
    assert _struct_fields(src, 'dv_mmd_grouped_desc') == [f[0] for f in _lib.MmdGrouped._fields_]      # untouched
    assert _lib.ABI_VERSION == int(re.search(r'#define DV_ABI_VERSION (\d+)', src).group(1))
    for name in ('dv_mmd_masked_fwd', 'dv_mmd_masked_bwd'):
        assert len(_lib.SIGNATURES[name]) == 2
    decl = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert set(re.findall(r'(?:int|const char\*)\s+(dv_\w+)\s*\(', decl)) == set(_lib.SIGNATURES)
    import drvae_amd.kernels as K
    for name, val in K.MMD_MASKED_MODEL.items():
        assert int(re.search(r'#define DV_MMD_GROUPS_%s (\d+)' % name.upper(), src).group(1)) == val


def test_entry_points_reject_bad_descriptors_without_gpu():
    import ctypes as C
    from drvae_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for fn in (lib.dv_mmd_masked_fwd, lib.dv_mmd_masked_bwd):
        assert fn(None, None) == -1
        ok = dict(kind=0, model=2, Z=5, B=4, L=1, Np=0, S=2, n_flags=4)
        assert fn(C.byref(_lib.MmdMasked(**ok)), None) == -1                        # no operands
        assert fn(C.byref(_lib.MmdMasked(**dict(ok, S=9))), None) == -1             # too many classes
        assert fn(C.byref(_lib.MmdMasked(**dict(ok, model=3))), None) == -1         # no such set of data groups
        assert fn(C.byref(_lib.MmdMasked(**dict(ok, Np=5, model=0))), None) == -1   # more pair slots than rows
        assert fn(C.byref(_lib.MmdMasked(**dict(ok, kind=2))), None) == -1


def _case(rs, model, S, kind, B=13, Np=7, L=2, Z=5, R=24, n_ds=40, table=True):
    """a masked problem as the launchers' operands (CPU tensors) plus what the fp64 reference needs"""
    if model == 'vfae':
        Np = 0
    Kc, G = (1 if S == 2 else S), MC.GROUPS[model]
    n_lists = L * (2 if Np else 1)
    T, n_z = n_lists * G * Kc, L * (B + Np)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32))
    rff = kind == 'rbf_fourier'
    n_fl = n_ds if table else B
    hx = rs.randint(0, 2, n_fl) if model != 'vfae' else None
    hy = rs.randint(0, 2, n_fl) if model != 'pvae' else None
    tab = rs.randint(0, n_ds, (3, B)) if table else None
    g = dict(z=f(rs.standard_normal((n_z, Z))), dz=torch.full((n_z, Z), float('nan')), kind=kind, model=model, R=R if rff else 0,
             S=S, cls=i(rs.randint(0, S, B)), Np=Np, L=L, a=1.0 / np.sqrt(Z), c=np.sqrt(2.0 / R) if rff else 1.0, w=0.5 / Kc,
             fac=-0.7 / B, diff=torch.full((T, R if rff else Z), float('nan')),
             cnt=torch.zeros(n_lists * G, S + 1, dtype=torch.int32), members=torch.zeros(n_lists * G, B, dtype=torch.int32),
             m2=torch.full((T,), float('nan')), value=torch.zeros(1), W=f(rs.standard_normal((T, Z, R))) if rff else None,
             b=f(rs.rand(T, R)) if rff else None, theta=torch.zeros(Kc * n_z, R) if rff else None,
             hx=None if hx is None else i(hx), hy=None if hy is None else i(hy))
    if table:
        g.update(table=i(tab), n_batches=3, ctr=i([7]), base=i([6]))
    return g, (hx, hy, tab)


def _ref(g, flags, b=1):
    hx, hy, tab = flags
    n = lambda t: None if t is None else t.numpy()
    fx, fy = MC.batch_flags(hx, hy, tab, b, g['cls'].numel())
    return (fx, fy), MC.masked_ref(n(g['z']), n(g['cls']), fx, fy, g['model'], g['Np'], g['L'], g['S'], g['kind'], g['w'],
                                   g['fac'], n(g['W']), n(g['b']), g['a'], g['c'])


@pytest.mark.parametrize('table', [True, False])
@pytest.mark.parametrize('kind', ['identity', 'rbf_fourier'])
@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('model', ['drvae', 'pvae', 'vfae'])
def test_standins_follow_the_fp64_reference(model, S, kind, table):
    rs = np.random.RandomState(7 + S)
    g, flags = _case(rs, model, S, kind, table=table)
    kernel_ref.mmd_masked_fwd(g)
    kernel_ref.mmd_masked_bwd(g)
    (fx, fy), ref = _ref(g, flags)
    assert np.array_equal(g['cnt'].numpy(), ref['cnt'])
    for tg, mem in enumerate(ref['members']):
        assert np.array_equal(g['members'][tg, :len(mem)].numpy(), mem)
    np.testing.assert_allclose(g['diff'].numpy(), ref['diff'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(g['m2'].numpy(), ref['m2'], rtol=2e-4, atol=1e-9)
    np.testing.assert_allclose(float(g['value']), ref['value'], rtol=1e-5)
    np.testing.assert_allclose(g['dz'].numpy(), ref['dz'], rtol=1e-3, atol=1e-7)
    assert ref['value'] < 0 and np.isfinite(g['dz'].numpy()).all()
    if g['Np']:      # the z2 rows of the slots without a pair: exact zeros
        B, Np, L = g['cls'].numel(), g['Np'], g['L']
        for l in range(L):
            rows = L * B + l * Np + np.nonzero(~fx[:Np])[0]
            assert len(rows) and (g['dz'][rows] == 0).all()


@pytest.mark.parametrize('kind', ['identity', 'rbf_fourier'])
@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('model', ['drvae', 'pvae', 'vfae'])
def test_reference_value_equals_the_grouped_reference_on_the_batchs_structure(model, S, kind):
    """the masked penalty of a batch IS the grouped penalty on the structure table of the batch's actual flags
    (``nuisance_cases.term_groups``): same value, same gradient on the rows both layouts have"""
    rs = np.random.RandomState(11 + S)
    g, flags = _case(rs, model, S, kind, B=17, Np=17)
    (fx, fy), ref = _ref(g, flags)
    n = lambda t: None if t is None else t.numpy()
    ptr, rows, src, zc, Wc, bc = MC.as_structure(model, fx, fy, g['Np'], g['L'], n(g['z']), n(g['W']), n(g['b']), S)
    diff, m2, value, dz, _, _ = NC.mmd_ref(zc, n(g['cls']), ptr, rows, src, S, kind, g['w'], g['fac'], Wc, bc, g['a'], g['c'])
    assert value < 0
    np.testing.assert_allclose(ref['value'], value, rtol=1e-12)
    B, L, Np = 17, g['L'], g['Np']
    np.testing.assert_allclose(ref['dz'][:L * B], dz[:L * B], rtol=1e-10, atol=1e-15)
    if Np:
        pairs = np.nonzero(fx)[0]
        got = np.concatenate([ref['dz'][L * B + l * Np + pairs] for l in range(L)])
        np.testing.assert_allclose(got, dz[L * B:], rtol=1e-10, atol=1e-15)


def _engines(kind, dim_s, use_mmd, dev='cpu', **bat_kw):
    from drvae_amd import data as D
    over = dict(use_MMD=True, mmd_rate=0.7, kernel_MMD='identity') if use_mmd else {}
    spec, big, ds = NC.dataset(kind, dim_s, dev, **over)
    params = M.init_params(spec, 3, as_numpy=True)
    bat = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, mode='sampler', carry_s='masked', **bat_kw)
    fed, a1 = make_engine(spec, params, dev)
    host, a0 = make_engine(spec, params, dev)
    return spec, big, ds, bat, fed, a1, host, a0


def _host_step(host, ds, big, rows, fed):
    """the same rows, classes and draws (``nuisance_masked_cases.step_noise``) on a plan of the batch's own structure"""
    i = torch.from_numpy(rows)
    hx, hy = big['has_x2'].reshape(-1)[rows], big['has_y'].reshape(-1)[rows]
    host.set_batch(ds.x1[i], ds.x2[i], ds.y[i], hx, hy, s=ds.s[i].cpu())
    assert not host.plan.carry_s and not host.plan.universal
    host.train_step(noise=MC.step_noise(fed.plan, fed.cfg, hy, big['y'].reshape(-1)[rows]))


@pytest.mark.parametrize('use_mmd', [False, True])
@pytest.mark.parametrize('dim_s', [2, 3])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_epoch_of_varying_batches_through_one_plan_equals_host_fed_steps_cpu(kind, dim_s, use_mmd, monkeypatch):
    """an epoch of tables whose composition of data groups AND classes differs from batch to batch, through ONE plan
    (eager steps that gather through the live feed), against a second engine fed per batch from the host (structure plans,
    host row lists)"""
    kernel_ref.install(monkeypatch)
    spec, big, ds, bat, fed, a1, host, a0 = _engines(kind, dim_s, use_mmd)
    tab = MC.varied_table(kind, big, dim_s, 6)
    MC.assert_cells_filled_and_counts_differ(kind, big, tab, dim_s)
    p = bat.bind(fed)
    assert p.universal and p.carry_s and p.key[-1] == 'carry_s' and (p.mmd_masked is not None) == use_mmd
    assert p.mmd_grouped is None and not hasattr(p, 'mmd_sig') and fed.carry_s == 'masked'
    bat.begin_epoch(n_batches=6, table=torch.from_numpy(tab))
    assert fed.plan.live_feed is not None and fed.plan.live_feed.s32.dtype == torch.int32
    for b in range(6):
        fed.train_step()
        np.testing.assert_array_equal(fed.plan.s_cls.numpy(), big['s'].reshape(-1)[tab[b]])
        _host_step(host, ds, big, tab[b], fed)
        if use_mmd:
            np.testing.assert_allclose(fed.plan.MMDval.numpy(), host.plan.MMDval.numpy(), rtol=2e-5)
            assert float(host.plan.MMDval) < 0
        lf, lh = fed.losses(), host.losses()
        for k in lf:
            np.testing.assert_allclose(lf[k], lh[k], rtol=1e-4, atol=1e-6)
    assert len(fed._plans) == 1
    assert float((a1.param - a0.param).norm() / a0.param.norm()) < 1e-4


def test_explicit_batches_and_buckets_feed_the_same_plan_kind_cpu(monkeypatch):
    """``feed()``, ``set_batch`` with a device ``s`` and the bucketed feed: every plan carries, the classes arrive through
    ``set_s_device`` / the shared feed, and the steps equal those of the unbucketed epoch feed"""
    kernel_ref.install(monkeypatch)
    spec, big, ds, bat, fed, a1, twin, a0 = _engines('drvae', 3, True)
    tab = MC.varied_table('drvae', big, 3, 4, seed=2)
    bat.bind(fed)
    bat.begin_epoch(n_batches=4, table=torch.from_numpy(tab))
    bat2 = type(bat)(ds, torch.ones(400), 24, seed=5, mode='sampler', carry_s='masked')
    bat2.bind(twin)
    hx, hy = big['has_x2'].reshape(-1), big['has_y'].reshape(-1)
    for b in range(4):
        fed.train_step()
        i = torch.from_numpy(tab[b])
        if b % 2:
            bat2.feed(i)
        else:
            twin.set_batch(ds.x1[i], ds.x2[i], ds.y[i], hx[tab[b]], hy[tab[b]], s=ds.s[i])
        assert twin.plan.universal and twin.plan.carry_s and twin.plan.live_feed is None
        assert torch.equal(twin.plan.s_cls, fed.plan.s_cls) and torch.equal(twin.plan.SOHd, fed.plan.SOHd)
        twin.train_step()
        assert fed.losses() == twin.losses()
    assert torch.equal(a1.param, a0.param) and len(twin._plans) == 1
    # buckets: plans by the batch's number of pairs / labeled run, all of them carrying, one shared feed
    spec, big, ds, bat, fed, a1, twin, a0 = _engines('drvae', 3, True, pair_bucket=8, label_bucket=4)
    bat.bind(fed)
    bat.begin_epoch(n_batches=4, table=torch.from_numpy(tab))
    plans = {bat._plan(sp) for sp in set(bat.batch_specs) | {bat._full_spec}}
    assert len(plans) > 1 and all(q.carry_s and q.mmd_masked is not None and q.feed is bat._feed for q in plans)
    assert bat._feed.s32 is not None
    for b in range(4):
        bat._plan(bat.batch_specs[b])
        fed.train_step()
        _host_step(twin, ds, big, bat._tab_sorted[b].numpy(), fed)
        np.testing.assert_allclose(fed.plan.MMDval.numpy(), twin.plan.MMDval.numpy(), rtol=2e-5)
        for k, v in fed.losses().items():
            np.testing.assert_allclose(v, twin.losses()[k], rtol=1e-4, atol=1e-6)


def test_cpu_generator_and_draw_ahead(monkeypatch):
    """``generator='cpu'`` (the reference's stream) and ``draw_ahead`` / ``rebase`` work with the masked carry"""
    kernel_ref.install(monkeypatch)
    from drvae_amd import data as D
    spec, big, ds = NC.dataset('vfae', 2, 'cpu', use_MMD=True, kernel_MMD='identity')
    eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True))
    w = torch.ones(400)
    torch.manual_seed(3)
    bat = D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', generator='cpu', carry_s='masked')
    bat.bind(eng)
    t = bat.begin_epoch().clone()
    torch.manual_seed(3)
    plain = D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', generator='cpu')
    assert torch.equal(plain._reference_epoch().to(torch.int32), t)
    eng.train_step()
    assert np.array_equal(eng.plan.s_cls.numpy(), big['s'].reshape(-1)[t[0].numpy()])
    bat = D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', carry_s='masked')
    bat.bind(eng)
    bat.begin_epoch()
    bat.draw_ahead()
    assert bat._ahead is not None
    t2 = bat.begin_epoch().clone()
    eng.train_step()
    bat.rebase()
    eng.train_step()
    assert np.array_equal(eng.plan.s_cls.numpy(), big['s'].reshape(-1)[t2[0].numpy()])
    assert all(np.isfinite(v) for v in eng.losses().values())


def test_what_is_refused_and_what_stays(monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd import data as D
    spec, big, ds = NC.dataset('drvae', 2, 'cpu', use_MMD=True, kernel_MMD='identity')
    w = torch.ones(400)
    with pytest.raises(ValueError):
        D.DeviceBatcher(ds, w, 24, seed=5, carry_s='masked')                       # stratified: the cheaper plan exists
    with pytest.raises(ValueError):
        D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', carry_s='yes')
    eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True))
    with pytest.raises(NotImplementedError):
        D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', carry_s=True).bind(eng)  # True keeps its refusal
    with pytest.raises(NotImplementedError):
        D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler').bind(eng)
    with pytest.raises(AssertionError, match='sharded'):                            # the penalty under data parallelism
        D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', carry_s='masked').bind(eng, dp=(0, 2))
    # use_s without the penalty under data parallelism: refused with a clear message
    spec2, _, ds2 = NC.dataset('drvae', 2, 'cpu')
    eng2, _ = make_engine(spec2, M.init_params(spec2, 3, as_numpy=True))
    with pytest.raises(NotImplementedError, match='data parallelism'):
        D.DeviceBatcher(ds2, w, 24, seed=5, mode='sampler', carry_s='masked').bind(eng2, dp=(0, 2))
    # without carry a use_s model keeps the structure plans, also with ``universal`` on
    eng2.universal = True
    assert not eng2.universal_ok()
    with pytest.raises(AssertionError, match='carry_s'):
        eng2.set_structure_universal(24)
    # kernels the device path does not have are refused when the plan is built
    spec3, _, ds3 = NC.dataset('drvae', 2, 'cpu', use_MMD=True, kernel_MMD='rbf')
    eng3, _ = make_engine(spec3, M.init_params(spec3, 3, as_numpy=True))
    with pytest.raises(AssertionError, match='kernel_MMD'):
        D.DeviceBatcher(ds3, w, 24, seed=5, mode='sampler', carry_s='masked').bind(eng3)
    # a model without use_s: 'masked' changes nothing
    spec4 = NC.C.tiny_spec('drvae')
    eng4, _ = make_engine(spec4, M.init_params(spec4, 3, as_numpy=True))
    p = D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler', carry_s='masked').bind(eng4)
    assert p.universal and not p.carry_s and p.key[-1] != 'carry_s' and eng4.carry_s is False
    q = D.DeviceBatcher(ds, w, 24, seed=5, mode='sampler').bind(eng4)
    assert q is p
