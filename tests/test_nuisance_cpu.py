"""CPU: the nuisance variable carried on the device -- C-ABI declarations, the stand-ins of the three launchers against
the fp64 formulas, and the engine / ``DeviceBatcher(carry_s=True)`` orchestration on the stand-ins (the kernels themselves:
tests/test_gpu_nuisance.py)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests import nuisance_cases as NC
from tests.test_engine_cpu import make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_is_additive_and_the_descriptor_matches_the_header():
    from drvae_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'drvae_hip.h')).read()
    body = re.search(r'typedef struct dv_mmd_grouped_desc \{(.*?)\} dv_mmd_grouped_desc;', src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.sub(r'.*[\s\*]', '', part.strip()) for st in body.split(';') if st.strip() for part in st.split(',')]
    assert names == [f[0] for f in _lib.MmdGrouped._fields_]
    assert _lib.ABI_VERSION == int(re.search(r'#define DV_ABI_VERSION (\d+)', src).group(1))
    for name in ('dv_nuisance_feed', 'dv_mmd_grouped_fwd', 'dv_mmd_grouped_bwd'):
        assert name in _lib.SIGNATURES


def test_entry_points_reject_bad_arguments_without_gpu():
    import ctypes as C
    from drvae_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.dv_nuisance_feed(None, None, 0, None, None, 4, None, 0, 1, 2, None, 2, None, 2, None, None) == -1
    assert lib.dv_mmd_grouped_fwd(None, None) == -1
    d = _lib.MmdGrouped(kind=1, n_groups=1, n_entries=4, max_rows=4, Z=5, n_z=4, B=4, S=9)      # too many classes, no operands
    assert lib.dv_mmd_grouped_fwd(C.byref(d), None) == -1
    assert lib.dv_mmd_grouped_bwd(C.byref(d), None) == -1


def _random_case(rs, kind, S, Z, sizes, R=24):
    """a grouped-MMD problem over len(sizes) groups of the given numbers of rows"""
    E = sum(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    rows = rs.permutation(E)
    B = E
    src = rs.permutation(B)
    cls = rs.randint(0, S, B)
    Kc = 1 if S == 2 else S
    T = len(sizes) * Kc
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32))
    rff = kind == 'rbf_fourier'
    z = rs.standard_normal((E, Z))
    g = dict(z=f(z), dz=torch.zeros(E, Z), kind=kind, R=R if rff else 0, S=S, cls=i(cls), grp_ptr=i(ptr), rows=i(rows),
             src=i(src), max_rows=max(sizes), a=1.0 / np.sqrt(Z), c=np.sqrt(2.0 / R) if rff else 1.0, w=0.5 / Kc, fac=-0.7 / B,
             diff=torch.zeros(T, R if rff else Z), cnt=torch.zeros(len(sizes), S, dtype=torch.int32), m2=torch.zeros(T),
             value=torch.zeros(1), W=f(rs.standard_normal((T, Z, R))) if rff else None, b=f(rs.rand(T, R)) if rff else None,
             theta=torch.zeros(Kc * E, R) if rff else None)
    return g


@pytest.mark.parametrize('kind', ['identity', 'rbf_fourier'])
@pytest.mark.parametrize('S', [2, 3])
def test_standins_follow_the_fp64_formulas(kind, S):
    rs = np.random.RandomState(3 + S)
    g = _random_case(rs, kind, S, 5, [6, 9, 4])
    g['cls'][g['src'][6:15].long()] = 1          # the second group: one class only -- an empty side
    kernel_ref.mmd_grouped_fwd(g)
    kernel_ref.mmd_grouped_bwd(g)
    n = lambda t: None if t is None else t.numpy()
    diff, m2, value, dz, theta, cnt = NC.mmd_ref(n(g['z']), n(g['cls']), n(g['grp_ptr']), n(g['rows']), n(g['src']), S, kind,
                                                 g['w'], g['fac'], n(g['W']), n(g['b']), g['a'], g['c'])
    np.testing.assert_allclose(g['diff'].numpy(), diff, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(float(g['value']), value, rtol=1e-5)
    np.testing.assert_allclose(g['dz'].numpy(), dz, rtol=1e-3, atol=1e-7)
    assert value < 0 and np.isfinite(g['dz'].numpy()).all()
    assert (g['dz'][g['rows'][6:15].long()] == 0).all() and float(g['m2'][1 if S == 2 else 3]) == 0.0


def _engines(kind, dim_s, use_mmd, dev='cpu'):
    from drvae_amd import data as D
    over = dict(use_MMD=True, mmd_rate=0.7, kernel_MMD='identity') if use_mmd else {}
    spec, big, ds = NC.dataset(kind, dim_s, dev, **over)
    params = M.init_params(spec, 3, as_numpy=True)
    bat = D.DeviceBatcher(ds, torch.ones(400), 24, group_counts=NC.group_counts(big), seed=5, carry_s=True)
    fed, a1 = make_engine(spec, params, dev)
    host, a0 = make_engine(spec, params, dev)
    return spec, big, ds, bat, fed, a1, host, a0


@pytest.mark.parametrize('use_mmd', [False, True])
@pytest.mark.parametrize('dim_s', [2, 3])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_epoch_feed_with_nuisance_classes_equals_host_fed_steps_cpu(kind, dim_s, use_mmd, monkeypatch):
    """CPU twin of the GPU epoch test: an epoch through ``begin_epoch(table=...)`` on the plan that carries the classes
    (eager steps that gather through the live feed) against a second engine fed the same rows and classes from the host"""
    kernel_ref.install(monkeypatch)
    spec, big, ds, bat, fed, a1, host, a0 = _engines(kind, dim_s, use_mmd)
    tab = NC.epoch_table(big, dim_s, 6)
    NC.assert_every_side_filled(kind, big, tab, dim_s, bat.has_x2 * (kind != 'vfae'), bat.has_y * (kind != 'pvae'))
    p = bat.bind(fed)
    assert p.carry_s and (p.mmd_grouped is not None) == use_mmd and not hasattr(p, 'mmd_sig')
    bat.begin_epoch(n_batches=6, table=torch.from_numpy(tab))
    assert fed.plan.live_feed is not None and fed.plan.live_feed.s32.dtype == torch.int32
    for b in range(6):
        fed.train_step()
        i = torch.from_numpy(tab[b])
        np.testing.assert_array_equal(fed.plan.s_cls.numpy(), big['s'].reshape(-1)[tab[b]])
        host.set_batch(ds.x1[i], ds.x2[i], ds.y[i], bat.has_x2, bat.has_y, s=ds.s[i])
        assert not host.plan.carry_s
        host.train_step()
        if use_mmd:
            np.testing.assert_allclose(fed.plan.MMDval.numpy(), host.plan.MMDval.numpy(), rtol=2e-5)
            assert float((fed.plan.DZMMD - host.plan.DZMMD).norm() / host.plan.DZMMD.norm()) < 2e-5
            assert float(host.plan.MMDval) < 0
        lf, lh = fed.losses(), host.losses()
        for k in lf:
            np.testing.assert_allclose(lf[k], lh[k], rtol=1e-4, atol=1e-6)
    if use_mmd:
        assert float((a1.param - a0.param).norm() / a0.param.norm()) < 1e-4
    else:
        assert torch.equal(a1.param, a0.param)


def test_explicit_batches_feed_the_same_class_vector_cpu(monkeypatch):
    """``DeviceBatcher.feed()`` and ``set_batch`` with a device ``s`` on the plan that carries the classes == the epoch feed"""
    kernel_ref.install(monkeypatch)
    spec, big, ds, bat, fed, a1, twin, a0 = _engines('drvae', 3, True)
    tab = NC.epoch_table(big, 3, 4, vary=True)
    bat.bind(fed)
    bat.begin_epoch(n_batches=4, table=torch.from_numpy(tab))
    bat2 = type(bat)(ds, torch.ones(400), 24, group_counts=NC.group_counts(big), seed=5, carry_s=True)
    bat2.bind(twin)
    assert twin.plan.key == fed.plan.key and twin.plan.key[-1] == 'carry_s'
    for b in range(4):
        fed.train_step()
        i = torch.from_numpy(tab[b])
        if b % 2:
            bat2.feed(i)
        else:
            twin.carry_s = True
            twin.set_batch(ds.x1[i], ds.x2[i], ds.y[i], bat.has_x2, bat.has_y, s=ds.s[i])
        assert twin.plan.live_feed is None and torch.equal(twin.plan.s_cls, fed.plan.s_cls)
        assert torch.equal(twin.plan.SOHe, fed.plan.SOHe) and torch.equal(twin.plan.SOHd, fed.plan.SOHd)
        twin.train_step()
        assert fed.losses() == twin.losses()
    assert torch.equal(a1.param, a0.param)
    assert len({tuple(np.bincount(big['s'].reshape(-1)[tab[b]], minlength=3)) for b in range(4)}) > 1


def test_what_is_still_refused(monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd import data as D
    for use_mmd in (False, True):
        over = dict(use_MMD=True, kernel_MMD='identity') if use_mmd else {}
        spec, big, ds = NC.dataset('drvae', 2, 'cpu', **over)
        params = M.init_params(spec, 3, as_numpy=True)
        eng, _ = make_engine(spec, params)
        plain = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5)
        assert plain.carry_s is False
        if use_mmd:
            with pytest.raises(NotImplementedError):
                plain.bind(eng)
        else:
            assert not plain.bind(eng).carry_s
            with pytest.raises(NotImplementedError):
                plain.begin_epoch()
        with pytest.raises(NotImplementedError):
            D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, mode='sampler', carry_s=True).bind(eng)
        if use_mmd:
            with pytest.raises(AssertionError, match='sharded'):
                D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, carry_s=True).bind(eng, dp=(0, 2))
    # a model without use_s: carry_s changes nothing
    spec = NC.C.tiny_spec('drvae')
    eng, _ = make_engine(spec, M.init_params(spec, 3, as_numpy=True))
    p = D.DeviceBatcher(ds, torch.ones(400), 24, seed=5, carry_s=True).bind(eng)
    assert not p.carry_s and p.key[-1] != 'carry_s'
