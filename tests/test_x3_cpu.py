"""CPU: the opt-in split-bf16 ("bf16x3") path without a device -- the contract's emulation (tests/x3_ref.py), the routing of
``StepConfig.matmul='bf16x3'`` through plan / chain (exactly the decoder-heads layer on the raw-heads route), and the C-ABI
surface of ``dv_gemm_x3`` / ``dv_gemm_x3_ok`` (pure host checks).  The kernels are checked on the GPU (tests/test_gpu_x3.py)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref, x3_ref
from tests.golden import cases as C


# ------------------------------------------------------------------------------------------------ the emulation
def full_significands(shape, seed):
    """normal-range fp32 numbers with all 24 significand bits in use (odd 24-bit integers times a power of two)"""
    rs = np.random.RandomState(seed)
    m = (rs.randint(2 ** 22, 2 ** 23, size=shape).astype(np.int64) * 2 + 1)
    e = rs.randint(-30, -10, size=shape)
    s = rs.choice([-1.0, 1.0], size=shape)
    v = (s * m * np.exp2(e.astype(np.float64))).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), s * m * np.exp2(e.astype(np.float64)))
    return torch.from_numpy(v)


def scaled_permutation(n, seed):
    rs = np.random.RandomState(seed)
    P = np.zeros((n, n), np.float32)
    P[np.arange(n), rs.permutation(n)] = np.exp2(rs.randint(-6, 7, size=n)).astype(np.float32)
    return torch.from_numpy(P)


def test_split_is_exact_for_normal_range_fp32():
    a = torch.cat([torch.randn(20000, generator=torch.Generator().manual_seed(1)),
                   full_significands((20000,), 2),
                   torch.randn(20000, generator=torch.Generator().manual_seed(3)) * 1e-20,
                   torch.randn(20000, generator=torch.Generator().manual_seed(4)) * 1e20])
    hi, mid, lo = x3_ref.split(a)
    for part in (hi, mid, lo):          # every part is a bf16 number
        assert torch.equal(part, part.to(torch.bfloat16).to(torch.float32))
    assert torch.equal(hi.double() + mid.double() + lo.double(), a.double())


def test_six_term_identities_hold_in_the_emulation():
    """the identities the GPU test asks of the kernel bit for bit: each needs some of the six terms and fails without them"""
    n = 48
    A, P = full_significands((37, n), 5), scaled_permutation(n, 6)
    exact = A.double() @ P.double()
    assert torch.equal(exact.float().double(), exact)                     # (a scaled permutation: exactly representable)
    assert torch.equal(x3_ref.matmul(A, P), exact)                        # needs hi hi, mid hi, lo hi
    for drop in ((0, 0), (1, 0), (2, 0)):
        assert not torch.equal(x3_ref.matmul(A, P, [t for t in x3_ref.TERMS if t != drop]), exact), drop
    B = full_significands((n, 29), 7)
    exact = P.double() @ B.double()
    assert torch.equal(x3_ref.matmul(P, B), exact)                        # needs hi hi, hi mid, hi lo
    for drop in ((0, 0), (0, 1), (0, 2)):
        assert not torch.equal(x3_ref.matmul(P, B, [t for t in x3_ref.TERMS if t != drop]), exact), drop
    a = torch.zeros(3, 16)
    a[1, 5] = 1 + 2.0 ** -10
    want = 1 + 2.0 ** -9 + 2.0 ** -20
    got = x3_ref.matmul(a, a.t().contiguous())
    assert float(got[1, 1]) == want and float(np.float32(want)) == want   # needs mid mid
    assert float(x3_ref.matmul(a, a.t().contiguous(), [t for t in x3_ref.TERMS if t != (1, 1)])[1, 1]) != want


# ------------------------------------------------------------------------------------------------ routing
RAW_TUNE = 'fuse_heads=0,raw_heads=2,nll_cs=2'
DV_ERR_UNSUPPORTED = -3          # include/drvae_hip.h


def make_engine(spec, params, **cfg_over):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    kw.update(cfg_over)
    cfg = E.StepConfig(**kw)
    arena = ParamArena(E.param_shapes(cfg), 'cpu', frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena), arena


def install_with_x3(monkeypatch, seen):
    """spies over the CPU stand-ins: note every PRODUCT a launcher call stands for together with its ``x3=`` flag, and run
    the fp32 stand-in whatever the flag says (the routing is what is tested here)"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)

    def gemm(Cm, A, B, a_kc, b_kc, x3=False, **kw):
        seen.append(('gemm', tuple(Cm.shape), bool(a_kc), bool(b_kc), bool(x3)))
        return kernel_ref.gemm(Cm, A, B, a_kc, b_kc, **kw)

    def linear_bwd_pair(dW, dbias, dx, dpre, x, W, x3=False, **kw):
        seen.append(('dW', tuple(dW.shape), False, False, bool(x3)))
        seen.append(('dX', tuple(dpre.shape[:1]) + tuple(W.shape[1:]), True, False, bool(x3)))
        return kernel_ref.linear_bwd_pair(dW, dbias, dx, dpre, x, W, **kw)
    monkeypatch.setattr(K, 'gemm', gemm)
    monkeypatch.setattr(K, 'linear_bwd_pair', linear_bwd_pair)


def run_steps(monkeypatch, tune, n_steps=2, **cfg_over):
    from drvae_amd import tuning as T
    if tune:
        monkeypatch.setenv('DRVAE_TUNE', tune)
    T.reload()
    try:
        seen = []
        install_with_x3(monkeypatch, seen)
        case = C.model_case('tiny_drvae')
        spec = case['spec']
        eng, arena = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), **cfg_over)
        t = lambda k: torch.from_numpy(case['batch'][k].copy())
        eng.set_batch(t('x1'), t('x2'), case['batch']['y'], case['batch']['has_x2'], case['batch']['has_y'])
        per_step = []
        for noise in case['noises'][:n_steps]:
            del seen[:]
            eng.train_step(noise)
            per_step.append(list(seen))
        assert all(np.isfinite(v) for v in eng.losses().values())
        return spec, eng, per_step
    finally:
        if tune:
            monkeypatch.delenv('DRVAE_TUNE')
        T.reload()


def test_bf16x3_routes_exactly_the_three_heads_products(monkeypatch):
    spec, eng, per_step = run_steps(monkeypatch, RAW_TUNE, matmul='bf16x3')
    X, H, Md = spec.dim_x, spec.h_de_x[-1], eng.plan.DPX.shape[0]
    for seen in per_step:
        x3 = [s for s in seen if s[-1]]
        assert sorted(s[:4] for s in x3) == sorted([('gemm', (Md, 2 * X), True, True), ('dW', (2 * X, H), False, False),
                                                    ('dX', (Md, H), True, False)]), x3
        assert len(seen) > len(x3)                 # ... and every other product of the step stays fp32
    # an evaluation pass on the same route: the heads' forward product only
    from drvae_amd import tuning as T
    monkeypatch.setenv('DRVAE_TUNE', RAW_TUNE)
    T.reload()
    try:
        seen = []
        install_with_x3(monkeypatch, seen)
        eng.training = False
        eng.forward()
        assert [s[:2] for s in seen if s[-1]] == [('gemm', (Md, 2 * X))]
    finally:
        monkeypatch.delenv('DRVAE_TUNE')
        T.reload()


def test_default_config_routes_nothing(monkeypatch):
    _, _, per_step = run_steps(monkeypatch, RAW_TUNE)
    assert all(seen and not any(s[-1] for s in seen) for seen in per_step)


def test_bf16x3_without_the_raw_heads_route_routes_nothing(monkeypatch):
    _, _, per_step = run_steps(monkeypatch, None, matmul='bf16x3')
    assert all(seen and not any(s[-1] for s in seen) for seen in per_step)


def test_bad_matmul_value_raises():
    from drvae_amd import engine as E
    for bad in ('bf16', 'tf32', '', None, 'FP32'):
        with pytest.raises(ValueError):
            E.StepConfig(matmul=bad)
    assert E.StepConfig().matmul == 'fp32' and E.StepConfig(matmul='bf16x3').matmul == 'bf16x3'
    from drvae_amd.DrVAE import DrVAE
    with pytest.raises(ValueError):
        DrVAE(dim_x=16, dim_s=2, dim_y=2, dim_z1=4, dim_z3=4, dim_h_en_z1=[8], dim_h_en_z3=[4], dim_h_de_z1=[4],
              dim_h_de_x=[8], dim_h_clf=[], device='cpu', matmul_precision='bf16')


def test_plan_refuses_a_heads_layer_the_kernels_do_not_run(monkeypatch):
    """decided once, where the plan is built: a WeightNorm model's heads cannot take the raw route at all (nothing routed),
    a decoder without hidden layers can, but its gradient products are no plain pair -> ValueError naming the reason"""
    from drvae_amd import tuning as T
    monkeypatch.setenv('DRVAE_TUNE', RAW_TUNE)
    T.reload()
    try:
        seen = []
        install_with_x3(monkeypatch, seen)
        spec = C.tiny_spec('drvae', h_de_x=[])
        b = M.make_batch(spec, 12, seed=3)
        eng, _ = make_engine(spec, M.init_params(spec, 4, as_numpy=True), matmul='bf16x3')
        t = lambda k: torch.from_numpy(b[k].copy())
        with pytest.raises(ValueError, match='dv_gemm_x3'):
            eng.set_batch(t('x1'), t('x2'), b['y'], b['has_x2'], b['has_y'])
    finally:
        monkeypatch.delenv('DRVAE_TUNE')
        T.reload()


# ------------------------------------------------------------------------------------------------ ABI surface
def desc(M_, N, K, a_kc, b_kc, lda, ldb, ldc, **over):
    from drvae_amd import _lib
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.a_kcontig, d.b_kcontig = M_, N, K, a_kc, b_kc
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = 0x10000, lda, 0x20000, ldb, 0x30000, ldc       # dummy 16-B aligned addresses
    d.alpha, d.split, d.K1 = 1.0, N, K
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_abi_surface_without_a_device():
    from drvae_amd import _lib
    lib = _lib.load()
    assert lib.dv_gemm_x3(None, None) == -1 and lib.dv_gemm_x3_ok(None) == 0
    ok = lambda d: lib.dv_gemm_x3_ok(ctypes.byref(d))
    # the three decoder-heads products of the wide configuration: 8192 rows, 2 x 20000 genes, 2048 hidden units
    fwd = desc(8192, 40000, 2048, 1, 1, 2048, 2048, 40000)
    dW = desc(40000, 2048, 8192, 0, 0, 40000, 2048, 2048)
    dWb = desc(40000, 2048, 8192, 0, 0, 40000, 2048, 2048, a_colsum=0x40000)
    dX = desc(8192, 2048, 40000, 1, 0, 40000, 2048, 2048, epilogue=_lib.EPI_BWD, yref=0x50000, ldy=2048, act0=1, act1=1)
    assert [ok(d) for d in (fwd, dW, dWb, dX)] == [1, 1, 1, 1]
    assert ok(desc(8192, 40000, 2048, 1, 1, 2048, 2048, 40000, beta=1.0, alpha=0.5)) == 1
    assert ok(desc(77, 33, 20, 1, 1, 20, 20, 33)) == 1 and ok(desc(0, 33, 20, 1, 1, 20, 20, 33)) == 1
    refused = dict(
        A2=desc(64, 64, 64, 1, 1, 64, 64, 64, A2=0x60000, lda2=32, K1=32),
        a_kscale=desc(64, 64, 64, 1, 0, 64, 64, 64, a_kscale=0x60000),
        epi_fwd=desc(64, 64, 64, 1, 1, 64, 64, 64, epilogue=_lib.EPI_FWD),
        epi_klq=desc(64, 64, 64, 1, 0, 64, 64, 128, epilogue=_lib.EPI_KLQ),
        k_mod_4=desc(64, 64, 62, 1, 1, 64, 64, 64),
        pub_flag=desc(64, 64, 64, 1, 1, 64, 64, 64, pub_flag=0x60000, pub_ctr=0x70000),
        lda=desc(64, 64, 64, 1, 1, 66, 64, 64), ldb=desc(64, 64, 64, 1, 1, 64, 66, 64),
        A_ptr=desc(64, 64, 64, 1, 1, 64, 64, 64, A=0x10004), B_ptr=desc(64, 64, 64, 1, 1, 64, 64, 64, B=0x20008),
        layout=desc(64, 64, 64, 0, 1, 64, 64, 64),
        colsum_layout=desc(64, 64, 64, 1, 0, 64, 64, 64, a_colsum=0x40000))
    for name, d in refused.items():
        assert ok(d) == 0, name
        assert lib.dv_gemm_x3(ctypes.byref(d), None) == DV_ERR_UNSUPPORTED, name
    # K % 4 != 0 runs only on the caller's word (flags) that the k-contiguous operands' row ends may be over-read
    assert ok(desc(64, 64, 62, 1, 1, 64, 64, 64, flags=3)) == 1 and ok(desc(64, 64, 62, 1, 1, 64, 64, 64, flags=1)) == 0
    assert ok(desc(64, 64, 62, 1, 0, 64, 64, 64, flags=1)) == 1 and ok(desc(64, 64, 62, 1, 0, 64, 64, 64, flags=2)) == 0
    assert ok(desc(64, 64, 62, 0, 0, 64, 64, 64)) == 1       # (rows along M / N: no chunk straddles K)
    assert lib.dv_abi_version() == _lib.ABI_VERSION
