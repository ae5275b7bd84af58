"""CPU: the cheaper rungs of the opt-in matmul precision ladder ("bf16x2", "bf16x1") without a device -- the contract's
emulation (tests/x3_ref.py with the rungs' term lists), the truncation bounds derived from bf16's unit roundoff, the routing
of ``StepConfig.matmul`` through plan / chain (exactly the decoder-heads layer on the raw-heads route, ``parts=`` only for
the new rungs) and the C-ABI surface of ``dv_gemm_split`` / ``dv_gemm_split_ok`` (pure host checks).  The kernels are checked
on the GPU (tests/test_gpu_split.py)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref, x3_ref
from tests.golden import cases as C
from tests.test_x3_cpu import DV_ERR_UNSUPPORTED, RAW_TUNE, desc, full_significands, make_engine, scaled_permutation

TERMS = {2: ((0, 0), (0, 1), (1, 0)), 1: ((0, 0),)}
DV_ERR_ARG = -1          # include/drvae_hip.h


# ------------------------------------------------------------------------------------------------ the emulation
def test_term_identities_hold_in_the_emulation():
    """the identities the GPU test asks of the kernels bit for bit: each kept term is needed (an identity that isolates it
    fails without it), and mid mid is absent from the two-part product"""
    n = 48
    A24, P = full_significands((37, n), 5), scaled_permutation(n, 6)
    hi, mid, _ = x3_ref.split(A24)
    A16 = hi + mid                                                      # 16 significand bits: two parts hold it exactly
    assert torch.equal(A16.double(), hi.double() + mid.double()) and bool((mid != 0).all())
    exact = A16.double() @ P.double()
    assert torch.equal(x3_ref.matmul(A16, P, TERMS[2]), exact)                           # needs hi hi, mid hi
    for drop in ((0, 0), (1, 0)):
        assert not torch.equal(x3_ref.matmul(A16, P, [t for t in TERMS[2] if t != drop]), exact), drop
    assert torch.equal(x3_ref.matmul(A16, P, [t for t in TERMS[2] if t != (0, 1)]), exact)   # (P has no mid part)
    B16 = A16[:29].t().contiguous()
    exact = P.double() @ B16.double()
    assert torch.equal(x3_ref.matmul(P, B16, TERMS[2]), exact)                           # needs hi hi, hi mid
    for drop in ((0, 0), (0, 1)):
        assert not torch.equal(x3_ref.matmul(P, B16, [t for t in TERMS[2] if t != drop]), exact), drop
    # two parts do NOT hold 24 bits: the lo terms of the three-part product are missing
    assert not torch.equal(x3_ref.matmul(A24, P, TERMS[2]), A24.double() @ P.double())
    # one part: bf16 numbers are exact, and the one term is needed
    assert torch.equal(x3_ref.matmul(hi, P, TERMS[1]), hi.double() @ P.double())
    assert not torch.equal(x3_ref.matmul(hi, P, ()), hi.double() @ P.double())
    assert not torch.equal(x3_ref.matmul(A16, P, TERMS[1]), A16.double() @ P.double())
    # mid mid is absent for two parts: (1 + 2^-10)^2 = 1 + 2^-9 + 2^-20 comes out as 1 + 2^-9 exactly
    a = torch.zeros(3, 16)
    a[1, 5] = 1 + 2.0 ** -10
    at = a.t().contiguous()
    assert float(x3_ref.matmul(a, at, TERMS[2])[1, 1]) == 1 + 2.0 ** -9
    assert float(x3_ref.matmul(a, at, TERMS[2] + ((1, 1),))[1, 1]) == 1 + 2.0 ** -9 + 2.0 ** -20
    assert float(x3_ref.matmul(a, at, TERMS[1])[1, 1]) == 1.0
    # round to nearest even, the ties the GPU test uses
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9 + 3 * 2.0 ** -17])
    hi, mid, _ = x3_ref.split(t)
    assert hi.tolist() == [1.0, 1 + 2.0 ** -6, 1.0, 1.0]
    assert mid.tolist()[2:] == [2.0 ** -9, 2.0 ** -9 * (1 + 2.0 ** -6)]


@pytest.mark.parametrize('Kdim', [4, 20, 100, 980, 2048])
def test_truncation_bounds(Kdim):
    """from bf16's unit roundoff u = 2^-8 (|a - hi| <= u |a|, |a - hi - mid| <= u^2 |a|): two parts
    |c_P - c64| <= (3 u^2 + 2^-30) sum |a||b|, one part |c_P - c64| <= (2 u + u^2) sum |a||b|, element-wise"""
    g = torch.Generator().manual_seed(1000 * Kdim)
    M_, N = (203, 331) if Kdim < 2048 else (389, 517)
    Aop, Bop = torch.randn(M_, Kdim, generator=g), torch.randn(Kdim, N, generator=g)
    c64, mag = Aop.double() @ Bop.double(), Aop.double().abs() @ Bop.double().abs()
    worst = {}
    for parts, bound in ((2, 3 * 2.0 ** -16 + 2.0 ** -30), (1, 2.0 ** -7 + 2.0 ** -16)):
        worst[parts] = float(((x3_ref.matmul(Aop, Bop, TERMS[parts]) - c64).abs() / (bound * mag)).max())
        assert worst[parts] <= 1.0, (parts, worst)
    print('truncation K=%d: worst |c_P - c64| / bound: two parts %.3f, one part %.3f' % (Kdim, worst[2], worst[1]))


# ------------------------------------------------------------------------------------------------ routing
def install_with_parts(monkeypatch, seen):
    """spies over the CPU stand-ins: note every PRODUCT a launcher call stands for with the keywords it was routed by
    (None: not routed; else the ``parts`` keyword, 'absent' when the call did not pass one) and run the fp32 stand-in
    whatever they say (the routing is what is tested here)"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)

    def how(kw):
        x3, parts = kw.pop('x3', False), kw.pop('parts', 'absent')
        assert x3 or parts == 'absent', 'parts= without x3=True'
        return parts if x3 else None

    def gemm(Cm, A, B, a_kc, b_kc, **kw):
        seen.append(('gemm', tuple(Cm.shape), bool(a_kc), bool(b_kc), how(kw)))
        return kernel_ref.gemm(Cm, A, B, a_kc, b_kc, **kw)

    def linear_bwd_pair(dW, dbias, dx, dpre, x, W, **kw):
        h = how(kw)
        seen.append(('dW', tuple(dW.shape), False, False, h))
        seen.append(('dX', tuple(dpre.shape[:1]) + tuple(W.shape[1:]), True, False, h))
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
        install_with_parts(monkeypatch, seen)
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
        del seen[:]
        eng.training = False
        eng.forward()
        assert all(np.isfinite(v) for v in eng.losses().values())
        return spec, eng, per_step, list(seen)
    finally:
        if tune:
            monkeypatch.delenv('DRVAE_TUNE')
        T.reload()


@pytest.mark.parametrize('mm,parts', [('bf16x2', 2), ('bf16x1', 1)])
def test_new_rungs_route_exactly_the_three_heads_products(monkeypatch, mm, parts):
    spec, eng, per_step, evaluation = run_steps(monkeypatch, RAW_TUNE, matmul=mm)
    X, H, Md = spec.dim_x, spec.h_de_x[-1], eng.plan.DPX.shape[0]
    assert eng.plan.c_decx.x3_last is True and eng.plan.c_decx.x3_parts == parts
    for seen in per_step:
        routed = [s for s in seen if s[-1] is not None]
        assert sorted(routed) == sorted([('gemm', (Md, 2 * X), True, True, parts), ('dW', (2 * X, H), False, False, parts),
                                         ('dX', (Md, H), True, False, parts)]), routed
        assert len(seen) > len(routed)             # ... and every other product of the step stays fp32
    # an evaluation pass on the same route: the heads' forward product only
    assert [s for s in evaluation if s[-1] is not None] == [('gemm', (Md, 2 * X), True, True, parts)]


@pytest.mark.parametrize('mm', ['bf16x2', 'bf16x1'])
def test_new_rungs_without_the_raw_heads_route_route_nothing(monkeypatch, mm):
    _, eng, per_step, evaluation = run_steps(monkeypatch, None, matmul=mm)
    assert all(seen and all(s[-1] is None for s in seen) for seen in per_step)
    assert all(s[-1] is None for s in evaluation)
    assert eng.plan.c_decx.x3_last is False


def test_fp32_and_bf16x3_pass_no_parts_keyword(monkeypatch):
    """for 'fp32' and 'bf16x3' the launcher calls are keyword for keyword what they were: ``x3=True`` alone means three parts"""
    _, eng, per_step, evaluation = run_steps(monkeypatch, RAW_TUNE, matmul='bf16x3')
    for seen in per_step + [evaluation]:
        assert [s[-1] for s in seen if s[-1] is not None] in (['absent'] * 3, ['absent'])
    assert eng.plan.c_decx.x3_last is True and eng.plan.c_decx.x3_parts == 3
    _, eng, per_step, evaluation = run_steps(monkeypatch, RAW_TUNE)
    assert all(seen and all(s[-1] is None for s in seen) for seen in per_step + [evaluation])
    assert eng.plan.c_decx.x3_last is False


def test_matmul_names():
    from drvae_amd import engine as E
    assert E.MATMUL_CHOICES == ('fp32', 'bf16x3', 'bf16x2', 'bf16x1')
    for mm in E.MATMUL_CHOICES:
        assert E.StepConfig(matmul=mm).matmul == mm
    for bad in ('bf16', 'bf16x4', 'bf16x0', 'BF16X2'):
        with pytest.raises(ValueError):
            E.StepConfig(matmul=bad)
    from drvae_amd.DrVAE import DrVAE
    from drvae_amd.PVAE import PVAE
    from drvae_amd.VFAE import VFAE
    import inspect
    for cls in (DrVAE, PVAE, VFAE):
        assert inspect.signature(cls.__init__).parameters['matmul_precision'].default == 'fp32'
    kw = dict(dim_x=16, dim_s=2, dim_y=2, dim_z1=4, dim_z3=4, dim_h_en_z1=[8], dim_h_en_z3=[4], dim_h_de_z1=[4],
              dim_h_de_x=[8], dim_h_clf=[], device='cpu')
    for mm in ('bf16x2', 'bf16x1'):
        mdl = DrVAE(matmul_precision=mm, **kw)
        assert mdl._matmul == mm
        assert list(mdl.state_dict().keys()) == list(DrVAE(**kw).state_dict().keys())
    with pytest.raises(ValueError):
        DrVAE(matmul_precision='bf16', **kw)


@pytest.mark.parametrize('mm', ['bf16x2', 'bf16x1'])
def test_plan_refuses_a_heads_layer_the_kernels_do_not_run(monkeypatch, mm):
    """decided once, where the plan is built: a decoder without hidden layers takes the raw route, but its gradient
    products are no plain pair -> ValueError naming the rung, the entry point and the reason"""
    from drvae_amd import tuning as T
    monkeypatch.setenv('DRVAE_TUNE', RAW_TUNE)
    T.reload()
    try:
        install_with_parts(monkeypatch, [])
        spec = C.tiny_spec('drvae', h_de_x=[])
        b = M.make_batch(spec, 12, seed=3)
        eng, _ = make_engine(spec, M.init_params(spec, 4, as_numpy=True), matmul=mm)
        t = lambda k: torch.from_numpy(b[k].copy())
        with pytest.raises(ValueError, match="matmul='%s'.*dv_gemm_split.*only one" % mm):
            eng.set_batch(t('x1'), t('x2'), b['y'], b['has_x2'], b['has_y'])
    finally:
        monkeypatch.delenv('DRVAE_TUNE')
        T.reload()


def test_refusals_take_parts():
    """``x3_refusal`` / ``x3_pair_refusal`` with ``parts=``: the library's verdict, with a reason (any device: nothing is launched)"""
    import drvae_amd.kernels as K
    x, W, out = torch.zeros(24, 8), torch.zeros(40, 8), torch.zeros(24, 40)
    for parts in (1, 2, 3):
        assert K.x3_refusal(out, x, W, True, True, parts=parts) is None
        assert 'epilogue' in K.x3_refusal(out, x, W, True, True, parts=parts, epi=K.EPI_FWD, bias=torch.zeros(40))
        dpre, dW, dx = torch.zeros(24, 40), torch.zeros(40, 8), torch.zeros(24, 8)
        assert K.x3_pair_refusal(dW, None, dx, dpre, x, W, parts=parts) is None
        assert 'a_kscale' in K.x3_pair_refusal(dW, None, dx, dpre, x, W, parts=parts, kscale=torch.zeros(40))
    assert K.x3_refusal(out, x, W, True, True) is None
    for bad in (0, 4):
        assert 'parts' in K.x3_refusal(out, x, W, True, True, parts=bad)
    x6 = torch.zeros(24, 8)[:, :6]
    assert 'K = 6' in K.x3_refusal(out, x6, W[:, :6], True, True, parts=2)
    assert K.x3_refusal(out, x6, W[:, :6], True, True, parts=2, overread=True) is None


# ------------------------------------------------------------------------------------------------ ABI surface
def test_abi_surface_without_a_device():
    from drvae_amd import _lib
    lib = _lib.load()
    ok = lambda d, p: lib.dv_gemm_split_ok(ctypes.byref(d), p)
    assert lib.dv_gemm_split_ok(None, 2) == 0
    for p in (1, 2, 3):
        assert lib.dv_gemm_split(None, p, None) == DV_ERR_ARG
    # the descriptors of tests/test_x3_cpu.py::test_abi_surface_without_a_device: the verdict is dv_gemm_x3_ok's for every rung
    fwd = desc(8192, 40000, 2048, 1, 1, 2048, 2048, 40000)
    dW = desc(40000, 2048, 8192, 0, 0, 40000, 2048, 2048)
    dWb = desc(40000, 2048, 8192, 0, 0, 40000, 2048, 2048, a_colsum=0x40000)
    dX = desc(8192, 2048, 40000, 1, 0, 40000, 2048, 2048, epilogue=_lib.EPI_BWD, yref=0x50000, ldy=2048, act0=1, act1=1)
    accepted = [fwd, dW, dWb, dX, desc(8192, 40000, 2048, 1, 1, 2048, 2048, 40000, beta=1.0, alpha=0.5),
                desc(77, 33, 20, 1, 1, 20, 20, 33), desc(0, 33, 20, 1, 1, 20, 20, 33),
                desc(64, 64, 62, 1, 1, 64, 64, 64, flags=3), desc(64, 64, 62, 1, 0, 64, 64, 64, flags=1),
                desc(64, 64, 62, 0, 0, 64, 64, 64)]
    refused = dict(
        A2=desc(64, 64, 64, 1, 1, 64, 64, 64, A2=0x60000, lda2=32, K1=32),
        a_kscale=desc(64, 64, 64, 1, 0, 64, 64, 64, a_kscale=0x60000),
        epi_fwd=desc(64, 64, 64, 1, 1, 64, 64, 64, epilogue=_lib.EPI_FWD),
        epi_klq=desc(64, 64, 64, 1, 0, 64, 64, 128, epilogue=_lib.EPI_KLQ),
        k_mod_4=desc(64, 64, 62, 1, 1, 64, 64, 64),
        k_mod_4_a_only=desc(64, 64, 62, 1, 1, 64, 64, 64, flags=1),
        k_mod_4_b_flag=desc(64, 64, 62, 1, 0, 64, 64, 64, flags=2),
        pub_flag=desc(64, 64, 64, 1, 1, 64, 64, 64, pub_flag=0x60000, pub_ctr=0x70000),
        lda=desc(64, 64, 64, 1, 1, 66, 64, 64), ldb=desc(64, 64, 64, 1, 1, 64, 66, 64),
        A_ptr=desc(64, 64, 64, 1, 1, 64, 64, 64, A=0x10004), B_ptr=desc(64, 64, 64, 1, 1, 64, 64, 64, B=0x20008),
        layout=desc(64, 64, 64, 0, 1, 64, 64, 64),
        colsum_layout=desc(64, 64, 64, 1, 0, 64, 64, 64, a_colsum=0x40000))
    for d in accepted:
        assert lib.dv_gemm_x3_ok(ctypes.byref(d)) == 1
        assert [ok(d, p) for p in (1, 2, 3)] == [1, 1, 1]
        assert [ok(d, p) for p in (0, 4, -1, 19)] == [0, 0, 0, 0]                 # parts outside 1..3
        for p in (0, 4):
            assert lib.dv_gemm_split(ctypes.byref(d), p, None) == DV_ERR_ARG
    for name, d in refused.items():
        assert lib.dv_gemm_x3_ok(ctypes.byref(d)) == 0, name
        for p in (1, 2, 3):
            assert ok(d, p) == 0, (name, p)
            assert lib.dv_gemm_split(ctypes.byref(d), p, None) == DV_ERR_UNSUPPORTED, (name, p)
    assert lib.dv_abi_version() == _lib.ABI_VERSION
