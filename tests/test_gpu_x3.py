"""GPU: the opt-in split-bf16 ("bf16x3") products -- ``dv_gemm_x3`` against its arithmetic contract (exact terms bit for
bit, accuracy against float64 next to the fp32 MFMA product on the same operands, bitwise reproducibility), the engine on
top of it (the reference's golden vectors at the tolerances of the fp32 step, capture / replay, the model keyword) and the
one thing the path is for: time (it must beat the fp32 path on the wide configuration's three products and step)."""
import os

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import ref64
from tests.golden import cases as C
from tests.test_gpu_engine import GRAD_RTOL, LOSS_RTOL, NORM_RTOL, close, rel_norm
from tests.test_x3_cpu import full_significands, scaled_permutation

pytestmark = pytest.mark.gpu

RAW_TUNE = 'fuse_heads=0,raw_heads=2,nll_cs=2'
U = 2.0 ** -24
LAYOUTS = ((True, True), (True, False), (False, False))


def K_():
    import drvae_amd.kernels as K
    return K


def store(op, kc, dev, pad=0, fill=float('nan')):
    """the (rows, k) operand ``op`` as a strided view into a wider device buffer, stored k-contiguous or not; the rest of
    the buffer is NaN: anything read outside the operand poisons the result"""
    t = op if kc else op.t()
    r, c = t.shape
    ld = (c + 3) // 4 * 4 + pad
    buf = torch.full((r, ld), fill, dtype=torch.float32, device=dev)
    buf[:, :c] = t.to(dev)
    return buf[:, :c]


def run_x3(dev, Aop, Bop, a_kc, b_kc, x3=True, Cinit=None, **kw):
    """Aop (M, K), Bop (K, N) host tensors -> device result of gemm(..., x3=x3) in the given layout"""
    K = K_()
    A = store(Aop, a_kc, dev)
    B = store(Bop.t(), b_kc, dev)
    M_, N = Aop.shape[0], Bop.shape[1]
    Cbuf = torch.full((M_, N + 5), 7.0, device=dev)
    Cm = Cbuf[:, :N]
    if Cinit is not None:
        Cm.copy_(Cinit.to(dev))
    K.gemm(Cm, A, B, a_kc, b_kc, **(dict(x3=True) if x3 else {}), **kw)
    torch.cuda.synchronize()
    assert bool((Cbuf[:, N:] == 7.0).all())          # nothing written past the row ends
    return Cm.cpu()


# ------------------------------------------------------------------------------------------------ 1. exact terms
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_exact_terms_bit_for_bit(dev, a_kc, b_kc):
    """each identity isolates some of the six terms; a missing one changes the result (tests/test_x3_cpu.py shows that on
    the emulation)"""
    n = 48
    A, P = full_significands((37, n), 5), scaled_permutation(n, 6)
    exact = (A.double() @ P.double()).float()
    assert torch.equal(run_x3(dev, A, P, a_kc, b_kc), exact)              # hi hi, mid hi, lo hi
    B = full_significands((n, 29), 7)
    exact = (P.double() @ B.double()).float()
    assert torch.equal(run_x3(dev, P, B, a_kc, b_kc), exact)              # hi hi, hi mid, hi lo
    # across tile edges and a K tail: 150 x 200 with K = 200 (permutation of 200)
    A, P = full_significands((150, 200), 8), scaled_permutation(200, 9)
    assert torch.equal(run_x3(dev, A, P, a_kc, b_kc), (A.double() @ P.double()).float())
    a = torch.zeros(3, 16)
    a[1, 5] = 1 + 2.0 ** -10
    got = run_x3(dev, a, a.t().contiguous(), a_kc, b_kc)
    assert float(got[1, 1]) == 1 + 2.0 ** -9 + 2.0 ** -20                 # mid mid
    assert float(got.abs().sum()) == float(got[1, 1])


# ------------------------------------------------------------------------------------------------ 2. accuracy
@pytest.mark.parametrize('Kdim', [4, 20, 100, 980, 2048])
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_accuracy_against_float64(dev, a_kc, b_kc, Kdim):
    """Element-wise (derived, not chosen): |c - c64| <= 1.01 (6 K + 4) 2^-24 sum_k |a_k| |b_k| |alpha| [|act'|] -- at most
    6 K - 1 fp32 additions of exact bf16 x bf16 products, dropped terms <= 2^-22 |a| |b| -- plus the fp32 roundings of the
    epilogue's own arithmetic: alpha * acc and * act' (one rounding each, and act' itself from y - shift: a few ulp of
    1 + |y|), + beta * C (two roundings of the magnitudes added).
    Norm-wise, the tight one: the error against float64 is at most 2 x that of the fp32 MFMA product (``dv_gemm``) on the
    same operands, measured here.  Operands are strided views into wider buffers filled with NaN."""
    K = K_()
    g = torch.Generator().manual_seed(1000 * Kdim + 10 * a_kc + b_kc)
    M_, N = (203, 331) if Kdim < 2048 else (389, 517)              # ragged: no multiple of the tile, of 32 or of 4
    Aop, Bop = torch.randn(M_, Kdim, generator=g), torch.randn(Kdim, N, generator=g)
    c64 = Aop.double() @ Bop.double()
    mag = Aop.double().abs() @ Bop.double().abs()
    for epi, beta, alpha in ((K.EPI_PLAIN, 0.0, 1.0), (K.EPI_PLAIN, 1.0, -0.37), (K.EPI_BWD, 0.0, 1.0), (K.EPI_BWD, 1.0, 0.5)):
        kw, scale, ymag = dict(alpha=alpha, beta=beta), torch.ones_like(c64), torch.zeros_like(c64)
        if epi == K.EPI_BWD:
            h = N // 2
            ys = torch.randn(M_, N, generator=g)
            ys[:, h:] = ys[:, h:].abs() + 0.5                            # (a softplus output lies above its shift)
            s1 = ref64.f32(1e-3)
            kw.update(epi=K.EPI_BWD, yref=store(ys, True, dev, fill=0.0), act0='elu', act1='softplus', shift0=0.0,
                      shift1=s1, split=h)
            scale = torch.cat([ref64.dact_from_y('elu', ys[:, :h]), ref64.dact_from_y('softplus', ref64.f64(ys[:, h:]) - s1)], 1)
            ymag = 1 + ref64.f64(ys).abs()
        C0 = torch.randn(M_, N, generator=g)
        a32 = ref64.f32(alpha)
        prod = c64 * a32
        want = prod * scale + (beta * C0.double() if beta else 0.0)
        bound = 1.01 * (6 * Kdim + 4) * U * mag * abs(a32) * scale.abs() \
            + U * (2 * (prod * scale).abs() + 8 * prod.abs() * ymag + 2 * (beta * C0.double()).abs() + 2 * want.abs())
        got = {}
        for x3 in (True, False):
            got[x3] = run_x3(dev, Aop, Bop, a_kc, b_kc, x3=x3, Cinit=C0, **kw).double()
        err = (got[True] - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        e3, e32 = float(torch.linalg.norm(got[True] - want)), float(torch.linalg.norm(got[False] - want))
        nw = float(torch.linalg.norm(want))
        print('x3 accuracy layout=(%d,%d) K=%d epi=%d beta=%g: max err/bound %.3f, norm-wise x3 %.3e fp32 %.3e ratio %.3f'
              % (a_kc, b_kc, Kdim, epi, beta, worst, e3 / nw, e32 / nw, e3 / max(e32, 1e-300)))
        assert worst <= 1.0, (epi, beta, worst)
        assert e3 <= 2.0 * e32, (epi, beta, e3, e32)


@pytest.mark.parametrize('Kdim', [26, 62, 33])
@pytest.mark.parametrize('a_kc,b_kc', [(True, True), (True, False)])
def test_k_tail_behind_an_overread_chunk_is_masked(dev, a_kc, b_kc, Kdim):
    """K % 4 != 0 runs where ``flags`` lets the k-contiguous operands' row ends be over-read: the 16-B chunk that straddles K
    is loaded whole and what lies past K counts as zero.  The operands are views into buffers whose row pads hold NaN
    (``store``: K = 26 / 62 / 33 leave 2 / 2 / 3 NaN behind every row, inside the allocation), so an unmasked tail poisons
    the result; the bound is the element-wise one of ``test_accuracy_against_float64``.  K = 62 and 33 put the tail in
    the second / first chunk of a k tile's second 16-deep step; without the caller's word the descriptor is refused."""
    K = K_()
    g = torch.Generator().manual_seed(77 * Kdim + 2 * a_kc + b_kc)
    M_, N = 139, 150
    Aop, Bop = torch.randn(M_, Kdim, generator=g), torch.randn(Kdim, N, generator=g)
    c64 = Aop.double() @ Bop.double()
    bound = 1.01 * (6 * Kdim + 4) * U * (Aop.double().abs() @ Bop.double().abs()) + 2 * U * c64.abs()
    got = run_x3(dev, Aop, Bop, a_kc, b_kc, overread=True).double()
    assert bool(torch.isfinite(got).all())
    worst = float(((got - c64).abs() / bound).max())
    print('x3 K tail layout=(%d,%d) K=%d: max err/bound %.3f' % (a_kc, b_kc, Kdim, worst))
    assert worst <= 1.0
    with pytest.raises(RuntimeError, match='x3=True'):
        run_x3(dev, Aop, Bop, a_kc, b_kc)


def test_colsum_rides_in_front_and_refusals_touch_nothing(dev):
    K = K_()
    g = torch.Generator().manual_seed(5)
    dy, x = torch.randn(300, 70, generator=g), torch.randn(300, 44, generator=g)        # dW = dy^T x, db = dy.sum(0)
    dyd, xd = store(dy.t(), False, dev), store(x.t(), False, dev)
    dW, db = torch.zeros(70, 44, device=dev), torch.full((70,), 2.0, device=dev)
    K.gemm(dW, dyd, xd, False, False, x3=True, a_colsum=db, colsum_beta=1.0)
    torch.cuda.synchronize()
    # (300 fp32 additions in whatever order: each rounds a partial sum no larger than the column's sum of magnitudes)
    assert bool(((db.cpu().double() - (2.0 + dy.double().sum(0))).abs() <= 301 * U * (2.0 + dy.double().abs().sum(0))).all())
    assert rel_norm(dW.cpu().numpy(), (dy.double().t() @ x.double()).numpy()) <= 1e-6
    # a descriptor the kernels do not run raises up front and leaves C alone
    Cm = torch.full((300, 70), 3.0, device=dev)
    with pytest.raises(RuntimeError, match='x3=True'):
        K.gemm(Cm, xd, store(torch.randn(70, 44, generator=g), False, dev), True, False, x3=True, epi=K.EPI_FWD,
               bias=torch.zeros(70, device=dev))
    with pytest.raises(RuntimeError, match='x3=True'):
        K.linear_bwd_pair(dW, None, torch.zeros(300, 44, device=dev), dyd, xd, torch.zeros(70, 44, device=dev),
                          kscale=torch.ones(70, device=dev), x3=True)
    torch.cuda.synchronize()
    assert bool((Cm == 3.0).all())


def test_non_finite_operands_poison_what_they_feed(dev):
    g = torch.Generator().manual_seed(6)
    Aop, Bop = torch.randn(70, 64, generator=g), torch.randn(64, 90, generator=g)
    Aop[3, 7], Aop[40, 63], Bop[5, 11] = float('nan'), float('inf'), float('-inf')
    for a_kc, b_kc in LAYOUTS:
        got = run_x3(dev, Aop, Bop, a_kc, b_kc)
        bad = ~torch.isfinite(got)
        want = torch.zeros_like(bad)
        want[3, :], want[40, :], want[:, 11] = True, True, True
        assert torch.equal(bad, want)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_two_launches_are_bitwise_equal(dev, a_kc, b_kc):
    g = torch.Generator().manual_seed(7)
    Aop, Bop = torch.randn(515, 1000, generator=g), torch.randn(1000, 770, generator=g)
    assert torch.equal(run_x3(dev, Aop, Bop, a_kc, b_kc), run_x3(dev, Aop, Bop, a_kc, b_kc))


# ------------------------------------------------------------------------------------------------ 4. golden cases
def make_engine(spec, params, dev, **cfg_over):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    kw.update(cfg_over)
    cfg = E.StepConfig(**kw)
    arena = ParamArena(E.param_shapes(cfg), dev, frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena), arena


def set_batch(eng, batch, dev):
    t = lambda k: torch.from_numpy(batch[k].copy()).to(dev)
    return eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'])


class tuned:
    def __init__(self, tune):
        self.tune = tune

    def __enter__(self):
        from drvae_amd import tuning as T
        self.old = os.environ.get('DRVAE_TUNE')
        if self.tune:
            os.environ['DRVAE_TUNE'] = self.tune
        T.reload()

    def __exit__(self, *a):
        from drvae_amd import tuning as T
        if self.tune:
            if self.old is None:
                del os.environ['DRVAE_TUNE']
            else:
                os.environ['DRVAE_TUNE'] = self.old
        T.reload()


def count_x3(monkeypatch):
    from drvae_amd import _lib
    n = {'x3': 0, 'all': 0}
    real = _lib.check

    def counting(code, what):
        n['all'] += 1
        n['x3'] += what == 'dv_gemm_x3'
        return real(code, what)
    monkeypatch.setattr(_lib, 'check', counting)
    return n


@pytest.mark.parametrize('name,tune', [('cfg5_wide', None), ('cfg2_drvae', RAW_TUNE), ('tiny_drvae', RAW_TUNE)])
def test_train_steps_match_reference_golden_bf16x3(name, tune, dev, monkeypatch):
    """the assertions and tolerances of tests/test_gpu_engine.py::test_train_steps_match_reference_golden, nothing
    loosened, with ``matmul='bf16x3'`` (cfg-5 at default tuning; the small ones on the raw-heads route by the tuning
    switches: 978 genes -- ragged tile edges --, and 13 genes: a K tail in the data-gradient product)"""
    with tuned(tune):
        n = count_x3(monkeypatch)
        case, gold = C.model_case(name), C.load('model_' + name)
        spec = case['spec']
        eng, arena = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), dev, matmul='bf16x3')
        set_batch(eng, case['batch'], dev)
        eng.training = False
        eng.set_noise(case['noises'][0])
        eng.forward()
        assert n['x3'] == 1
        for k, v in eng.losses().items():
            close(v, gold['eval/' + k], LOSS_RTOL, 1e-5)
        eng.training = True
        eng.set_noise(case['noises'][0])
        eng.forward()
        eng.backward()
        assert n['x3'] == 1          # (the unfused forward / backward pair finishes the heads in the product's epilogue: fp32)
        for k in arena.shapes:
            g = arena.g(k).cpu().numpy()
            if case['full']:
                ref = gold['grad/' + k]
                close(g, ref, GRAD_RTOL, 2e-5 * max(1.0, float(np.abs(ref).max())))
                if float(np.abs(ref).max()) > 1e-6:
                    assert rel_norm(g, ref) <= NORM_RTOL, (k, rel_norm(g, ref))
            else:
                close(np.sqrt((g.astype(np.float64) ** 2).sum()), gold['gradnorm/' + k], NORM_RTOL, 1e-7)
                ref = gold['gradsample/' + k]
                close(g.reshape(-1)[C.sample_index(g.size)], ref, GRAD_RTOL, 1e-4 * max(1e-3, float(np.abs(ref).max())))
        nsteps = len(case['noises'])
        for step, noise in enumerate(case['noises']):
            eng.train_step(noise)
            for k, v in eng.losses().items():
                close(v, gold['step%d/%s' % (step, k)], LOSS_RTOL, 1e-5)
            if step in (0, nsteps - 1):
                for k in arena.shapes:
                    a = arena.p(k).cpu().numpy()
                    if case['full']:
                        close(a, gold['param%d/%s' % (step, k)], 2e-4, 5e-5)
                        assert rel_norm(a, gold['param%d/%s' % (step, k)]) <= NORM_RTOL, (step, k)
                    else:
                        close(a.astype(np.float64).sum(), gold['paramsum%d/%s' % (step, k)], 2e-4, 5e-3)
                        close(a.reshape(-1)[C.sample_index(a.size)], gold['paramsample%d/%s' % (step, k)], 2e-4, 5e-5)
        assert n['x3'] == 1 + 3 * nsteps          # per train step: the heads' forward, dW and dX


# ------------------------------------------------------------------------------------------------ 5. capture
def wide_spec():
    return C.MODEL_CASES['cfg5_wide'][0]()


def captured_calls(eng, monkeypatch):
    """C-ABI calls of the captured step (as tests/test_gpu_engine.py::test_launch_count_of_the_captured_step counts them)"""
    from drvae_amd import _lib
    counts = {'n': 0, 'on': False}
    real = _lib.check

    def counting(code, what):
        if counts['on']:
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


def test_captured_step_replays_like_the_eager_one(dev, monkeypatch):
    """cfg-5 at 256 rows: train_step(); capture(); replay() x 3.  Counted in C-ABI calls (what the project's launch-count
    test counts), the captured fp32 step makes 34 and the bf16x3 step 35: the heads' weight- and
    data-gradient are two ``dv_gemm_x3`` calls where the fp32 step makes ONE ``dv_gemm_pair`` call.  That call is two
    launches on the device for a chip-filling pair (``dv_gemm_pair``: "otherwise two launches"), so the number of device
    launches of the two captured steps is EQUAL: the design adds none."""
    spec = wide_spec()
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 256, seed=5)
    calls, finals = {}, {}
    for mm in ('fp32', 'bf16x3'):
        eng, arena = make_engine(spec, params, dev, matmul=mm)
        set_batch(eng, batch, dev)
        eng.train_step()
        p0 = arena.param.clone()
        calls[mm] = captured_calls(eng, monkeypatch)
        for _ in range(3):
            eng.replay()
        torch.cuda.synchronize()
        eng.check_sync()
        losses = eng.losses()
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert not torch.equal(p0, arena.param)
        finals[mm] = (losses, arena.param.clone())
        if mm == 'bf16x3':
            # the same four steps eagerly from identical state: Philox noise is keyed by the step counter
            eng2, arena2 = make_engine(spec, params, dev, matmul=mm)
            set_batch(eng2, batch, dev)
            for _ in range(4):
                eng2.train_step()
            torch.cuda.synchronize()
            assert eng2.losses() == losses
            assert torch.equal(arena2.param, arena.param)
        del eng
    print('captured step C-ABI calls: fp32 %d, bf16x3 %d' % (calls['fp32'], calls['bf16x3']))
    assert (calls['fp32'], calls['bf16x3']) == (34, 35)
    assert rel_norm(finals['bf16x3'][1].cpu().numpy(), finals['fp32'][1].cpu().numpy()) <= NORM_RTOL


# ------------------------------------------------------------------------------------------------ 6. model level
def test_model_keyword_runs_a_train_batch(dev):
    """``DrVAE(..., matmul_precision='bf16x3')`` at a size whose decoder heads take the raw-heads route on their own (40000
    head columns x 1000+ decoder rows): a train batch runs, and its losses agree with the fp32 model from the same seed"""
    from tests.test_gpu_models import build_model, kwargs_for
    spec = M.ModelSpec(kind='drvae', L=2, dim_x=20000, dim_z1=64, dim_z3=64, h_en_z1=[256], h_de_x=[512])
    batch = M.make_batch(spec, 256, seed=11)
    params = M.init_params(spec, 5, as_numpy=True)
    out = {}
    for mm in ('fp32', 'bf16x3'):
        mdl = build_model(spec, dev) if mm == 'fp32' else None
        if mdl is None:
            import drvae_amd.DrVAE as D
            real = D.DrVAE

            class WithX3(real):                 # (``build_model`` does not know the keyword: same arguments + the new one)
                def __init__(self, *a, **k):
                    real.__init__(self, *a, matmul_precision='bf16x3', **k)
            D.DrVAE = WithX3
            try:
                mdl = build_model(spec, dev)
            finally:
                D.DrVAE = real
        assert list(mdl.state_dict().keys()) == list(params.keys())           # state_dict keys are unaffected
        mdl.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        mdl.add_noise = spec.add_noise_var > 0
        res = mdl.run_on_batch(train_mode=True, **kwargs_for(spec, batch, dev))
        torch.cuda.synchronize()
        out[mm] = {k: float(v) for k, v in res.items()}
        assert mdl._engine.cfg.matmul == mm and mdl._engine.plan.c_decx.x3_last == (mm == 'bf16x3')
        assert mdl.finished_training_iters == 1
        del mdl
    print('model losses fp32   %s' % out['fp32'])
    print('model losses bf16x3 %s' % out['bf16x3'])
    assert all(np.isfinite(v) for v in out['bf16x3'].values())
    for k in out['fp32']:
        np.testing.assert_allclose(out['bf16x3'][k], out['fp32'][k], rtol=LOSS_RTOL, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 7. speed
def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, rounds, inner=1, warm=3):
    """run the candidates alternately in one process (A B A B ...): ``rounds`` timed repetitions each, after warm-up"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            out[k].append(timed(f, inner))
    return out


def wide_products(dev, rows=8192, X=20000, H=2048):
    """the three decoder-heads products of the wide configuration as launcher calls: name -> {precision: callable}"""
    K = K_()
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(rows, H, device=dev, generator=g)
    W = torch.randn(2 * X, H, device=dev, generator=g) * 0.02
    dpre = torch.randn(rows, 2 * X, device=dev, generator=g)
    out, dW, dx = torch.empty(rows, 2 * X, device=dev), torch.empty(2 * X, H, device=dev), torch.empty(rows, H, device=dev)
    yref = torch.randn(rows, H, device=dev, generator=g)
    mk = lambda f: {'fp32': lambda: f({}), 'bf16x3': lambda: f(dict(x3=True))}
    return {
        'forward %d x %d x %d' % (rows, 2 * X, H): mk(lambda k: K.gemm(out, x, W, True, True, overread=True, **k)),
        'dW %d x %d x %d' % (2 * X, H, rows): mk(lambda k: K.gemm(dW, dpre, x, False, False, overread=True, **k)),
        'dX %d x %d x %d' % (rows, H, 2 * X): mk(lambda k: K.gemm(dx, dpre, W, True, False, epi=K.EPI_BWD, yref=yref,
                                                                  act0='elu', act1='elu', overread=True, **k)),
    }


def test_bf16x3_is_faster_than_fp32_on_the_wide_products(dev):
    for name, fns in wide_products(dev).items():
        t = alternate(fns, rounds=20)
        med3, min32 = float(np.median(t['bf16x3'])), float(np.min(t['fp32']))
        print('%s: fp32 min %.3f median %.3f ms | bf16x3 median %.3f ms (min %.3f max %.3f)'
              % (name, min32, float(np.median(t['fp32'])), med3, min(t['bf16x3']), max(t['bf16x3'])))
        assert med3 < min32, (name, med3, min32)


def test_bf16x3_is_faster_than_fp32_on_the_captured_wide_step(dev):
    spec = wide_spec()
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 1024, seed=5)
    engs = {}
    for mm in ('fp32', 'bf16x3'):                # both engines fit in memory together at this size
        eng, _ = make_engine(spec, params, dev, matmul=mm)
        set_batch(eng, batch, dev)
        eng.train_step()
        eng.capture()
        engs[mm] = eng
    t = alternate({mm: e.replay for mm, e in engs.items()}, rounds=20)
    for e in engs.values():
        e.check_sync()
        assert all(np.isfinite(v) for v in e.losses().values())
    med3, min32 = float(np.median(t['bf16x3'])), float(np.min(t['fp32']))
    print('captured cfg-5 step: fp32 min %.3f median %.3f ms | bf16x3 median %.3f ms (min %.3f max %.3f)'
          % (min32, float(np.median(t['fp32'])), med3, min(t['bf16x3']), max(t['bf16x3'])))
    assert med3 < min32, (med3, min32)
