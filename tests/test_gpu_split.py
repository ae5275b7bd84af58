"""GPU: the cheaper rungs of the opt-in matmul precision ladder -- ``dv_gemm_split`` with two parts ("bf16x2": hi hi, hi mid,
mid hi) and one part ("bf16x1": hi hi) -- against their arithmetic contract (exact terms bit for bit, the element-wise bounds
against the float64 emulation of the contract and against float64, the order of the ladder, K tail, side effects, non-finite
operands, bitwise reproducibility), the engine on top of them (the step against the CPU step whose three heads products are
evaluated by the contract's emulation; ``bf16x2`` against the reference's golden vectors at the fp32 step's tolerances;
capture / replay; the model keyword) and time (each rung faster than the one above it on the wide forward product)."""
import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref, ref64, x3_ref
from tests.golden import cases as C
from tests.test_gpu_engine import GRAD_RTOL, LOSS_RTOL, NORM_RTOL, close, rel_norm
from tests.test_gpu_x3 import LAYOUTS, RAW_TUNE, U, alternate, make_engine, set_batch, store, tuned
from tests.test_x3_cpu import make_engine as make_cpu_engine
from tests.test_x3_cpu import scaled_permutation

pytestmark = pytest.mark.gpu

TERMS = {3: x3_ref.TERMS, 2: ((0, 0), (0, 1), (1, 0)), 1: ((0, 0),)}
# |c_P - c64| <= TRUNC[P] sum |a||b| before accumulation, from bf16's unit roundoff u = 2^-8: |a - hi| <= u |a|,
# |a - hi - mid| <= u^2 |a|.  Two parts: a b - (hi hi + hi mid + mid hi) = (a - hi - mid) b + a (b - hi - mid) - (a - hi - mid)
# (b - hi - mid) + mid mid <= (2 u^2 + u^4 + u^2) |a||b|, rounded up to 3 u^2 + 2^-30; one part: a b - hi hi <= (2 u + u^2) |a||b|
TRUNC = {2: 3 * 2.0 ** -16 + 2.0 ** -30, 1: 2.0 ** -7 + 2.0 ** -16}
NAME = {3: 'bf16x3', 2: 'bf16x2', 1: 'bf16x1'}
RUNGS = (2, 1)


def K_():
    import drvae_amd.kernels as K
    return K


def kw_of(parts):
    """launcher keywords of a rung (0: the fp32 product; 3: ``x3=True`` alone, as ever)"""
    return {0: {}, 3: dict(x3=True)}.get(parts, dict(x3=True, parts=parts))


def run_split(dev, Aop, Bop, a_kc, b_kc, parts, Cinit=None, **kw):
    """Aop (M, K), Bop (K, N) host tensors -> device result of gemm(..., x3=True, parts=parts) in the given layout; the
    operands are strided views into wider buffers filled with NaN (``store``)"""
    K = K_()
    A = store(Aop, a_kc, dev)
    B = store(Bop.t(), b_kc, dev)
    M_, N = Aop.shape[0], Bop.shape[1]
    Cbuf = torch.full((M_, N + 5), 7.0, device=dev)
    Cm = Cbuf[:, :N]
    if Cinit is not None:
        Cm.copy_(Cinit.to(dev))
    K.gemm(Cm, A, B, a_kc, b_kc, **kw_of(parts), **kw)
    torch.cuda.synchronize()
    assert bool((Cbuf[:, N:] == 7.0).all())          # nothing written past the row ends
    return Cm.cpu()


def significands16(shape, seed):
    """normal-range fp32 numbers with exactly 16 significand bits in use (odd 16-bit integers times a power of two): their
    first two bf16 parts hold them exactly, hi + mid == a"""
    rs = np.random.RandomState(seed)
    m = rs.randint(2 ** 14, 2 ** 15, size=shape).astype(np.int64) * 2 + 1
    e = rs.randint(-30, -10, size=shape)
    s = rs.choice([-1.0, 1.0], size=shape)
    v = (s * m * np.exp2(e.astype(np.float64))).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), s * m * np.exp2(e.astype(np.float64)))
    t = torch.from_numpy(v)
    hi, mid, _ = x3_ref.split(t)
    assert torch.equal(hi.double() + mid.double(), t.double()) and bool((mid != 0).any())
    return t


def bf16_numbers(shape, seed):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(torch.float32)
    return t


# ------------------------------------------------------------------------------------------------ 5. exact terms
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_two_parts_exact_terms_bit_for_bit(dev, a_kc, b_kc):
    """16-bit significands times a scaled permutation: exact with hi hi + mid hi (A P) and with hi hi + hi mid (P B), wrong
    without either correction term (tests/test_split_cpu.py shows that on the emulation); 37 x 48 x 29 in one tile,
    150 x 200 x 200 across tile edges with a K tail"""
    for (m, n, k), seed in (((37, 29, 48), 5), ((150, 200, 200), 8)):
        A, P = significands16((m, k), seed), scaled_permutation(k, seed + 1)
        want = x3_ref.matmul(A, P, TERMS[2])
        assert torch.equal(want, A.double() @ P.double())
        assert torch.equal(run_split(dev, A, P, a_kc, b_kc, 2), want.float())               # hi hi, mid hi
        B = significands16((k, n), seed + 2)
        want = x3_ref.matmul(P, B, TERMS[2])
        assert torch.equal(want, P.double() @ B.double())
        assert torch.equal(run_split(dev, P, B, a_kc, b_kc, 2), want.float())               # hi hi, hi mid
    # round to nearest EVEN in the second part, and no mid mid: a = 1 + r with hi = 1 and r a tie between two bf16 numbers
    a = torch.zeros(4, 16)
    a[1, 5] = 1 + 2.0 ** -9 + 2.0 ** -17          # r = 2^-9 (1 + 2^-8): tie, down to the even 2^-9
    a[2, 7] = 1 + 2.0 ** -9 + 3 * 2.0 ** -17      # r = 2^-9 (1 + 3 2^-8): tie, up to the even 2^-9 (1 + 2^-6)
    a[3, 9] = 1 + 2.0 ** -10                      # (1 + 2^-10)^2 without mid mid: 1 + 2^-9 exactly
    got = run_split(dev, a, a.t().contiguous(), a_kc, b_kc, 2)
    assert torch.equal(got, x3_ref.matmul(a, a.t().contiguous(), TERMS[2]).float())
    assert float(got[1, 1]) == 1 + 2.0 ** -8 and float(got[2, 2]) == 1 + 2.0 ** -8 * (1 + 2.0 ** -6)
    assert float(got[3, 3]) == 1 + 2.0 ** -9


@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_one_part_exact_terms_bit_for_bit(dev, a_kc, b_kc):
    """bf16-representable operands times a scaled permutation are exact with hi hi alone, in both orders"""
    for (m, n, k), seed in (((37, 29, 48), 15), ((150, 200, 200), 18)):
        A, P = bf16_numbers((m, k), seed), scaled_permutation(k, seed + 1)
        want = x3_ref.matmul(A, P, TERMS[1])
        assert torch.equal(want, A.double() @ P.double())
        assert torch.equal(run_split(dev, A, P, a_kc, b_kc, 1), want.float())
        B = bf16_numbers((k, n), seed + 2)
        assert torch.equal(run_split(dev, P, B, a_kc, b_kc, 1), (P.double() @ B.double()).float())
    # operands that are NOT bf16 numbers are rounded, to nearest even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    a = torch.zeros(3, 16)
    a[1, 5], a[2, 7] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8
    got = run_split(dev, a, a.t().contiguous(), a_kc, b_kc, 1)
    assert torch.equal(got, x3_ref.matmul(a, a.t().contiguous(), TERMS[1]).float())
    assert float(got[1, 1]) == 1.0 and float(got[2, 2]) == (1 + 2.0 ** -6) ** 2
    assert float(got.abs().sum()) == float(got[1, 1]) + float(got[2, 2])


# ------------------------------------------------------------------------------------------------ 6. accuracy
@pytest.mark.parametrize('Kdim', [4, 20, 100, 980, 2048])
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_accuracy_against_the_contract_and_float64(dev, a_kc, b_kc, Kdim):
    """Element-wise against the float64 emulation c_P of the rung's contract (derived: at most T K fp32 additions of exact
    products, T = 3 / 1 terms): |c - c_P| <= 1.01 (T K + 4) 2^-24 sum_k |a_k| |b_k| |alpha| [|act'|] plus the fp32 roundings
    of the epilogue's own arithmetic (as tests/test_gpu_x3.py::test_accuracy_against_float64); against float64: plus the
    truncation bound TRUNC[P] sum |a||b| |alpha| [|act'|].  And the ladder is ordered: norm-wise against float64 on the
    same operands e(bf16x3) < e(bf16x2) < e(bf16x1).  Same ragged shapes, epilogues and NaN surroundings as that test."""
    K = K_()
    g = torch.Generator().manual_seed(1000 * Kdim + 10 * a_kc + b_kc)
    M_, N = (203, 331) if Kdim < 2048 else (389, 517)
    Aop, Bop = torch.randn(M_, Kdim, generator=g), torch.randn(Kdim, N, generator=g)
    c64 = Aop.double() @ Bop.double()
    cP = {p: x3_ref.matmul(Aop, Bop, TERMS[p]) for p in RUNGS}
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
        old = beta * C0.double() if beta else 0.0
        want64 = c64 * a32 * scale + old
        err64 = {}
        for p in (3, 2, 1):
            got = run_split(dev, Aop, Bop, a_kc, b_kc, p, Cinit=C0, **kw).double()
            err64[p] = float(torch.linalg.norm(got - want64) / torch.linalg.norm(want64))
            if p == 3:
                continue
            T = len(TERMS[p])
            prod = cP[p] * a32
            want = prod * scale + old
            bound = 1.01 * (T * Kdim + 4) * U * mag * abs(a32) * scale.abs() \
                + U * (2 * (prod * scale).abs() + 8 * prod.abs() * ymag + 2 * (beta * C0.double()).abs() + 2 * want.abs())
            worst = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
            bound64 = bound + TRUNC[p] * mag * abs(a32) * scale.abs()
            worst64 = float(((got - want64).abs() / bound64.clamp_min(1e-300)).max())
            print('%s accuracy layout=(%d,%d) K=%d epi=%d beta=%g: max err/bound contract %.3f float64 %.3f, norm-wise %.3e'
                  % (NAME[p], a_kc, b_kc, Kdim, epi, beta, worst, worst64, err64[p]))
            assert worst <= 1.0, (p, epi, beta, worst)
            assert worst64 <= 1.0, (p, epi, beta, worst64)
        assert err64[3] < err64[2] < err64[1], (epi, beta, err64)


# ------------------------------------------------------------------------------------------------ 7. K tail
@pytest.mark.parametrize('parts', RUNGS)
@pytest.mark.parametrize('Kdim', [26, 62, 33])
@pytest.mark.parametrize('a_kc,b_kc', [(True, True), (True, False)])
def test_k_tail_behind_an_overread_chunk_is_masked(dev, a_kc, b_kc, Kdim, parts):
    """as tests/test_gpu_x3.py: the row pads behind K hold NaN, the chunk that straddles K is loaded whole on the caller's
    word and what lies past K counts as zero (also in the second sub-tile of a deeper K tile); refused without the word"""
    g = torch.Generator().manual_seed(77 * Kdim + 2 * a_kc + b_kc)
    M_, N = 139, 150
    Aop, Bop = torch.randn(M_, Kdim, generator=g), torch.randn(Kdim, N, generator=g)
    c64, cP = Aop.double() @ Bop.double(), x3_ref.matmul(Aop, Bop, TERMS[parts])
    mag = Aop.double().abs() @ Bop.double().abs()
    bound = 1.01 * (len(TERMS[parts]) * Kdim + 4) * U * mag + 2 * U * cP.abs()
    got = run_split(dev, Aop, Bop, a_kc, b_kc, parts, overread=True).double()
    assert bool(torch.isfinite(got).all())
    worst, worst64 = float(((got - cP).abs() / bound).max()), float(((got - c64).abs() / (bound + TRUNC[parts] * mag)).max())
    print('%s K tail layout=(%d,%d) K=%d: max err/bound contract %.3f float64 %.3f' % (NAME[parts], a_kc, b_kc, Kdim, worst, worst64))
    assert worst <= 1.0 and worst64 <= 1.0
    with pytest.raises(RuntimeError, match='x3=True'):
        run_split(dev, Aop, Bop, a_kc, b_kc, parts)


# ------------------------------------------------------------------------------------------------ 8. side effects
@pytest.mark.parametrize('parts', RUNGS)
def test_colsum_rides_in_front_and_refusals_touch_nothing(dev, parts):
    K = K_()
    g = torch.Generator().manual_seed(5)
    dy, x = torch.randn(300, 70, generator=g), torch.randn(300, 44, generator=g)        # dW = dy^T x, db = dy.sum(0)
    dyd, xd = store(dy.t(), False, dev), store(x.t(), False, dev)
    dW, db = torch.zeros(70, 44, device=dev), torch.full((70,), 2.0, device=dev)
    K.gemm(dW, dyd, xd, False, False, a_colsum=db, colsum_beta=1.0, **kw_of(parts))
    torch.cuda.synchronize()
    assert bool(((db.cpu().double() - (2.0 + dy.double().sum(0))).abs() <= 301 * U * (2.0 + dy.double().abs().sum(0))).all())
    cP, mag = x3_ref.matmul(dy.t().contiguous(), x, TERMS[parts]), dy.double().abs().t() @ x.double().abs()
    assert bool(((dW.cpu().double() - cP).abs() <= 1.01 * (len(TERMS[parts]) * 300 + 4) * U * mag).all())
    Cm = torch.full((300, 70), 3.0, device=dev)
    with pytest.raises(RuntimeError, match='x3=True'):
        K.gemm(Cm, xd, store(torch.randn(70, 44, generator=g), False, dev), True, False, epi=K.EPI_FWD,
               bias=torch.zeros(70, device=dev), **kw_of(parts))
    with pytest.raises(RuntimeError, match='x3=True'):
        K.linear_bwd_pair(dW, None, torch.zeros(300, 44, device=dev), dyd, xd, torch.zeros(70, 44, device=dev),
                          kscale=torch.ones(70, device=dev), **kw_of(parts))
    with pytest.raises(RuntimeError, match='parts'):
        K.gemm(Cm, xd, store(torch.randn(70, 44, generator=g), False, dev), True, False, x3=True, parts=4)
    torch.cuda.synchronize()
    assert bool((Cm == 3.0).all())


@pytest.mark.parametrize('parts', RUNGS)
def test_non_finite_operands_poison_what_they_feed(dev, parts):
    g = torch.Generator().manual_seed(6)
    Aop, Bop = torch.randn(70, 64, generator=g), torch.randn(64, 90, generator=g)
    Aop[3, 7], Aop[40, 63], Bop[5, 11] = float('nan'), float('inf'), float('-inf')
    for a_kc, b_kc in LAYOUTS:
        got = run_split(dev, Aop, Bop, a_kc, b_kc, parts)
        bad = ~torch.isfinite(got)
        want = torch.zeros_like(bad)
        want[3, :], want[40, :], want[:, 11] = True, True, True
        assert torch.equal(bad, want)


# ------------------------------------------------------------------------------------------------ 9. reproducibility
@pytest.mark.parametrize('parts', RUNGS)
@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_two_launches_are_bitwise_equal(dev, a_kc, b_kc, parts):
    g = torch.Generator().manual_seed(7)
    Aop, Bop = torch.randn(515, 1000, generator=g), torch.randn(1000, 770, generator=g)
    assert torch.equal(run_split(dev, Aop, Bop, a_kc, b_kc, parts), run_split(dev, Aop, Bop, a_kc, b_kc, parts))


# ------------------------------------------------------------------------------------------------ 10. the step
def count_split(monkeypatch):
    from drvae_amd import _lib
    n = {'split': 0, 'x3': 0}
    real = _lib.check

    def counting(code, what):
        n['split'] += what == 'dv_gemm_split'
        n['x3'] += what == 'dv_gemm_x3'
        return real(code, what)
    monkeypatch.setattr(_lib, 'check', counting)
    return n


def install_contract(monkeypatch, seen):
    """the CPU stand-ins, whose routed products follow the rung's contract (``kernel_ref.routed_product``), with the ``parts``
    of every routed product noted in ``seen``"""
    kernel_ref.install(monkeypatch)
    routed = kernel_ref.routed_product

    def noting(Cm, A, B, a_kc, b_kc, parts, **kw):
        seen.append(parts)
        return routed(Cm, A, B, a_kc, b_kc, parts, **kw)
    monkeypatch.setattr(kernel_ref, 'routed_product', noting)


def contract_step_on_cpu(case, mm):
    """eval losses, per-step losses and the parameters after the first and the last train step of the CPU step whose three
    heads products follow the rung's contract"""
    with pytest.MonkeyPatch.context() as mp:
        seen = []
        install_contract(mp, seen)
        spec = case['spec']
        eng, arena = make_cpu_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), matmul=mm)
        t = lambda k: torch.from_numpy(case['batch'][k].copy())
        eng.set_batch(t('x1'), t('x2'), case['batch']['y'], case['batch']['has_x2'], case['batch']['has_y'])
        eng.training = False
        eng.set_noise(case['noises'][0])
        eng.forward()
        out = {'eval': dict(eng.losses()), 'steps': [], 'params': {}}
        assert len(seen) == 1
        eng.training = True
        nsteps = len(case['noises'])
        for step, noise in enumerate(case['noises']):
            eng.train_step(noise)
            out['steps'].append(dict(eng.losses()))
            if step in (0, nsteps - 1):
                out['params'][step] = {k: arena.p(k).clone().numpy() for k in arena.shapes}
        assert len(seen) == 1 + 3 * nsteps
        return out


_CONTRACT = {}


def contract_step(name, mm):
    if (name, mm) not in _CONTRACT:            # (computed once, shared, left unchanged)
        _CONTRACT[name, mm] = contract_step_on_cpu(C.model_case(name), mm)
    return _CONTRACT[name, mm]


@pytest.mark.parametrize('parts', RUNGS)
@pytest.mark.parametrize('name', ['tiny_drvae', 'cfg2_drvae'])
def test_step_matches_the_cpu_step_of_its_own_contract(name, parts, dev, monkeypatch):
    """the device step -- eval losses, then the golden case's train steps -- against the CPU step whose three heads products
    are ``x3_ref.matmul`` with the rung's terms, at the fp32 step's own tolerances (the device adds only fp32 summation
    order to the contract).  13 genes: a K tail in dX; 978 genes: ragged tiles.  1 routed product per evaluation forward,
    3 per train step.  The parameter tolerances are applied as tests/test_gpu_engine.py applies them to the two cases:
    every element and the norm of the ``full`` case, the sum and the sampled elements of cfg 2.  (cfg 2's Adam steps divide
    gradients of the size of their own rounding error by their magnitude: the fp32 device step is 1.2e-4 norm-wise from the
    fp32 CPU stand-in in ``decoder_z2Fz1.W_mu`` after the first step, and a handful of 782400 first-layer weights move by
    2 lr -- measured, profiles/r10_experiments.md; the norm-wise figure of every case is printed.)"""
    mm = NAME[parts]
    with tuned(RAW_TUNE):
        ref = contract_step(name, mm)
        n = count_split(monkeypatch)
        case = C.model_case(name)
        spec = case['spec']
        eng, arena = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), dev, matmul=mm)
        set_batch(eng, case['batch'], dev)
        assert eng.plan.c_decx.x3_last and eng.plan.c_decx.x3_parts == parts
        eng.training = False
        eng.set_noise(case['noises'][0])
        eng.forward()
        assert (n['split'], n['x3']) == (1, 0)
        for k, v in eng.losses().items():
            close(v, ref['eval'][k], LOSS_RTOL, 1e-5)
        eng.training = True
        nsteps = len(case['noises'])
        for step, noise in enumerate(case['noises']):
            eng.train_step(noise)
            for k, v in eng.losses().items():
                close(v, ref['steps'][step][k], LOSS_RTOL, 1e-5)
            if step in (0, nsteps - 1):
                worst = max((rel_norm(arena.p(k).cpu().numpy(), ref['params'][step][k]), k) for k in arena.shapes)
                print('%s %s step %d: parameters norm-wise <= %.2e from the contract step\'s (%s)' % ((name, mm, step) + worst))
                for k in arena.shapes:
                    a, b = arena.p(k).cpu().numpy(), ref['params'][step][k]
                    if case['full']:
                        close(a, b, 2e-4, 5e-5)
                        assert rel_norm(a, b) <= NORM_RTOL, (step, k, rel_norm(a, b))
                    else:
                        close(a.astype(np.float64).sum(), b.astype(np.float64).sum(), 2e-4, 5e-3)
                        i = C.sample_index(a.size)
                        close(a.reshape(-1)[i], b.reshape(-1)[i], 2e-4, 5e-5)
        assert (n['split'], n['x3']) == (1 + 3 * nsteps, 0)


# ------------------------------------------------------------------------------------------------ 11. golden cases
def golden_run(name, mm, dev, monkeypatch, hold):
    """tests/test_gpu_engine.py::test_train_steps_match_reference_golden with ``matmul=mm`` on the raw-heads route; ``hold``:
    assert its tolerances, nothing loosened -- else only measure.  Returns the worst loss error in units of its tolerance
    and the worst norm-wise parameter distance."""
    worst = {'loss': 0.0, 'param': 0.0}

    def loss_close(v, ref):
        worst['loss'] = max(worst['loss'], abs(float(v) - float(ref)) / (1e-5 + LOSS_RTOL * abs(float(ref))))
        if hold:
            close(v, ref, LOSS_RTOL, 1e-5)
    with tuned(RAW_TUNE):
        n = count_split(monkeypatch)
        case, gold = C.model_case(name), C.load('model_' + name)
        spec = case['spec']
        eng, arena = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), dev, matmul=mm)
        set_batch(eng, case['batch'], dev)
        eng.training = False
        eng.set_noise(case['noises'][0])
        eng.forward()
        assert n['split'] == 1
        for k, v in eng.losses().items():
            loss_close(v, gold['eval/' + k])
        eng.training = True
        eng.set_noise(case['noises'][0])
        eng.forward()
        eng.backward()
        assert n['split'] == 1       # (the unfused forward / backward pair finishes the heads in the product's epilogue: fp32)
        if hold:
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
                loss_close(v, gold['step%d/%s' % (step, k)])
            if step in (0, nsteps - 1):
                for k in arena.shapes:
                    a = arena.p(k).cpu().numpy()
                    if case['full']:
                        ref = gold['param%d/%s' % (step, k)]
                        if float(np.abs(ref).max()) > 0:
                            worst['param'] = max(worst['param'], rel_norm(a, ref))
                        if hold:
                            close(a, ref, 2e-4, 5e-5)
                            assert rel_norm(a, ref) <= NORM_RTOL, (step, k)
                    elif hold:
                        close(a.astype(np.float64).sum(), gold['paramsum%d/%s' % (step, k)], 2e-4, 5e-3)
                        close(a.reshape(-1)[C.sample_index(a.size)], gold['paramsample%d/%s' % (step, k)], 2e-4, 5e-5)
        assert n['split'] == 1 + 3 * nsteps
    return worst


@pytest.mark.parametrize('name', ['tiny_drvae', 'cfg2_drvae'])
def test_train_steps_match_reference_golden_bf16x2(name, dev, monkeypatch):
    """``bf16x2`` is held to the reference's golden vectors at the tolerances of the fp32 step, nothing loosened.  ``bf16x1``
    is a different dtype and is NOT held to them: its distance is printed (and recorded in profiles/r10_precision_ladder.txt)"""
    w2 = golden_run(name, 'bf16x2', dev, monkeypatch, hold=True)
    w1 = golden_run(name, 'bf16x1', dev, monkeypatch, hold=False)
    for mm, w in (('bf16x2', w2), ('bf16x1', w1)):
        print('%s %s against the golden vectors: worst loss error %.3f of its tolerance, parameters norm-wise <= %.2e (NORM_RTOL %.0e)'
              % (name, mm, w['loss'], w['param'], NORM_RTOL))


# ------------------------------------------------------------------------------------------------ 12. capture, model
@pytest.mark.parametrize('parts', RUNGS)
def test_captured_step_replays_like_the_eager_one(dev, parts):
    """cfg-2 on the raw-heads route: train_step(); capture(); replay() x 3 equals four eager steps from the same state bit
    for bit (Philox noise is keyed by the step counter)"""
    mm = NAME[parts]
    with tuned(RAW_TUNE):
        case = C.model_case('cfg2_drvae')
        spec = case['spec']
        params = M.init_params(spec, case['param_seed'], as_numpy=True)
        eng, arena = make_engine(spec, params, dev, matmul=mm)
        set_batch(eng, case['batch'], dev)
        assert eng.plan.c_decx.x3_last and eng.plan.c_decx.x3_parts == parts
        eng.train_step()
        p0 = arena.param.clone()
        eng.capture()
        for _ in range(3):
            eng.replay()
        torch.cuda.synchronize()
        eng.check_sync()
        losses = eng.losses()
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert not torch.equal(p0, arena.param)
        eng2, arena2 = make_engine(spec, params, dev, matmul=mm)
        set_batch(eng2, case['batch'], dev)
        for _ in range(4):
            eng2.train_step()
        torch.cuda.synchronize()
        assert eng2.losses() == losses
        assert torch.equal(arena2.param, arena.param)


def test_model_keyword_runs_a_train_batch(dev):
    """``DrVAE(..., matmul_precision='bf16x2' | 'bf16x1')`` on the raw-heads route: a train batch runs on the rung asked for,
    ``state_dict`` is unaffected, and the ``bf16x2`` losses agree with the fp32 model's from the same seed"""
    from tests.test_gpu_models import build_model, kwargs_for
    import drvae_amd.DrVAE as D
    spec = M.ModelSpec(kind='drvae', L=2, dim_x=200, dim_z1=16, dim_z3=16, h_en_z1=[32], h_de_x=[48])
    batch = M.make_batch(spec, 64, seed=11)
    params = M.init_params(spec, 5, as_numpy=True)
    out = {}
    with tuned(RAW_TUNE):
        for mm in ('fp32', 'bf16x2', 'bf16x1'):
            real = D.DrVAE

            class WithPrecision(real):          # (``build_model`` does not know the keyword: same arguments + the new one)
                def __init__(self, *a, **k):
                    real.__init__(self, *a, matmul_precision=mm, **k)
            D.DrVAE = WithPrecision
            try:
                mdl = build_model(spec, dev)
            finally:
                D.DrVAE = real
            assert list(mdl.state_dict().keys()) == list(params.keys())
            mdl.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
            mdl.add_noise = spec.add_noise_var > 0
            res = mdl.run_on_batch(train_mode=True, **kwargs_for(spec, batch, dev))
            torch.cuda.synchronize()
            out[mm] = {k: float(v) for k, v in res.items()}
            chain = mdl._engine.plan.c_decx
            assert mdl._engine.cfg.matmul == mm and chain.x3_last == (mm != 'fp32')
            assert mm == 'fp32' or NAME[chain.x3_parts] == mm
            assert mdl.finished_training_iters == 1
            del mdl
    for mm, v in out.items():
        print('model losses %-6s %s' % (mm, v))
        assert all(np.isfinite(x) for x in v.values())
    for k in out['fp32']:
        np.testing.assert_allclose(out['bf16x2'][k], out['fp32'][k], rtol=LOSS_RTOL, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 13. time
def test_each_rung_is_faster_than_the_one_above_on_the_wide_forward_product(dev):
    """8192 x 40000 x 2048, all four precisions alternating in one process, 3 warm-up rounds, 10 timed repetitions: the
    medians are ordered bf16x1 < bf16x2 < bf16x3 (the ratios belong to profiles/r10_precision_ladder.txt)"""
    K = K_()
    rows, X, H = 8192, 20000, 2048
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(rows, H, device=dev, generator=g)
    W = torch.randn(2 * X, H, device=dev, generator=g) * 0.02
    out = torch.empty(rows, 2 * X, device=dev)
    fns = {('fp32' if p == 0 else NAME[p]): (lambda p=p: K.gemm(out, x, W, True, True, overread=True, **kw_of(p))) for p in (0, 3, 2, 1)}
    t = alternate(fns, rounds=10)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print('wide forward product, medians (ms): ' + ', '.join('%s %.3f' % kv for kv in med.items()))
    assert med['bf16x1'] < med['bf16x2'] < med['bf16x3'], med
