"""The MMD row kernels launched directly (``dv_mmd_mix_fwd / _bwd / _combine``, ``dv_mmd_identity_fwd / _bwd``,
``dv_mmd_rff_fwd / _bwd``), the operations built on them (``blocks.mmd_objective``) and the grouped penalty
(``dv_mmd_grouped_*``), against the float64 references and componentwise bounds of tests/mmd_bn_ref.py (held themselves
by tests/test_mmd_bn_ref_cpu.py).

Shapes are the smallest that cross each kernel's strides: a mixture row is strided by 256 threads (N = 255, 256, 257,
600), the identity's columns likewise (Z = 255, 257, 600), the RFF means take 64 features per workgroup and four row
groups (R = 63, 64, 65, 500).  Every operand is a row-strided view (ld = width + 3 or + 5) in a buffer whose pads and
guard rows hold NaN, every output sits in a buffer pre-filled with a sentinel that must survive bit for bit, and every
launch runs twice and must store the same bits."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import mmd_bn_ref as R, ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


# --------------------------------------------------------------------------------------------------- the mixture
@pytest.mark.parametrize('kind', ['poly', 'rbf'])
@pytest.mark.parametrize('nb', R.MIX_NB)
@pytest.mark.parametrize('M,N', R.MIX_SHAPES)
def test_mixture_rows(K, dev, M, N, nb, kind):
    """part (forward), W and rs (backward, coef * gout of 0.7, of -2 / (n1 n2) and of 0.7 * 1.3) on rows around 0 and rows
    offset by 3 and by 10 (gamma d2 passes 104: the exponential underflows), one pair of identical rows; sa / sb are the
    diagonals of separate square matrices with their own ld whose other elements are NaN"""
    R.report(R.run_mix(K, dev, R.mix_case(M, N, nb, kind), coefs=R.mix_coefs(M, N)))


@pytest.mark.parametrize('nb', R.MIX_NB)
def test_mixture_clamp(K, dev, nb):
    """sa = sb = s = 1e4, G = s (1 + 2**-22): the raw squared distance is negative; k = 1 and dk = -mean(gamma) exactly"""
    R.report(R.run_mix_clamped(K, dev, nb))


@pytest.mark.parametrize('n', R.COMBINE_LENGTHS)
def test_mixture_combine(K, dev, n):
    """partial lengths 1, 9, 600; a count of 4097^2, which the launch receives as fp32"""
    R.report(R.run_combine(K, dev, n))


@pytest.mark.parametrize('what', ['nb=0', 'nb=9', 'kind', 'rbf without sa'])
def test_mixture_refusals(K, dev, what):
    """each raises and leaves the outputs untouched"""
    c = R.mix_case(3, 9, 5, 'rbf')
    kind, gam, with_sa = 'rbf', c['gammas'], True
    if what == 'nb=0':
        gam = []
    elif what == 'nb=9':
        gam = [0.1 * (i + 1) for i in range(9)]
    elif what == 'kind':
        kind = 'laplace'
    else:
        with_sa = False
    fr = R.Frame(dev)
    G, sb, gout = fr.inp(c['G']), fr.inp(R.diag_matrix(c['sb'])), fr.inp(torch.tensor([1.0]))
    sa = fr.inp(R.diag_matrix(c['sa'])) if with_sa else None
    part, W, rs = fr.out((3,)), fr.out((3, 9)), fr.out((3,))
    with pytest.raises((RuntimeError, KeyError, ValueError)):
        K.mmd_mix_fwd(part, G, kind, gam, sa, sb)
    with pytest.raises((RuntimeError, KeyError, ValueError)):
        K.mmd_mix_bwd(W, rs, G, kind, gam, gout, 0.7, sa, sb)
    fr.verify(untouched=True)


# --------------------------------------------------------------------------------------------------- identity, RFF
@pytest.mark.parametrize('offset', [False, True], ids=['around0', 'offset100'])
@pytest.mark.parametrize('n1,n2,Z', R.IDENTITY_SHAPES)
def test_identity_rows(K, dev, n1, n2, Z, offset):
    """diff and out[0]; the backward with both signs of coef.  ``offset100``: a common offset of 100 under populations
    that differ by 1e-3"""
    R.report(R.run_identity(K, dev, n1, n2, Z, offset))


@pytest.mark.parametrize('n1,n2,Rr', R.RFF_SHAPES)
def test_rff_rows(K, dev, n1, n2, Rr):
    """theta over [-50, 50] and a column of exact fp32 multiples of pi / 2; the backward on both populations"""
    R.report(R.run_rff(K, dev, n1, n2, Rr))


# --------------------------------------------------------------------------------------------------- whole operations
OBJ_SHAPES = ((300, 40, 13), (40, 300, 100), (257, 257, 5))
BWS = 1. / (2 * (np.array([1., 2., 5., 8., 10]) ** 2))


def _direct(x1, x2, kernel):
    """``mmd_objective`` in float64, rbf in the direct-difference form (``_mmd_objective_host`` of tests/test_gpu_blocks.py)"""
    if kernel == 'identity':
        return torch.sqrt(((x1.mean(0) - x2.mean(0)) ** 2).sum())

    def k(a, b, gam):
        if kernel == 'poly':
            return (gam * a @ b.t() + 1.0) ** 2
        return torch.exp(-gam * ((a[:, None, :] - b[None, :, :]) ** 2).sum(2))
    tot = 0.0
    for bw in BWS:
        gam = ref64.f32(math.sqrt(x1.shape[1]) * float(bw))
        tot = tot + (k(x1, x1, gam).mean() - 2 * k(x1, x2, gam).mean() + k(x2, x2, gam).mean()) / len(BWS)
    return torch.sqrt(tot)


def _rows(n1, n2, Z, shift):
    """rows as in ``test_mmd_objective_mixture_kernels_on_hip``, on a grid of 2**-18 so that the translation by 3 is exact
    in fp32"""
    g = torch.Generator().manual_seed(n1 * 100 + n2)
    q = lambda t: torch.round(t * 2.0 ** 18) / 2.0 ** 18
    x1, x2 = q(torch.randn(n1, Z, generator=g) * 0.3), q(torch.randn(n2, Z, generator=g) * 0.3 + 0.2)
    assert torch.equal(((x1 + 3.0).double() - 3.0).float(), x1)
    return x1 + shift, x2 + shift


@functools.lru_cache(maxsize=None)
def _objective_reference(kernel, n1, n2, Z, shift):
    """(value, d/dx1, d/dx2, MMD^2 and its bound).  rbf and identity are translation invariant: their translated value is
    the untranslated one (the gradients too)"""
    x1, x2 = _rows(n1, n2, Z, shift if kernel == 'poly' else 0.0)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    v = _direct(a, b, kernel)
    v.backward()
    gam = [math.sqrt(Z) * float(bw) for bw in BWS]
    m2, e_m2 = R.objective(*_rows(n1, n2, Z, shift), kernel, gam)
    return float(v.detach()), a.grad, b.grad, float(m2), float(e_m2)


@pytest.mark.parametrize('shift', [0.0, 3.0], ids=['around0', 'translated3'])
@pytest.mark.parametrize('kernel', ['poly', 'rbf', 'identity'])
@pytest.mark.parametrize('n1,n2,Z', OBJ_SHAPES)
def test_mmd_objective(dev, kernel, n1, n2, Z, shift):
    """``blocks.mmd_objective``: the value under the bound of the row kernels with the Gram launches' error propagated; the
    gradients at the tolerances of ``test_mmd_objective_mixture_kernels_on_hip`` with both sides, and with one side at a
    time requiring a gradient (the ``needs_input_grad`` branches of ``ops.MMDMix`` / ``ops.MMDIdentity``)"""
    import drvae_amd.blocks as blk
    want, g1, g2, m2, e_m2 = _objective_reference(kernel, n1, n2, Z, shift)
    x1, x2 = _rows(n1, n2, Z, shift)
    assert abs(m2 - want * want) <= 1e-3 * e_m2          # (the Gram form and the direct form in float64: the same number)
    e_v = float(R.root_bound(want * want, e_m2))
    for need1, need2 in ((True, True), (True, False), (False, True)):
        c = x1.clone().to(dev).requires_grad_(need1)
        d = x2.clone().to(dev).requires_grad_(need2)
        got = blk.mmd_objective(c, d, kernel=kernel, bandwidths=BWS)
        got.backward()
        ex = abs(float(got.detach()) - want) / e_v
        print('EXCESS %-34s %.3g   (value %.6g, bound %.3g)' % ('mmd_objective %s value' % kernel, ex, want, e_v))
        assert math.isfinite(float(got.detach())) and ex <= 1.0, (float(got.detach()), want, e_v)
        for t, ref, need in ((c, g1, need1), (d, g2, need2)):
            if not need:
                assert t.grad is None
                continue
            sc = float(ref.abs().max()) + 1e-12
            np.testing.assert_allclose(t.grad.cpu().numpy(), ref.float().numpy(), rtol=2e-3, atol=2e-4 * sc)


def test_mmd_fourier_one_side_at_a_time(dev):
    """``ops.MMDRff`` with one side detached: the other side's gradient as with both, None for the detached one"""
    from drvae_amd import ops
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.randn(37, 13, generator=g), torch.randn(52, 13, generator=g) * 0.5 + 0.3
    W, b = torch.randn(13, 65, generator=g).to(dev), torch.rand(65, generator=g).to(dev)
    a, c = 1.0 / math.sqrt(13), math.sqrt(2.0 / 65)
    t1, t2 = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    rf = lambda x: ref64.f32(c) * torch.cos(ref64.f32(a) * (x @ W.cpu().double()) + 2 * math.pi * b.cpu().double()[None, :])
    ((rf(t1).mean(0) - rf(t2).mean(0)) ** 2).sum().backward()
    for need1, need2 in ((True, True), (True, False), (False, True)):
        p, q = x1.clone().to(dev).requires_grad_(need1), x2.clone().to(dev).requires_grad_(need2)
        ops.MMDRff.apply(p, q, W, b, a, c).backward()
        for t, ref, need in ((p, t1.grad, need1), (q, t2.grad, need2)):
            if not need:
                assert t.grad is None
                continue
            np.testing.assert_allclose(t.grad.cpu().numpy(), ref.float().numpy(), rtol=5e-3, atol=5e-6)


# --------------------------------------------------------------------------------------------------- grouped penalty
@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('kernel', ['rbf_fourier', 'identity'])
@pytest.mark.parametrize('shape', ['tiny', 'cfg4', 'drvae4'])
def test_grouped_penalty_under_the_rule(shape, kernel, S, dev):
    """the three problems of tests/test_gpu_nuisance.py and their float64 reference as they stand: theta, diff, m2 and the
    value under the componentwise rule (``mmd_bn_ref.grouped``); dz keeps its tolerance"""
    import drvae_amd.kernels as K
    from tests.test_gpu_nuisance import GRAD_ATOL, GRAD_RTOL, _problem, _reference
    g, lay = _problem(shape, kernel, S, dev, seed=11)
    K.mmd_grouped_fwd(g)
    K.mmd_grouped_bwd(g)
    ref = _reference(g, lay)
    diff, m2, value, dz, theta, cnt = ref
    ptr, rows, src, cls = lay
    n = lambda t: None if t is None else t.cpu().numpy()
    e_theta, e_diff, e_m2, e_val = R.grouped(n(g['z']), cls, ptr, rows, src, S, kernel, g['w'], ref, n(g['W']), n(g['b']),
                                             g['a'], g['c'])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    res = {}
    if theta is not None:
        res['grouped theta'] = ref64.check('mmd_grouped_fwd theta', g['theta'], T(theta), T(e_theta))
    res['grouped diff'] = ref64.check('mmd_grouped_fwd diff', g['diff'], T(diff), T(e_diff))
    res['grouped m2'] = ref64.check('mmd_grouped_bwd m2', g['m2'], T(m2), T(e_m2))
    res['grouped value'] = ref64.check('mmd_grouped_bwd value', g['value'], T([value]), T([e_val]))
    R.report(res)
    np.testing.assert_allclose(g['dz'].cpu().numpy().astype(np.float64), dz, rtol=GRAD_RTOL, atol=GRAD_ATOL)
