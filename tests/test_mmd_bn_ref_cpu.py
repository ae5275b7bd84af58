"""Holds the float64 references and bounds of tests/mmd_bn_ref.py themselves (no device):

1. the references against independent float64 statements of the model (``F.batch_norm`` and its autograd, the
   direct-difference form of the kernel mixture, autograd on the RFF / identity formulas), to 1e-12 relative;
2. the fp32 stand-ins of tests/kernel_ref.py inside the bounds at every case the device tests run;
3. faulty variants of the reference ("mutants"): each lands at least 4x outside the bound at one case or more --
   otherwise the case list would be too weak to notice that fault in a kernel."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_ref, mmd_bn_ref as R, ref64
from tests.ref64 import U, excess, f64

CPU = torch.device('cpu')


def agree(a, b, what):
    a, b = f64(a), f64(b)
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1e-300), '%s: %.3g relative' % (
        what, float((a - b).abs().max()) / max(scale, 1e-300))


# ----------------------------------------------------------------------------- 1. the references against the model
@pytest.mark.parametrize('M,N', [(2, 3), (5, 65), (67, 130)])
@pytest.mark.parametrize('momentum', [0.1, 1.0])
def test_bn_reference_equals_torch_float64(M, N, momentum):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, N, generator=g).double()
    p = {k: v.double() for k, v in R.bn_params(N).items()}
    dy = torch.randn(M, N, generator=g).double()
    mom = ref64.f32(momentum)
    for training in (True, False):
        xx, w, b = x.clone().requires_grad_(True), p['w'].clone().requires_grad_(True), p['b'].clone().requires_grad_(True)
        rm, rv = p['rm'].clone(), p['rv'].clone()
        y = F.batch_norm(xx, rm, rv, w, b, training, mom, ref64.f32(1e-5))
        (y * dy).sum().backward()
        r = R.bn_fwd(x, p['w'], p['b'], p['rm'], p['rv'], 1e-5, momentum, training)
        agree(r['y'], y, 'y')
        if training:
            agree(r['running_mean'], rm, 'running_mean')
            agree(r['running_var'], rv, 'running_var')
            agree(r['mean'], x.mean(0), 'mean')
        else:
            assert torch.equal(rm, p['rm']) and torch.equal(r['mean'], p['rm'])
        bw = R.bn_bwd(dy, x, r['mean'], r['rstd'], p['w'], training)
        agree(bw['dx'], xx.grad, 'dx')
        agree(bw['dw'], w.grad, 'dw')
        agree(bw['db'], b.grad, 'db')
    r = R.bn_fwd(x, None, None, None, None, 0.0, momentum, True)               # no affine, no statistics, eps = 0
    agree(r['y'], (x - x.mean(0)) / x.std(0, unbiased=False), 'y without affine')       # (torch refuses eps = 0)
    assert 'running_mean' not in r


def _direct_mixture(a, b, kind, gammas):
    """k(a_i, b_j) of the mixture in the direct-difference form (rbf as ``_mmd_objective_host`` of tests/test_gpu_blocks.py)"""
    tot = 0.0
    for gam in gammas:
        if kind == 'poly':
            tot = tot + (gam * a @ b.t() + 1.0) ** 2
        else:
            tot = tot + torch.exp(-gam * ((a[:, None, :] - b[None, :, :]) ** 2).sum(2))
    return tot / len(gammas)


@pytest.mark.parametrize('kind', ['poly', 'rbf'])
@pytest.mark.parametrize('nb', [1, 5, 8])
def test_mixture_reference_equals_direct_difference_form(kind, nb):
    g = torch.Generator().manual_seed(nb)
    a, b = torch.randn(7, 6, generator=g).double(), (torch.randn(9, 6, generator=g) * 0.5 + 0.2).double()
    gam = [ref64.f32(x) for x in R.mix_gammas(nb, kind)]
    G, sa, sb = a @ b.t(), (a * a).sum(1), (b * b).sum(1)
    e = R.mix_elements(G, kind, gam, sa, sb)
    agree(e['k'], _direct_mixture(a, b, kind, gam), 'k')
    agree(R.mix_fwd(G, kind, gam, sa, sb)['part'], _direct_mixture(a, b, kind, gam).sum(1), 'part')
    # dk against autograd: w.r.t. G (poly) or the squared distance (rbf)
    if kind == 'poly':
        v = G.clone().requires_grad_(True)
        sum(((gm * v + 1.0) ** 2 for gm in gam)).div(nb).sum().backward()
    else:
        v = (sa[:, None] + sb[None, :] - 2 * G).clamp_min(0).requires_grad_(True)
        sum((torch.exp(-gm * v) for gm in gam)).div(nb).sum().backward()
    agree(e['dk'], v.grad, 'dk')
    bw = R.mix_bwd(G, kind, gam, torch.tensor([1.3]), -2.0 / 63, sa, sb)
    c = ref64.f32(-2.0 / 63) * float(torch.tensor([1.3]).double())
    agree(bw['W'], c * v.grad, 'W')
    agree(bw['rs'], (c * v.grad).sum(1), 'rs')
    # and the whole objective's gradient w.r.t. the rows, as ops.MMDMix assembles it from W and rs (the cross term)
    aa = a.clone().requires_grad_(True)
    _direct_mixture(aa, b, kind, gam).sum().backward()
    W1 = R.mix_bwd(G, kind, gam, torch.tensor([1.0]), 1.0, sa, sb)
    da = W1['W'] @ b if kind == 'poly' else 2 * (W1['rs'][:, None] * a - W1['W'] @ b)
    agree(da, aa.grad, 'd/da through W and rs')
    m = R.combine(e['k'].sum(1), e['k'].sum(1), e['k'].sum(1), 63.0, 63.0, 63.0)['out']
    agree(m[1], _direct_mixture(a, b, kind, gam).mean(), 'combine mean')
    assert abs(float(m[0])) <= 1e-12 * float(m[1])


def test_rff_and_identity_references_equal_autograd_on_the_formulas():
    th1, th2, c = R.rff_case(5, 3, 65)
    c32 = ref64.f32(c)
    t1, t2 = th1.double().requires_grad_(True), th2.double().requires_grad_(True)
    rf = lambda t: c32 * torch.cos(t)
    m = ((rf(t1).mean(0) - rf(t2).mean(0)) ** 2).sum()
    m.backward()
    r = R.rff_fwd(th1, th2, c)
    agree(r['mmd2'], m.reshape(1), 'mmd2')
    agree(r['diff'], rf(t1).mean(0) - rf(t2).mean(0), 'diff')
    one = torch.tensor([1.0])
    as32 = lambda coef: ref64.f32(coef) / coef              # (a launch receives its coefficient as fp32)
    agree(R.rff_bwd(th1, r['diff'], one, 2.0 * c32 / 5)['G'], t1.grad * as32(2.0 * c32 / 5), 'd mmd2 / d theta1')
    agree(R.rff_bwd(th2, r['diff'], one, -2.0 * c32 / 3)['G'], t2.grad * as32(-2.0 * c32 / 3), 'd mmd2 / d theta2')
    x1, x2 = R.identity_case(7, 3, 255, False)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    o = ((a.mean(0) - b.mean(0)) ** 2).sum()
    o.backward()
    r = R.identity_fwd(x1, x2)
    agree(r['out'], o.reshape(1), 'identity out')
    agree(R.identity_bwd(r['diff'], one, 2.0 / 7, 7)['dx'], a.grad * as32(2.0 / 7), 'identity dx1')
    agree(R.identity_bwd(r['diff'], one, -2.0 / 3, 3)['dx'], b.grad * as32(-2.0 / 3), 'identity dx2')


# ----------------------------------------------------------------------------- 2. the stand-ins inside the bounds
class StandIn:
    """tests/kernel_ref.py behind the launchers' signatures (its BatchNorm takes the affine pair as given)"""

    def __getattr__(self, name):
        return getattr(kernel_ref, name)

    @staticmethod
    def bn_fwd(y, x, w, b, mean, rstd, rm, rv, eps=1e-5, momentum=0.1, training=True):
        N = x.shape[1]
        kernel_ref.bn_fwd(y, x, torch.ones(N) if w is None else w, torch.zeros(N) if b is None else b, mean, rstd, rm, rv,
                          eps=eps, momentum=momentum, training=training)

    @staticmethod
    def bn_bwd(dx, dw, db, dy, x, mean, rstd, w, training=True):
        kernel_ref.bn_bwd(dx, dw, db, dy, x, mean, rstd, torch.ones(x.shape[1]) if w is None else w, training=training)


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(title, worst):
    for k in sorted(worst):
        print('%s: %-32s worst excess %.3g' % (title, k, worst[k]))


def test_stand_ins_stay_inside_the_mmd_bounds():
    K, worst = StandIn(), {}
    for (M, N), nb, kind in itertools.product(R.MIX_SHAPES, R.MIX_NB, ('poly', 'rbf')):
        _merge(worst, R.run_mix(K, CPU, R.mix_case(M, N, nb, kind), coefs=R.mix_coefs(M, N)))
    for nb in R.MIX_NB:
        _merge(worst, R.run_mix_clamped(K, CPU, nb))
    for n in R.COMBINE_LENGTHS:
        _merge(worst, R.run_combine(K, CPU, n))
    for (n1, n2, Z), off in itertools.product(R.IDENTITY_SHAPES, (False, True)):
        _merge(worst, R.run_identity(K, CPU, n1, n2, Z, off))
    for n1, n2, Rr in R.RFF_SHAPES:
        _merge(worst, R.run_rff(K, CPU, n1, n2, Rr))
    _report('stand-in', worst)
    assert max(worst.values()) <= 1.0


def test_stand_ins_stay_inside_the_bn_and_dropout_bounds():
    K, worst = StandIn(), {}
    for M, N, mode in itertools.product(R.BN_M, R.BN_N, R.BN_FWD_MODES):
        _merge(worst, R.run_bn_fwd(K, CPU, M, N, mode))
    _merge(worst, R.run_bn_fwd(K, CPU, 1, 65, R.BN_FWD_MODES[4]))
    for M, N, mode in itertools.product(R.BN_M, R.BN_N, R.BN_BWD_MODES):
        _merge(worst, R.run_bn_bwd(K, CPU, M, N, mode))
    for (M, N), scale in itertools.product(R.MASK_SHAPES, R.MASK_SCALES):
        _merge(worst, R.run_mask_scale(K, CPU, M, N, scale))
    _report('stand-in', worst)
    assert max(worst.values()) <= 1.0


# ----------------------------------------------------------------------------- 3. mutants
def _bn_mutant_excess(name):
    """worst excess of faulty BatchNorm variant ``name`` over the device tests' cases"""
    w = 0.0
    for M, N in itertools.product(R.BN_M, R.BN_N):
        x, p = R.bn_input(M, N), R.bn_params(N)
        r = R.bn_fwd(x, p['w'], p['b'], p['rm'], p['rv'], 1e-5, 0.1, True)
        x64, mom = x.double(), ref64.f32(0.1)
        if name == 'one-pass variance':                         # E[x^2] - mu^2 in fp32, as a one-pass kernel would
            mu = x.mean(0)
            var = ((x * x).mean(0) - mu * mu).clamp_min(0.0)
            w = max(w, float(excess(torch.rsqrt(var + ref64.f32(1e-5)), r['rstd'], r['rstd_b']).max()))
        elif name == 'biased running_var':
            got = (1 - mom) * p['rv'].double() + mom * r['var']
            w = max(w, float(excess(got.float(), r['running_var'], r['running_var_b']).max()))
        elif name == 'momentum on the old value':
            got = mom * p['rm'].double() + (1 - mom) * r['mean']
            w = max(w, float(excess(got.float(), r['running_mean'], r['running_mean_b']).max()))
        elif name == 'eps left out of rstd':
            xn = R.bn_input(M, N, with_constant=False)          # (with the constant column it is simply infinite)
            rn = R.bn_fwd(xn, p['w'], p['b'], p['rm'], p['rv'], 1e-5, 0.1, True)
            w = max(w, float(excess((1 / torch.sqrt(rn['var'])).float(), rn['rstd'], rn['rstd_b']).max()))
        elif name == 'eval dx by the training formula':
            mean, rstd = R.bn_saved(x)
            dy = torch.randn(M, N, generator=torch.Generator().manual_seed(M))
            good, bad = R.bn_bwd(dy, x, mean, rstd, p['w'], False), R.bn_bwd(dy, x, mean, rstd, p['w'], True)
            w = max(w, float(excess(bad['dx'].float(), good['dx'], good['dx_b']).max()))
        elif name == 'last partial row group dropped':
            got = x64[:M - M % 4].sum(0) / M
            w = max(w, float(excess(got.float(), r['mean'], r['mean_b']).max()))
    return w


def _mix_mutant_excess(name):
    w = 0.0
    if name == 'rbf without the clamp':                          # the constructed case is held to the bit: its bound is 0
        for nb in R.MIX_NB:
            c = R.mix_clamped_case(nb)
            raw = f64(c['sa'])[:, None] + f64(c['sb'])[None, :] - 2 * f64(c['G'])
            assert float(raw.max()) < 0
            k = sum(torch.exp(-ref64.f32(g) * raw) for g in c['gammas']) / nb
            w = max(w, float(excess(k.float(), torch.ones_like(k), torch.zeros_like(k)).max()))
        return w
    for (M, N), nb, kind in itertools.product(R.MIX_SHAPES, R.MIX_NB, ('poly', 'rbf')):
        c = R.mix_case(M, N, nb, kind)
        e = R.mix_elements(c['G'], kind, c['gammas'], c['sa'], c['sb'])
        fw = R.mix_fwd(c['G'], kind, c['gammas'], c['sa'], c['sb'])
        if name == 'row tail dropped':
            got = e['k'][:, :N - N % 256].sum(1)
            w = max(w, float(excess(got.float(), fw['part'], fw['part_b']).max()))
        elif name == '1/nb missing':
            w = max(w, float(excess((e['k'] * nb).sum(1).float(), fw['part'], fw['part_b']).max()))
        elif name == 'poly derivative without its 2' and kind == 'poly':
            w = max(w, float(excess((e['dk'] / 2).float(), e['dk'], e['dk_b']).max()))
        elif name == 'sa read with stride ld' and kind == 'rbf':
            sa_bad = (c['a'].double() @ c['a'].double().t())[:, 0].float()       # element (i, 0) of a a^T instead of (i, i)
            bad = R.mix_fwd(c['G'], kind, c['gammas'], sa_bad, c['sb'])
            w = max(w, float(excess(bad['part'].float(), fw['part'], fw['part_b']).max()))
    return w


def _means_mutant_excess(name):
    w = 0.0
    if name == 'identity diff over n1 on both sides':
        for (n1, n2, Z), off in itertools.product(R.IDENTITY_SHAPES, (False, True)):
            x1, x2 = R.identity_case(n1, n2, Z, off)
            r = R.identity_fwd(x1, x2)
            got = x1.double().sum(0) / n1 - x2.double().sum(0) / n1
            w = max(w, float(excess(got.float(), r['diff'], r['diff_b']).max()))
    else:                                                        # RFF: sin in place of cos
        for n1, n2, Rr in R.RFF_SHAPES:
            th1, th2, c = R.rff_case(n1, n2, Rr)
            r = R.rff_fwd(th1, th2, c)
            got = ref64.f32(c) * (torch.sin(th1.double()).mean(0) - torch.sin(th2.double()).mean(0))
            w = max(w, float(excess(got.float(), r['diff'], r['diff_b']).max()))
    return w


MUTANTS = [(_bn_mutant_excess, n) for n in ('one-pass variance', 'biased running_var', 'momentum on the old value',
                                            'eps left out of rstd', 'eval dx by the training formula',
                                            'last partial row group dropped')] + \
          [(_mix_mutant_excess, n) for n in ('row tail dropped', '1/nb missing', 'rbf without the clamp',
                                             'poly derivative without its 2', 'sa read with stride ld')] + \
          [(_means_mutant_excess, n) for n in ('identity diff over n1 on both sides', 'RFF sin in place of cos')]


@pytest.mark.parametrize('fn,name', MUTANTS, ids=[n.replace(' ', '_') for _, n in MUTANTS])
def test_mutant_lands_outside_the_bound(fn, name):
    w = fn(name)
    print('mutant %-40s worst excess %.3g' % (name, w))
    assert w >= 4.0, 'the cases do not notice "%s": worst excess %.3g' % (name, w)


def test_bounds_keep_the_rule():
    assert max(R.c_mix(nb) for nb in range(1, 9)) <= ref64.C_MAX and R.C_TRIG <= ref64.C_MAX
    t = torch.ones(10, 3)
    assert torch.equal(R.col_sum_bound(t, 10, 4), torch.full((3,), (3 + 3) * U * 10, dtype=torch.float64))
    assert np.isclose(R.FLOOR, 2.0 ** -126) and math.isfinite(R.FLOOR)
