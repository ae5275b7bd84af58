"""Float64 reference of the element-wise math of the HIP row kernels and GEMM epilogues, and the one error-bound rule the
numerics tests (``tests/test_gpu_numerics.py``) hold them to.

Independent of ``tests/kernel_ref.py`` (an fp32 restatement of the kernels' own formulas): values follow the model's
semantics in float64, evaluated on the exact fp32 inputs a kernel received, and gradients are float64 autograd through
the same expression.  Paths that receive a pre-activation are compared with ``F.softplus(pre) + shift``; paths that
receive a finished output ``s`` with the derivative written in terms of the output, evaluated in float64 on that ``s``.

The bound rule, componentwise (never relative to a tensor's maximum):

    |got - ref| <= C * U * (sum of |components|) + 2 * U * extra,      U = 2**-24, C <= 64

* the components of a value are the magnitudes of the terms and factors it is formed from (an NLL term: log 2 pi,
  |2 log sd| and t^2);
* a derivative computed from an output y adds the condition term |y_stored * g'(y)| (the rounding of the stored output);
* a row sum of X terms adds (ceil(X / 256) + 16) * U * sum |terms|  (``row_sum_bound``);
* ``extra``: where a hardware exp sees an argument a, its two roundings (a * log2 e) cost |a| U relative each.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_MAX = 64
LOG_2PI = math.log(2.0 * math.pi)
ACTS = ('elu', 'softplus', 'sigmoid', 'tanh', 'relu', 'leaky_relu', 'selu', 'softsign')
SELU_L, SELU_A = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def f64(t):
    """float64 host copy of the exact values a kernel received (or wrote)"""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    return t.detach().to('cpu', torch.float64)


def f32(v):
    """the fp32 value of a host scalar, as a kernel argument carries it"""
    return float(np.float32(v))


# --------------------------------------------------------------------------------------------- activations
def act(name, x):
    """the model's activation in float64 (torch semantics: softplus with threshold 20, leaky slope 0.1)"""
    x = f64(x) if not torch.is_tensor(x) or x.dtype != torch.float64 else x
    return {'identity': lambda v: v, 'elu': F.elu, 'softplus': F.softplus, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh,
            'relu': torch.relu, 'leaky_relu': lambda v: F.leaky_relu(v, 0.1), 'selu': F.selu,
            'softsign': F.softsign}[name](x)


def dact(name, x):
    """d act / dx at x: float64 autograd through ``act``"""
    p = f64(x).requires_grad_(True)
    act(name, p).backward(torch.ones_like(p))
    return p.grad


def dact_from_y(name, y):
    """the derivative written in terms of the output y = act(x), in float64 (softplus: -expm1(-y), not 1 - exp(-y))"""
    y = f64(y)
    one = torch.ones_like(y)
    if name == 'identity':
        return one
    if name == 'elu':
        return torch.where(y > 0, one, y + 1)
    if name == 'softplus':
        return -torch.expm1(-y)
    if name == 'sigmoid':
        return y * (1 - y)
    if name == 'tanh':
        return 1 - y * y
    if name == 'relu':
        return (y > 0).double()
    if name == 'leaky_relu':
        return torch.where(y > 0, one, 0.1 * one)
    if name == 'selu':
        return torch.where(y > 0, SELU_L * one, y + SELU_L * SELU_A)
    if name == 'softsign':
        return (1 - y.abs()) ** 2
    raise KeyError(name)


def dact_from_y_slope(name, y):
    """|g'(y)| of g = ``dact_from_y``: times the magnitude of the stored output, the condition term of a derivative taken
    from a rounded output"""
    y = f64(y)
    zero = torch.zeros_like(y)
    if name in ('identity', 'relu', 'leaky_relu'):
        return zero
    if name in ('elu', 'selu'):
        return torch.where(y > 0, zero, torch.ones_like(y))
    if name == 'softplus':
        return torch.exp(-y)
    if name == 'sigmoid':
        return (1 - 2 * y).abs()
    if name == 'tanh':
        return 2 * y.abs()
    if name == 'softsign':
        return 2 * (1 - y.abs()).abs()
    raise KeyError(name)


def act_exp_extra(name, x):
    """magnitude of what a hardware exp contributes to act(x), times |its argument| (the ``extra`` of the rule):
    elu evaluates exp(x) - 1 on the hardware exp for x <= -0.5, softplus exp(-|x|)"""
    x = f64(x)
    if name == 'elu':
        return torch.where(x <= -0.5, x.abs() * torch.exp(torch.clamp(x, max=0.0)), torch.zeros_like(x))
    if name == 'softplus':
        return x.abs() * torch.exp(-x.abs())
    return torch.zeros_like(x)


# ------------------------------------------------------------------------------------ Gaussian (sigma) NLL
def nll_sigma_pre(x, m, pre, shift, coef=1.0, sd_act='softplus', hw_exp=True, from_output=False):
    """one Gaussian log-likelihood term per element for sd = act(pre) + shift (the raw and fused paths, which receive the
    pre-activation): ``term`` = log 2pi + 2 log sd + t^2 (the row value is -0.5 * sum of terms), ``gm`` / ``gs`` =
    coef * d(-0.5 term)/d(mu, pre); each with its components (``*_c``) and hardware-exp extra (``*_x``: softplus on
    exp(-|pre|) when ``hw_exp``).  ``from_output``: the kernel takes the activation's derivative from its rounded output
    (the condition term |sd * g'(sd - shift)| joins the components of ``gs``)"""
    x, m, p = f64(x), f64(m), f64(pre)
    c = f64(coef)
    mm, pp = m.clone().requires_grad_(True), p.clone().requires_grad_(True)
    sd = act(sd_act, pp) + shift
    t = (x - mm) / sd
    term = LOG_2PI + 2 * torch.log(sd) + t * t
    (-0.5 * term).backward(torch.ones_like(term))
    sd, t, term = sd.detach(), t.detach(), term.detach()
    a = p.abs()
    g = dact(sd_act, p).abs()
    rho = a * torch.sigmoid(-a) / sd if hw_exp else torch.zeros_like(sd)   # relative error of sd per U from exp(-|pre|)
    t2 = t * t
    cond = sd * dact_from_y_slope(sd_act, sd - shift) if from_output else torch.zeros_like(sd)
    return dict(sd=sd, t=t, term=term, gm=c * mm.grad, gs=c * pp.grad,
                term_c=LOG_2PI + (2 * torch.log(sd)).abs() + t2,
                term_x=(2 + 2 * t2) * rho,
                gm_c=(c * t / sd).abs(),
                gm_x=2 * (c * t / sd).abs() * rho,
                gs_c=c.abs() / sd * (t2 + 1) * (g + cond),
                gs_x=c.abs() * g / sd * ((t2 + 1) * a * float(hw_exp) + (3 * t2 + 1) * rho))


def nll_sigma_finished(x, m, s, shift, sd_act='softplus', coef=1.0, s_rounded=False):
    """the same terms for the paths that receive the finished sd ``s`` (exact fp32 input): the value on that s, the
    derivative through the sd activation written in terms of the output, g(s - shift), in float64.  ``s_rounded``: the
    kernel formed s itself from the pre-activation (its rounding of s enters the condition term through |s g'|; for an
    exact input s the condition term is |y g'(y)|, y = s - shift)"""
    x, m, s = f64(x), f64(m), f64(s)
    c = f64(coef)
    d = x - m
    t = d / s
    t2 = t * t
    y = s - shift
    g = dact_from_y(sd_act, y) if sd_act != 'identity' else torch.ones_like(s)
    cond = (s if s_rounded else y).abs() * dact_from_y_slope(sd_act, y)
    return dict(term=LOG_2PI + 2 * torch.log(s) + t2,
                gm=c * d / (s * s), gs=c * (t2 - 1) / s * g,
                term_c=LOG_2PI + (2 * torch.log(s)).abs() + t2,
                gm_c=(c * d / (s * s)).abs(),
                gs_c=c.abs() * (t2 + 1) / s * (g.abs() + cond))


def nll_logvar(x, m, lv, coef=1.0):
    """log-variance mode: term = log 2pi + lv + d^2 exp(-lv); gm, gs = coef * d(-0.5 term)/d(mu, lv)"""
    x, m, lv = f64(x), f64(m), f64(lv)
    c = f64(coef)
    d = x - m
    iv = torch.exp(-lv)
    q = d * d * iv
    return dict(term=LOG_2PI + lv + q, gm=c * d * iv, gs=c * -0.5 * (1 - q),
                term_c=LOG_2PI + lv.abs() + q, gm_c=(c * d * iv).abs(), gs_c=0.5 * c.abs() * (1 + q))


def row_sum_bound(comps, X):
    """summation part of the bound for a row sum of X terms with the given components (rows along dim 1)"""
    return (math.ceil(X / 256) + 16) * U * comps.sum(1)


# ---------------------------------------------------------------------------------------------- the rule
def bound(C, comps, extra=None):
    assert 0 < C <= C_MAX, 'C = %g exceeds the rule' % C
    b = C * U * f64(comps)
    if extra is not None:
        b = b + 2 * U * f64(extra)
    return b


def excess(got, ref, bnd):
    """|got - ref| / bound per element (<= 1 passes); non-finite got where ref is finite counts as inf"""
    got, ref, bnd = f64(got), f64(ref), f64(bnd)
    err = (got - ref).abs()
    r = err / torch.clamp(bnd, min=1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def check(site, got, ref, bnd, **where):
    """assert the rule elementwise; the message names the kernel site and the worst element with its inputs"""
    r = excess(got, ref, bnd)
    worst = float(r.max()) if r.numel() else 0.0
    if worst <= 1.0:
        return worst
    flat = int(torch.argmax(torch.nan_to_num(r, posinf=1e300)).item())
    info = {k: float(f64(v).reshape(-1)[flat]) for k, v in where.items()}
    g, rf = f64(got).reshape(-1)[flat], f64(ref).reshape(-1)[flat]
    n_bad = int((r > 1).sum())
    raise AssertionError('%s: %d of %d elements outside the bound; worst %.3g x bound: got %.9g ref %.9g (rel %.3g) at %s'
                         % (site, n_bad, r.numel(), worst, float(g), float(rf), float(abs(g - rf) / max(abs(rf), 1e-300)),
                            info))
