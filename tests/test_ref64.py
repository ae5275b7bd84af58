"""CPU: the float64 reference of tests/ref64.py against closed forms, and the bound rule's teeth -- fp32 emulations of
the formulas that lose accuracy must fail it, their accurate replacements must pass."""
import math

import numpy as np
import pytest
import torch

from tests import ref64
from tests.ref64 import U, bound, excess, f32

SHIFT = f32(1e-3)


def _grid(lo, hi, n):
    return torch.from_numpy(np.linspace(lo, hi, n).astype(np.float32))


def test_act_and_derivative_match_closed_forms():
    x = _grid(-30.0, 30.0, 2401).double()
    sp = torch.tensor([v if v > 20 else max(v, 0.0) + math.log1p(math.exp(-abs(v))) for v in x.tolist()],
                      dtype=torch.float64)
    assert torch.allclose(ref64.act('softplus', x), sp, rtol=1e-15, atol=0)
    sig = torch.tensor([1.0 if v > 20 else 1.0 / (1.0 + math.exp(-v)) for v in x.tolist()], dtype=torch.float64)
    assert torch.allclose(ref64.dact('softplus', x), sig, rtol=1e-15, atol=0)
    elu = torch.tensor([v if v > 0 else math.expm1(v) for v in x.tolist()], dtype=torch.float64)
    assert torch.allclose(ref64.act('elu', x), elu, rtol=1e-15, atol=0)
    # the derivative in terms of the output is the derivative, to fp64 rounding of y (the condition term |y g'(y)|)
    for a in ref64.ACTS:
        y = ref64.act(a, x)
        g = ref64.dact(a, x)
        tol = 1e-15 * (g.abs() + y.abs() * ref64.dact_from_y_slope(a, y))
        if a == 'softplus':         # (above the threshold torch's softplus is x, slope 1: 1 - e^-x differs by e^-x)
            tol = tol + torch.where(x > 20, torch.exp(-x), torch.zeros_like(x))
        assert bool(((ref64.dact_from_y(a, y) - g).abs() <= tol).all()), a
    y = torch.tensor([1e-30, 1e-12, 1e-6, 0.25, 3.0], dtype=torch.float64)
    ref = torch.tensor([-math.expm1(-v) for v in y.tolist()], dtype=torch.float64)
    assert torch.equal(ref64.dact_from_y('softplus', y), ref)


def test_nll_terms_match_closed_forms():
    pre = torch.tensor([-30.0, -12.0, -0.5, 0.0, 3.0, 25.0], dtype=torch.float64)
    x = torch.tensor([1.0, 0.5, -2.0, 0.0, 1.5, 10.0], dtype=torch.float64)
    m = torch.tensor([0.999, 0.5, -1.0, 0.1, -8.5, 0.0], dtype=torch.float64)
    r = ref64.nll_sigma_pre(x, m, pre, SHIFT, coef=-0.5)
    for i in range(pre.numel()):
        p, xv, mv = float(pre[i]), float(x[i]), float(m[i])
        sd = (p if p > 20 else max(p, 0.0) + math.log1p(math.exp(-abs(p)))) + SHIFT
        t = (xv - mv) / sd
        sg = 1.0 if p > 20 else 1.0 / (1.0 + math.exp(-p))
        assert r['term'][i].item() == pytest.approx(ref64.LOG_2PI + 2 * math.log(sd) + t * t, rel=1e-14)
        assert r['gm'][i].item() == pytest.approx(-0.5 * t / sd, rel=1e-14)
        assert r['gs'][i].item() == pytest.approx(-0.5 * (t * t - 1) / sd * sg, rel=1e-13)
    s = ref64.act('softplus', pre) + SHIFT
    f = ref64.nll_sigma_finished(x, m, s, SHIFT, 'softplus', coef=-0.5)
    assert torch.allclose(f['term'], r['term'], rtol=1e-14) and torch.allclose(f['gm'], r['gm'], rtol=1e-14)
    assert torch.allclose(f['gs'], r['gs'], rtol=1e-10)
    lv = torch.tensor([-30.0, 0.0, 30.0], dtype=torch.float64)
    q = ref64.nll_logvar(x[:3], m[:3], lv)
    for i in range(3):
        d, v = float(x[i] - m[i]), float(lv[i])
        assert q['term'][i].item() == pytest.approx(ref64.LOG_2PI + v + d * d * math.exp(-v), rel=1e-14)
        assert q['gs'][i].item() == pytest.approx(-0.5 * (1 - d * d * math.exp(-v)), rel=1e-12, abs=1e-300)


# ---------------------------------------------------------------- the rule has teeth: fp32 emulations
def _softplus32(pre, kahan):
    """the kernels' softplus in numpy fp32: max(p, 0) + log1p(exp(-|p|)), log1p as log(1 + e) or Kahan's quotient"""
    p = pre.numpy().astype(np.float32)
    e = np.exp(-np.abs(p)).astype(np.float32)
    u = (np.float32(1) + e).astype(np.float32)
    if kahan:
        dd = (u - np.float32(1)).astype(np.float32)
        with np.errstate(invalid='ignore', divide='ignore'):
            lg = np.where(dd == 0, e, np.log(u) * (e / dd)).astype(np.float32)
    else:
        lg = np.log(u).astype(np.float32)
    return torch.from_numpy(np.where(p > 20, p, (np.maximum(p, np.float32(0)) + lg).astype(np.float32)))


def _dsoftplus32(y, accurate):
    y = y.numpy().astype(np.float32)
    g = -np.expm1(-y) if accurate else np.float32(1) - np.exp(-y)
    return torch.from_numpy(g.astype(np.float32))


PRE = _grid(-17.0, -8.0, 901)


def test_rule_rejects_one_minus_exp_and_accepts_expm1():
    y = ref64.act('softplus', PRE).float()              # a stored softplus output in the hard regime
    ref = ref64.dact_from_y('softplus', y)
    comps = ref.abs() + y.double().abs() * ref64.dact_from_y_slope('softplus', y)
    bd = bound(ref64.C_MAX, comps)
    assert float(excess(_dsoftplus32(y, accurate=False), ref, bd).max()) > 1.0
    assert float(excess(_dsoftplus32(y, accurate=True), ref, bound(4, comps)).max()) <= 1.0


@pytest.mark.parametrize('d', [0.0, 1e-3, 0.1])
def test_rule_rejects_log_one_plus_e_and_accepts_kahan(d):
    """an sd formed with log(1 + e) fails the bound of d NLL / d pre over pre in [-17, -8]; Kahan's quotient passes"""
    x = torch.full_like(PRE, 0.5)
    m = (x.double() - d).float()
    r = ref64.nll_sigma_pre(x, m, PRE, SHIFT)
    bd = bound(ref64.C_MAX, r['gs_c'], r['gs_x'])

    def gs32(kahan):
        # everything after sd in float64: only the softplus is under test
        sd = (_softplus32(PRE, kahan) + np.float32(SHIFT)).double()
        t = (x.double() - m.double()) / sd
        return (t * t - 1) / sd * torch.sigmoid(PRE.double())
    assert float(excess(gs32(False), r['gs'], bd).max()) > 1.0
    assert float(excess(gs32(True), r['gs'], bound(8, r['gs_c'], r['gs_x'])).max()) <= 1.0
    sd_ref = ref64.act('softplus', PRE) + SHIFT
    a = PRE.double().abs()
    sd_bd = bound(ref64.C_MAX, sd_ref, a * torch.sigmoid(-a))
    assert float(excess((_softplus32(PRE, False) + np.float32(SHIFT)).double(), sd_ref, sd_bd).max()) > 1.0


def test_bound_rule_limits():
    with pytest.raises(AssertionError):
        bound(65, torch.ones(1))
    assert float(bound(1, torch.ones(1))) == U
    r = excess(torch.tensor([1.0, float('nan')]), torch.tensor([1.0, 1.0]), torch.tensor([0.0, 1.0]))
    assert float(r[0]) == 0.0 and math.isinf(float(r[1]))
