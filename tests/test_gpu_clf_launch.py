"""-m gpu: the classifier-head launch -- ``dv_smalln_linear_fwd`` with its y-marginalisation and fprop-KL riders, both of
its kernels -- against the staged float64 reference of ``tests/clf_launch_ref.py``: every stage within its componentwise
bound, selections exact, nothing written outside the outputs' extent, every element inside it written, two launches
bit-equal, the free-bits tie weighted 1/2.  The separate launches the fused one replaces run on the same inputs and are
held to the same reference, so both routes and the unfused sequence carry identical obligations.  With ``-s`` the module
prints the worst excess (|got - ref| / bound) per stage and route.

Also here: the clamp-gated softmax backward inside ``dv_smalln_linear_bwd_data`` / ``_bwd_weight`` at the 1e-10 clamp."""
import math

import numpy as np
import pytest
import torch

from tests import clf_launch_ref as L
from tests.ref64 import U, bound, check, f64

pytestmark = pytest.mark.gpu

ROUTES = ('fast', 'generic', 'separate')


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


@pytest.fixture(scope='module', autouse=True)
def table():
    """worst excess per (stage, route) over the module's tests, printed when the module is done (visible with -s)"""
    worst = {}
    yield worst
    print('\nclassifier-head launch: worst |got - ref| / bound per stage and route')
    print('%-8s' % 'stage' + ''.join('%10s' % r for r in ROUTES))
    for st in L.STAGES:
        print('%-8s' % st + ''.join('%10s' % ('%.3f' % worst[(st, r)] if (st, r) in worst else '-') for r in ROUTES))


def note(table, rt, worst):
    for st, v in worst.items():
        if st in L.STAGES:
            table[(st, rt)] = max(table.get((st, rt), 0.0), v)


def on_dev(prior, dev):
    return prior.to(dev) if torch.is_tensor(prior) else prior


def fused(K, case, o, dev, kl_min, prior, **kw):
    out = L.alloc(case, dev, klfp=kw.pop('klfp', None))
    L.launch(K, case, o, out, kl_min, prior, **kw)
    torch.cuda.synchronize()
    return L.to_host(out)


def separate(K, case, o, dev, kl_min, prior):
    out = L.alloc(case, dev)
    L.launch_separate(K, case, o, out, kl_min, prior)
    torch.cuda.synchronize()
    return L.to_host(out)


def hold(K, dev, table, case, settings):
    """the fused launch and the separate launches of one case at every prior form and kl_min setting, then the tie"""
    o = L.operands(case, dev)
    rt = L.route(case['shape'])
    at_zero = None
    for pname, prior in L.priors(case):
        pd = on_dev(prior, dev)
        for sname, kl_min in settings:
            site = '%s prior=%s kl_min=%s' % (case['name'], pname, sname)
            host = fused(K, case, o, dev, kl_min, pd)
            note(table, rt, L.verify(case, host, kl_min, prior, site=site + ' fused'))
            assert L.selections(case, host, kl_min) == [], site
            if sname == 'above':      # the gate is 0 everywhere
                assert bool((host['dq'][1] == 0.0).all()) and bool((host['dp'][1] == 0.0).all()), site
                assert bool((host['klfp'][1] == 2 * kl_min).all()), site
            sep = separate(K, case, o, dev, kl_min, pd)
            note(table, 'separate', L.verify(case, sep, kl_min, prior, site=site + ' separate'))
            assert L.selections(case, sep, kl_min) == [], site
            again = fused(K, case, o, dev, kl_min, pd)
            for k in host:
                assert torch.equal(host[k][0], again[k][0]), '%s: two launches differ in %s' % (site, k)
            if at_zero is None and kl_min == 0.0:
                at_zero = host
    # the tie: kl_min set to a raw1 the launch itself stored -- that row sits exactly on the gate and gets weight 1/2
    # (c * 0.5 is exact, so its gradient rows are bitwise half of the open gate's); its neighbours keep their side
    raw1 = at_zero['raw1'][1]
    order = torch.argsort(raw1)
    t = int(order[raw1.numel() // 2])
    kl_min = float(raw1[t])
    prior = case['prior_scalar']
    host = fused(K, case, o, dev, kl_min, prior)
    site = '%s kl_min=tie' % case['name']
    note(table, rt, L.verify(case, host, kl_min, prior, site=site))
    assert L.selections(case, host, kl_min) == [], site
    ties = host['raw1'][1] == kl_min
    assert bool(ties[t]) and torch.equal(host['raw1'][1], raw1), site
    for k in ('dq', 'dp'):
        assert torch.equal(host[k][1][ties], 0.5 * at_zero[k][1][ties]), site
        assert torch.equal(host[k][1][raw1 > kl_min], at_zero[k][1][raw1 > kl_min]), site
        assert bool((host[k][1][raw1 < kl_min] == 0.0).all()), site
    assert bool((raw1 > kl_min).any()) and bool((raw1 < kl_min).any())


@pytest.mark.parametrize('case', L.CASES, ids=[L.case_id(c) for c in L.CASES])
def test_fused_launch_and_separate_launches_against_float64(K, dev, table, case):
    hold(K, dev, table, case, L.kl_min_settings(case))


@pytest.mark.parametrize('case', L.EDGE_CASES, ids=[L.case_id(c) for c in L.EDGE_CASES])
def test_fused_launch_at_the_input_edges(K, dev, table, case):
    """log-variances over [-30, 30] in both KL terms; classifier probabilities on both sides of the 1e-10 clamp"""
    hold(K, dev, table, case, (('0', 0.0), ('between', case['kl_min_between'])))


@pytest.mark.parametrize('case', [L.CASES[1], L.CASES[7]], ids=[L.case_id(L.CASES[1]), L.case_id(L.CASES[7])])
def test_riders_left_out(K, dev, table, case):
    """the y-marginalisation alone (klfp an input: evaluation-free train steps of VFAE), and either form without the logits
    output: everything else bit-equal to the launch that stores them, the logits buffer untouched"""
    o = L.operands(case, dev)
    klfp = torch.rand(case['F'], generator=torch.Generator().manual_seed(3)) * 5 + 0.5
    for pname, prior in L.priors(case):
        pd = on_dev(prior, dev)
        site = '%s prior=%s ymarg alone' % (case['name'], pname)
        host = fused(K, case, o, dev, 0.0, pd, fprop=False, klfp=klfp)
        note(table, 'generic', L.verify(case, host, 0.0, prior, fprop=False, site=site))
        assert torch.equal(host['klfp'][1], klfp), site
        for fprop in (False, True):
            kw = dict(fprop=False, klfp=klfp) if not fprop else {}
            kl_min = case['kl_min_between'] if fprop else 0.0
            full = fused(K, case, o, dev, kl_min, pd, **kw)
            bare = fused(K, case, o, dev, kl_min, pd, logits=False, **kw)
            L.verify(case, bare, kl_min, prior, fprop=fprop, logits=False, site=site + ' logits=None')
            assert bool((bare['logits'][0] == L.SENTINEL).all()), site
            for k in full:
                if k != 'logits':
                    assert torch.equal(full[k][0], bare[k][0]), '%s logits=None: %s differs' % (site, k)


# ------------------------------------------------------------------ the softmax backward of the weight / data gradients
@pytest.mark.parametrize('case', L.EDGE_CASES[2:], ids=[L.case_id(c) for c in L.EDGE_CASES[2:]])
def test_smalln_backward_at_the_clamp(K, dev, case):
    """softmax_clamp_bwd_row inside dv_smalln_linear_bwd_data / _bwd_weight on stored probabilities on both sides of the 1e-10
    clamp, against float64 P * (g_masked - <g_masked, P>).  W = I: the data gradient IS d logits (a sum with one non-zero
    product is exact); the weight gradient is its product with the logit grid, a row sum over M"""
    M, Y = case['shape'][:2]
    o = L.operands(case, dev)
    out = L.alloc(case, dev)
    L.launch(K, case, o, out, 0.0, case['prior_scalar'])
    probs = out['probs'][1]
    P = f64(probs)
    assert bool((P == L.P_MIN).any()) and bool((P > L.P_MIN).any())
    g = torch.from_numpy(np.random.default_rng(Y).standard_normal((M, Y + 1)).astype(np.float32)).to(dev)[:, :Y]
    x = f64(o['a1'])
    G = f64(g)
    gm = torch.where(P > L.P_MIN, G, torch.zeros_like(P))
    dl = P * (gm - (gm * P).sum(1, keepdim=True))
    # C = 8 as softmax_clamp_bwd: a dot product of Y terms, a difference and a product
    dl_b = bound(8, P * (gm.abs() + (gm * P).abs().sum(1, keepdim=True)))
    for probs_arg, ref, ref_b in ((probs, dl, dl_b), (None, G, torch.zeros_like(G))):
        name = 'at the clamp' if probs_arg is not None else 'probs=None'
        buf = torch.full((M + 2, Y + 3), L.SENTINEL, device=dev)
        K.smalln_bwd_data([(buf[:M, :Y], 0, 1.0, 0.0)], g, probs_arg, o['W'])
        torch.cuda.synchronize()
        check('smalln_bwd_data ' + name, buf[:M, :Y].cpu(), ref, ref_b, p=P)
        assert bool((buf[M:] == L.SENTINEL).all()) and bool((buf[:, Y:] == L.SENTINEL).all())
        wbuf, db = torch.full((Y + 2, Y + 3), L.SENTINEL, device=dev), torch.full((Y + 3,), L.SENTINEL, device=dev)
        K.smalln_bwd_weight(wbuf[:Y, :Y], db[:Y], g, probs_arg, o['a1'])
        torch.cuda.synchronize()
        # every term dl[r, j] x[r, k] within the bound of dl (and one rounding of the product), the sum over M by the row
        # sum's rule
        terms = ref.abs().t() @ x.abs()
        sum_b = (math.ceil(M / 256) + 16) * U
        check('smalln_bwd_weight dW ' + name, wbuf[:Y, :Y].cpu(), ref.t() @ x, ref_b.t() @ x.abs() + (sum_b + U) * terms)
        check('smalln_bwd_weight db ' + name, db[:Y].cpu(), ref.sum(0), ref_b.sum(0) + sum_b * ref.abs().sum(0))
        assert bool((wbuf[Y:] == L.SENTINEL).all()) and bool((wbuf[:, Y:] == L.SENTINEL).all())
        assert bool((db[Y:] == L.SENTINEL).all())
