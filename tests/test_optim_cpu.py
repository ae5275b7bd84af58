"""The checks of tests/test_gpu_optim.py, proven on the host (no GPU): the float64 reference and componentwise bound of
tests/optim_ref.py admit both fp32 emulations of the optimiser kernels (every operation rounded; multiply-adds fused) and
both ``tests/kernel_ref.py`` optimisers on every case class, and every faulty emulation fails exactly the checks named for
it -- so the bound is neither too tight for a correct sweep nor too loose to see a wrong one.  Also here: how far the fp32
betas of ``dv_adam_hyper`` move a trajectory, measured two ways and held to what the perturbation allows.  With ``-s`` the
module prints the worst |error| / bound per stored quantity and case class."""
import numpy as np
import pytest
import torch

from tests import kernel_ref
from tests import optim_ref as R


@pytest.fixture(scope='module', autouse=True)
def table():
    worst = {}
    yield worst
    print('\noptimiser sweeps on the host: worst |got - float64| / bound (quantity: rounded emulation / fused emulation / kernel_ref)')
    for kind in R.KINDS:
        for cls, _ in R.cases(kind):
            row = []
            for q in R.STORED[kind]:
                row.append('%s %s' % (q, ' / '.join('%.3f' % worst.get((kind, cls, q, who), float('nan'))
                                                    for who in ('rounded', 'fused', 'kernel_ref'))))
            print('  %-7s %-10s %s' % (kind, cls, '   '.join(row)))
    for k in sorted(k for k in worst if k[0] == 'beta'):
        print('  %s: %.3e' % (' '.join(k[1:]), worst[k]))


def run_kernel_ref(kind, arrays, t, h):
    p, g, m, v = (torch.from_numpy(a.copy()) for a in arrays)
    fn = kernel_ref.adam_l2 if kind == 'adam' else kernel_ref.adamax_l2
    fn(p, g, m, v, torch.tensor([t], dtype=torch.int32), lr=h['lr'], beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'],
       weight_decay=h['weight_decay'], gscale=h['gscale'])
    return {'p': p.numpy(), 'm': m.numpy(), R.STORED[kind][2]: v.numpy()}


ALL = [(k, c) for k in R.KINDS for c, _ in R.cases(k)]


@pytest.mark.parametrize('kind,cls', ALL, ids=['%s-%s' % kc for kc in ALL])
def test_emulations_and_kernel_ref_within_the_bound(table, kind, cls):
    for t, gs, wd in R.settings(cls):
        arrays, h, ref = R.case_ref(kind, cls, t, gs, wd)
        site = '%s %s t=%d gscale=%g wd=%g' % (kind, cls, t, gs, wd)
        runs = {'rounded': R.emulate(kind, *arrays, t, h, fused=False), 'fused': R.emulate(kind, *arrays, t, h, fused=True),
                'kernel_ref': run_kernel_ref(kind, arrays, t, h)}
        for who, got in runs.items():
            failed, worst, _ = R.verify(kind, got, arrays, t, h, site=site, ref=ref)
            for q, w in worst.items():
                table[(kind, cls, q, who)] = max(table.get((kind, cls, q, who), 0.0), w)
            assert failed == set(), (site, who, worst)
            assert all(np.isfinite(a).all() for a in got.values()), (site, who)
        if cls == 'pads' and kind == 'adam':
            for who, got in runs.items():
                assert all(not R.bits(a).any() for a in got.values()), (site, who, 'pads must stay bit-zero')


def test_the_cancelling_gradient_is_why_the_bound_is_in_operand_magnitudes():
    """with weight decay, g + wd p cancels.  Parameters placed so that one part in 10^4 of g is left: the fp32 v' is
    thousands of ulps of v' away from float64 where wd p is rounded before it is added, and inside the bound"""
    _, g, m, v = R.case('normal')
    h = R.hyper32(weight_decay=0.05)
    p = (-g.astype(np.float64) / h['weight_decay'] * (1 + 1e-4)).astype(np.float32)
    want, bound = R.reference('adam', p, g, m, v, 3, h)
    for fused in (False, True):
        got = R.emulate('adam', p, g, m, v, 3, h, fused=fused)
        ulps = np.abs(got['v'].astype(np.float64) - want['v']) / (R.U * want['v'])
        assert fused or np.median(ulps) > 1000, np.median(ulps)      # (fused: wd p enters unrounded, g2 is good to an ulp)
        failed, worst, _ = R.verify('adam', got, (p, g, m, v), 3, h, ref=(want, bound))
        assert failed == set(), worst


FAULTS = [('adam', f) for f in R.ADAM_FAULTS] + [('adamax', f) for f in R.ADAMAX_FAULTS]


@pytest.mark.parametrize('kind,fault', FAULTS, ids=[f for _, f in FAULTS])
def test_faulty_arithmetic_fails_its_checks_and_no_other(kind, fault):
    expected = (R.ADAM_FAULTS if kind == 'adam' else R.ADAMAX_FAULTS)[fault]
    failed, where = set(), set()
    for cls, _ in R.cases(kind):
        for t, gs, wd in R.settings(cls):
            arrays, h, ref = R.case_ref(kind, cls, t, gs, wd)
            f, _, _ = R.verify(kind, R.emulate(kind, *arrays, t, h, fused=True, fault=fault), arrays, t, h, ref=ref)
            failed |= f
            if f:
                where.add(cls)
    assert failed == expected, (fault, failed, sorted(where))
    if fault in ('eps_in_root', 'eps_before_bc2'):
        assert 'tiny' in where      # (sqrt(v) of the order of eps: every element is off, not the few with a small gradient)


def _framed_step(n, lead):
    h, t = R.hyper32(weight_decay=0.05), 1
    inputs = R.frame_inputs(n)
    before, sl = {}, None
    for k, a in zip('pgmv', inputs):
        before[k], sl = R.framed(a, lead=lead)
    got = R.emulate('adam', *(before[k][sl] for k in 'pgmv'), t, h, fused=True)
    after = {k: a.copy() for k, a in before.items()}
    for k in 'pmv':
        after[k][sl] = got[k]
    return inputs, before, after, sl, t, h


def _frame_checks(inputs, before, after, sl, t, h):
    bad = R.memory_faults(before, after, sl)
    failed, _, _ = R.verify('adam', {k: after[k][sl] for k in 'pmv'}, inputs, t, h)
    return bad | failed


@pytest.mark.parametrize('n', [255, 1023])
def test_faulty_indexing_fails_its_checks_and_no_other(n):
    inputs, before, after, sl, t, h = _framed_step(n, lead=1)
    assert _frame_checks(inputs, before, after, sl, t, h) == set()
    for name, expected in R.INDEX_FAULTS.items():
        bad = _frame_checks(inputs, before, R.index_fault(name, before, after, sl), sl, t, h)
        assert bad == expected, (name, bad)


# ------------------------------------------------------------------------------------------------ the betas
def _gamma():
    rs = np.random.RandomState(4)
    return rs.randn(R.N_CASE).astype(np.float32), rs.randn(R.N_CASE).astype(np.float32)


def _torch_adam(p0, gamma, T):
    ref = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=R.HYPER['lr'])
    for k in range(1, T + 1):
        ref.grad = torch.from_numpy(gamma * np.float32(R.long_scale(k)))
        opt.step()
    st = opt.state[ref]
    return dict(p=ref.detach().numpy(), m=st['exp_avg'].numpy(), v=st['exp_avg_sq'].numpy())


def _within(table, name, got, want, bound):
    for q in 'pmv':
        d = np.abs(np.asarray(got[q], np.float64) - np.asarray(want[q], np.float64))
        table[('beta', name, q, 'max distance')] = float(d.max())
        table[('beta', name, q, 'max distance / bound')] = float((d / bound[q]).max())
        assert (d <= bound[q]).all(), (name, q, float((d / bound[q]).max()))


@pytest.mark.parametrize('T', [3, R.T_LONG])
def test_what_the_fp32_betas_move(table, T):
    """(a) the float64 reference with the carried betas against the same reference with python's, free-running: within the
    beta part of ``trajectory_bounds``; (b) kernel_ref.adam_l2 as shipped (python betas) against torch.optim.Adam: within the
    rounding part; (c) the fused emulation (carried betas, fp32) against torch.optim.Adam: within the sum -- what
    tests/test_gpu_optim.py asks of the device"""
    p0, gamma = _gamma()
    h = R.hyper32()
    # (pmax: |update| <= lr RHO a step, 0.3 over 200 steps)
    both, beta = R.trajectory_bounds(T, h, gamma, pmax=float(np.abs(p0).max()) + 1.0)
    rounding = {q: both[q] - beta[q] for q in both}
    runs = {}
    for name, betas in (('carried', None), ('python', (0.9, 0.999))):
        s = dict(p=p0.astype(np.float64), m=np.zeros(p0.size), v=np.zeros(p0.size))
        for k in range(1, T + 1):
            s, _ = R.ref_adam(s['p'], gamma.astype(np.float64) * R.long_scale(k), s['m'], s['v'], k, h, betas=betas)
        runs[name] = s
    _within(table, 'T=%d float64, carried betas vs python betas' % T, runs['carried'], runs['python'], beta)
    want = _torch_adam(p0, gamma, T)
    p, m, v = (torch.from_numpy(a.copy()) for a in (p0, np.zeros_like(p0), np.zeros_like(p0)))
    for k in range(1, T + 1):
        kernel_ref.adam_l2(p, torch.from_numpy(gamma * np.float32(R.long_scale(k))), m, v, torch.tensor([k]), lr=R.HYPER['lr'])
    _within(table, 'T=%d kernel_ref as shipped vs torch.optim.Adam' % T, dict(p=p.numpy(), m=m.numpy(), v=v.numpy()), want, rounding)
    s = dict(p=p0, m=np.zeros_like(p0), v=np.zeros_like(p0))
    for k in range(1, T + 1):
        s = R.emulate('adam', s['p'], gamma * np.float32(R.long_scale(k)), s['m'], s['v'], k, h, fused=True)
    _within(table, 'T=%d fused emulation vs torch.optim.Adam' % T, s, want, both)
