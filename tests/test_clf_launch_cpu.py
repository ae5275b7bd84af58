"""CPU: the checks of the classifier-head launch's tests (tests/test_gpu_clf_launch.py) have teeth, and a correct
implementation passes them -- no device, no library.  On the exact cases the GPU tests use: the fp32 host sequence
``kernel_ref.smalln_fwd(ymarg=, fprop_kl=)`` passes every stage of the staged float64 reference of tests/clf_launch_ref.py,
and every faulty emulation of ``FAULTS`` fails the check that is meant to catch it."""
import pytest
import torch

from tests import clf_launch_ref as L
from tests import kernel_ref
from tests.ref64 import f64

ALL_CASES = L.CASES + L.EDGE_CASES
IDS = [L.case_id(c) for c in ALL_CASES]


def run(mod, case, kl_min, prior, **kw):
    out = L.alloc(case)
    L.launch(mod, case, L.operands(case), out, kl_min, prior, **kw)
    return L.to_host(out)


def tie_kl_min(case, mod=kernel_ref):
    """a raw1 the launch itself stored: rerun with it as kl_min, that row sits exactly on the tie"""
    raw1 = run(mod, case, 0.0, case['prior_scalar'])['raw1'][1]
    return float(raw1[torch.argsort(raw1)[raw1.numel() // 2]])


def settings(case):
    return L.kl_min_settings(case) + (('tie', tie_kl_min(case)),)


# --------------------------------------------------------------------------------------------- the host sequence passes
@pytest.mark.parametrize('case', ALL_CASES, ids=IDS)
def test_host_sequence_passes_every_stage(case):
    for _, prior in L.priors(case):
        for name, kl_min in settings(case):
            host = run(kernel_ref, case, kl_min, prior)
            worst = L.verify(case, host, kl_min, prior, site='%s kl_min=%s' % (case['name'], name))
            assert set(worst) == set(L.STAGES) | {'pads', 'written'}
            assert L.selections(case, host, kl_min) == []
            if name == 'above':      # the gate is 0 everywhere
                assert bool((host['dq'][1] == 0).all()) and bool((host['dp'][1] == 0).all())
                assert bool((host['klfp'][1] == 2 * kl_min).all())
            if name == 'tie':
                assert int((host['raw1'][1] == kl_min).sum()) >= 1


@pytest.mark.parametrize('case', L.CASES[:2] + L.EDGE_CASES[2:], ids=IDS[:2] + IDS[-2:])
def test_host_sequence_passes_without_the_fprop_rider(case):
    klfp = torch.rand(case['F'], generator=torch.Generator().manual_seed(3)) * 5 + 0.5
    for _, prior in L.priors(case):
        out = L.alloc(case, klfp=klfp)
        L.launch(kernel_ref, case, L.operands(case), out, 0.0, prior, fprop=False)
        L.verify(case, L.to_host(out), 0.0, prior, fprop=False, site=case['name'])


def test_the_separate_launches_are_the_same_host_sequence():
    case = L.CASES[1]
    a, b = L.alloc(case), L.alloc(case)
    L.launch(kernel_ref, case, L.operands(case), a, case['kl_min_between'], case['prior_vector'])
    L.launch_separate(kernel_ref, case, L.operands(case), b, case['kl_min_between'], case['prior_vector'])
    for k in a:
        assert torch.equal(a[k][0], b[k][0]), k


# ------------------------------------------------------------------------------------------------------ the faults fail
def test_the_emulation_without_a_fault_is_the_host_sequence():
    for case in L.CASES:
        for _, kl_min in L.kl_min_settings(case):
            a, b = run(kernel_ref, case, kl_min, case['prior_vector']), run(L.Faulty(None), case, kl_min, case['prior_vector'])
            for k in a:
                assert torch.equal(a[k][0], b[k][0]), (case['name'], k)


@pytest.mark.parametrize('fault', sorted(L.FAULTS))
def test_every_fault_fails_the_check_meant_to_catch_it(fault):
    meant = L.FAULTS[fault]

    def caught():
        for case in L.CASES:
            for pname, prior in L.priors(case):
                for name, kl_min in L.kl_min_settings(case) + (('tie', tie_kl_min(case, L.Faulty(fault))),):
                    host = run(L.Faulty(fault), case, kl_min, prior)
                    if L.verify(case, host, kl_min, prior, raises=False)[meant] > 1.0:
                        return case['name'], pname, name
    assert caught() is not None, 'fault %r passes the check %r on every case, prior form and kl_min setting' % (fault, meant)


def test_the_labeled_slot_fault_also_fails_the_exact_statement():
    case = L.CASES[0]
    host = run(L.Faulty('slot_row_reads_first_slot'), case, 0.0, case['prior_scalar'])
    assert 'kld of labeled rows is the klfp of their slot' in L.selections(case, host, 0.0)


# ------------------------------------------------------------------------------------------- the builder's conditions
@pytest.mark.parametrize('case', L.CASES, ids=IDS[:len(L.CASES)])
def test_case_conditions(case):
    M, Y, K1, K2, Z1, Z3 = case['shape']
    o = L.operands(case)
    assert M % 4 != 0                                               # a workgroup owns 4 rows
    assert sorted(set(case['kind'].tolist())) == [0, 1, 2]         # all three row kinds: fp_ptr is ragged
    nf = (o['fp_ptr'][1:] - o['fp_ptr'][:-1]).long()
    assert bool((nf[case['kind'] == 1] == 1).all()) and bool((nf[case['kind'] != 1] == Y).all())
    assert bool((o['label'][case['kind'] == 2] <= -2).all()) and bool((o['label'][case['kind'] == 1] >= 0).all())
    assert bool((o['label'][case['kind'] == 2] < -2).any())        # a labeled-slot row whose class is not slot 0
    q = o['qidx'].long()
    assert q.numel() == case['F'] and q.unique().numel() < q.numel() and int(q.max()) < o['Q'].shape[0]
    for k in ('a1', 'a2', 'W', 'Q', 'P', 'Q3'):
        assert o[k] is None or o[k].stride(0) > o[k].shape[1]
    for k, (buf, view) in L.alloc(case).items():
        assert buf.numel() > view.numel() and (view.dim() == 1 or view.stride(0) > view.shape[1])
    # both sides of each gate are populated at the setting between the extremes; none / all at the other two
    raw1, raw3 = (f64(v) for v in L._raw_ref(o)[:2])
    assert min(L.side_fractions(raw1, raw3, case['kl_min_between'])) >= 0.25
    assert bool((raw1 > 0).all()) and bool((raw3 > 0).all())
    assert case['kl_min_above'] > float(raw1.max()) and case['kl_min_above'] > float(raw3.max())
    assert L.route(case['shape']) == case['name'].split('-')[0]


def test_the_cases_sit_on_both_sides_of_the_route_boundary():
    routes = {c['shape']: L.route(c['shape']) for c in L.CASES}
    assert routes[(6, 2, 128, 128, 128, 128)] == 'fast'
    for s in ((6, 2, 129, 128, 128, 128), (6, 2, 128, 128, 129, 128), (6, 2, 128, 128, 128, 129)):
        assert routes[s] == 'generic'
    assert sorted(set(routes.values())) == ['fast', 'generic']
    assert {c['name']: L.route(c['shape']) for c in L.EDGE_CASES} == {
        'edge-logvar-fast': 'fast', 'edge-logvar-generic': 'generic', 'edge-clamp-fast': 'fast', 'edge-clamp-generic': 'generic'}


def test_the_edge_grids_reach_both_sides_of_the_clamp_and_the_logvar_range():
    for case in L.EDGE_CASES[2:]:
        p = run(kernel_ref, case, 0.0, case['prior_scalar'])['probs'][1]
        assert bool((p == L.P_MIN).any()) and bool(((p > L.P_MIN) & (p < 1e-9)).any())
        logits = f64(L.operands(case)['a1'])
        p64 = torch.softmax(logits, 1)
        assert bool((p64 < L.P_MIN).any()) and bool(((p64 > L.P_MIN) & (p64 < 1e-8)).any())
    for case in L.EDGE_CASES[:2]:
        o = L.operands(case)
        Z1, Z3 = case['shape'][4:]
        for lv in (o['Q'][:, Z1:], o['P'][:, Z1:], o['Q3'][:, Z3:]):
            assert float(lv.min()) == -30.0 and float(lv.max()) == 30.0
        assert sorted({round(v, 3) for v in (o['Q'][:, :Z1] - o['P'][:, :Z1]).abs().unique().tolist()}) == sorted(L.D_VALUES)
