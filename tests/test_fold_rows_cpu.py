"""CPU: ``Tail.fold_rows`` -- the pairs' KL rows formed by ``z2f_post_bwd``, the classifier's data gradient by its forward
launch.  (1) the checks of ``tests/fold_rows_ref.py`` hold the fp32 stand-ins of the folded launches and catch faulty
emulations of them; (2) on the stand-ins of ``tests/kernel_ref.py`` the folded dual-graph step, RUN in an order its
device flags allow, leaves what the unfolded step leaves; its recorded chains pass the checks of the FLAGS / SITES table;
(3) with ``fold_rows=0`` the recorded step is the one recorded in
front of this schedule, argument for argument (``tests/golden/fold_rows_trace.json``)."""
import json

import numpy as np
import pytest
import torch

from tests import clf_launch_ref as CL
from tests import fold_rows_ref as R
from tests import fold_trace as FT
from tests import kernel_ref


# ------------------------------------------------------------------------------------------- (1) the checks
def _run(mod, case):
    o = R.z2f_operands(case)
    out = R.z2f_alloc(case, o)
    R.z2f_launch(mod, case, o, out)
    return o, R.to_host(out)


def _tied(case):
    """the case with kl_min at a raw value the stand-in computes: above, below and a tie"""
    if not case['shape'][3]:
        return case
    _, host = _run(kernel_ref, case)
    tied = R.with_tie(case, host['raw'][1])
    raw = host['raw'][1]
    assert (raw == tied['kl_min']).any() and (raw > tied['kl_min']).any()
    assert (raw < tied['kl_min']).any() or raw.numel() < 3
    return tied


def _kl_bits(case, o, host):
    """0 where raw / kl equal the separate launch bit for bit, inf otherwise"""
    Z, L, B, Np = case['shape']
    if not Np:
        return 0.0
    kl, raw = R.kl_rows_separate(kernel_ref, case, o)
    return 0.0 if (torch.equal(host['raw'][1], raw) and torch.equal(host['kl'][1], kl)) else float('inf')


@pytest.mark.parametrize('case', R.Z2F_CASES, ids=lambda c: c['name'])
def test_the_stand_in_of_the_folded_launch_passes_every_check(case):
    for c in (case, _tied(case)):
        o, host = _run(kernel_ref, c)
        worst = R.z2f_verify(c, host, site=c['name'])
        assert max(worst.values()) <= 1.0 and _kl_bits(c, o, host) == 0.0
        # ... and the faultless emulation is bitwise the stand-in
        _, again = _run(R.FaultyZ2F(None), c)
        for k in host:
            assert torch.equal(host[k][0], again[k][0]), (c['name'], k)


@pytest.mark.parametrize('fault', sorted(R.Z2F_FAULTS))
def test_a_faulty_emulation_fails_the_check_meant_for_it(fault):
    caught = 0
    for case in R.Z2F_CASES:
        Z, L, B, Np = case['shape']
        if not Np or not case['seg'] or Z < 64:
            continue
        c = _tied(case)
        o, host = _run(R.FaultyZ2F(fault), c)
        worst = R.z2f_verify(c, host, raises=False)
        worst['kl_bits'] = _kl_bits(c, o, host)
        assert worst[R.Z2F_FAULTS[fault]] > 1.0, (fault, case['name'], worst)
        caught += 1
    assert caught >= 4


@pytest.mark.parametrize('shape', [(9, 2, 5, 5, 5, 4), (21, 3, 100, 100, 100, 37)], ids=['N2-K10', 'N3-K200'])
def test_the_classifier_rider_s_stand_in_is_within_the_float64_bound(shape):
    case = CL.make_case(shape, seed=3)
    M, Y, K1, K2, Z1, Z3 = shape
    o, out = CL.operands(case), CL.alloc(case)
    v = {k: b[1] for k, b in out.items()}
    ym = (v['yl'], v['kld'], v['cfp'], v['dqy'], o['label'], o['fp_ptr'], v['klfp'], case['prior_scalar'], o['c_kld'], o['c_yl'])
    kf = dict(Q=o['Q'], qidx=o['qidx'], P=o['P'], Q3=o['Q3'], Z1=Z1, Z3=Z3, kl_min=case['kl_min_between'], raw1=v['raw1'],
              raw3=v['raw3'], dq=v['dq'], dp=v['dp'])
    d0, d1 = torch.randn(M, K1), torch.randn(M, K2)
    old = [d0.clone(), d1.clone()]
    dsts = [(d0, 0, 1.0, 0.5, K1, -1.0), (d1, K1, 1.0, 0.0)]
    kernel_ref.smalln_fwd(v['probs'], v['logits'], o['a1'], o['W'], o['bias'], o['a2'], ymarg=ym, fprop_kl=kf, dgrad=dsts)
    for (dst, *_), (ref, bnd) in zip(dsts, R.dgrad_reference(v['dqy'], v['probs'], o['W'], dsts, old)):
        assert float(R.excess(dst, ref, bnd).max()) <= 1.0
    # ... and a rider that forgets the second column block is not
    d0b = old[0].clone()
    kernel_ref.smalln_bwd_data([(d0b, 0, 1.0, 0.5)], v['dqy'], v['probs'], o['W'])
    ref, bnd = R.dgrad_reference(v['dqy'], v['probs'], o['W'], dsts, old)[0]
    assert float(R.excess(d0b, ref, bnd).max()) > 1.0


# ------------------------------------------------------------------------------------------- (2) the step
def _tail(eng, monkeypatch, fold):
    import drvae_amd.tuning as T
    if fold:
        monkeypatch.delenv('DRVAE_TUNE', raising=False)
    else:
        monkeypatch.setenv('DRVAE_TUNE', 'fold_rows=0')
    monkeypatch.setattr(T, '_VALUES', None)
    tail = eng._step_tail(False, on_gpu=True)
    monkeypatch.setattr(T, '_VALUES', None)
    return tail


def _three_steps(name, universal, fold, monkeypatch):
    eng, arena, case = FT.make(name, universal, kernel_ref.install, monkeypatch)
    tail = _tail(eng, monkeypatch, fold)
    assert tail.dual and tail.fold_rows == fold
    losses, recs = [], []
    for _ in range(3):
        recs.append(FT.step(eng, tail, kernel_ref.FUNCTIONS))
        losses.append(dict(eng.losses()))
    assert int(eng.sync_err[0::2].abs().sum()) == 0, 'a wait of the step found its flag unpublished'
    return eng, arena.param.clone(), losses, recs


@pytest.mark.parametrize('name,universal', [('tiny_drvae', False), ('tiny_drvae', True), ('tiny_drvae_prior', False)])
def test_the_folded_step_leaves_what_the_unfolded_step_leaves(name, universal, monkeypatch):
    _, p1, l1, r1 = _three_steps(name, universal, True, monkeypatch)
    assert kernel_ref.CALLS['folded_kl'] == 3 and kernel_ref.CALLS['folded_dgrad'] == 3
    _, p0, l0, r0 = _three_steps(name, universal, False, monkeypatch)
    assert kernel_ref.CALLS['folded_kl'] == 0 and kernel_ref.CALLS['folded_dgrad'] == 0
    for a, b in zip(l1, l0):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=1e-7, err_msg=k)
    assert float((p1 - p0).norm() / p0.norm()) <= 1e-4
    # two launches less, one on either chain's stretch in front of the join
    n1, n0 = [n for _, n in r1[-1].order], [n for _, n in r0[-1].order]
    assert len(n0) - len(n1) == 2
    assert n0.count('kl_rows_fwd') - n1.count('kl_rows_fwd') == 1 and 'smalln_bwd_data' in n0 and 'smalln_bwd_data' not in n1


@pytest.mark.parametrize('universal', [False, True])
def test_the_folded_chains_pass_the_checks_of_the_flag_table(universal, monkeypatch):
    """the statements of ``tests/test_step_sync.py`` (its ``Recorder``, reused) on the folded step's recorded chains, and where
    the loss scalars now run: behind the side tail's wait for flag ``noise``"""
    import drvae_amd.kernels as K
    from drvae_amd.schedule import FLAGS, SITES
    from tests.test_step_sync import OTHER, Recorder
    eng, _, case = FT.make('tiny_drvae', universal, kernel_ref.install, monkeypatch)
    eng.set_noise(case['noises'][0])
    tail = _tail(eng, monkeypatch, True)
    assert tail.fold_rows
    with pytest.MonkeyPatch.context() as inner:
        rec = Recorder(eng, K, inner)
        with eng._recording('main', tail):
            rec.begin('main')
            eng._launch_sequence()
        with eng._recording('side', tail):
            rec.begin('side')
            eng._launch_sequence(draw=False, optimizer=False)
    owner, sites = {f[0]: f[1] for f in FLAGS}, {s[0]: s for s in SITES}
    assert rec.waits
    for chain, launcher, flag, value, site in rec.waits:
        met = [p for p in rec.pubs if p[0] == OTHER[chain] and p[2] == flag]
        assert len(met) == 1 and met[0][3] - (1 if site == 'next_step' else 0) == value, (chain, launcher, flag, site, met)
        assert sites[site][1] == chain and flag in sites[site][2]
    for chain, launcher, flag, value in rec.pubs:
        assert owner[flag] == chain
    assert len({(p[0], p[2]) for p in rec.pubs}) == len(rec.pubs)
    assert {p[2] for p in rec.pubs} - {w[2] for w in rec.waits} <= {f[0] for f in FLAGS if f[2]}
    side = [n for c, n in rec.launches if c == 'side']
    noise_wait = [i for i, w in enumerate(rec.waits) if w[0] == 'side' and w[4] == 'noise']
    assert len(noise_wait) == 1
    # the side chain's launches in order: ... flag_wait(rows), adam, flag_wait(noise), loss_assemble, the draw, the counters
    assert side[-5:] == ['adam_l2', 'flag_wait', 'loss_assemble', 'fill_normal_rows', 'counters_add2'], side[-6:]
    assert [t for c, t in rec.loss_terms if c == 'side' and t] and 'KLZ2' in [t for c, t in rec.loss_terms if c == 'side'][0]
    assert 'kl_rows_fwd' not in [n for c, n in rec.launches if c == 'main']
    assert 'smalln_bwd_data' not in side


# ---------------------------------------------------------------------------------- (3) the unfolded forms stay
@pytest.fixture(scope='module')
def golden():
    with open(FT.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('name,universal', FT.CASES)
def test_fold_rows_0_records_the_old_sequence(name, universal, golden, monkeypatch):
    monkeypatch.setenv('DRVAE_TUNE', 'fold_rows=0')
    got = FT.default_trace(name, universal)
    assert got == golden['%s/%s' % (name, 'universal' if universal else 'structure')]


def test_only_the_schedules_the_fold_is_for_take_it(monkeypatch):
    """on: the single-process dual-graph train step of a DrVAE with the single-Linear classifier on [z1, z2Fz1 - z1]; off:
    exchange forms, the clipped step, plans with dropout sites, VFAE / PVAE, a regression head, a hidden classifier layer"""
    import drvae_amd.tuning as T
    from tests.golden import cases as C
    from tests.test_clip_cpu import make_engine as clip_engine
    from tests.test_dropout_cpu import make_engine as drop_engine
    from tests.test_engine_cpu import set_batch
    from oracle import models_ref as M
    kernel_ref.install(monkeypatch)
    monkeypatch.delenv('DRVAE_TUNE', raising=False)
    monkeypatch.setattr(T, '_VALUES', None)
    seen = {}
    for name in C.SMALL_MODEL_CASES:
        eng, _, case = FT.make(name, False, kernel_ref.install, monkeypatch)
        for split in (False, True, 'captured', 'overlap'):
            t = eng._step_tail(split, on_gpu=True)
            cfg = eng.cfg
            want = bool(split is False and cfg.kind == 'drvae' and not cfg.cont and eng.clf_small and cfg.clf_z1z2
                        and t.dual and t.fold_join and t.side_loss and t.noise_ahead)
            assert t.fold_rows == want, (name, split, t)
            seen[(name, split)] = t.fold_rows
    assert seen[('tiny_drvae', False)] and not seen[('tiny_drvae', True)]
    assert not any(v for (n, s), v in seen.items() if 'vfae' in n or 'pvae' in n or '1sig' in n or 'nolp' in n)
    case = C.model_case('tiny_drvae')
    params = M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    for eng in (clip_engine(case['spec'], params, max_grad_norm=1.0)[0], drop_engine(case['spec'], params, rate=0.25)[0]):
        set_batch(eng, case['batch'])
        assert not eng._step_tail(False, on_gpu=True).fold_rows
    monkeypatch.setattr(T, '_VALUES', None)
