"""-m gpu: ``Tail.fold_rows`` on the device -- ``dv_z2f_post_bwd`` forming the pairs' KL rows and summing the fprop rows'
d/dz1, ``dv_smalln_linear_fwd`` with its ``dv_clf_dgrad`` rider -- held to the staged float64 reference of
``tests/fold_rows_ref.py``, to the separate launches they replace (bit for bit where the arithmetic is the same) and to the
memory contract; then the folded dual-graph step against the unfolded one.  The worst excess per output is written to
``profiles/r15_fold_rows_checks.txt`` when ``DRVAE_WRITE_CHECKS=1``."""
import os

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import clf_launch_ref as CL
from tests import fold_rows_ref as R
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = os.path.join(ROOT, 'profiles', 'r15_fold_rows_checks.txt')


def _report(title, rows):
    if os.environ.get('DRVAE_WRITE_CHECKS') == '1':
        R.report(CHECKS, title, rows)


# ------------------------------------------------------------------------------------------------ the kernel
def _launch(K, case, dev, **kw):
    o = R.z2f_operands(case, dev)
    out = R.z2f_alloc(case, o, dev)
    R.z2f_launch(K, case, o, out, **kw)
    torch.cuda.synchronize()
    return o, out, R.to_host(out)


@pytest.mark.parametrize('case', R.Z2F_CASES, ids=lambda c: c['name'])
def test_folded_z2f_post_bwd_against_float64_the_separate_launches_and_its_memory_contract(case, dev):
    import drvae_amd.kernels as K
    Z, L, B, Np = case['shape']
    _, _, first = _launch(K, case, dev)
    cases = [('between', case)]
    if Np:       # kl_min at a raw value the kernel computed: rows above, below and exactly at it
        tied = R.with_tie(case, first['raw'][1])
        raw = first['raw'][1]
        assert (raw == tied['kl_min']).any() and (raw > tied['kl_min']).any()
        cases.append(('tie', tied))
    rows = {}
    for tag, c in cases:
        o, out, host = _launch(K, c, dev)
        worst = R.z2f_verify(c, host, raises=False)
        # determinism: a second launch from the same state leaves the same bits, pads included
        _, _, again = _launch(K, c, dev)
        worst['determinism'] = 0.0 if all(torch.equal(host[k][0], again[k][0]) for k in host) else float('inf')
        if Np:
            # the KL rows: bit for bit those of the separate launch
            kl, raw = R.kl_rows_separate(K, c, o, dev)
            torch.cuda.synchronize()
            worst['kl_bits'] = 0.0 if (torch.equal(host['raw'][1], raw.cpu()) and torch.equal(host['kl'][1], kl.cpu())) \
                else float('inf')
        # the unfolded sequence: [kl_rows_fwd ->] smalln_bwd_data-style share (segment sum + dz1b, - dz2f) -> the old form of
        # the launch fed that raw.  dp2 / dq2 bit for bit; dz1 within the bound (here: the same association, so the same bits)
        share = torch.zeros(L * B, Z, device=dev)
        if c['seg']:
            K.rows_segment_sum(share, o['seg_src'], seg_ptr=o['seg_ptr'], beta=0.0, width=Z)
        share = share + o['dz1b'] if c['seg'] else o['dz1b'].clone()
        if c['has_dz2f']:
            share = share - o['dz2f']
        old = R.z2f_alloc(c, o, dev)
        v = {k: b[1] for k, b in old.items()}
        K.z2f_post_bwd(v['dp2'], v['dz1'], v['dq2'][:Np] if Np else None, o['dz2f'], o['pert'][:L * Np] if Np else None,
                       o['slot'], o['eps'], o['p2'], o['q2'][:Np] if Np else None, o['coef'][:L * Np],
                       out['raw'][1][:L * Np], c['kl_min'], share, L, B, Np)
        torch.cuda.synchronize()
        oh = R.to_host(old)
        keys = ('dp2', 'dq2') if Np else ('dp2',)
        worst['grad_bits'] = 0.0 if all(torch.equal(host[k][1], oh[k][1]) for k in keys) else float('inf')
        ref, bnd = R.z2f_reference(c, {k: b[1] for k, b in oh.items() if k != 'raw'} | {'raw': host['raw'][1]})['dz1']
        worst['dz1_vs_unfolded'] = float((R.excess(host['dz1'][1], oh['dz1'][1], 2 * bnd)).max())
        rows['%s %s' % (c['name'], tag)] = worst
        print(c['name'], tag, worst)
    _report('dv_z2f_post_bwd, folded form (worst excess per output, <= 1 passes)', rows)
    for name, worst in rows.items():
        assert max(worst.values()) <= 1.0, (name, worst)


def test_the_old_form_of_z2f_post_bwd_is_unchanged_by_null_fields(dev):
    """both new outputs NULL, no segment source: the launch reads ``raw`` and behaves as before (held to the reference)"""
    import drvae_amd.kernels as K
    for case in (R.Z2F_CASES[4], R.Z2F_CASES[6]):
        c = dict(case, seg=False, has_dz2f=False)
        _, _, folded = _launch(K, c, dev)
        o = R.z2f_operands(c, dev)
        out = R.z2f_alloc(c, o, dev)
        out['raw'][1].copy_(folded['raw'][1].to(dev))
        R.z2f_launch(K, c, o, out, fold_kl=False)
        torch.cuda.synchronize()
        host = R.to_host(out)
        assert (host['kl'][0] == R.SENTINEL).all(), 'kl_out written by the old form'
        for k in ('dp2', 'dq2', 'dz1'):
            assert torch.equal(host[k][0], folded[k][0]), k


# ------------------------------------------------------------------------------------------------- the rider
RIDER_SHAPES = ((9, 2, 6, 6, 6, 4),               # fast route, the goldens' size: K1 + K2 = 12
                (37, 2, 100, 100, 100, 100),      # fast route, K1 + K2 = 200: second lane chunk partly full
                (9, 3, 6, 6, 6, 4),               # N = 3: past the N <= 2 route boundary, the generic kernel
                (21, 3, 100, 100, 100, 37),       # generic, K1 + K2 = 200
                (6, 2, 129, 129, 128, 128))       # N = 2 but past the fast route's width (K1 + K2 = 258 > 256)


@pytest.mark.parametrize('shape', RIDER_SHAPES, ids=lambda s: '%s-%s' % (CL.route(s), 'x'.join(map(str, s))))
def test_classifier_rider_against_float64_and_the_separate_launch(shape, dev):
    import drvae_amd.kernels as K
    case = CL.make_case(shape, seed=5, need_split=False)
    Mr, Y, K1, K2, Z1, Z3 = shape
    o, out = CL.operands(case, dev), CL.alloc(case, dev)
    plain = CL.alloc(case, dev)
    g = torch.Generator().manual_seed(3)
    bufs = [torch.full((Mr + R.PAD_ROWS, n + R.PAD_COLS), R.SENTINEL) for n in (K1, K2)]
    olds = [torch.randn(Mr, n, generator=g) for n in (K1, K2)]
    rows = {}
    for tag, mk in (('w1-w2|w2', lambda d: [(d[0], 0, 1.0, 0.0, K1, -1.0), (d[1], K1, 1.0, 0.0)]),
                    ('beta', lambda d: [(d[0], 0, 0.5, 0.25), (d[1], K1, -2.0, 1.0)])):
        dev_bufs = [b.clone().to(dev) for b in bufs]
        views = [b[:Mr, :n] for b, n in zip(dev_bufs, (K1, K2))]
        for v, od in zip(views, olds):
            v.copy_(od.to(dev))
        dsts = mk(views)
        v = {k: b[1] for k, b in out.items()}
        ym = (v['yl'], v['kld'], v['cfp'], v['dqy'], o['label'], o['fp_ptr'], v['klfp'], case['prior_scalar'], o['c_kld'],
              o['c_yl'])
        kf = dict(Q=o['Q'], qidx=o['qidx'], P=o['P'], Q3=o['Q3'], Z1=Z1, Z3=Z3, kl_min=case['kl_min_between'], raw1=v['raw1'],
                  raw3=v['raw3'], dq=v['dq'], dp=v['dp'])
        K.smalln_fwd(v['probs'], v['logits'], o['a1'], o['W'], o['bias'], o['a2'], ymarg=ym, fprop_kl=kf, dgrad=dsts)
        torch.cuda.synchronize()
        # everything else the launch writes: what it writes without the rider, bit for bit
        CL.launch(K, case, o, plain, case['kl_min_between'], case['prior_scalar'])
        torch.cuda.synchronize()
        worst = {'others': 0.0 if all(torch.equal(out[k][0], plain[k][0]) for k in out) else float('inf')}
        # float64 on the stored dqy / probs
        for t, ((dst, *_), (ref, bnd)) in enumerate(zip(dsts, R.dgrad_reference(v['dqy'], v['probs'], o['W'], dsts, olds))):
            worst['dst%d' % t] = float(R.excess(dst, ref, bnd).max())
        # the separate launch on the DQY the same launch stored: bit for bit
        sep = [od.clone().to(dev) for od in olds]
        K.smalln_bwd_data([(s,) + tuple(d[1:]) for s, d in zip(sep, dsts)], v['dqy'], v['probs'], o['W'])
        torch.cuda.synchronize()
        worst['bits'] = 0.0 if all(torch.equal(s, d[0]) for s, d in zip(sep, dsts)) else float('inf')
        pads = True
        for b, n in zip(dev_bufs, (K1, K2)):
            hb = b.cpu()
            pads &= bool((hb[Mr:] == R.SENTINEL).all()) and bool((hb[:, n:] == R.SENTINEL).all())
        worst['pads'] = 0.0 if pads else float('inf')
        rows['%s %s' % (case['name'], tag)] = worst
        print(case['name'], tag, worst)
    _report('dv_smalln_linear_fwd with dv_clf_dgrad (worst excess per output, <= 1 passes)', rows)
    for name, worst in rows.items():
        assert max(worst.values()) <= 1.0, (name, worst)


# -------------------------------------------------------------------------------------------------- the step
def _engine(spec, params, batch, dev):
    from tests.test_engine_cpu import make_engine, set_batch
    eng, arena = make_engine(spec, params, dev)
    set_batch(eng, batch, dev)
    return eng, arena


def _count_capture(eng, monkeypatch):
    """C-ABI calls of the captured step, counted as ``test_launch_count_of_the_captured_step`` counts them"""
    from drvae_amd import _lib
    counts = {'n': 0, 'on': False}
    real = _lib.check

    def counting(code, what):
        if counts['on'] and not what.startswith('dv_gemm_set_option'):
            counts['n'] += 1
        return real(code, what)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, 'check', counting)
        real_capture_main = eng._capture_main

        def capture_main(*a, **k):
            counts['on'] = True
            return real_capture_main(*a, **k)
        mp.setattr(eng, '_capture_main', capture_main)
        eng.capture()
        counts['on'] = False
    return counts['n']


def _step_case(which):
    if which == 'tiny':          # 12 rows, dim_x = 16
        spec = C.tiny_spec('drvae', dim_x=16)
        return spec, M.init_params(spec, 4, as_numpy=True), M.make_batch(spec, 12, seed=3), None
    spec = M.ModelSpec(kind='drvae', L=2)           # the cfg-2 shape at 150 rows
    return spec, M.init_params(spec, 3, as_numpy=True), M.make_batch(spec, 150, seed=5), (31, 33)


@pytest.mark.parametrize('which', ['tiny', 'cfg2'])
def test_folded_step_against_the_eager_and_the_unfolded_step(which, dev, monkeypatch):
    from tests.test_gpu_x3 import tuned
    spec, params, batch, counts = _step_case(which)
    res = {}
    for tag, tune in (('folded', ''), ('unfolded', 'fold_rows=0')):
        with tuned(tune):
            eng, arena = _engine(spec, params, batch, dev)
            eng.train_step()
            n = _count_capture(eng, monkeypatch)
            assert eng._side_graph is not None and eng._step_tail(False).fold_rows == (tag == 'folded')
            for _ in range(3):
                eng.replay()
            torch.cuda.synchronize()
            eng.check_sync()
            res[tag] = (eng.losses(), arena.param.clone(), n)
    eager, a0 = _engine(spec, params, batch, dev)
    for _ in range(4):
        eager.train_step()
    torch.cuda.synchronize()
    print(which, 'launch calls folded / unfolded:', res['folded'][2], res['unfolded'][2])
    # the captured folded step is, bit for bit, the eager step from the same state (3 replays behind one eager step)
    assert eager.losses() == res['folded'][0] and torch.equal(a0.param, res['folded'][1])
    # ... and agrees with the unfolded captured step at the golden tolerances
    for k, v in res['folded'][0].items():
        np.testing.assert_allclose(v, res['unfolded'][0][k], rtol=1e-4, atol=1e-7, err_msg=k)
    assert float((res['folded'][1] - res['unfolded'][1]).norm() / res['unfolded'][1].norm()) <= 1e-4
    assert res['unfolded'][2] - res['folded'][2] == 2
    if counts is not None:
        assert res['folded'][2] <= counts[0] and res['unfolded'][2] == counts[1], res


def test_sampler_feed_on_bucketed_plans_folded_equals_unfolded(dev):
    """the sampler-feed step with bucketed plans (pairs first, one captured plan per number-of-pairs bucket): 8 batches,
    finite, folded against ``fold_rows=0`` at the golden tolerances"""
    from drvae_amd import data as D
    from tests.test_engine_cpu import make_engine
    from tests.test_gpu_x3 import tuned
    spec = M.ModelSpec(kind='drvae', L=2)
    params = M.init_params(spec, 3, as_numpy=True)
    big = M.make_batch(spec, 640, seed=9)
    t = lambda k: torch.from_numpy(big[k].copy())         # noqa: E731
    res = {}
    for tag, tune in (('folded', ''), ('unfolded', 'fold_rows=0')):
        with tuned(tune):
            ds = D.DrVAEDataset(t('x1'), t('x2'), t('s'), t('y'), t('has_x2'), t('has_y')).to(dev)
            bat = D.DeviceBatcher(ds, D.compute_balanced_weights(np.arange(640) % 7), 64, seed=5, mode='sampler', pair_bucket=4)
            fed, arena = make_engine(spec, params, dev)
            bat.bind(fed)
            bat.begin_epoch(n_batches=8)
            bat.prepare_epoch(lambda e: e.capture())
            keys = set()
            for k in range(8):
                bat.select(k)
                keys.add(fed.plan.key)
                fed.replay()
            torch.cuda.synchronize()
            fed.check_sync()
            res[tag] = (fed.losses(), arena.param.clone(), keys)
    assert len(res['folded'][2]) > 1 and res['folded'][2] == res['unfolded'][2]
    assert all(np.isfinite(v) for v in res['folded'][0].values()) and bool(torch.isfinite(res['folded'][1]).all())
    for k, v in res['folded'][0].items():
        np.testing.assert_allclose(v, res['unfolded'][0][k], rtol=1e-4, atol=1e-7, err_msg=k)
    assert float((res['folded'][1] - res['unfolded'][1]).norm() / res['unfolded'][1].norm()) <= 1e-4
