"""GPU: raw-count inputs (``x_transform='log1p'``, ``library_size=True``) on the real kernels -- the split form of
``dv_batch_feed`` against float64 with its memory contract and refusals, the library-scaled kinds of ``dv_rec_nll_rows`` against
float64 within the bound of ``tests/counts_ref.py``, the fused step against the model-level float64 reference (eager, captured,
host-fed against the graph-resident feed) and ``fit`` on overdispersed counts of varying depth."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests import counts_ref as CR
from tests import nb_ref as R
from tests import ref64
from tests.test_counts_cpu import (COMBINED, SWITCHES, _counts_dataset, combined_against_reference, host_fed_equals_feed,
                                   run_against_reference)

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GPU_TOL = ((1e-4, 2e-5), None, (2e-4, 5e-5))      # losses / (gradients: not compared) / parameters: tests/test_gpu_nb.py's


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert _lib.REC_KIND['poisson_lib'] == 3 and _lib.REC_KIND['nb_lib'] == 4
    return K


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def _banded(rows, X, ld, dev):
    """a (rows, X) view one row and one float-quadruple inside a sentinel-filled buffer: (view, whole buffer)"""
    big = torch.full((rows + 2, ld), SENTINEL, device=dev)
    return big[1:rows + 1, :X], big


def _band_intact(big, rows, X):
    b = host(big)
    return bool((b[0] == SENTINEL).all() and (b[rows + 1] == SENTINEL).all() and (b[1:rows + 1, X:] == SENTINEL).all())


# -------------------------------------------------------------------------------------------- 1. the feed
@pytest.mark.parametrize('noisy', [False, True], ids=['plain', 'noise'])
@pytest.mark.parametrize('X', [6, 1030])
def test_split_feed_against_float64(K, dev, X, noisy):
    """X = 6: the scalar path; 1030: the 16-byte path into its second round of 256 groups, with a tail of 2"""
    B, Np, nb, N = 5, 3, 3, 11
    rs = np.random.RandomState(X)
    ld_src = X if X == 6 else X + 2                       # (1032: rows allow 16-byte access)
    src1, src2 = (torch.zeros(N, ld_src, device=dev)[:, :X] for _ in range(2))
    src1.copy_(torch.from_numpy(rs.poisson(rs.gamma(2.0, 40.0, (N, X))).astype(np.float32)))
    src2.copy_(torch.from_numpy(rs.poisson(rs.gamma(2.0, 60.0, (N, X))).astype(np.float32)))
    src1[0, :2] = torch.tensor([0.0, 30000.0])
    table = torch.from_numpy(np.stack([rs.permutation(N)[:B] for _ in range(nb)]).astype(np.int32)).to(dev)
    pair_rows = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    noise = torch.randn(B + Np, X + 2, device=dev)[:, :X] if noisy else None
    sigma = 0.01
    base = torch.tensor([10], dtype=torch.int32, device=dev)
    ld = X + 2
    for ctr_v, b in ((10, 0), (11, 1), (57, 2)):          # the first, a middle and the clamped-last batch
        ctr = torch.tensor([ctr_v], dtype=torch.int32, device=dev)
        tb = table[b].long()
        rows = torch.cat([src1[tb], src2[tb[pair_rows.long()]]])
        for transform in ('log1p', None):
            (xin, xin_big), (xt, xt_big) = _banded(B + Np, X, ld, dev), _banded(B + Np, X, ld, dev)
            K.batch_feed(xin, src1, src2, None, table, nb, ctr, base, pair_rows=pair_rows, noise=noise, sigma=sigma, xt=xt,
                         transform=transform)
            want_t, want, bnd = CR.feed_reference(host(rows), noise=host(noise) if noisy else None, sigma=sigma, transform=transform)
            assert torch.equal(host(xt), want_t), 'xt is the source row, bit for bit'
            e = float(ref64.excess(host(xin), want, bnd).max())
            print('split feed X=%d b=%d transform=%s noise=%s: worst |err| / bound %.3g' % (X, b, transform, noisy, e))
            assert e <= 1
            assert _band_intact(xin_big, B + Np, X) and _band_intact(xt_big, B + Np, X)
            if transform is None:
                plain_view, plain_big = _banded(B + Np, X, ld, dev)
                K.batch_feed(plain_view, src1, src2, None, table, nb, ctr, base, pair_rows=pair_rows, noise=noise, sigma=sigma)
                gathered = torch.empty(B + Np, X, device=dev)
                K.rows_gather(gathered, rows.contiguous(), None, noise=noise, sigma=sigma)
                # xt == NULL: the launch as it is today (== the explicit path's gather of the same rows); and the split
                # form without a transform writes the same encoder rows
                assert torch.equal(host(plain_view), host(gathered)) and torch.equal(host(xin), host(plain_view))
                assert _band_intact(plain_big, B + Np, X)


def test_split_feed_refusals(K, dev, monkeypatch):
    B, X = 4, 8
    x1 = torch.ones(6, X, device=dev)
    table = torch.arange(B, dtype=torch.int32, device=dev)[None, :]
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    xin, xt = torch.zeros(B, X, device=dev), torch.full((B, X), SENTINEL, device=dev)
    monkeypatch.setitem(K.FEED_TRANSFORM, 'bad', 2)
    with pytest.raises(RuntimeError, match='dv_batch_feed'):
        K.batch_feed(xin, x1, None, None, table, 1, z, z, xt=xt, transform='bad')
    with pytest.raises(RuntimeError, match='dv_batch_feed'):
        K.batch_feed(xin, x1, None, None, table, 1, z, z, transform='log1p')            # a transform without targets
    off = torch.full((B * X + 4,), SENTINEL, device=dev)[1:1 + B * X].view(B, X)       # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match='dv_batch_feed'):
        K.batch_feed(xin, x1, None, None, table, 1, z, z, xt=off, transform='log1p')
    assert bool((host(xt) == SENTINEL).all()) and bool((host(off) == SENTINEL).all()) and bool((host(xin) == 0).all())
    K.batch_feed(xin, x1, None, None, table, 1, z, z, xt=xt, transform='log1p')
    assert torch.equal(host(xt), torch.ones(B, X)) and torch.equal(host(xin), torch.full((B, X), float(np.log1p(np.float32(1)))))


# -------------------------------------------------------------------------------------------- 2. the rows
def _targets(X, rs):
    """three target rows: all zero (s = 1/X); total exactly X (s = 1); counts to 30000 with a total just under 2^24 where X
    allows it (559 entries of 30000 and the remainder spread: above that the row sum would leave fp32's exact integers)"""
    x = np.zeros((3, X), np.float32)
    x[1] = 1.0
    n = min(X, 559)
    x[2, :n] = 30000.0
    if X > 560:
        x[2, n] = 2 ** 24 - 1 - 30000.0 * n - (X - n - 1)
        x[2, n + 1:] = 1.0
        assert x[2].astype(np.float64).sum() == 2 ** 24 - 1
    return x


@pytest.mark.parametrize('kind', ['poisson', 'nb'])
@pytest.mark.parametrize('X', [5, 8, 1027, 1028])
def test_library_rows_against_float64(K, dev, X, kind):
    """M = 7 decoder rows over 3 target rows through a permuted, repeating xidx; X: scalar and 16-byte paths (nb), each once
    within one 256-thread pass and once beyond it"""
    rs = np.random.RandomState(X)
    Mr = 7
    x = torch.from_numpy(_targets(X, rs))
    xidx = torch.tensor([2, 0, 1, 1, 2, 0, 2], dtype=torch.int32)
    W = 2 * X if kind == 'nb' else X
    a = torch.from_numpy(rs.uniform(-4, 6, (Mr, W)))
    v = F.softplus(a).float()
    v[:, :X] += np.float32(R.MU_SHIFT)
    if kind == 'nb':
        v[:, X:] += np.float32(R.THETA_SHIFT)
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25, 1.5, -1.0, 0.75])
    xs = x[xidx.long()]
    ref = CR.reference(kind, xs, v[:, :X], v[:, X:] if kind == 'nb' else None, coef=coef)
    s = CR.size_factor32(xs)
    assert s[1] == np.float32(1.0 / X) and s[2] == 1.0
    xd, vd, id_, cd = x.to(dev), v.to(dev), xidx.to(dev), coef.to(dev)
    ldd = W + 4
    outs = []
    for rep in range(2):
        out_big = torch.full((Mr + 2,), SENTINEL, device=dev)
        dpre, dpre_big = _banded(Mr, W, ldd, dev)
        K.rec_nll_rows(out_big[1:Mr + 1], xd, vd, kind=kind, shift=R.MU_SHIFT, xidx=id_, coef=cd, dpre=dpre, library=True)
        outs.append((host(out_big), host(dpre).clone()))
        assert _band_intact(dpre_big, Mr, W), 'nothing beyond %d columns' % W
        assert float(outs[-1][0][0]) == SENTINEL and float(outs[-1][0][-1]) == SENTINEL
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'run to run'
    got, gd = outs[0][0][1:Mr + 1], outs[0][1]
    worst = [float(ref64.excess(got, ref['rows'], ref['rows_bound']).max()),
             float(ref64.excess(gd[:, :X], ref['gm'], ref['gm_bound']).max())]
    if kind == 'nb':
        worst.append(float(ref64.excess(gd[:, X:], ref['gt'], ref['gt_bound']).max()))
    print('library rows %s X=%d, worst |err| / bound: %s' % (kind, X, '  '.join('%.3g' % w for w in worst)))
    ref64.check('rec_nll_rows (%s, library) rows' % kind, got, ref['rows'], ref['rows_bound'])
    ref64.check('rec_nll_rows (%s, library) d/da_m' % kind, gd[:, :X], ref['gm'], ref['gm_bound'])
    if kind == 'nb':
        ref64.check('rec_nll_rows (nb, library) d/da_t', gd[:, X:], ref['gt'], ref['gt_bound'])
    # s = 1 (the rows whose target's total is X): the unscaled kind's output, bit for bit
    out1, dpre1 = torch.empty(Mr, device=dev), torch.empty(Mr, W, device=dev)
    K.rec_nll_rows(out1, xd, vd, kind=kind, shift=R.MU_SHIFT, xidx=id_, coef=cd, dpre=dpre1)
    one = (xidx == 1)
    assert int(one.sum()) == 2 and torch.equal(host(out1)[one], got[one]) and torch.equal(host(dpre1)[one], gd[one])
    assert not torch.equal(host(out1)[~one], got[~one])
    # without coef: the rows alone, dpre untouched
    out2 = torch.empty(Mr, device=dev)
    dpre2, dpre2_big = _banded(Mr, W, ldd, dev)
    K.rec_nll_rows(out2, xd, vd, kind=kind, shift=R.MU_SHIFT, xidx=id_, dpre=dpre2, library=True)
    assert torch.equal(host(out2), got) and bool((host(dpre2_big) == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- 3. the step
def _eager_equals_captured(kind, variant, dev):
    from oracle import models_ref as M
    from tests.test_counts_cpu import _case, _use_s_case
    from tests.test_nb_cpu import make_engine, set_batch
    spec, batch = _use_s_case(kind) if variant == 'use_s' else _case(kind)
    ref = R.ModelRef(spec, seed=9)
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb', **SWITCHES['both'])
        eng.universal = variant == 'universal'
        set_batch(eng, batch, dev)
        eng.train_step()
        losses = [eng.losses()]
        for _ in range(2):
            if captured:
                if eng._graph_key is None:
                    eng.capture()
                eng.replay()
            else:
                eng.train_step()
            losses.append(eng.losses())
        torch.cuda.synchronize()
        out.append(([getattr(arena, w).clone() for w in ('param', 'exp_avg', 'exp_avg_sq')], losses))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0])) and out[0][1] == out[1][1]
    assert all(np.isfinite(v) for l in out[0][1] for v in l.values())


@pytest.mark.parametrize('kind,variant', [('drvae', 'plain'), ('vfae', 'use_s'), ('pvae', 'universal')])
def test_fused_step_matches_the_float64_model_reference(kind, variant, dev):
    """both switches, input noise on: three Adam steps against the model-level float64 reference, then eager == captured"""
    eng = run_against_reference(kind, variant, 'both', dev, tol=GPU_TOL)
    assert eng._route().nll == 'rec'
    _eager_equals_captured(kind, variant, dev)


@pytest.mark.parametrize('kind,use_s', [('drvae', False), ('pvae', False), ('vfae', True)], ids=['drvae', 'pvae', 'vfae-use_s'])
@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
def test_host_fed_step_equals_the_graph_resident_feed(kind, use_s, captured, dev):
    """(the sampler feed binds the batch-independent plan: every case, the PVAE's too, runs on it; the VFAE conditions on the
    nuisance variable, its classes carried by the masked sampler feed)"""
    host_fed_equals_feed(kind, dev, captured=captured, use_s=use_s)


def test_combined_riders_match_the_float64_model_reference(dev):
    """dropout (column masks), clipping, KL annealing and the parameter average together with both switches: losses, parameters
    and averaged parameters against ``counts_ref.RidersRef`` at the tolerances of the plain comparison"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        combined_against_reference(dev, tol=GPU_TOL)


def test_combined_riders_host_fed_equals_feed(dev):
    """dropout, clipping, KL annealing and the parameter average with both switches, through the captured feed step"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        host_fed_equals_feed('drvae', dev, extra=COMBINED, captured=True)


# --------------------------------------------------------------------------------------------------- 4. fit
# depths log-uniform over two decades, 10^-1.5 .. 10^0.5 times gene means of 1 .. 4 (counts to ~80, some all-zero rows).  The
# position of the two decades is chosen so that the PLAIN model trains at all: with depths 1 .. 100 (counts to 2000) and with
# 0.1 .. 10 (counts to 230) the plain 'nb' model's encoder, reading the raw counts, is at NaN within the 12 steps on the CPU
# stand-ins and on the GPU alike -- there is then no likelihood to compare with.  On the stand-ins (12 steps, same sizes) this
# range gives -19.74 (log1p + library size) against -26.76 (plain): the plain model alone does not win
DEPTH_DECADES, DEPTH_LO = 2.0, -1.5


def test_fit_on_counts_of_varying_depth_beats_the_plain_nb_model(dev, tmp_path):
    """``fit`` for 3 epochs on 64 rows of Gamma-Poisson counts (theta = 2) whose depths are log-uniform over two decades (``DEPTH_LO``): the
    'nb' model with x_transform='log1p', library_size=True ends at a strictly higher held-out log-likelihood per row than the
    plain 'nb' model on the same data and seed"""
    from drvae_amd import data as D
    from tests.test_fit import _loader
    from tests.test_gpu_nb import _model
    tr, va = _counts_dataset('drvae', 64, 1, dev, DEPTH_DECADES, DEPTH_LO), _counts_dataset('drvae', 32, 2, dev, DEPTH_DECADES, DEPTH_LO)
    w = D.compute_balanced_weights(np.arange(64) % 5)
    ll = {}
    for tag, sw in (('counts', SWITCHES['both']), ('plain', {})):
        model = _model('drvae', 'nb', dev, epochs=3, **sw)
        bat = D.DeviceBatcher(tr, w, 16, seed=3)
        model.fit(bat, _loader(va, 8), add_noise=False, verbose=False, early_stop=False, model_filename=str(tmp_path / 'b.pth'))
        assert model.finished_training_iters == 3 * 4
        perf, _ = model.evaluate_performance_on_dataset(va)
        assert np.isfinite(float(perf['losses']['ELBO']))
        res = model.forward(va.x1)
        ll[tag] = float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean())
        assert perf['x1_ll'] == pytest.approx(ll[tag], rel=1e-5)      # (the step-by-step evaluation reports it, at the scaled mean)
    print('held-out mean log-likelihood per row: log1p + library size %.4f  plain nb %.4f' % (ll['counts'], ll['plain']))
    assert np.isfinite(ll['counts']) and np.isfinite(ll['plain']) and ll['counts'] > ll['plain']
    # the regime the switches are for: depths 1 .. 100, counts in the thousands (where the plain model's encoder is at NaN within
    # these 12 steps) -- the model with both switches trains and stays finite
    tr, va = _counts_dataset('drvae', 64, 1, dev, DEPTH_DECADES, 0.0), _counts_dataset('drvae', 32, 2, dev, DEPTH_DECADES, 0.0)
    assert float(tr.x1.max()) > 1000
    model = _model('drvae', 'nb', dev, epochs=3, **SWITCHES['both'])
    model.fit(D.DeviceBatcher(tr, w, 16, seed=3), _loader(va, 8), add_noise=False, verbose=False, early_stop=False,
              model_filename=str(tmp_path / 'd.pth'))
    perf, _ = model.evaluate_performance_on_dataset(va)
    deep = float(model.decoder_x.logp_perx(va.x1, *model.forward(va.x1)['px1']).mean())
    print('depths 1 .. 100: held-out mean log-likelihood per row, log1p + library size %.4f' % deep)
    assert np.isfinite(deep) and np.isfinite(float(perf['losses']['ELBO'])) and bool(torch.isfinite(model.engine().arena.param).all())


# ----------------------------------------------------------------------------- 5. two ranks on one GPU
def _dp_case(dev):
    from drvae_amd import data as D
    from tests.test_gpu_nb import _model
    model = _model('drvae', 'nb', dev, epochs=2, **SWITCHES['both'])
    model.add_noise_var = 0.01
    ds = _counts_dataset('drvae', 128, 3, dev, DEPTH_DECADES, DEPTH_LO)
    return model, ds, D.compute_balanced_weights(np.arange(128) % 7)


def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK='0', DRVAE_DIST_BACKEND='gloo', DRVAE_SIDE_CUS='64')
        import torch.distributed as dist
        from tests.test_gpu_dp import _fit_epochs
        torch.cuda.set_device(0)
        dev = torch.device('cuda', 0)
        model, ds, w = _dp_case(dev)
        assert model.enable_data_parallel() == (rank, world)
        means, tabs, bat = _fit_epochs(model, ds, w, 32 // world, {})
        eng = model.engine()
        torch.cuda.synchronize()
        eng.check_sync()
        assert len(eng._graphs) == 2 and eng.plan.XT is not None       # split graphs around the exchange, split mode
        q.put((rank, dict(means=means, tabs=tabs, param=eng.arena.param.cpu().numpy(), iters=model.finished_training_iters)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_on_one_gpu_equal_one_rank(dev):
    """``enable_data_parallel()`` + the device epochs of ``fit`` on the sampler feed with both switches: two ranks (one GPU, gloo)
    with 16 rows each, through captured split graphs around one exchange, train like one process on 32-row batches of the same
    table -- the comparison and tolerances of ``tests/test_gpu_dp.py::test_fit_epochs_sampler_feed_two_ranks_equal_one_rank``"""
    from tests.test_gpu_dp import _fit_epochs
    model, ds, w = _dp_case(dev)
    means, tabs, _ = _fit_epochs(model, ds, w, 32, {})
    torch.cuda.synchronize()
    single = model.engine().arena.param.cpu().numpy()
    assert np.isfinite(single).all() and np.isfinite(means).all()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    from tests.test_dp_gloo import _free_port
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])      # (each child under its own time limit)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    for r, o in got:
        assert isinstance(o, dict), o
    r0, r1 = got[0][1], got[1][1]
    for ep in range(2):
        np.testing.assert_array_equal(np.concatenate([r0['tabs'][ep], r1['tabs'][ep]], 1), tabs[ep])
    assert r0['iters'] == r1['iters'] == model.finished_training_iters == 2 * (128 // 32)
    for r in (r0, r1):
        np.testing.assert_allclose(r['means'], means, rtol=1e-4)
        err = np.linalg.norm(r['param'] - single) / np.linalg.norm(single)
        assert err < 1e-4, err
    np.testing.assert_array_equal(r0['param'], r1['param'])
