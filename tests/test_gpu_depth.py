"""GPU: the depth-normalised encoder input (``x_transform='log1p_norm'``) on the real kernels -- ``dv_batch_feed`` with
``transform`` == 3 against float64 within the bound of ``tests/depth_ref.py`` with its memory contract and refusals (every width
at which the kernel changes path, both access paths, rows sharing a workgroup), the fused step against the model-level float64
reference (eager, captured, host-fed against the graph-resident feed), the captured whole-set evaluation and ``fit`` on
overdispersed counts of varying depth."""
import warnings

import numpy as np
import pytest
import torch

from tests import depth_ref as DR
from tests import ref64
from tests.test_counts_cpu import _counts_dataset
from tests.test_depth_cpu import NORM, combined_against_reference, host_fed_equals_feed, run_against_reference
from tests.test_gpu_counts import DEPTH_DECADES, DEPTH_LO, GPU_TOL, SENTINEL, _band_intact, _banded, host

pytestmark = pytest.mark.gpu

XS = (1, 3, 4, 5, 255, 256, 978, 1020, 1024, 1028, 2052)      # 1024: one outer iteration of a wave; 1028, 2052: two walks + a tail
SIZES = ((1, 0), (2, 2), (3, 2), (5, 4))                      # (B, Np): 1, 4, 5 and 9 rows -- four rows share a workgroup
N_SRC = 7
SIGMA = 0.01


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert K.FEED_TRANSFORM[NORM] == 3
    return K


def _counts(X, seed):
    """N_SRC rows of integer counts, totals below 2^22 (four times a row still sums exactly): row 0 all zero, row 1 all ones
    (total X: s = 1), row 2 a single 1, row 3 holding a 30000 and a 0, the rest Gamma-Poisson of mean 80"""
    rs = np.random.RandomState(seed)
    x = rs.poisson(rs.gamma(2.0, 40.0, (N_SRC, X))).astype(np.float32)
    x[0] = 0
    x[1] = 1
    x[2] = 0
    x[2, X // 2] = 1
    x[3, 0] = 30000
    x[3, X - 1] = 0 if X > 1 else 30000
    assert x.astype(np.float64).sum(1).max() < 2 ** 22
    return x


def _source(x, path, dev):
    """``x`` on the device as the launch's source -- 'vec': 16-byte aligned with a stride of whole 16-byte groups; 'offset': the
    base 4 bytes off a 16-byte boundary; 'stride': an odd row stride (both force the scalar path)"""
    n, X = x.shape
    if path == 'stride':
        ld = X + (2 if X % 2 else 1)
        assert ld % 2 == 1
    else:
        ld = (X + 3) // 4 * 4 + 4
    off = 1 if path == 'offset' else 0
    buf = torch.zeros(n * ld + 8, device=dev)
    view = buf[off:off + n * ld].view(n, ld)[:, :X]
    view.copy_(torch.from_numpy(x).to(dev))
    assert (view.data_ptr() % 16 == 0) == (path != 'offset')
    return view


@pytest.mark.parametrize('path', ['vec', 'offset', 'stride'])
@pytest.mark.parametrize('X', XS)
def test_normalised_feed_against_float64(K, dev, X, path):
    x1, x2 = _counts(X, X), _counts(X, X + 1)[::-1].copy()            # (x2's totals differ from x1's in every slot)
    s1, s2 = _source(x1, path, dev), _source(x2, path, dev)
    q1, q2 = _source(4 * x1, path, dev), _source(4 * x2, path, dev)
    ld = (X + 3) // 4 * 4 + 4
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    worst = 0.0
    for B, Np in SIZES:
        tb = np.array([1, 0, 3, 2, 5][:B], np.int32)
        pr = np.arange(B, dtype=np.int32)[::-1][:Np].copy()
        table = torch.from_numpy(tb[None, :]).to(dev)
        pair_rows = torch.from_numpy(pr).to(dev) if Np else None
        rows = torch.from_numpy(np.concatenate([x1[tb], x2[tb[pr]]]))
        at_one = rows.double().sum(1) == X
        assert bool(at_one[0])
        for noisy in (False, True):
            noise = torch.randn(B + Np, ld, device=dev)[:, :X] if noisy else None

            def launch(a, b, transform=NORM):
                (xin, xin_big), (xt, xt_big) = _banded(B + Np, X, ld, dev), _banded(B + Np, X, ld, dev)
                K.batch_feed(xin, a, b if Np else None, None, table, 1, z, z, pair_rows=pair_rows, noise=noise, sigma=SIGMA, xt=xt,
                             transform=transform)
                assert _band_intact(xin_big, B + Np, X) and _band_intact(xt_big, B + Np, X), 'a guard band was written'
                return host(xin), host(xt)
            xin, xt = launch(s1, s2)
            want_t, want, bnd = DR.feed_reference(rows, noise=host(noise) if noisy else None, sigma=SIGMA)
            assert torch.equal(xt, want_t), 'xt is the source row, bit for bit'
            site = 'dv_batch_feed (log1p_norm) X=%d %s B=%d Np=%d noise=%s' % (X, path, B, Np, noisy)
            worst = max(worst, ref64.check(site, xin, want, bnd))          # (every element; asserts)
            again, _ = launch(s1, s2)
            assert torch.equal(xin.view(torch.int32), again.view(torch.int32)), 'run to run'
            deep, deep_t = launch(q1, q2)
            assert torch.equal(xin.view(torch.int32), deep.view(torch.int32)), 'four times the depth: the same bits'
            assert torch.equal(deep_t, 4 * want_t)
            plain, _ = launch(s1, s2, 'log1p')
            assert torch.equal(xin[at_one].view(torch.int32), plain[at_one].view(torch.int32)), 'total X: the log1p feed'
            assert bool((~at_one).any()) == (B > 1) and (B == 1 or X < 3 or not torch.equal(xin[~at_one], plain[~at_one]))
            if not noisy and B > 1:
                assert bool((xin[1] == 0).all()), 'an all-zero row gives T = 0 exactly'
    print('normalised feed X=%d %s: worst |err| / bound %.3g' % (X, path, worst))


def test_normalised_feed_refusals(K, dev, monkeypatch):
    B, X = 4, 8
    x1 = torch.ones(6, X, device=dev)
    table = torch.arange(B, dtype=torch.int32, device=dev)[None, :]
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    xin, xt = torch.zeros(B, X, device=dev), torch.full((B, X), SENTINEL, device=dev)
    with pytest.raises(RuntimeError, match='dv_batch_feed'):
        K.batch_feed(xin, x1, None, None, table, 1, z, z, transform=NORM)                 # code 3 without targets
    for code in (4, 5, -1, -3):
        monkeypatch.setitem(K.FEED_TRANSFORM, 'bad', code)
        with pytest.raises(RuntimeError, match='dv_batch_feed'):
            K.batch_feed(xin, x1, None, None, table, 1, z, z, xt=xt, transform='bad')
    assert bool((host(xt) == SENTINEL).all()) and bool((host(xin) == 0).all()), 'a refused call wrote'
    K.batch_feed(xin, x1, None, None, table, 1, z, z, xt=xt, transform=NORM)
    assert torch.equal(host(xt), torch.ones(B, X)) and torch.equal(host(xin), torch.full((B, X), float(np.log1p(np.float32(1)))))


# ---------------------------------------------------------------------------------------------- 2. the step
def _eager_equals_captured(kind, variant, lib, dev):
    from tests import nb_ref as R
    from tests.test_counts_cpu import _case, _use_s_case
    from tests.test_nb_cpu import make_engine, set_batch
    spec, batch = _use_s_case(kind) if variant == 'use_s' else _case(kind)
    ref = R.ModelRef(spec, seed=9)
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, ref.engine_params(), dev, type_rec='nb', x_transform=NORM, library_size=lib)
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


@pytest.mark.parametrize('kind,variant,lib', [('drvae', 'plain', True), ('vfae', 'use_s', True), ('pvae', 'universal', False)])
def test_fused_step_matches_the_float64_model_reference(kind, variant, lib, dev):
    """input noise on: three Adam steps against the model-level float64 reference, then eager == captured bit for bit"""
    run_against_reference(kind, variant, lib, dev, tol=GPU_TOL)
    _eager_equals_captured(kind, variant, lib, dev)


@pytest.mark.parametrize('kind,use_s', [('drvae', False), ('pvae', False), ('vfae', True)], ids=['drvae', 'pvae', 'vfae-use_s'])
@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
def test_host_fed_step_equals_the_graph_resident_feed(kind, use_s, captured, dev):
    """(the VFAE conditions on the nuisance variable, its classes carried by the masked sampler feed)"""
    host_fed_equals_feed(kind, dev, captured=captured, use_s=use_s)


def test_combined_riders(dev):
    """dropout, clipping, KL annealing and the parameter average with the normalised feed: against the float64 reference, and
    host-fed == feed through the captured step"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        combined_against_reference(dev, tol=GPU_TOL)
        from tests.test_counts_cpu import COMBINED
        host_fed_equals_feed('drvae', dev, extra=COMBINED, captured=True)


# ------------------------------------------------------------------------------------------ 3. evaluation
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_captured_evaluation_reports_the_step_by_step_numbers(kind, dev):
    """the ``_EvalGraph`` replay of an 'nb' model with the normalised feed and ``library_size`` (its loss pass through the split
    feed with sigma = 0, its inference through ``_enc_x``) against ``_evaluate``, key by key, at the tolerances of
    ``tests/test_gpu_eval_counts.py``"""
    from drvae_amd import fit as F
    from tests.test_gpu_eval_counts import _compare, _dataset, _model, _step_by_step
    model = _model(kind, 'nb', dev, dim_x=16, x_transform=NORM, library_size=True)
    va = _dataset(kind, 'nb', 48, 2, dev, 16)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and ev.graph is not None, 'the captured path was not taken'
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and txt == txt_ref and np.isfinite(got['x1_ll'])
    _compare(model, va, got, ref, '%s-nb-log1p_norm' % kind)


# --------------------------------------------------------------------------------------------------- 4. fit
def test_fit_on_counts_of_varying_depth(dev, tmp_path):
    """``fit`` for 3 epochs on 64 rows of Gamma-Poisson counts (theta = 2) whose depths are log-uniform over two decades (the
    generator and settings of ``tests/test_gpu_counts.py``'s ``fit`` test): every loss finite, the training ELBO of the last
    epoch above the first's, and z1 of the held-out rows the same bits at four times their depth.  Prints the held-out
    log-likelihood per row next to a 'log1p' model trained the same way -- which wins was not known: no sign is asserted.
    Measured: see profiles/r25_depth_feed.md"""
    from drvae_amd import data as D
    from tests.test_fit import _loader
    from tests.test_gpu_nb import _model
    tr, va = _counts_dataset('drvae', 64, 1, dev, DEPTH_DECADES, DEPTH_LO), _counts_dataset('drvae', 32, 2, dev, DEPTH_DECADES, DEPTH_LO)
    w = D.compute_balanced_weights(np.arange(64) % 5)
    ll = {}
    for tag in (NORM, 'log1p'):
        model = _model('drvae', 'nb', dev, epochs=3, x_transform=tag, library_size=True)
        seen, real = [], model.evaluate_performance_on_dataset

        def recording(ds, *a, _real=real, _seen=seen, **k):
            perf, txt = _real(ds, *a, **k)
            _seen.append((ds is tr, {n: float(v) for n, v in perf['losses'].items()}))
            return perf, txt
        model.evaluate_performance_on_dataset = recording
        model.fit(D.DeviceBatcher(tr, w, 16, seed=3), _loader(va, 8), add_noise=False, verbose=False, early_stop=False,
                  model_filename=str(tmp_path / 'b.pth'))
        model.evaluate_performance_on_dataset = real
        assert model.finished_training_iters == 3 * 4 and len(seen) == 6
        assert all(np.isfinite(v) for _, l in seen for v in l.values())
        elbo = [l['ELBO'] for on_train, l in seen if on_train]
        print('%s: training ELBO per epoch %s' % (tag, ' '.join('%.4f' % v for v in elbo)))
        assert len(elbo) == 3 and elbo[-1] > elbo[0]
        assert bool(torch.isfinite(model.engine().arena.param).all())
        res = model.forward(va.x1)
        ll[tag] = float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean())
        assert np.isfinite(ll[tag])
        same = torch.equal(res['z1'], model.forward(4 * va.x1)['z1'])
        assert same == (tag == NORM), 'z1 at four times the depth'
    print('held-out mean log-likelihood per row: log1p_norm + library size %.4f  log1p + library size %.4f' % (ll[NORM], ll['log1p']))
