"""GPU: the count rows with a gene-wise inverse dispersion (the count kinds of ``dv_gauss_nll_rows_raw_cs``;
``drvae_amd.gene_rows``) against the float64 reference and bounds of ``tests/gene_disp_ref.py`` -- in sentinel-filled buffers
with guard bands, on both access paths, over row blocks with a short last block, with and without ``xidx``, forward only --
then the fused step (float64 reference, eager == captured, host-fed == feed), the captured whole-set evaluation against the
step-by-step path, and ``fit``."""
import warnings

import numpy as np
import pytest
import torch

from tests import counts_ref as CR
from tests import gene_disp_ref as GR
from tests import ref64
from tests import zinb_ref as Z
from tests.test_gene_disp_cpu import (FAMILIES, FP32_TOL, SWITCHES, _case, _ref, combined_against_reference, host_fed_equals_feed,
                                      run_against_reference)
from tests.test_nb_cpu import make_engine, set_batch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 8
XS = (1, 3, 4, 978, 1023, 1024, 1025, 1028, 2052)      # one gene; below / at a quad; the main width; around the chunk seam; three chunks
ROWS = ((1, (1,)), (2, (1, 2)), (7, (1, 7, 2, 3)), (9, (1, 9, 2, 3)))       # M, row_blocks: 7 / 2, 7 / 3 and 9 / 2 end in a short block


@pytest.fixture(scope='module')
def G(dev):
    import drvae_amd.gene_rows as G
    from drvae_amd import _lib
    _lib.load()
    return G


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def _flat(n, dev):
    """n floats between two guard bands of a sentinel-filled buffer: (view, whole buffer)"""
    big = torch.full((n + 2 * GUARD,), SENTINEL, device=dev)
    return big[GUARD:GUARD + n], big


def _flat_intact(big, n):
    b = host(big)
    return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all())


def _banded(rows, X, dev, off=0):
    """a (rows, X) view inside a sentinel-filled buffer, a row above and below and at least four columns to its right; ``off`` =
    1: the view starts one float off a 16-byte boundary (the forced scalar path)"""
    ld = (X + 3) // 4 * 4 + 8
    big = torch.full((rows + 2, ld), SENTINEL, device=dev)
    return big[1:rows + 1, off:off + X], big


def _band_intact(big, rows, X, off=0):
    b = host(big)
    return bool((b[0] == SENTINEL).all() and (b[rows + 1] == SENTINEL).all() and (b[1:rows + 1, off + X:] == SENTINEL).all()
                and (b[1:rows + 1, :off] == SENTINEL).all())


def _inputs(kind, X, seed):
    """nine decoder rows over eleven target rows (fp32): counts with zeros, an all-zero row and one of 30000s; means over
    softplus(-6 .. 4); raw theta over -30 .. 10; logits over the edge values; the row coefficients"""
    rs = np.random.RandomState(seed)
    x = rs.poisson(rs.gamma(2.0, 20.0, (11, X))).astype(np.float32) * (rs.rand(11, X) < 0.6)
    x[3] = 0
    x[5, :min(X, 500)] = 30000.0
    a = rs.uniform(-6, 4, (9, X))
    mu = (np.log1p(np.exp(-np.abs(a))) + np.maximum(a, 0) + 1e-6).astype(np.float32)
    raw = rs.normal(0, 2, X).astype(np.float32)
    raw[::7] = -30.0
    raw[3::11] = 10.0
    logit = rs.choice(np.asarray(Z.LOGITS + (-3.0, 2.5)), (9, X)).astype(np.float32)
    coef = np.asarray([1.0, -0.5, 2.0, 0.25], np.float32)[np.arange(9) % 4]
    xidx = rs.permutation(11)[:9].astype(np.int32)
    return x, mu, raw, logit if kind == 'zinb' else None, coef, xidx


@pytest.mark.parametrize('X', XS)
@pytest.mark.parametrize('library', [False, True], ids=['plain', 'lib'])
@pytest.mark.parametrize('family', FAMILIES)
def test_the_launch_against_float64_in_guarded_buffers(family, library, X, G, dev):
    import drvae_amd.kernels as K
    x, mu, raw, logit, coef, xidx = _inputs(family, X, 100 + X)
    t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(dev)
    chunks = -(-X // 1024)
    worst, refs = {}, {}
    paths = (0, 1) if X % 4 == 0 else (0,)
    for Mr, rbs in ROWS:
        for use_idx in (False, True):
            idx = xidx[:Mr] if use_idx else None
            xs = x[idx] if use_idx else x[:Mr]
            ref = GR.reference(family, torch.from_numpy(xs), torch.from_numpy(mu[:Mr]), torch.from_numpy(raw),
                               None if logit is None else torch.from_numpy(logit[:Mr]), coef=torch.from_numpy(coef[:Mr]), library=library)
            s_ref = torch.from_numpy(CR.size_factor32(xs))
            for off in paths:
                xv, _ = _banded(11, X, dev, off)
                xv.copy_(t(x))
                mv, _ = _banded(Mr, X, dev, off)
                mv.copy_(t(mu[:Mr]))
                lv = None
                if logit is not None:
                    lv, _ = _banded(Mr, X, dev, off)
                    lv.copy_(t(logit[:Mr]))
                rawd, cf, idx_d = t(raw), t(coef[:Mr]), None if idx is None else t(idx)
                for rb in rbs:
                    for fwd_only in (False, True):
                        bits = []
                        for rep in range(2):
                            out, out_big = _flat(Mr * chunks, dev)
                            out = out.view(Mr, chunks)
                            size, size_big = _flat(Mr, dev)
                            kw = dict(kind=family, shift=1e-6, logit=lv, xidx=idx_d, library=library, size=size if library else None)
                            if fwd_only:
                                G.gene_rows(out, xv, mv, rawd, row_blocks=rb, **kw)
                            else:
                                dm, dm_big = _banded(Mr, X, dev, off)
                                dl, dl_big = _banded(Mr, X, dev, off) if logit is not None else (None, None)
                                ws, ws_big = _banded(rb, X, dev)
                                G.gene_rows(out, xv, mv, rawd, coef=cf, dmu=dm, dlogit=dl, ws=ws, **kw)
                                grad, grad_big = _flat(X, dev)
                                K.colsum(grad, ws)
                            got = dict(parts=host(out).clone())
                            assert _flat_intact(out_big, Mr * chunks) and _flat_intact(size_big, Mr)
                            if library:      # the same s with one chunk (formed in the pass) and with several (the launch in front)
                                assert torch.equal(host(size), s_ref), (X, Mr, rb)
                            else:
                                assert bool((host(size) == SENTINEL).all())
                            if not fwd_only:
                                got.update(gm=host(dm).clone(), ws=host(grad).clone(), wsb=host(ws).clone())
                                assert _band_intact(dm_big, Mr, X, off) and _band_intact(ws_big, rb, X) and _flat_intact(grad_big, X)
                                if dl is not None:
                                    got['gd'] = host(dl).clone()
                                    assert _band_intact(dl_big, Mr, X, off)
                                # a block past the last row owns none: zeros in its row of ws
                                for b, (r0, r1) in enumerate(GR.blocks(Mr, rb)):
                                    if r0 == r1:
                                        assert bool((got['wsb'][b] == 0).all())
                            bits.append(got)
                        assert all(torch.equal(bits[0][k], bits[1][k]) for k in bits[0]), 'two launches, equal bits'
                        e = GR.excess({k: v.numpy() for k, v in bits[0].items()}, ref, None if fwd_only else coef)
                        for k, v in e.items():
                            worst[k] = max(worst.get(k, 0.0), v)
                        assert all(v <= 1 for v in e.values()), (family, library, X, Mr, rb, use_idx, off, fwd_only, e)
                        if not fwd_only:
                            refs[(Mr, use_idx)] = (bits[0], xs)
    print('%s%s X=%d: worst |err| / bound  ' % (family, ' lib' if library else '', X) + '  '.join('%s %.3g' % kv for kv in worst.items()))
    # REPORTED, only the bounds are asserted: elements whose bits differ from dv_rec_nll_rows fed the same theta as a full block
    if X <= 1024:
        got, xs = refs[(9, True)]
        nh = 3 if family == 'zinb' else 2
        th = GR.theta32(torch.from_numpy(raw))[None, :].expand(9, X)
        v = torch.cat([torch.from_numpy(mu), th] + ([torch.from_numpy(logit)] if logit is not None else []), 1).to(dev).contiguous()
        out, dpre = torch.zeros(9, device=dev), torch.zeros(9, nh * X, device=dev)
        K.rec_nll_rows(out, t(x), v, kind=family, shift=1e-6, xidx=t(xidx), coef=t(coef), dpre=dpre, **(dict(library=True) if library else {}))
        d = host(dpre)
        n_out = int((host(out) != got['parts'][:, 0]).sum())
        n_gm = int((d[:, :X] != got['gm']).sum())
        n_gd = int((d[:, 2 * X:] != got['gd']).sum()) if logit is not None else 0
        print('  bits that differ from dv_rec_nll_rows at the same theta: out %d / %d  g_m %d / %d  g_d %d / %d'
              % (n_out, 9, n_gm, 9 * X, n_gd, 9 * X if logit is not None else 0))


def test_launcher_refusals_on_the_device(G, dev):
    X, Mr = 8, 3
    z = lambda *s: torch.full(s, SENTINEL, device=dev)
    out, x, mu, raw = z(Mr, 1), torch.ones(Mr, X, device=dev), torch.ones(Mr, X, device=dev), torch.zeros(X, device=dev)
    dm, ws, cf = z(Mr, X), z(2, X), torch.ones(Mr, device=dev)
    with pytest.raises(RuntimeError, match='gene-wise theta'):      # an NB kind with a logit gradient
        G.gene_rows(out, x, mu, raw, kind='nb', coef=cf, dmu=dm, dlogit=z(Mr, X), ws=ws)
    with pytest.raises(RuntimeError, match='gene-wise theta'):      # a ZINB kind without its logit
        G.gene_rows(out, x, mu, raw, kind='zinb')
    with pytest.raises(RuntimeError, match='gene-wise theta'):      # more row blocks than rows
        G.gene_rows(out, x, mu, raw, kind='nb', row_blocks=Mr + 1)
    with pytest.raises(RuntimeError, match='gene-wise theta'):      # gradients without coef
        G.gene_rows(out, x, mu, raw, kind='nb', dmu=dm, ws=ws)
    assert all(bool((host(b) == SENTINEL).all()) for b in (out, dm, ws))


# ------------------------------------------------------------------------------------------- the fused step
@pytest.mark.parametrize('sw', ['off', 'both'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_matches_float64_and_eager_equals_captured(family, kind, sw, dev):
    """16 rows at ``tiny_spec`` sizes: a train-mode pass and three Adam steps against the model-level float64 reference; then
    three steps eager and captured (Philox noise): equal bit for bit"""
    eng = run_against_reference(family, kind, 'plain', sw, dev, tol=FP32_TOL)
    assert eng._route().nll == 'gene'
    spec, batch = _case(family, kind, sw)
    params = _ref(family, spec, sw).engine_params()
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, params, dev, type_rec=family, dispersion='gene', **SWITCHES[sw])
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
    assert not torch.equal(arena.p(GR.RAW).cpu(), torch.from_numpy(params[GR.RAW]))


@pytest.mark.parametrize('variant,sw', [('weight_norm', 'both'), ('universal', 'both'), ('use_s', 'both'), ('plain', 'norm')])
def test_fused_step_variants_match_float64(variant, sw, dev):
    run_against_reference('nb', 'drvae', variant, sw, dev, tol=FP32_TOL)


@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
@pytest.mark.parametrize('family', FAMILIES)
def test_host_fed_step_equals_feed_step_bit_for_bit(family, captured, dev):
    host_fed_equals_feed(family, 'drvae', dev, captured=captured)


def test_combined_riders_match_the_float64_model_reference(dev):
    combined_against_reference('zinb', dev, tol=FP32_TOL)


# ----------------------------------------------------------------------------- the captured whole-set evaluation
@pytest.mark.parametrize('sw', [None, 'both'])
@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_captured_evaluation_equals_the_step_by_step_path(family, kind, sw, dev):
    """``fit._EvalGraph`` of a gene-wise model: the theta row written into the theta block once per replay, the recon kinds as
    they are -- held key by key to the rule of the 'gene-cell' evaluations' tests"""
    from drvae_amd import fit as F
    from tests.test_fit import _tiny_model
    if family == 'zinb':
        from tests.test_gpu_eval_zinb import _compare, _dataset, _step_by_step
        ds = lambda: _dataset(kind, 48, 2, dev, 13)
    else:
        from tests.test_gpu_eval_counts import _compare, _dataset, _step_by_step
        ds = lambda: _dataset(kind, 'nb', 48, 2, dev, 13)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = _tiny_model(kind, device=dev, type_rec=family, dispersion='gene', add_noise_var=0.0, **(SWITCHES[sw] if sw else {}))
    with torch.no_grad():      # (away from its start: thetas over 0.2 .. 7)
        model.decoder_x.decoder_t.raw_theta.copy_(torch.linspace(-1.5, 7.0, 13))
    va = ds()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        ev = F._EvalGraph.get(model, va)
    assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
    assert ev is not None and ev.graph is not None, 'the captured path was not taken'
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and txt == txt_ref and np.isfinite(got['x1_ll'])
    _compare(model, va, got, ref, '%s-%s-gene-%s' % (kind, family, sw))
    # the replay follows the vector
    with torch.no_grad():
        model.decoder_x.decoder_t.raw_theta.add_(1.0)
    moved, _ = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and moved['x1_ll'] != got['x1_ll'] and moved['x1_rmse'] == got['x1_rmse']


@pytest.mark.parametrize('family', FAMILIES)
def test_fit_three_epochs_on_counts_with_a_per_gene_theta(family, dev, tmp_path):
    """``fit`` for three epochs is finite.  REPORTED, not asserted: the held-out ``ll`` next to the 'gene-cell' model's and the
    rank correlation of learned and true theta"""
    import scipy.stats as st
    from tests.test_fit import _loader, _tiny_model
    zi = family == 'zinb'
    tr = GR.gp_dataset('drvae', 512, 1, dev, depth=50.0, zero_inflated=zi)
    va = GR.gp_dataset('drvae', 64, 101, dev, depth=50.0, zero_inflated=zi)
    ll = {}
    for disp in ('gene', 'gene-cell'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = _tiny_model('drvae', device=dev, type_rec=family, dispersion=disp, add_noise_var=0.0, x_transform='log1p',
                                epochs=3, learning_rate=5e-2, random_seed=5)
        model.w2log = lambda *a: None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            model.fit(_loader(tr, 16), _loader(va, 8), add_noise=False, verbose=False, early_stop=False,
                      model_filename=str(tmp_path / 'b.pth'))
            perf, _ = model.evaluate_performance_on_dataset(va)
        assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
        assert np.isfinite(float(perf['losses']['ELBO'])) and np.isfinite(perf['x1_ll']) and np.isfinite(perf['x2_ll'])
        ll[disp] = perf['x1_ll']
        if disp == 'gene':
            theta = model.decoder_x.decoder_t.theta().detach().cpu().numpy()
            assert np.all(np.isfinite(theta)) and np.all(theta > 0)
            rho = st.spearmanr(theta, GR.gene_theta(13, seed=1)).correlation
            res = model.forward(va.x1)
            with torch.no_grad():
                direct = float(model.decoder_x.logp_perx(va.x1, *res['px1']).mean())
            assert perf['x1_ll'] == pytest.approx(direct, rel=1e-5)
    print('%s: held-out x1_ll  gene %.4f | gene-cell %.4f;  Spearman(learned theta, true theta) = %.3f' % (family, ll['gene'], ll['gene-cell'], rho))
