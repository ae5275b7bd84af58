"""GPU: the count rows with an inverse dispersion per (nuisance class, gene) (``drvae_amd.gene_batch_rows``; the count kinds of
``dv_gauss_nll_rows_raw_cs`` with ``n_cls >= 1``) against the float64 reference and bounds of ``tests/gene_batch_ref.py`` AND, bit
for bit, against the ``'gene'`` launch of the same library at the class's theta row -- in sentinel-filled buffers with guard bands,
on both access paths, over row blocks with a short last block, with and without ``xidx`` / ``cls_src``, over four class layouts,
forward only -- then the fused step, the captured whole-set evaluation, two ranks on one GPU and ``fit``."""
import itertools
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import counts_ref as CR
from tests import gene_batch_ref as BR
from tests import gene_disp_ref as GR
from tests.test_gene_batch_cpu import (FAMILIES, _case, _dp_case, _ref, _run_steps, _worker, combined_against_reference,
                                       host_fed_equals_feed, run_against_reference)
from tests.test_gene_disp_cpu import FP32_TOL, SWITCHES
from tests.test_gpu_gene_disp import (GUARD, ROWS, SENTINEL, XS, _band_intact, _banded, _flat, _flat_intact, _inputs, host)
from tests.test_nb_cpu import make_engine, set_batch

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 3, 8)
LAYOUTS = ('alternating', 'sorted', 'absent_block', 'absent')


@pytest.fixture(scope='module')
def L(dev):
    """(gene_batch_rows, gene_rows, kernels)"""
    import drvae_amd.gene_batch_rows as GB
    import drvae_amd.gene_rows as G
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return GB, G, K


def layout(name, Mr, S, rb):
    """the class of every row: alternating; sorted; class 0 absent from the first row block; the last class absent altogether"""
    c = np.arange(Mr) % S
    if name == 'sorted':
        c = np.sort(c)
    elif name == 'absent_block' and S > 1:
        r0, r1 = GR.blocks(Mr, rb)[0]
        c[r0:r1] = 1 + np.arange(r1 - r0) % (S - 1)
    elif name == 'absent' and S > 1:
        c = np.arange(Mr) % (S - 1)
    return c.astype(np.int32)


def _table(raw, S, seed):
    """S rows of pre-activations: the edge values of ``_inputs`` at other genes in every class"""
    rs = np.random.RandomState(seed)
    return np.stack([np.roll(raw, 3 * k) + (rs.normal(0, 0.5, raw.size).astype(np.float32) if k else 0) for k in range(S)]).astype(np.float32)


@pytest.mark.parametrize('X', XS)
@pytest.mark.parametrize('library', [False, True], ids=['plain', 'lib'])
@pytest.mark.parametrize('family', FAMILIES)
def test_the_launch_against_float64_and_the_gene_launch_in_guarded_buffers(family, library, X, L, dev):
    GB, G, K = L
    x, mu, raw, logit, coef, xidx = _inputs(family, X, 100 + X)
    t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(dev)
    chunks = -(-X // 1024)
    worst = {}
    paths = (0, 1) if X % 4 == 0 else (0,)
    # every (S, M, row blocks) with the other switches cycling through all their combinations
    others = itertools.cycle(itertools.product((False, True), (False, True), LAYOUTS, paths))
    seen = set()
    for S, (Mr, rbs) in itertools.product(CLASSES, ROWS):
        table = _table(raw, S, X + S)
        for rb in rbs:
            use_idx, use_src, lay, off = next(others)
            seen.add((use_idx, use_src, lay, off))
            c = layout(lay, Mr, S, rb)
            idx = xidx[:Mr] if use_idx else None
            xs = x[idx] if use_idx else x[:Mr]
            if use_src:      # the classes behind an indirection: row r reads entry perm[r] of a longer vector
                perm = np.random.RandomState(Mr + S).permutation(Mr + 3)[:Mr].astype(np.int32)
                cvec = np.full(Mr + 3, S + 5, np.int32)       # (entries no row reads: out of range)
                cvec[perm] = c
            else:
                perm, cvec = None, c
            ref = BR.reference(family, torch.from_numpy(xs), torch.from_numpy(mu[:Mr]), torch.from_numpy(table), c,
                               None if logit is None else torch.from_numpy(logit[:Mr]), coef=torch.from_numpy(coef[:Mr]),
                               library=library, row_blocks=rb)
            s_ref = torch.from_numpy(CR.size_factor32(xs))
            xv, _ = _banded(11, X, dev, off)
            xv.copy_(t(x))
            mv, _ = _banded(Mr, X, dev, off)
            mv.copy_(t(mu[:Mr]))
            lv = None
            if logit is not None:
                lv, _ = _banded(Mr, X, dev, off)
                lv.copy_(t(logit[:Mr]))
            tab_v, tab_big = _banded(S, X, dev, off)      # (a class stride that is no multiple of 4 on the scalar path)
            tab_v.copy_(t(table))
            cf, idx_d, cls_d, src_d = t(coef[:Mr]), None if idx is None else t(idx), t(cvec), None if perm is None else t(perm)
            kw = dict(kind=family, shift=1e-6, logit=lv, xidx=idx_d, library=library)

            def launch(fwd_only):
                out, out_big = _flat(Mr * chunks, dev)
                out = out.view(Mr, chunks)
                size, size_big = _flat(Mr, dev)
                got, bands = dict(), [lambda: _flat_intact(out_big, Mr * chunks), lambda: _flat_intact(size_big, Mr)]
                if fwd_only:
                    GB.gene_batch_rows(out, xv, mv, tab_v, cls_d, cls_src=src_d, row_blocks=rb, size=size if library else None, **kw)
                else:
                    dm, dm_big = _banded(Mr, X, dev, off)
                    dl, dl_big = _banded(Mr, X, dev, off) if logit is not None else (None, None)
                    ws, ws_big = _banded(rb, S * X, dev)
                    GB.gene_batch_rows(out, xv, mv, tab_v, cls_d, cls_src=src_d, coef=cf, dmu=dm, dlogit=dl, ws=ws,
                                       size=size if library else None, **kw)
                    grad, grad_big = _flat(S * X, dev)
                    K.colsum(grad, ws)
                    got.update(gm=host(dm).clone(), ws_blocks=host(ws).clone(), grad=host(grad).clone())
                    bands += [lambda: _band_intact(dm_big, Mr, X, off), lambda: _band_intact(ws_big, rb, S * X),
                              lambda: _flat_intact(grad_big, S * X)]
                    if dl is not None:
                        got['gd'] = host(dl).clone()
                        bands.append(lambda: _band_intact(dl_big, Mr, X, off))
                got.update(parts=host(out).clone(), size=host(size).clone())
                assert all(b() for b in bands) and _band_intact(tab_big, S, X, off), 'a guard band was written'
                return got
            tag = (family, library, X, S, Mr, rb, use_idx, use_src, lay, off)
            a, b = launch(False), launch(False)
            assert all(torch.equal(a[k], b[k]) for k in a), ('two launches, equal bits', tag)
            fwd = launch(True)       # forward only: the same row partials, no gradient buffer exists to be written
            assert torch.equal(fwd['parts'], a['parts']) and torch.equal(fwd['size'], a['size'])
            if library:
                assert torch.equal(a['size'], s_ref), tag
            else:
                assert bool((a['size'] == SENTINEL).all())
            # against float64
            e = BR.excess({k: v.numpy() for k, v in a.items()}, ref, coef)
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert all(v <= 1 for v in e.values()), (tag, e)
            # exact: the 'gene' launch of the same library at the class's theta row, coef zeroed on the other classes' rows
            for k in range(S):
                mine = torch.from_numpy(c == k)
                out = torch.zeros(Mr, chunks, device=dev)
                size = torch.zeros(Mr, device=dev)
                dm, _ = _banded(Mr, X, dev, off)
                dl = _banded(Mr, X, dev, off)[0] if logit is not None else None
                ws, _ = _banded(rb, X, dev)
                G.gene_rows(out, xv, mv, tab_v[k].contiguous(), coef=torch.where(mine.to(dev), cf, torch.zeros_like(cf)), dmu=dm,
                            dlogit=dl, ws=ws, size=size if library else None, **kw)
                assert torch.equal(host(out)[mine], a['parts'][mine]) and torch.equal(host(dm)[mine], a['gm'][mine]), (tag, k)
                if dl is not None:
                    assert torch.equal(host(dl)[mine], a['gd'][mine]), (tag, k)
                seg = a['ws_blocks'][:, k * X:(k + 1) * X]
                assert bool((host(ws) == seg).all()), (tag, k)       # (==: a block without rows of the class holds +0)
                if not bool(mine.any()):
                    assert bool((seg == 0).all()) and bool((a['grad'][k * X:(k + 1) * X] == 0).all()), (tag, k)
    assert len(seen) == 2 * 2 * len(LAYOUTS) * len(paths), 'every combination of xidx / cls_src / layout / path was run'
    print('%s%s X=%d: worst |err| / bound  ' % (family, ' lib' if library else '', X) + '  '.join('%s %.3g' % kv for kv in worst.items()))


@pytest.mark.parametrize('family,library,X', [('nb', True, 36), ('zinb', False, 37), ('zinb', True, 1028)])
def test_a_long_block_of_runs_of_odd_length_equals_the_gene_launches(family, library, X, L, dev):
    """4100 rows in ONE row block, three classes in runs of 1, 3 and 5 rows: a workgroup skips runs of odd length between the
    rows it takes, so the two slots of its row partials are taken in turn over the rows TAKEN -- every row partial equals the
    'gene' launch's at the class's theta row"""
    GB, G, K = L
    Mr, S = 4100, 3
    rs = np.random.RandomState(X)
    c = np.repeat(np.arange(2000) % S, np.asarray([1, 3, 5])[np.arange(2000) % 3])[:Mr].astype(np.int32)
    assert c.size == Mr
    x = rs.poisson(rs.gamma(2.0, 10.0, (Mr, X))).astype(np.float32)
    a_ = rs.uniform(-4, 4, (Mr, X))
    mu = (np.log1p(np.exp(-np.abs(a_))) + np.maximum(a_, 0) + 1e-6).astype(np.float32)
    table = rs.normal(0, 2, (S, X)).astype(np.float32)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    xv, mv, tab, cf, cls_d = t(x), t(mu), t(table), t(rs.uniform(-1, 1, Mr).astype(np.float32)), t(c)
    lv = t(rs.normal(0, 2, (Mr, X)).astype(np.float32)) if family == 'zinb' else None
    chunks = -(-X // 1024)
    z = lambda *s: torch.full(s, SENTINEL, device=dev)
    kw = dict(kind=family, shift=1e-6, logit=lv, library=library)
    out, dm, dl, ws, size = z(Mr, chunks), z(Mr, X), z(Mr, X) if lv is not None else None, z(1, S * X), z(Mr)
    GB.gene_batch_rows(out, xv, mv, tab, cls_d, coef=cf, dmu=dm, dlogit=dl, ws=ws, size=size if library else None, **kw)
    got = host(out)
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any())
    for k in range(S):
        mine = torch.from_numpy(c == k)
        o2, d2, l2, w2, s2 = z(Mr, chunks), z(Mr, X), z(Mr, X) if lv is not None else None, z(1, X), z(Mr)
        G.gene_rows(o2, xv, mv, tab[k].contiguous(), coef=torch.where(mine.to(dev), cf, torch.zeros_like(cf)), dmu=d2, dlogit=l2,
                    ws=w2, size=s2 if library else None, **kw)
        assert torch.equal(host(o2)[mine], got[mine]) and torch.equal(host(d2)[mine], host(dm)[mine]), k
        assert lv is None or torch.equal(host(l2)[mine], host(dl)[mine])
        assert bool((host(w2) == host(ws)[:, k * X:(k + 1) * X]).all()), k
        if library:
            assert torch.equal(host(s2), host(size))


def test_launcher_refusals_on_the_device(L, dev):
    GB, _, _ = L
    X, Mr = 8, 3
    z = lambda *s: torch.full(s, SENTINEL, device=dev)
    out, x, mu, raw = z(Mr, 1), torch.ones(Mr, X, device=dev), torch.ones(Mr, X, device=dev), torch.zeros(2, X, device=dev)
    cls = torch.zeros(Mr, dtype=torch.int32, device=dev)
    dm, cf = z(Mr, X), torch.ones(Mr, device=dev)
    with pytest.raises(RuntimeError, match='theta per class'):      # gradients without coef
        GB.gene_batch_rows(out, x, mu, raw, cls, kind='nb', dmu=dm, ws=z(2, 2 * X))
    with pytest.raises(RuntimeError, match='theta per class'):      # a ZINB kind without its logit
        GB.gene_batch_rows(out, x, mu, raw, cls, kind='zinb')
    with pytest.raises(AssertionError):                              # ws narrower than S X
        GB.gene_batch_rows(out, x, mu, raw, cls, kind='nb', coef=cf, dmu=dm, ws=z(2, X))
    assert all(bool((host(b) == SENTINEL).all()) for b in (out, dm))


# ------------------------------------------------------------------------------------------- the fused step
@pytest.mark.parametrize('mode,sw', [('structure', 'both'), ('carried', 'off'), ('universal', 'both')])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_matches_float64_and_eager_equals_captured(family, kind, mode, sw, dev):
    """16 rows in three classes at ``tiny_spec`` sizes: a train-mode pass and three Adam steps against the model-level float64
    reference; then three steps eager and captured (Philox noise): equal bit for bit"""
    from tests.test_gene_batch_cpu import _plan_mode
    eng = run_against_reference(family, kind, mode, sw, dev, tol=FP32_TOL)
    assert eng._route().nll == 'gene'
    spec, batch = _case(family, kind, sw)
    params = _ref(family, spec, sw).engine_params()
    out = []
    for captured in (False, True):
        eng, arena = make_engine(spec, params, dev, type_rec=family, dispersion='gene-batch', **SWITCHES[sw])
        _plan_mode(eng, mode)
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
    moved = (arena.p(GR.RAW).cpu() != torch.from_numpy(params[GR.RAW])).any(1)
    assert bool(moved.all()), 'every class trains its row'


@pytest.mark.parametrize('mode,sw,wn', [('structure', 'both', True), ('carried', 'norm', False), ('carried', 'lib', False)])
def test_fused_step_variants_match_float64(mode, sw, wn, dev):
    run_against_reference('nb', 'drvae', mode, sw, dev, tol=FP32_TOL, weight_norm=wn)


@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_at_a_width_whose_weight_rows_are_padded(family, dev):
    """18 genes: weight rows of that width are padded to 16 bytes in the arena, the table is not (978 genes is such a width)"""
    run_against_reference(family, 'drvae', 'carried', 'both', dev, tol=FP32_TOL, dim_x=18)


@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_host_fed_step_equals_feed_step_bit_for_bit(kind, captured, dev):
    host_fed_equals_feed('zinb' if kind != 'pvae' else 'nb', kind, dev, captured=captured)


def test_combined_riders_match_the_float64_model_reference(dev):
    combined_against_reference('zinb', dev, tol=FP32_TOL)


def test_two_ranks_on_one_gpu_equal_one_process(dev):
    """two child processes on the one GPU (gloo), six rows each, against one process on the twelve: each rank's column sum covers
    its rows of every class and the existing all-reduce adds them"""
    from tests.test_dp_gloo import _free_port
    kind = 'drvae'
    spec, batch, noises, params = _dp_case(kind)
    single = _run_steps(spec, params, batch, noises, None, None, dev=dev)
    assert np.isfinite(single[1]).all() and all(np.abs(single[3][k]).max() > 0 for k in range(2))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, kind, q, 'cuda:0')) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])      # (each child under its own time limit)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    for rank, counts, losses, prm, grad, graw in got:
        np.testing.assert_allclose(losses, single[0], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(graw, single[3], rtol=1e-3, atol=1e-5 * np.abs(single[2]).max())
        np.testing.assert_allclose(prm, single[1], rtol=2e-4, atol=5e-5)
    np.testing.assert_array_equal(got[0][3], got[1][3])                          # replicas stay bit-identical


# ----------------------------------------------------------------------------- the captured whole-set evaluation
@pytest.mark.parametrize('sw', [None, 'both'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_captured_evaluation_equals_the_step_by_step_path(family, kind, sw, dev):
    """``fit._EvalGraph`` of a 'gene-batch' model: the theta block filled once per replay with every evaluation row's own theta
    row (a gather of the finished table by the set's classes, on the device), the recon kinds as they are -- held key by key
    to the rule of the 'gene-cell' evaluations' tests"""
    from drvae_amd import fit as F
    from tests.test_fit import _tiny_model
    if family == 'zinb':
        from tests.test_gpu_eval_zinb import _compare, _dataset, _step_by_step
        va = _dataset(kind, 48, 2, dev, 13)
    else:
        from tests.test_gpu_eval_counts import _compare, _dataset, _step_by_step
        va = _dataset(kind, 'nb', 48, 2, dev, 13)
    va.s = torch.from_numpy(np.random.RandomState(8).randint(0, 3, 48)).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = _tiny_model(kind, device=dev, type_rec=family, dispersion='gene-batch', use_s=True, dim_s=3, add_noise_var=0.0,
                            **(SWITCHES[sw] if sw else {}))
    with torch.no_grad():      # (away from its start: thetas over 0.2 .. 7, another order in every class)
        base = torch.linspace(-1.5, 7.0, 13)
        model.decoder_x.decoder_t.raw_theta.copy_(torch.stack([base, base.flip(0), base.roll(4)]))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        ev = F._EvalGraph.get(model, va)
    assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
    assert ev is not None and ev.graph is not None, 'the captured path was not taken'
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and txt == txt_ref and np.isfinite(got['x1_ll'])
    _compare(model, va, got, ref, '%s-%s-gene-batch-%s' % (kind, family, sw))
    # the replay follows the table
    with torch.no_grad():
        model.decoder_x.decoder_t.raw_theta[1].add_(1.0)
    moved, _ = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and moved['x1_ll'] != got['x1_ll'] and moved['x1_rmse'] == got['x1_rmse']


@pytest.mark.parametrize('family', FAMILIES)
def test_fit_three_epochs_on_counts_whose_classes_differ_in_dispersion(family, dev, tmp_path):
    """``fit`` for three epochs on Gamma-Poisson counts whose two classes have true theta 0.5 and 20 in every gene, depths
    spread over a factor of four: finite losses and a finite table.  REPORTED, not asserted: the held-out ``ll`` next to the
    'gene' model's and the per-class median of the learned theta"""
    from tests.test_fit import _loader, _tiny_model
    tr = BR.class_dataset('drvae', 512, 1, dev)
    va = BR.class_dataset('drvae', 64, 101, dev)
    ll = {}
    for disp in ('gene-batch', 'gene'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = _tiny_model('drvae', device=dev, type_rec=family, dispersion=disp, use_s=True, dim_s=2, add_noise_var=0.0,
                                x_transform='log1p', library_size=True, epochs=3, learning_rate=5e-2, random_seed=5)
        model.w2log = lambda *a: None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            model.fit(_loader(tr, 16), _loader(va, 8), add_noise=False, verbose=False, early_stop=False,
                      model_filename=str(tmp_path / 'b.pth'))
            perf, _ = model.evaluate_performance_on_dataset(va)
        assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
        assert np.isfinite(float(perf['losses']['ELBO'])) and np.isfinite(perf['x1_ll']) and np.isfinite(perf['x2_ll'])
        ll[disp] = perf['x1_ll']
        if disp == 'gene-batch':
            theta = model.decoder_x.decoder_t.theta().detach().cpu().numpy()
            assert theta.shape == (2, 13) and np.all(np.isfinite(theta)) and np.all(theta > 0)
            med = np.median(theta, 1)
    print('%s: held-out x1_ll  gene-batch %.4f | gene %.4f;  median learned theta: class 0 (true 0.5) %.3f, class 1 (true 20) %.3f'
          % (family, ll['gene-batch'], ll['gene'], med[0], med[1]))
