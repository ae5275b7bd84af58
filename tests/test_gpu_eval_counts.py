"""-m gpu: the count kinds of ``dv_recon_rows`` against the float64 reference and bounds of ``tests/eval_counts_ref.py``, and
the captured whole-set evaluation (``fit._EvalGraph``) of the count-decoder models ('binary' / 'poisson' / 'nb', with the
raw-count switches) against the step-by-step evaluation ``model._evaluate`` and a float64 evaluation of the same formulas."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import eval_counts_ref as ER
from tests import nb_ref as R
from tests import ref64
from tests.test_counts_cpu import SWITCHES, _counts_dataset
from tests.test_fit import _loader, _tiny_model

pytestmark = pytest.mark.gpu

MS, XS = (1, 5, 67), (1, 13, 16, 257, 1028)
PROFILE = {}        # worst fraction of the bound per (case, output), as the kernel tests measure it


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    return K


# ------------------------------------------------------------------------------------------ guarded operands
def _guarded(t, dev, misalign=False):
    """``t`` (M, X) inside a NaN-filled buffer: two guard rows above and below, a padded row stride with NaN pads, the base
    16-byte aligned with a stride of whole 16-byte groups -- or (``misalign``) one float off.  -> (view, buffer)"""
    M, X = t.shape
    ld = (X + 3) // 4 * 4 + 8
    off = 4 + (1 if misalign else 0)
    buf = torch.full(((M + 4) * ld + 8,), float('nan'), device=dev)
    view = buf[2 * ld:(2 + M) * ld].view(M, ld)[:, off:off + X]
    view.copy_(t.to(dev))
    return view, buf


def _guarded_vec(n, dev):
    buf = torch.full((n + 16,), float('nan'), device=dev)
    return buf[8:8 + n], buf


def _outside_untouched(view, buf, before):
    """nothing outside ``view`` changed in ``buf`` (``before``: the buffer's bits before the launch)"""
    now = buf.clone()
    mask = torch.ones_like(buf, dtype=torch.bool)
    M, X = (view.shape[0], view.shape[1]) if view.dim() == 2 else (1, view.numel())
    start = (view.data_ptr() - buf.data_ptr()) // 4
    ld = view.stride(0) if view.dim() == 2 and M > 1 else 0
    for i in range(M):
        mask[start + i * ld:start + i * ld + X] = False
    return torch.equal(now.view(torch.int32)[mask], before.view(torch.int32)[mask])


def _launch(K, dev, kind, x, mu, th, size, *, misalign=False, alias=False, want_ll=True, rec=True):
    """one guarded launch -> dict(rows, ll, rec) on the host, after checking the guard bands of every operand and output"""
    M, X = x.shape
    xg, xb = _guarded(x, dev, misalign)
    mg, mb = _guarded(mu, dev, misalign)
    tg, tb = _guarded(th, dev, misalign) if th is not None else (None, None)
    same = size is not None and size is x
    sg, sb = (xg, xb) if same else (_guarded(size, dev, misalign) if size is not None else (None, None))
    rows, rowsb = _guarded_vec(M * 6, dev)
    rows = rows.view(M, 6)
    ll, llb = _guarded_vec(M, dev) if want_ll else (None, None)
    og, ob = (None, None)
    if rec and size is not None:
        og, ob = (mg, mb) if alias else _guarded(torch.zeros(M, X), dev, misalign)
    bufs = [(xg, xb), (mg, mb), (rows.view(-1), rowsb)] + ([(tg, tb)] if tg is not None else []) + \
        ([(sg, sb)] if sg is not None and not same else []) + ([(ll, llb)] if ll is not None else []) + \
        ([(og, ob)] if og is not None and not alias else [])
    before = [b.clone() for _, b in bufs]
    inputs = [xg.clone(), tg.clone() if tg is not None else None, sg.clone() if sg is not None else None]
    K.recon_rows(rows, ll, xg, mg, tg, kind=kind, size_from=sg, rec_out=og)
    torch.cuda.synchronize()
    for (v, b), b0 in zip(bufs, before):
        assert _outside_untouched(v, b, b0), 'a launch wrote outside its views'
    assert torch.equal(xg, inputs[0]) and (tg is None or torch.equal(tg, inputs[1])) and (sg is None or torch.equal(sg, inputs[2]))
    if og is None or not alias:
        assert torch.equal(mg.cpu(), mu), 'the mean head was written'
    out = dict(rows=rows.cpu(), ll=ll.cpu() if ll is not None else None, rec=og.cpu() if og is not None else None)
    for k, v in out.items():
        assert v is None or bool(torch.isfinite(v).all()), 'a pad reached %s' % k
    return out


def _check(tag, got, ref, keys):
    for k in keys:
        if got[k] is None:
            continue
        w = ref64.check('%s %s' % (tag, k), got[k], ref[k], ref[k + '_bound'])
        PROFILE[(tag.split()[0], k)] = max(PROFILE.get((tag.split()[0], k), 0.0), w)


# ------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('kind,scaled', ER.COMBOS)
def test_count_rows_against_float64(kind, scaled, K, dev):
    """every shape (one row, several workgroups; one gene, odd widths, 16, beyond a thread's first trip, beyond 1024) x both
    paths (16-byte, and the scalar one forced by a misaligned base) x both size sources: rows, ll and the stored mean within
    their bounds, guard bands intact, two launches bit-equal"""
    name = kind + ('-scaled' if scaled else '')
    for M in MS:
        for X in XS:
            for other in ((False, True) if scaled else (False,)):
                for counts in (('mixed', 'thousands') if (kind != 'binary' and X == 257) else ('mixed',)):
                    x, mu, th, size = ER.case(kind, M, X, seed=3, scaled=scaled, other=other, counts=counts)
                    if scaled and not other:
                        size = x
                    ref = ER.reference(kind, x, mu, th, size)
                    for misalign in (False, True):
                        tag = '%s M=%d X=%d other=%d %s misaligned=%d' % (name, M, X, other, counts, misalign)
                        got = _launch(K, dev, kind, x, mu, th, size, misalign=misalign)
                        _check(tag, got, ref, ('rows', 'll', 'rec'))
                        again = _launch(K, dev, kind, x, mu, th, size, misalign=misalign)
                        for k in got:
                            assert got[k] is None or torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (tag, k)
    print('%s: worst fraction of the bound: rows %.3f  ll %.3f  rec %.3f' % (
        name, PROFILE.get((name, 'rows'), 0), PROFILE.get((name, 'll'), 0), PROFILE.get((name, 'rec'), 0)))


@pytest.mark.parametrize('kind', ['poisson', 'nb'])
def test_call_forms_give_the_same_bits(kind, K, dev):
    """``ll=None``, ``rec_out`` aliased with the mean head / separate / absent: the same rows (and log-likelihoods, and
    stored means) bit for bit, on both paths"""
    for X in (13, 16, 1028):
        x, mu, th, size = ER.case(kind, 5, X, seed=4, scaled=True, other=True)
        for misalign in (False, True):
            base = _launch(K, dev, kind, x, mu, th, size, misalign=misalign)
            for form in (dict(want_ll=False), dict(alias=True), dict(rec=False), dict(alias=True, want_ll=False)):
                got = _launch(K, dev, kind, x, mu, th, size, misalign=misalign, **form)
                for k in ('rows', 'll', 'rec'):
                    if got[k] is not None:
                        assert torch.equal(got[k].view(torch.int32), base[k].view(torch.int32)), (kind, X, misalign, form, k)


@pytest.mark.parametrize('scaled', [False, True])
def test_negative_binomial_edge_grid(scaled, K, dev):
    """mu = 1e-6 .. 1e4 x theta = 1e-3 .. 1e6 x counts 0 .. 30 000 (``nb_ref.edge_grid``, the grid of
    ``tests/test_gpu_nb.py``), plain and scaled (size source: another matrix, of small counts, with an all-zero row)"""
    x, mu, th, _ = R.edge_grid(X=256)          # (256 genes of at most 30 000: row totals below 2^24)
    size = None
    if scaled:
        rs = np.random.RandomState(5)
        size = torch.from_numpy(rs.poisson(rs.gamma(2.0, 2.0, tuple(x.shape))).astype(np.float32))
        size[0] = 0.0
    ref = ER.reference('nb', x, mu, th, size)
    got = _launch(K, dev, 'nb', x, mu, th, size)
    name = 'nb-grid' + ('-scaled' if scaled else '')
    _check(name, got, ref, ('rows', 'll', 'rec'))
    print('%s: worst fraction of the bound: rows %.3f  ll %.3f' % (name, PROFILE[(name, 'rows')], PROFILE[(name, 'll')]))


def test_launcher_refusals_on_the_device(K, dev):
    x, mu, th, size = [t.to(dev) if t is not None else None for t in ER.case('nb', 3, 8, scaled=True)]
    rows = torch.zeros(3, 6, device=dev)
    with pytest.raises(RuntimeError, match='dv_recon_rows'):
        K.recon_rows(rows, None, x, mu, None, kind='binary', size_from=size)
    with pytest.raises(RuntimeError, match='dv_recon_rows'):
        K.recon_rows(rows, None, x, mu, th, kind='nb', rec_out=mu.clone())
    assert float(rows.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------- 2. the models
def _model(kind, type_rec, dev, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return _tiny_model(kind, device=dev, type_rec=type_rec, add_noise_var=0.0, **kw)


def _dataset(kind, type_rec, n, seed, dev, dim_x=13):
    ds = _counts_dataset(kind, n, seed, dev, 1.0, -1.0)      # (depths 0.1 .. 1: an untrained encoder reading RAW counts stays finite)
    if dim_x != 13:
        reps = -(-dim_x // 13)
        ds.x1 = ds.x1.repeat(1, reps)[:, :dim_x].contiguous()
        if kind != 'vfae':
            ds.x2 = ds.x2.repeat(1, reps)[:, :dim_x].contiguous()
    if type_rec == 'binary':
        ds.x1 = (ds.x1 > 2).float()
        if kind != 'vfae':
            ds.x2 = (ds.x2 > 2).float() * ds.has_x2[:, None].float()
    return ds


def _step_by_step(model, ds):
    g = lambda k: getattr(ds, k, None)
    return model._evaluate(g('x1'), g('x2'), g('s'), g('y'), g('has_x2'), g('has_y'))


def _float64_metrics(model, ds):
    """the reported reconstruction metrics in float64 from the fp32 heads ``model.forward`` returns, and the kernel-level
    bounds propagated to them -> ({key: value}, {key: bound})"""
    kind, tr = model.kind, model.type_rec
    res = model.forward(ds.x1, getattr(ds, 's', []))
    lib = bool(getattr(model, 'library_size', False))
    model.library_size = False
    try:
        heads = model.forward(ds.x1, getattr(ds, 's', []))          # (the unscaled heads: what the row pass is handed)
    finally:
        model.library_size = lib
    val, bnd = {}, {}
    for tag, key, x, idx in (('x1', 'px1', ds.x1, None),) + ((('x2', 'px2', ds.x2, torch.nonzero(ds.has_x2.reshape(-1)).reshape(-1)),)
                                                            if kind != 'vfae' else ()):
        if idx is not None and len(idx) == 0:
            continue
        sl = (lambda t: t.cpu() if idx is None else t[idx].cpu())
        xs, r = sl(x), sl(res[key][0])
        th = sl(res[key][1]) if tr == 'nb' else None
        ll = R.logp64(ref64.f64(xs), ref64.f64(r), ref64.f64(th)).sum(1) if tr == 'nb' else None
        kref = ER.reference(tr, xs, sl(heads[key][0]), th, sl(ds.x1) if lib else None)
        for k, v in ER.metrics64(xs, r, ll).items():
            val['%s_%s' % (tag, k)] = v
        for k, v in ER.metrics_bound(xs, r, kref['rows_bound'], kref['ll_bound'] if tr == 'nb' else None).items():
            bnd['%s_%s' % (tag, k)] = v
    return val, bnd


def _compare(model, ds, got, ref, tag):
    """key by key: nan where the step-by-step path has nan; else the captured value no farther from float64 than twice the
    step-by-step value's own distance plus the propagated kernel bound.  Sampled loss terms loosely (another Philox draw)."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    val, bnd = _float64_metrics(model, ds)
    for k, v in ref.items():
        if k in ('losses', 'model_class'):
            continue
        if k.startswith('y_'):
            assert got[k] == pytest.approx(v, abs=1e-6, nan_ok=True), (k, got[k], v)
            continue
        if np.isnan(v):
            assert np.isnan(got[k]), (tag, k, got[k])
            continue
        d_cap, d_ref = abs(got[k] - val[k]), abs(v - val[k])
        print('%-28s %-8s float64 %.10g  captured off by %.3g  step by step off by %.3g  kernel bound %.3g' % (
            tag, k, val[k], d_cap, d_ref, bnd[k]))
        assert d_cap <= 2 * d_ref + bnd[k], (tag, k, got[k], v, val[k], d_cap, d_ref, bnd[k])
    assert list(got['losses']) == list(ref['losses'])
    for k, v in ref['losses'].items():
        a, b = float(got['losses'][k]), float(v)
        assert np.isfinite(b), (k, b)
        assert abs(a - b) <= 0.2 * max(1.0, abs(b)), (k, a, b)


CASES = [(kind, tr, sw) for kind in ('drvae', 'pvae', 'vfae') for tr, sws in (('binary', (None,)), ('poisson', (None, 'log1p', 'lib', 'both')),
                                                                              ('nb', (None, 'log1p', 'lib', 'both'))) for sw in sws]


@pytest.mark.parametrize('kind,type_rec,sw', CASES, ids=['%s-%s-%s' % c for c in CASES])
def test_captured_evaluation_of_count_models(kind, type_rec, sw, dev):
    from drvae_amd import fit as F
    dim_x = 16 if (sw == 'both' or type_rec == 'binary') else 13
    model = _model(kind, type_rec, dev, dim_x=dim_x, **(SWITCHES[sw] if sw else {}))
    va = _dataset(kind, type_rec, 48, 2, dev, dim_x)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and ev.graph is not None, 'the captured path was not taken'
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and txt == txt_ref
    assert np.isfinite(got['x1_ll']) if type_rec == 'nb' else np.isnan(got['x1_ll'])
    _compare(model, va, got, ref, '%s-%s-%s' % (kind, type_rec, sw))


def _nb_both(kind, dev, **kw):
    return _model(kind, 'nb', dev, **dict(SWITCHES['both'], **kw))


def test_the_size_source_of_x2_is_x1(dev):
    """an x2 ten times as deep as x1: the x2 metrics are those at x1's size factor (``forward``'s), which a kernel scaling
    by the target's own depth misses by a factor"""
    model = _nb_both('drvae', dev)
    va = _dataset('drvae', 'nb', 48, 3, dev)
    va.x2 = (va.x2 * 10).contiguous()
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert txt == txt_ref
    _compare(model, va, got, ref, 'x2 ten times as deep')
    res = model.forward(va.x1)
    idx = torch.nonzero(va.has_x2).reshape(-1)
    wrong = ER.metrics64(va.x2[idx].cpu(), (res['px2'][0] / model.size_factor(va.x1)[:, None] * model.size_factor(va.x2)[:, None])[idx].cpu())
    assert abs(wrong['rmse'] - got['x2_rmse']) > 0.1 * got['x2_rmse']


def test_no_pairs_and_a_plan_in_another_row_order(dev):
    from drvae_amd import fit as F
    model = _nb_both('drvae', dev)
    va = _dataset('drvae', 'nb', 48, 4, dev)
    va.has_x2.zero_()
    va.x2.zero_()
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is not None and txt == txt_ref and 'no x2 data' in txt and np.isnan(got['x2_rmse'])
    _compare(model, va, got, ref, 'no pairs')
    # the supervised-only VFAE: the plan holds the labeled rows only (``sel``), the encoder of the inference reads log1p(x1)
    from drvae_amd.VFAE import VFAE
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = VFAE(dim_x=13, dim_s=1, dim_y=2, dim_h_en_z1=[7], dim_h_de_x=[8], dim_z1=5, type_rec='nb', nonlinearity='elu',
                     learning_rate=5e-3, L=2, weight_decay=0.01, add_noise_var=0.0, use_MMD=False, random_seed=5, epochs=2,
                     batch_size=8, dim_h_de_z1=[6], dim_h_en_z2=[6], dim_h_clf=[], dim_z2=4, semi_supervised=False, device=dev,
                     **SWITCHES['both'])
    va = _dataset('vfae', 'nb', 48, 5, dev)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and ev.sel is not None
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert txt == txt_ref
    _compare(model, va, got, ref, 'sel')


def test_the_replay_follows_parameters_and_data(dev):
    from drvae_amd import fit as F
    model = _nb_both('drvae', dev, epochs=2)
    va = _dataset('drvae', 'nb', 48, 6, dev)
    got, _ = model.evaluate_performance_on_dataset(va)
    ev = F._EvalGraph.get(model, va)
    again, _ = model.evaluate_performance_on_dataset(va)
    assert again['x1_rmse'] == got['x1_rmse'] and again['x1_ll'] == got['x1_ll'] and F._EvalGraph.get(model, va) is ev
    batch = tuple(getattr(va, f) for f in va.FIELDS)
    for _ in range(5):
        model.run_on_batch(train_mode=True, **model._batch_kwargs(batch))
    moved, _ = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and moved['x1_ll'] != got['x1_ll']
    _compare(model, va, moved, _step_by_step(model, va)[0], 'trained')
    va.x1.mul_(2.0)                                   # edited in place: evaluated as edited, by the same graph
    edited, _ = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and edited['x1_rmse'] != moved['x1_rmse']
    _compare(model, va, edited, _step_by_step(model, va)[0], 'edited')
    va.x1 = va.x1.clone()                             # tensors replaced: captured again
    assert F._EvalGraph.get(model, va) is not ev


def test_averaged_parameters_and_mid_ramp_annealing(dev):
    from drvae_amd import fit as F
    model = _nb_both('drvae', dev, optim_alg='adamw', ema_decay=0.9, anneal_kl=True, anneal_kl_itermax=20)
    va = _dataset('drvae', 'nb', 48, 7, dev)
    batch = tuple(getattr(va, f) for f in va.FIELDS)
    for _ in range(6):
        model.run_on_batch(train_mode=True, **model._batch_kwargs(batch))
    live, _ = model.evaluate_performance_on_dataset(va)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None
    _compare(model, va, live, _step_by_step(model, va)[0], 'mid-ramp')
    with model.averaged_parameters():
        avg, _ = model.evaluate_performance_on_dataset(va)
        assert F._EvalGraph.get(model, va) is ev
        _compare(model, va, avg, _step_by_step(model, va)[0], 'averaged')
    assert avg['x1_ll'] != live['x1_ll']


def test_a_wide_model_beyond_the_gaussian_pass(dev):
    from drvae_amd import fit as F
    import drvae_amd.kernels as K
    X = 1028
    assert X > K.RECON_ROWS_MAX_X
    model = _nb_both('vfae', dev, dim_x=X)
    va = _dataset('vfae', 'nb', 48, 8, dev, X)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert txt == txt_ref
    _compare(model, va, got, ref, 'wide')


def test_fit_on_a_device_batcher_evaluates_through_graphs(dev, tmp_path):
    from drvae_amd import data as D
    import drvae_amd.kernels as K
    model = _nb_both('drvae', dev, epochs=2)
    model.w2log = lambda *a: None
    tr, va = _dataset('drvae', 'nb', 64, 1, dev), _dataset('drvae', 'nb', 32, 2, dev)
    calls, real = [], K.recon_rows
    K.recon_rows = lambda *a, **kw: (calls.append((kw.get('kind'), kw.get('size_from') is not None)), real(*a, **kw))[1]
    try:
        model.fit(D.DeviceBatcher(tr, D.compute_balanced_weights(np.arange(64) % 5), 16, seed=3), _loader(va, 8), add_noise=False,
                  verbose=False, early_stop=False, model_filename=str(tmp_path / 'b.pth'))
    finally:
        K.recon_rows = real
    # two datasets x (warm-up + capture) x (x1, x2): launched while the graphs were built, never again by the replays
    assert calls == [('nb', True)] * 8, calls
    assert len(model._eval_graphs) == 2 and all(e.graph is not None for e in model._eval_graphs.values())


# ----------------------------------------------------------------------------------- 3. two ranks on one GPU
def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK='0', DRVAE_DIST_BACKEND='gloo', DRVAE_SIDE_CUS='64')
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dev = torch.device('cuda', 0)
        model = _nb_both('drvae', dev)
        ds = _dataset('drvae', 'nb', 96, 9, dev)
        assert model.enable_data_parallel() == (rank, world)
        eng = model.engine()
        ctr = eng.rng_ctr.clone()
        out = {}
        for tag, shard in (('sharded', True), ('whole', False)):
            model.shard_evaluation = shard
            eng.rng_ctr.copy_(ctr)
            perf, txt = model.evaluate_performance_on_dataset(ds)
            out[tag] = {k: float(v) for k, v in perf.items() if k not in ('losses', 'model_class')}
            out[tag].update({'loss_' + k: float(v) for k, v in perf['losses'].items()})
            if shard:
                ev = model._eval_graphs[id(ds)]
                out['rows'] = (ev.lo, ev.hi) if ev.dp is not None else None
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:      # noqa: BLE001 -- the parent reports it
        import traceback
        q.put((rank, 'rank %d: %s\n%s' % (rank, e, traceback.format_exc())))


def test_sharded_evaluation_of_a_count_model_equals_the_one_rank_evaluation(dev):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29650 + (os.getpid() * 5) % 200
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r, o in got:
        assert isinstance(o, dict), o
    r0, r1 = got[0][1], got[1][1]
    assert r0['rows'] == (0, 48) and r1['rows'] == (48, 96)
    for r in (r0, r1):
        a, b = r['sharded'], r['whole']
        assert set(a) == set(b)
        for k in a:
            if k.startswith('loss_'):
                assert abs(a[k] - b[k]) <= 2e-5 * max(1.0, abs(b[k])), (k, a[k], b[k])
            elif k.startswith('y_'):
                assert a[k] == b[k], (k, a[k], b[k])
            elif np.isnan(b[k]):
                assert np.isnan(a[k]), k
            else:
                assert abs(a[k] - b[k]) <= 1e-6 * max(1.0, abs(b[k])), (k, a[k], b[k])
    assert r0['sharded'] == r1['sharded']
