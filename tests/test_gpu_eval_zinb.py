"""-m gpu: the zero-inflated kind of ``dv_recon_rows`` (``kernels.recon_rows(kind='zinb')``) against the float64 reference and
bounds of ``tests/eval_zinb_ref.py``, and the captured whole-set evaluation (``fit._EvalGraph``) of ``type_rec='zinb'`` models
(with the raw-count switches) against the step-by-step evaluation ``model._evaluate`` and a float64 evaluation of the same
formulas.  The model tests mirror the negative binomial's in ``tests/test_gpu_eval_counts.py`` at their sizes."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import counts_ref as CR
from tests import eval_counts_ref as ER
from tests import eval_zinb_ref as EZ
from tests import ref64
from tests import zinb_ref as Z
from tests.test_counts_cpu import SWITCHES
from tests.test_fit import _loader, _tiny_model
from tests.test_gpu_eval_counts import _guarded, _guarded_vec, _outside_untouched

pytestmark = pytest.mark.gpu

MS = (1, 3, 9)
# one lane; under a quad; one quad; odd; 16; around the scalar walk's trip boundary (256 threads); around the 16-byte walk's
# (256 quads); a third trip of the 16-byte walk
XS = (1, 3, 4, 13, 16, 255, 256, 257, 1020, 1024, 1028, 2052)
SW = dict(SWITCHES, norm_lib=dict(x_transform='log1p_norm', library_size=True))
PROFILE = {}        # worst fraction of the bound per (case, output), as the kernel tests measure it


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    assert _lib.RECON_ZINB == 4
    return K


# ------------------------------------------------------------------------------------------ guarded operands
def _launch(K, dev, x, mu, th, a, size, *, misalign=False, want_ll=True, rec=True, kind='zinb'):
    """one guarded launch -> dict(rows, ll, rec) on the host: every operand a view inside a NaN-filled buffer with guard rows
    and NaN pads; ``sd`` the (M, 2X) pair [theta | logit] in ONE such buffer (``kind='nb'``: theta alone).  Guard bands and
    inputs are checked after the launch"""
    M, X = x.shape
    xg, xb = _guarded(x, dev, misalign)
    mg, mb = _guarded(mu, dev, misalign)
    tg, tb = _guarded(torch.cat([th, a], 1) if kind == 'zinb' else th, dev, misalign)
    same = size is not None and size is x
    sg, sb = (xg, xb) if same else (_guarded(size, dev, misalign) if size is not None else (None, None))
    rows, rowsb = _guarded_vec(M * 6, dev)
    rows = rows.view(M, 6)
    ll, llb = _guarded_vec(M, dev) if want_ll else (None, None)
    og, ob = _guarded(torch.zeros(M, X), dev, misalign) if (rec and size is not None) else (None, None)
    bufs = [(xg, xb), (mg, mb), (tg, tb), (rows.view(-1), rowsb)] + ([(sg, sb)] if sg is not None and not same else []) + \
        ([(ll, llb)] if ll is not None else []) + ([(og, ob)] if og is not None else [])
    before = [b.clone() for _, b in bufs]
    inputs = [xg.clone(), mg.clone(), tg.clone(), sg.clone() if sg is not None else None]
    K.recon_rows(rows, ll, xg, mg, tg, kind=kind, size_from=sg, rec_out=og)
    torch.cuda.synchronize()
    for (v, b), b0 in zip(bufs, before):
        assert _outside_untouched(v, b, b0), 'a launch wrote outside its views'
    assert torch.equal(xg, inputs[0]) and torch.equal(mg, inputs[1]) and torch.equal(tg, inputs[2]), 'an input was written'
    assert sg is None or torch.equal(sg, inputs[3])
    out = dict(rows=rows.cpu(), ll=ll.cpu() if ll is not None else None, rec=og.cpu() if og is not None else None)
    for k, v in out.items():
        assert v is None or bool(torch.isfinite(v).all()), 'a pad reached %s' % k
    return out


def _check(tag, got, ref, keys=('rows', 'll', 'rec')):
    for k in keys:
        if got[k] is None:
            continue
        w = ref64.check('%s %s' % (tag, k), got[k], ref[k], ref[k + '_bound'])
        PROFILE[(tag.split()[0], k)] = max(PROFILE.get((tag.split()[0], k), 0.0), w)


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('variant', ['plain', 'scaled-own', 'scaled-other'])
def test_zero_inflated_rows_against_float64(variant, K, dev):
    """every shape x both paths (16-byte, and the scalar one forced by a misaligned base): rows, ll and the stored mean within
    their bounds, guard bands and inputs intact, two launches bit-equal"""
    scaled, other = variant != 'plain', variant == 'scaled-other'
    name = 'zinb-' + variant
    for M in MS:
        for X in XS:
            x, mu, th, a, size = EZ.case(M, X, seed=3, scaled=scaled, other=other)
            ref = EZ.reference(x, mu, th, a, size)
            for misalign in (False, True):
                tag = '%s M=%d X=%d misaligned=%d' % (name, M, X, misalign)
                got = _launch(K, dev, x, mu, th, a, size, misalign=misalign)
                assert (got['rec'] is not None) == scaled
                _check(tag, got, ref)
                again = _launch(K, dev, x, mu, th, a, size, misalign=misalign)
                for k in got:
                    assert got[k] is None or torch.equal(_bits(got[k]), _bits(again[k])), (tag, k)
    print('%s: worst fraction of the bound: rows %.3f  ll %.3f  rec %.3f' % (
        name, PROFILE.get((name, 'rows'), 0), PROFILE.get((name, 'll'), 0), PROFILE.get((name, 'rec'), 0)))


# --------------------------------------------------------------------------- 2. the evaluation's own call form
@pytest.mark.parametrize('X', [13, 16, 1028])
def test_the_evaluations_call_form_gives_the_same_bits(X, K, dev):
    """ONE (M, 3X) heads buffer [mu | theta | logit]: mu = buf[:, :X], sd = buf[:, X:], rec_out = mu -- with and without ``ll``:
    bit-equal to each other and to the launch on separate buffers (same path: X % 4 decides it for both)"""
    M = 5
    x, mu, th, a, size = EZ.case(M, X, seed=4, scaled=True, other=True)
    base = _launch(K, dev, x, mu, th, a, size)
    xd, sz = x.to(dev), size.to(dev)
    got = {}
    for want_ll in (True, False):
        buf = torch.cat([mu, th, a], 1).to(dev)
        tail0 = buf[:, X:].clone()
        rows, ll = torch.zeros(M, 6, device=dev), (torch.zeros(M, device=dev) if want_ll else None)
        K.recon_rows(rows, ll, xd, buf[:, :X], buf[:, X:], kind='zinb', size_from=sz, rec_out=buf[:, :X])
        torch.cuda.synchronize()
        assert torch.equal(buf[:, X:], tail0), 'theta or the logit was written'
        got[want_ll] = dict(rows=rows.cpu(), ll=ll.cpu() if want_ll else None, rec=buf[:, :X].cpu())
    assert torch.equal(_bits(got[True]['rows']), _bits(got[False]['rows'])) and torch.equal(_bits(got[True]['rec']), _bits(got[False]['rec']))
    for k in ('rows', 'll', 'rec'):
        assert torch.equal(_bits(got[True][k]), _bits(base[k])), (X, k)
    _check('zinb-callform X=%d' % X, got[True], EZ.reference(x, mu, th, a, size))


# ------------------------------------------------------------------------------------- 3. equality with kind 3
@pytest.mark.parametrize('scaled', [False, True])
def test_rows_and_the_stored_mean_are_the_negative_binomials(scaled, K, dev):
    """rows and rec_out bit-equal to ``kind='nb'`` on the same x, mu, theta and size source, for any logits; with every logit
    at -30 (pi = 1e-13) ``ll`` is the negative binomial's within the sum of both kinds' bounds.  (At a zero the two
    log-probabilities differ by log1p(pi (e^{-L0} - 1)): the means under the zeros are held at <= 1e-3 here, where that is
    below 1e-16 -- with L0 = -1e4 the zero-inflated term is log pi = -30, another number by right)"""
    for X in (13, 16, 257, 1028):
        x, mu, th, a, size = EZ.case(6, X, seed=5, scaled=scaled, other=True)
        for misalign in (False, True):
            nb = _launch(K, dev, x, mu, th, a, size, misalign=misalign, kind='nb')
            zi = _launch(K, dev, x, mu, th, a, size, misalign=misalign)
            for k in ('rows', 'rec'):
                assert (zi[k] is None and nb[k] is None) or torch.equal(_bits(zi[k]), _bits(nb[k])), (X, misalign, k)
        s = torch.from_numpy(CR.size_factor32(size))[:, None] if scaled else torch.ones(len(x), 1)
        mu0 = torch.where(x == 0, torch.minimum(mu, 1e-3 / s), mu)          # (the scaled mean under a zero: <= 1e-3)
        lo = torch.full_like(a, -30.0)
        nb = _launch(K, dev, x, mu0, th, lo, size, kind='nb')
        zi = _launch(K, dev, x, mu0, th, lo, size)
        rn, rz = ER.reference('nb', x, mu0, th, size), EZ.reference(x, mu0, th, lo, size)
        apart = (rn['ll'] - rz['ll']).abs()          # (what the two kinds differ by in float64: not an error of either launch)
        assert float(apart.max()) <= 1e-9, 'the case does not make the two kinds agree in float64'
        w = ref64.check('zinb at logit -30 against nb, X=%d' % X, zi['ll'], nb['ll'].double(), rn['ll_bound'] + rz['ll_bound'] + apart)
        print('logit -30 against nb, X=%d scaled=%d: %.3f of the two bounds' % (X, scaled, w))


# ------------------------------------------------------------------------------------------- 4. the edge grid
@pytest.mark.parametrize('scaled', [False, True])
def test_zero_inflated_edge_grid(scaled, K, dev):
    """``zinb_ref.edge_grid`` (mu = 1e-6 .. 1e4 x theta = 1e-3 .. 1e6 x counts 0 .. 30 000 x logits -30 .. 30, each block again
    with every count at zero), plain and scaled by a matrix of small counts with an all-zero row"""
    x, mu, th, a, _ = Z.edge_grid(X=256)
    size = None
    if scaled:
        rs = np.random.RandomState(5)
        size = torch.from_numpy(rs.poisson(rs.gamma(2.0, 2.0, tuple(x.shape))).astype(np.float32))
        size[0] = 0.0
    ref = EZ.reference(x, mu, th, a, size)
    got = _launch(K, dev, x, mu, th, a, size)
    assert bool(torch.isfinite(got['ll']).all())
    name = 'zinb-grid' + ('-scaled' if scaled else '')
    _check(name, got, ref)
    print('%s: worst fraction of the bound: rows %.3f  ll %.3f' % (name, PROFILE[(name, 'rows')], PROFILE[(name, 'll')]))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_launcher_refusals_on_the_device(K, dev):
    x, mu, th, a, size = [t.to(dev) for t in EZ.case(3, 8, scaled=True, other=True)]
    sd = torch.cat([th, a], 1)
    rows, ll = torch.zeros(3, 6, device=dev), torch.zeros(3, device=dev)
    keep = [t.clone() for t in (x, mu, sd, size)]
    with pytest.raises(RuntimeError, match='dv_recon_rows'):
        K.recon_rows(rows, ll, x, mu, sd, kind='zinb', rec_out=mu.clone())          # rec_out without a size source
    with pytest.raises(AssertionError):
        K.recon_rows(rows, ll, x, mu, th, kind='zinb', size_from=size)              # theta alone: no logit block
    with pytest.raises(AssertionError):
        K.recon_rows(rows, ll, x, mu, None, kind='zinb')
    with pytest.raises(AssertionError):
        K.recon_rows(rows, ll, x, mu, sd, kind='zinb', bias=(mu[0], mu[0]))
    with pytest.raises(RuntimeError, match='unit inner stride'):
        K.recon_rows(rows, ll, x, mu, torch.cat([th, a], 1).repeat_interleave(2, 1)[:, ::2], kind='zinb')
    torch.cuda.synchronize()
    assert float(rows.abs().sum()) == 0.0 and float(ll.abs().sum()) == 0.0
    assert all(torch.equal(t, k) for t, k in zip((x, mu, sd, size), keep))


# ------------------------------------------------------------------------------------------- 6. the models
def _model(kind, dev, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return _tiny_model(kind, device=dev, type_rec='zinb', add_noise_var=0.0, **kw)


def _dataset(kind, n, seed, dev, dim_x=13):
    """``zinb_ref.zi_dataset`` at depth 0.5 (gene means 0.5 .. 3.6: an untrained encoder reading RAW counts stays finite)"""
    return Z.zi_dataset(kind, n, seed, dev, X=dim_x, depth=0.5)


def _step_by_step(model, ds):
    g = lambda k: getattr(ds, k, None)
    return model._evaluate(g('x1'), g('x2'), g('s'), g('y'), g('has_x2'), g('has_y'))


def _float64_metrics(model, ds):
    """the reported reconstruction metrics in float64 from the fp32 heads ``model.forward`` returns (the zero-inflated
    log-likelihood: ``zinb_ref.logp64``), and the kernel-level bounds propagated to them -> ({key: value}, {key: bound})"""
    kind = model.kind
    s = getattr(ds, 's', [])
    res = model.forward(ds.x1, s)
    lib = bool(getattr(model, 'library_size', False))
    model.library_size = False
    try:
        heads = model.forward(ds.x1, s)          # (the unscaled heads: what the row pass is handed)
    finally:
        model.library_size = lib
    val, bnd = {}, {}
    for tag, key, x, idx in (('x1', 'px1', ds.x1, None),) + ((('x2', 'px2', ds.x2, torch.nonzero(ds.has_x2.reshape(-1)).reshape(-1)),)
                                                            if kind != 'vfae' else ()):
        if idx is not None and len(idx) == 0:
            continue
        sl = (lambda t: t.cpu() if idx is None else t[idx].cpu())
        xs, r, th, a = sl(x), sl(res[key][0]), sl(res[key][1]), sl(res[key][2])
        ll = Z.logp64(ref64.f64(xs), ref64.f64(r), ref64.f64(th), ref64.f64(a)).sum(1)
        kref = EZ.reference(xs, sl(heads[key][0]), th, a, sl(ds.x1) if lib else None)
        for k, v in ER.metrics64(xs, r, ll).items():
            val['%s_%s' % (tag, k)] = v
        for k, v in ER.metrics_bound(xs, r, kref['rows_bound'], kref['ll_bound']).items():
            bnd['%s_%s' % (tag, k)] = v
    return val, bnd


def _compare(model, ds, got, ref, tag):
    """the rule of ``tests/test_gpu_eval_counts.py::_compare``, key by key: nan where the step-by-step path has nan; else the
    captured value no farther from float64 than twice the step-by-step value's own distance plus the propagated kernel bound.
    Sampled loss terms loosely (another Philox draw); the MMD penalty's value as ``tests/test_gpu_eval_variants.py`` holds it"""
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
        frac = d_cap / (2 * d_ref + bnd[k]) if (2 * d_ref + bnd[k]) > 0 else (0.0 if d_cap == 0 else np.inf)
        PROFILE[('model', k[3:])] = max(PROFILE.get(('model', k[3:]), 0.0), frac)
        print('%-28s %-8s float64 %.10g  captured off by %.3g  step by step off by %.3g  kernel bound %.3g  (%.3f of the allowance)' % (
            tag, k, val[k], d_cap, d_ref, bnd[k], frac))
        assert d_cap <= 2 * d_ref + bnd[k], (tag, k, got[k], v, val[k], d_cap, d_ref, bnd[k])
    assert list(got['losses']) == list(ref['losses'])
    for k, v in ref['losses'].items():
        a, b = float(got['losses'][k]), float(v)
        assert np.isfinite(b), (k, b)
        if k == 'MMD':
            assert np.isfinite(a) and a <= 0 and b <= 0, (a, b)
        else:
            assert abs(a - b) <= 0.2 * max(1.0, abs(b)), (k, a, b)


CASES = [(kind, sw) for kind in ('drvae', 'pvae', 'vfae') for sw in (None, 'log1p', 'lib', 'both', 'norm_lib')]


@pytest.mark.parametrize('kind,sw', CASES, ids=['%s-%s' % c for c in CASES])
def test_captured_evaluation_of_zero_inflated_models(kind, sw, dev):
    from drvae_amd import fit as F
    dim_x = 16 if sw in ('both', 'norm_lib') else 13
    model = _model(kind, dev, dim_x=dim_x, **(SW[sw] if sw else {}))
    va = _dataset(kind, 48, 2, dev, dim_x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        ev = F._EvalGraph.get(model, va)
    assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
    assert ev is not None and ev.graph is not None, 'the captured path was not taken'
    assert ev.rec_kind == 'zinb' and ev.fam.recon_kind == 4
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and txt == txt_ref
    assert np.isfinite(got['x1_ll'])
    _compare(model, va, got, ref, '%s-zinb-%s' % (kind, sw))


# ------------------------------------------------------------------------------------- 7. evaluation behaviour
def _zinb_both(kind, dev, **kw):
    return _model(kind, dev, **dict(SWITCHES['both'], **kw))


def test_the_size_source_of_x2_is_x1(dev):
    """an x2 ten times as deep as x1: the x2 metrics are those at x1's size factor (``forward``'s), which a kernel scaling
    by the target's own depth misses by a factor"""
    model = _zinb_both('drvae', dev)
    va = _dataset('drvae', 48, 3, dev)
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
    model = _zinb_both('drvae', dev)
    va = _dataset('drvae', 48, 4, dev)
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
        model = VFAE(dim_x=13, dim_s=1, dim_y=2, dim_h_en_z1=[7], dim_h_de_x=[8], dim_z1=5, type_rec='zinb', nonlinearity='elu',
                     learning_rate=5e-3, L=2, weight_decay=0.01, add_noise_var=0.0, use_MMD=False, random_seed=5, epochs=2,
                     batch_size=8, dim_h_de_z1=[6], dim_h_en_z2=[6], dim_h_clf=[], dim_z2=4, semi_supervised=False, device=dev,
                     **SWITCHES['both'])
    va = _dataset('vfae', 48, 5, dev)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and ev.sel is not None
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert txt == txt_ref
    _compare(model, va, got, ref, 'sel')


def test_the_replay_follows_parameters_and_data(dev):
    from drvae_amd import fit as F
    model = _zinb_both('drvae', dev, epochs=2)
    va = _dataset('drvae', 48, 6, dev)
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
    model = _zinb_both('drvae', dev, optim_alg='adamw', ema_decay=0.9, anneal_kl=True, anneal_kl_itermax=20)
    va = _dataset('drvae', 48, 7, dev)
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


def test_nuisance_classes_with_the_grouped_mmd_penalty(dev):
    """``use_s`` (two classes, every class in every data group) with ``use_MMD``: the whole set's plan carries the classes on
    the device, the penalty comes from its grouped launches, the zero-inflated rows from the decoder conditioned on s"""
    from drvae_amd import fit as F
    model = _zinb_both('vfae', dev, use_s=True, dim_s=2, use_MMD=True, kernel_MMD='rbf_fourier', mmd_rate=1.0)
    va = _dataset('vfae', 48, 8, dev)
    va.s = torch.from_numpy(((np.arange(48) // 4 + np.arange(48) // 12) % 2).astype(np.int64)).to(dev)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and ev.graph is not None and ev.plan.carry_s and ev.plan.mmd_grouped is not None
    ref, txt_ref = _step_by_step(model, va)
    got, txt = model.evaluate_performance_on_dataset(va)
    assert txt == txt_ref and float(got['losses']['MMD']) < 0 and np.isfinite(got['x1_ll'])
    _compare(model, va, got, ref, 'use_s + mmd')
    va.s.copy_((va.s + 1) % 2)                        # classes edited in place: the same graph reads them
    edited, _ = model.evaluate_performance_on_dataset(va)
    assert F._EvalGraph.get(model, va) is ev and edited['x1_ll'] != got['x1_ll']
    _compare(model, va, edited, _step_by_step(model, va)[0], 'use_s edited')


def test_a_moved_model_drops_its_graphs(dev):
    """the graphs of a 'zinb' model live under a key of their own (``_EvalGraph.cache``); ``.cpu().cuda()`` retires the engine
    and drops them like every other model's, and the next evaluation captures again"""
    from drvae_amd import fit as F
    model = _zinb_both('drvae', dev)
    va = _dataset('drvae', 48, 6, dev)
    got, _ = model.evaluate_performance_on_dataset(va)
    ev = F._EvalGraph.get(model, va)
    assert ev is not None and F._EvalGraph.cache(model) == {id(va): ev} and not model.__dict__.get('_eval_graphs')
    model.cpu()
    model.cuda()
    assert not any(model.__dict__.get(k) for k in F._EvalGraph.CACHE_KEYS)
    again, _ = model.evaluate_performance_on_dataset(va)
    ev2 = F._EvalGraph.get(model, va)
    assert ev2 is not None and ev2 is not ev and ev2.graph is not None
    assert again['x1_rmse'] == pytest.approx(got['x1_rmse'], rel=1e-6) and again['x1_ll'] == pytest.approx(got['x1_ll'], rel=1e-6)


# ------------------------------------------------------------------------------------------------- 8. fit
def test_fit_on_a_device_batcher_never_evaluates_step_by_step(dev, tmp_path, monkeypatch):
    from drvae_amd import data as D
    import drvae_amd.kernels as K
    model = _zinb_both('drvae', dev, epochs=2)
    model.w2log = lambda *a: None
    tr, va = _dataset('drvae', 64, 1, dev), _dataset('drvae', 32, 2, dev)

    def _never(*a, **kw):
        raise AssertionError('the step-by-step evaluation was called')
    monkeypatch.setattr(model, '_evaluate', _never)
    calls, real = [], K.recon_rows
    monkeypatch.setattr(K, 'recon_rows', lambda *a, **kw: (calls.append((kw.get('kind'), kw.get('size_from') is not None,
                                                                           tuple(a[4].shape))), real(*a, **kw))[1])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        model.fit(D.DeviceBatcher(tr, D.compute_balanced_weights(np.arange(64) % 5), 16, seed=3), _loader(va, 8), add_noise=False,
                  verbose=False, early_stop=False, model_filename=str(tmp_path / 'b.pth'))
    assert not [m for m in w if 'could not be built' in str(m.message)], [str(m.message) for m in w]
    # two datasets x (warm-up + capture) x (x1, x2): launched while the graphs were built, never again by the replays
    assert calls == [('zinb', True, (64, 26))] * 4 + [('zinb', True, (32, 26))] * 4, calls
    from drvae_amd import fit as F
    graphs = F._EvalGraph.cache(model)
    assert len(graphs) == 2 and all(e.graph is not None for e in graphs.values())
    assert model.finished_training_iters == 2 * (64 // 16)


# ----------------------------------------------------------------------------------- 9. two ranks on one GPU
def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK='0', DRVAE_DIST_BACKEND='gloo', DRVAE_SIDE_CUS='64')
        import torch.distributed as dist
        from drvae_amd import fit as F
        torch.cuda.set_device(0)
        dev = torch.device('cuda', 0)
        model = _zinb_both('drvae', dev)
        ds = _dataset('drvae', 96, 9, dev)
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
            ev = F._EvalGraph.cache(model)[id(ds)]
            if shard:
                out['rows'] = (ev.lo, ev.hi) if ev.dp is not None else None
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:      # noqa: BLE001 -- the parent reports it
        import traceback
        q.put((rank, 'rank %d: %s\n%s' % (rank, e, traceback.format_exc())))


def test_sharded_evaluation_of_a_zero_inflated_model_equals_the_one_rank_evaluation(dev):
    import queue
    import time
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29850 + (os.getpid() * 5) % 200
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got, deadline = [], time.monotonic() + 240          # (each child's own limit; the parent stops at the first non-zero exit)
    try:
        while len(got) < len(procs):
            try:
                got.append(q.get(timeout=0.5))
                continue
            except queue.Empty:
                pass
            bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not bad, 'a rank exited with %s' % bad
            assert time.monotonic() < deadline, 'a rank ran into its time limit'
    finally:
        for p in procs:
            p.join(timeout=60 if len(got) == len(procs) else 0.1)
            if p.is_alive():
                p.kill()
    got.sort(key=lambda t: t[0])
    for r, o in got:
        assert isinstance(o, dict), o
    r0, r1 = got[0][1], got[1][1]
    assert r0['rows'] == (0, 48) and r1['rows'] == (48, 96)
    for r in (r0, r1):
        a, b = r['sharded'], r['whole']
        assert set(a) == set(b) and np.isfinite(a['x1_ll']) and np.isfinite(a['x2_ll'])
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
