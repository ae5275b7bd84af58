"""CPU: the gene-wise inverse dispersion of the 'nb' / 'zinb' decoders (``dispersion='gene'``) -- the bounds of
``tests/gene_disp_ref.py`` against fp32 emulations of the launch (a careful one inside, six faulty ones caught), the refusals of
the C entry point without a launch, the launcher module against its stand-in, construction and refusals, 'gene-cell' as the
code stood, the fused step on stand-ins against the model-level float64 reference, host-fed == feed, a state round trip, data
parallelism over gloo and ``fit``.  The kernel itself: ``tests/test_gpu_gene_disp.py``."""
import ctypes as C_
import inspect
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import gene_disp_ref as GR
from tests import kernel_ref
from tests import nb_ref as R
from tests import zinb_ref as Z
from tests.golden import cases as C
from tests.test_dropout_cpu import tiny_model
from tests.test_nb_cpu import LR, close, make_engine, set_batch

SWITCHES = {'off': {}, 'log1p': dict(x_transform='log1p'), 'lib': dict(library_size=True),
            'both': dict(x_transform='log1p', library_size=True), 'norm': dict(x_transform='log1p_norm', library_size=True)}
FAMILIES = ('nb', 'zinb')
# a step whose rows come from fp32 arithmetic (the careful emulation; the GPU): losses / gradients not compared / parameters --
# the tolerances every fp32 step of the count decoders is held to (``tests/test_gpu_counts.py``)
FP32_TOL = ((1e-4, 2e-5), None, (2e-4, 5e-5))


# ------------------------------------------------------------------------------------- 1. the bound on the edge grids
COLS = 6 * 172          # 1032 genes: two chunks, the second 8 wide; theta cycles through ``nb_ref.THETAS`` by column


def gene_grid(family):
    """the edge grids of ``nb_ref`` / ``zinb_ref`` laid out for a per-gene theta: column g carries theta THETAS[g % 6], the
    (mean, count) cases walk along the rows; 'zinb': crossed with the logits, each block as it is and with every count 0.
    Returns fp32 numpy (x, mu, raw, logit or None, coef)"""
    mus = np.concatenate([np.log1p(np.exp(-np.abs(R.A_M))) + np.maximum(R.A_M, 0) + R.MU_SHIFT, np.asarray(R.MU_EXTRA)])
    per_row = COLS // 6
    rows = -(-mus.size * len(R.COUNTS) // per_row)
    k = np.arange(rows)[:, None] * per_row + (np.arange(COLS) // 6)[None, :]
    mu = mus[k % mus.size].astype(np.float32)
    x = np.asarray(R.COUNTS)[(k // mus.size) % len(R.COUNTS)].astype(np.float32)
    th = np.asarray(R.THETAS)[np.arange(COLS) % 6]
    y = th - R.THETA_SHIFT
    raw = np.where(y > 30, y, np.log(np.expm1(np.clip(y, 1e-300, 30)))).clip(-30, None).astype(np.float32)
    logit = None
    if family == 'zinb':
        xs, ms, ls = [], [], []
        for l in Z.LOGITS:
            for zero in (False, True):
                xs.append(np.zeros_like(x) if zero else x), ms.append(mu), ls.append(np.full_like(x, l))
        x, mu, logit = np.concatenate(xs), np.concatenate(ms), np.concatenate(ls)
    coef = np.asarray([1.0, -0.5, 2.0, 0.25], np.float32)[np.arange(x.shape[0]) % 4]
    return x, mu, raw, logit, coef


@pytest.fixture(scope='module', params=[(f, l) for f in FAMILIES for l in (False, True)], ids=lambda p: '%s%s' % (p[0], '-lib' if p[1] else ''))
def grid(request):
    family, library = request.param
    x, mu, raw, logit, coef = gene_grid(family)
    Mr = x.shape[0]
    xidx = np.arange(Mr)[::-1].copy()            # every row reads another row's target
    # (library: rows scaled so that the size factors differ from row to row; the totals pass 2^24, so s comes from the
    # emulation -- the float64 total rounded once -- and the reference is handed the same s)
    rb = 5
    assert GR.blocks(Mr, rb)[-1][1] - GR.blocks(Mr, rb)[-1][0] < GR.blocks(Mr, rb)[0][1] - GR.blocks(Mr, rb)[0][0]
    kw = dict(logit=logit, coef=coef, library=library, xidx=xidx, row_blocks=rb)
    careful = GR.emulate(family, x, mu, raw, **kw)
    t = torch.from_numpy
    ref = GR.reference(family, t(x[xidx]), t(mu), t(raw), None if logit is None else t(logit), coef=t(coef), library=library,
                       s=careful['size'])
    assert ref['parts'].shape[1] == 2
    return dict(family=family, library=library, x=x, mu=mu, raw=raw, kw=kw, ref=ref, coef=coef, careful=careful)


def test_careful_emulation_of_the_launch_stays_inside_every_bound(grid):
    e = GR.excess(grid['careful'], grid['ref'], grid['coef'])
    print('%s%s careful emulation, worst |err| / bound: ' % (grid['family'], ' lib' if grid['library'] else '')
          + '  '.join('%s %.3g' % kv for kv in e.items()))
    assert all(v <= 1 for v in e.values()), e


@pytest.mark.parametrize('fault', GR.FAULTS)
def test_each_faulty_emulation_lands_outside(grid, fault):
    if fault == 'wrong_s' and not grid['library']:      # (no size factor in the unscaled kinds: nothing to get wrong)
        same = GR.emulate(grid['family'], grid['x'], grid['mu'], grid['raw'], fault=fault, **grid['kw'])
        assert all(np.array_equal(same[k], grid['careful'][k]) for k in ('parts', 'gm', 'ws'))
        return
    e = GR.excess(GR.emulate(grid['family'], grid['x'], grid['mu'], grid['raw'], fault=fault, **grid['kw']), grid['ref'], grid['coef'])
    print('%s%s %s, |err| / bound: ' % (grid['family'], ' lib' if grid['library'] else '', fault) + '  '.join('%s %.3g' % kv for kv in e.items()))
    assert max(e.values()) > 1, (fault, e)
    if fault in ('no_coef', 'no_slope', 'no_clear', 'seam'):
        assert e['ws'] > 1, 'a fault of the theta sum shows in the theta sum'


def test_theta32_is_the_head_at_a_zero_product():
    th = GR.theta32(torch.zeros(3))
    assert th.dtype == torch.float32 and float(th[0]) == pytest.approx(np.log(2.0) + 1e-3, rel=1e-7)
    # far below zero the shift is all that is left; far above, the pre-activation itself
    assert float(GR.theta32(torch.tensor([-200.0]))[0]) == np.float32(1e-3)
    assert float(GR.theta32(torch.tensor([50.0]))[0]) == np.float32(50.001)


# --------------------------------------------------------------------- 2. refusals at the C level, without a launch
A, ODD = 0x10000, 0x10004       # addresses that are looked at and never dereferenced


def _desc(kind='nb', M=0, X=2052, grad=True, **over):
    from drvae_amd import _lib
    zi = kind.startswith('zinb')
    d = dict(coef=A if grad else None, x=A, ldx=X, xidx=None, mu=A, sd=A if zi else None, ldp=X, M=M, X=X, shift=1e-6, out_part=A,
             chunks=-(-X // 1024), dmu=A if grad else None, dsd=A if (grad and zi) else None, ldd=X, ws=A if grad else None,
             ldw=X if grad else 0, row_blocks=1, kind=_lib.REC_KIND[kind], theta_raw=A, size=A if kind.endswith('_lib') else None)
    d.update(over)
    return _lib.NllRawCs(**d)


@pytest.mark.parametrize('M', [0, 4])
def test_the_entry_point_refuses_before_any_launch(M):
    from drvae_amd import _lib
    lib = _lib.load()
    call = lambda d: lib.dv_gauss_nll_rows_raw_cs(C_.byref(d), None)
    for kind in ('nb', 'nb_lib', 'zinb', 'zinb_lib'):
        if M == 0:      # (nothing to do and nothing wrong: 0, without a launch -- with rows the same call would launch)
            assert call(_desc(kind, M)) == 0 and call(_desc(kind, M, grad=False)) == 0
        zi = kind.startswith('zinb')
        bad = [dict(theta_raw=None), dict(sd=None if zi else A), dict(bias_mu=A), dict(bias_sd=A), dict(sd_off=4),
               dict(chunks=2), dict(chunks=4), dict(row_blocks=0), dict(row_blocks=max(M, 1) + 1), dict(ldw=2051), dict(coef=None),
               dict(ws=None), dict(dmu=None), dict(x=None), dict(mu=None), dict(out_part=None), dict(X=0, chunks=0),
               dict(dsd=None if zi else A)]
        if kind.endswith('_lib'):
            bad.append(dict(size=None))
        for over in bad:
            assert call(_desc(kind, M, **over)) == -1, (kind, over)
        assert call(_desc(kind, M, grad=False, ws=A)) == -1 and call(_desc(kind, M, grad=False, dsd=A)) == -1
    for k in (1, 3, 7, -1):      # Poisson, its library kind, past the table, negative: no such pass
        assert call(_lib.NllRawCs(**dict({f[0]: getattr(_desc('nb', M), f[0]) for f in _lib.NllRawCs._fields_}, kind=k))) == -1
    # one chunk: a library kind forms s itself, ``size`` is optional
    assert call(_desc('nb_lib', 0, X=1024, size=None)) == 0 and call(_desc('zinb_lib', 0, X=978, size=None)) == 0
    # all three new fields zero: the Gaussian pass and ITS checks, as ever (4 | X there; a count kind takes any X >= 1)
    gauss = lambda X: _lib.NllRawCs(coef=A, x=A, ldx=8, mu=A, sd=A, ldp=8, M=0, X=X, out_part=A, chunks=1, dmu=A, dsd=A, ldd=8,
                                    bias_mu=A, bias_sd=A, ws=A, ldw=16, sd_off=8, row_blocks=0)
    assert call(gauss(8)) == 0 and call(gauss(6)) == -1
    assert call(_desc('nb', 0, X=6, ldw=6)) == 0
    assert _lib.ABI_VERSION == 13 and len(_lib.SIGNATURES) == 84


def test_the_launcher_module_and_its_stand_in_agree():
    """every public function of ``drvae_amd.gene_rows`` has a stand-in in ``tests/gene_disp_ref.py`` with the same positional
    parameters, and every keyword of the launcher binds in the stand-in (and the other way round)"""
    import drvae_amd.gene_rows as G
    public = sorted(n for n, f in vars(G).items() if inspect.isfunction(f) and f.__module__ == G.__name__ and not n.startswith('_'))
    assert public == sorted(GR.FUNCTIONS)
    for name in public:
        a, b = inspect.signature(getattr(G, name)), inspect.signature(getattr(GR, name))
        pos = lambda s: [p.name for p in s.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        kws = lambda s: sorted(p.name for p in s.parameters.values() if p.kind == p.KEYWORD_ONLY)
        assert pos(a) == pos(b) and kws(a) == kws(b), name
    assert G.shape(900, 978) == GR.shape(900, 978) and G.shape(7, 2052, 3) == (3, 3)
    # the rule: within [1, M], at least MIN_ROWS rows a block where M allows, about TARGET_WORKGROUPS workgroups
    for Mr, X in ((1, 1), (3, 978), (900, 978), (2048, 20000), (8192, 20000), (100000, 978)):
        rb = G.row_blocks_for(Mr, X)
        assert 1 <= rb <= Mr and (Mr < G.MIN_ROWS or -(-Mr // rb) >= G.MIN_ROWS) and rb <= -(-G.TARGET_WORKGROUPS // -(-X // 1024))
    with pytest.raises(ValueError, match="'nb' or 'zinb'"):
        G.gene_rows(torch.zeros(1, 1), torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(4), kind='poisson')


# ------------------------------------------------------------------------------- 3. construction and refusals
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_build_the_gene_wise_decoder(kind, family, monkeypatch):
    GR.install(monkeypatch)
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    torch.manual_seed(0)
    model = tiny_model(kind, type_rec=family, dispersion='gene')
    dt = model.decoder_x.decoder_t
    assert type(dt) is blk.GeneDispersion and not any(isinstance(m_, torch.nn.Linear) for m_ in dt.modules())
    assert [n for n, _ in dt.named_parameters()] == ['raw_theta'] and tuple(dt.raw_theta.shape) == (13,)
    assert torch.equal(dt.raw_theta.detach().cpu(), torch.zeros(13))
    keys = [k for k in model.state_dict() if k.startswith('decoder_x.decoder_')]
    want = [GR.RAW, 'decoder_x.decoder_m.linear_m.weight', 'decoder_x.decoder_m.linear_m.bias']
    if family == 'zinb':
        want += ['decoder_x.decoder_d.linear_d.weight', 'decoder_x.decoder_d.linear_d.bias']
    assert keys == want and list(model.state_dict()) == list(E.param_shapes(model._step_config()))
    # no random draw is consumed: every other parameter starts as the 'gene-cell' model's of the same seed
    cell = tiny_model(kind, type_rec=family)
    sd, sc = model.state_dict(), cell.state_dict()
    assert all(torch.equal(sd[k], sc[k]) for k in sd if k != GR.RAW and 'decoder_d' not in k)
    cfg = model._step_config()
    assert cfg.dispersion == 'gene' and cfg.rec.gene and len(cfg.rec.heads) == (2 if family == 'zinb' else 1)
    a = model.engine().arena
    assert a.shapes[GR.RAW] == (13,) and a.p(GR.RAW).data_ptr() == dt.raw_theta.data_ptr()
    if family == 'zinb':      # [mu | a_d] back to back, the vector in front of them, the heads the arena's tail
        q = 'decoder_x.decoder_%s.linear_%s.%s'
        for leaf in ('weight', 'bias'):
            assert a.offsets[q % ('d', 'd', leaf)] == a.offsets[q % ('m', 'm', leaf)] + a.numel(q % ('m', 'm', leaf))
    assert a.offsets[GR.RAW] < a.offsets['decoder_x.decoder_m.linear_m.weight']
    assert model.engine()._side_adam_layout()[0] == cell.engine()._side_adam_layout()[0]
    # inference: px1 keeps its shape, theta expanded over the rows: log 2 + 1e-3 at the start
    res = model.forward(torch.ones(4, 13))
    assert len(res['px1']) == (3 if family == 'zinb' else 2) and all(tuple(t.shape) == (4, 13) for t in res['px1'])
    assert float(res['px1'][1].min()) == float(res['px1'][1].max()) == pytest.approx(np.log(2.0) + 1e-3, rel=1e-6)
    rec = model.reconstruct(x1=torch.ones(4, 13))
    assert rec[1][1].shape == (4, 13)
    # WeightNorm does not apply to a vector; dropout puts nothing in front of it
    wn = tiny_model(kind, type_rec=family, dispersion='gene', weight_norm=True)
    assert not any(k.startswith('decoder_x.decoder_t') and k != GR.RAW for k in wn.state_dict())
    assert list(wn.state_dict()) == list(E.param_shapes(wn._step_config()))
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        drop = tiny_model(kind, type_rec=family, dispersion='gene', dropout_rate=0.25)
    assert not hasattr(drop.decoder_x.decoder_t, 'dropout')


def test_refusals_on_the_models_the_blocks_and_the_config():
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    for kind in ('drvae', 'pvae', 'vfae'):
        for tr in ('diag_gaussian', 'binary', 'poisson'):
            with pytest.raises(ValueError, match="dispersion='gene' is for"):
                tiny_model(kind, type_rec=tr, dispersion='gene')
        with pytest.raises(ValueError, match="'gene-cell' or 'gene'"):
            tiny_model(kind, type_rec='nb', dispersion='cell')
    for tr in ('diag_gaussian', 'binary', 'poisson'):
        with pytest.raises(ValueError, match="dispersion='gene' is for"):
            E.StepConfig(type_rec=tr, dispersion='gene')
    with pytest.raises(ValueError, match="'gene-cell' or 'gene'"):
        E.StepConfig(type_rec='nb', dispersion=None)
    for cls in (blk.NegativeBinomialDecoder, blk.ZeroInflatedNegativeBinomialDecoder):
        with pytest.raises(ValueError, match="'gene-cell' or 'gene'"):
            cls([5], [8], 13, dispersion='per-gene')
        assert cls([5], [8], 13, dispersion='gene').decoder_t.raw_theta.shape == (13,)
    assert E.StepConfig(type_rec='nb').dispersion == 'gene-cell' and not E.StepConfig(type_rec='zinb').rec.gene
    assert E.StepConfig(type_rec='zinb', dispersion='gene').rec.heads[1].act == 'identity'


@pytest.mark.parametrize('family', FAMILIES)
def test_gene_cell_is_the_model_as_it_stood(family):
    """the default and the explicit 'gene-cell' build the same modules, keys, bits and step configuration; the launch lists of
    the 'gene-cell' steps are pinned by ``tests/test_zinb_cpu.py`` / ``tests/test_depth_cpu.py``, untouched"""
    from drvae_amd import engine as E
    a, b = tiny_model('drvae', type_rec=family), tiny_model('drvae', type_rec=family, dispersion='gene-cell')
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert a._step_config() == b._step_config() and [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert 'decoder_x.decoder_t.linear_t.weight' in a.state_dict() and GR.RAW not in a.state_dict()
    assert E.rec_family(family) is E.REC_FAMILIES[family] and E.REC_FAMILIES[family].gene is False


def test_block_level_path_broadcasts_theta_and_sums_its_gradient():
    """the explicit path: theta is the broadcast view, and autograd's gradient of ``raw_theta`` is the column sum of the theta
    block's gradient -- checked against the float64 reference's ``ws``"""
    from drvae_amd import blocks as blk
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.poisson(3.0, (6, 13)).astype(np.float32))
    mu = torch.from_numpy(rs.uniform(0.5, 5, (6, 13)).astype(np.float32))
    dec = blk.NegativeBinomialDecoder([5], [8], 13, dispersion='gene')
    with torch.no_grad():
        dec.decoder_t.raw_theta.copy_(torch.from_numpy(rs.normal(0, 1, 13).astype(np.float32)))
    th = dec.decoder_t(6)
    assert tuple(th.shape) == (6, 13) and th.stride(0) == 0
    dec.logp_perx(x, mu, th).sum().backward()
    ref = GR.reference('nb', x, mu, dec.decoder_t.raw_theta.detach(), coef=torch.ones(6))
    close(dec.decoder_t.raw_theta.grad, ref['ws'].numpy(), 2e-4, 2e-5)
    close(th.detach()[0], ref['theta'].numpy(), 2e-7, 0)


# ----------------------------------------------------------------------- 4. the fused step on the stand-ins
def _case(family, kind, sw, **over):
    nz = 0.01 if SWITCHES[sw] else 0.0
    if over.pop('use_s', False):
        from tests.test_zinb_cpu import _use_s_case
        spec, batch = _use_s_case(kind, add_noise_var=nz, **over)
    else:
        spec = C.tiny_spec(kind, add_noise_var=nz, learning_rate=LR, **over)
        batch = CR.count_batch(spec, 16, seed=3)
    if family == 'zinb':
        for k in ('x1', 'x2'):      # zero-inflate: a third of the entries
            batch[k] = batch[k] * (np.random.RandomState(5).rand(*batch[k].shape) > 0.33).astype(np.float32)
    return spec, batch


def _ref(family, spec, sw, **riders):
    kw = dict(SWITCHES[sw])
    if kw.get('x_transform') == 'log1p_norm':
        return GR.ModelRef(family, spec, seed=9, norm=True, library_size=kw['library_size'], **riders)
    return GR.ModelRef(family, spec, seed=9, **kw, **riders)


CASES = [('plain', 'off'), ('plain', 'log1p'), ('plain', 'lib'), ('plain', 'both'), ('weight_norm', 'both'), ('use_s', 'both'),
         ('universal', 'both'), ('universal', 'off')]


def run_against_reference(family, kind, variant, sw, dev='cpu', tol=((2e-5, 2e-6), (3e-4, 2e-6), (1e-4, 2e-5))):
    """losses and gradients of a train-mode pass with input noise, then three Adam steps at 16 rows, against the model-level
    float64 reference (the tolerances of ``tests/test_counts_cpu.py`` on float64 stand-ins); returns the engine"""
    spec, batch = _case(family, kind, sw, weight_norm=variant == 'weight_norm', use_s=variant == 'use_s')
    ref = _ref(family, spec, sw)
    params = ref.engine_params()
    eng, arena = make_engine(spec, params, dev, type_rec=family, dispersion='gene', **SWITCHES[sw])
    assert set(arena.shapes) == set(params) and GR.RAW in params
    eng.universal = variant == 'universal'
    set_batch(eng, batch, dev)
    p, X = eng.plan, spec.dim_x
    nh = 2 if family == 'zinb' else 1
    assert p.universal == (variant == 'universal') and p.DPX.shape[1] == nh * X and p.c_decx.out[-1].shape[1] == nh * X
    from drvae_amd.schedule import TRAIN, heads_route
    r = heads_route(eng, p, TRAIN)
    assert r.nll == 'gene' and r.rows == 'NLLG' and not r.raw_last and not r.x3 and not r.db_done
    noise = M.make_noise(spec, 16, seed=4)
    want, _ = ref.loss(batch, noise, True)
    with ref.context():
        want['CMPL'].backward()
    eng.training = True
    eng.set_noise(noise)
    eng.forward()
    eng.backward()
    for k, v in eng.losses().items():
        close(v, float(want[k].detach()), *tol[0])
    if tol[1] is not None:
        for k, g in ref.grads().items():
            close(arena.g(k), g, *tol[1])
    assert float(np.abs(ref.grads()[GR.RAW]).max()) > 1e-3
    for prm in ref.tr.params.values():
        prm.grad = None
    for step in range(3):
        nzs = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nzs)
        eng.train_step(nzs)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), *tol[0])
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    return eng


@pytest.mark.parametrize('variant,sw', CASES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_matches_the_float64_model_reference(family, kind, variant, sw, monkeypatch):
    GR.install(monkeypatch, exact=True)
    run_against_reference(family, kind, variant, sw)
    lib = bool(SWITCHES[sw].get('library_size'))
    assert (GR.CALLS['gene_rows_lib'] > 0) == lib and (GR.CALLS['gene_rows'] > 0) == (not lib)
    assert all(kernel_ref.CALLS[k] == 0 for k in ('nb', 'zinb', 'zinb_lib', 'lib_rows', 'other'))      # no theta-head launch


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_with_the_depth_normalised_feed(kind, monkeypatch):
    GR.install(monkeypatch, exact=True)
    run_against_reference('nb', kind, 'plain', 'norm')


@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_on_the_fp32_emulation_of_the_launch(family, monkeypatch):
    """the same step with the launch's careful fp32 emulation as its stand-in, held to the fp32 steps' tolerances"""
    GR.install(monkeypatch)
    run_against_reference(family, 'drvae', 'plain', 'both', tol=FP32_TOL)


COMBINED = dict(dropout_rate=0.25, max_grad_norm=1.0, anneal_kl=True, anneal_kl_itermax=10, ema_decay=0.9)


def combined_against_reference(family, dev='cpu', tol=((2e-5, 2e-6), None, (1e-4, 2e-5)), steps=3):
    """dropout (column masks), clipping at a norm the gradients exceed, KL annealing and the parameter average TOGETHER with both
    count switches, DrVAE, against the reference with its riders on: the vector is clipped, decayed and averaged like any
    parameter"""
    from tests.test_dropout_cpu import column_masks
    spec, batch = _case(family, 'drvae', 'both')
    rid = {k: v for k, v in COMBINED.items() if k != 'dropout_rate'}
    base = _ref(family, spec, 'both').engine_params()
    eng, arena = make_engine(spec, base, dev, type_rec=family, dispersion='gene', **SWITCHES['both'], **COMBINED)
    set_batch(eng, batch, dev)
    sites = eng.dropout_sites()
    assert eng.plan.universal and len(sites) == 4 and all(s['layer'] == 1 for s in sites)
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (sites[i]['M'], 1)) for i, m in cols.items()})
    ref = _ref(family, spec, 'both', sched=dict(anneal_kl=True, anneal_kl_itermax=rid['anneal_kl_itermax']),
               max_grad_norm=rid['max_grad_norm'], ema_decay=rid['ema_decay'], keep=1.0 - COMBINED['dropout_rate'],
               cols={CR.chain_block(spec, s['chain']): cols[i] for i, s in enumerate(sites)})
    clipped = 0
    for step in range(steps):
        nz = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nz)
        eng.train_step(nz)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), *tol[0])
        st = eng.clip_stats()
        assert st['n_skipped'] == 0
        clipped += st['coef'] < 1.0
    assert clipped == steps, 'the threshold is one the gradients exceed'
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    for k, e in ref.averaged().items():
        close(arena.e(k), e, *tol[2])
    assert not torch.equal(arena.e(GR.RAW), arena.p(GR.RAW))
    return eng


@pytest.mark.parametrize('family', FAMILIES)
def test_combined_riders_match_the_float64_model_reference(family, monkeypatch):
    GR.install(monkeypatch, exact=True)
    combined_against_reference(family)


def host_fed_equals_feed(family, kind, dev, extra=None, steps=3, captured=False):
    """two engines from one set of weights: one trains on the graph-resident feed's batches, the other on the same rows through
    ``set_batch``; same seed, same Philox draws -- parameters, moments and losses agree bit for bit.  Both count switches on"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR)
    ds = GR.gp_dataset(kind, 48, 4, dev, zero_inflated=family == 'zinb')
    params = _ref(family, spec, 'off').engine_params()
    kw = dict(type_rec=family, dispersion='gene', x_transform='log1p', library_size=True, **(extra or {}))
    fed, a1 = make_engine(spec, params, dev, **kw)
    twin, a0 = make_engine(spec, params, dev, **kw)
    bat = D.DeviceBatcher(ds, torch.ones(48), 16, seed=5, mode='sampler')
    bat.bind(fed)
    bat.begin_epoch()
    twin.universal = True
    table = fed.plan.live_feed.table.cpu().numpy()
    losses = []
    for b in range(steps):
        if captured:
            if fed._graph_key is None:
                fed.capture()
                bat.rebase()
            fed.replay()
        else:
            fed.train_step()
        i = torch.from_numpy(table[b].astype(np.int64)).to(dev)
        g = lambda name: getattr(ds, name)[i] if hasattr(ds, name) else None
        twin.set_batch(ds.x1[i], g('x2'), ds.y[i], g('has_x2').cpu() if kind != 'vfae' else np.zeros(16, np.int64),
                       ds.has_y[i].cpu() if kind != 'pvae' else np.zeros(16, np.int64))
        twin.train_step()
        assert torch.equal(fed.plan.XT, twin.plan.XT) and torch.equal(fed.plan.XIN, twin.plan.XIN)
        assert fed.losses() == twin.losses()
        losses.append(fed.losses())
    assert all(torch.equal(getattr(a1, w), getattr(a0, w)) for w in ('param', 'exp_avg', 'exp_avg_sq'))
    assert all(np.isfinite(v) for l in losses for v in l.values())
    assert not torch.equal(a1.p(GR.RAW), torch.from_numpy(params[GR.RAW]).to(dev))
    return losses


@pytest.mark.parametrize('family', FAMILIES)
def test_host_fed_step_equals_feed_step_bit_for_bit(family, monkeypatch):
    GR.install(monkeypatch)
    host_fed_equals_feed(family, 'drvae', 'cpu')
    assert GR.CALLS['gene_rows_lib'] >= 6


def test_training_state_round_trip(monkeypatch, tmp_path):
    """``save_training_state`` / ``load_training_state`` carry the vector, its moments and its average like any parameter: a
    restored twin continues bit for bit"""
    GR.install(monkeypatch)
    from tests.test_fit import _loader
    mk = lambda: tiny_model('drvae', type_rec='zinb', dispersion='gene', x_transform='log1p', library_size=True, ema_decay=0.9, epochs=1)
    a = mk()
    a.w2log = lambda *args: None
    tr = GR.gp_dataset('drvae', 32, 1, zero_inflated=True)
    a.fit(_loader(tr, 8), _loader(tr, 8), add_noise=True, verbose=False, model_filename=str(tmp_path / 'best.pth'))
    path = str(tmp_path / 'state.pth')
    a.save_training_state(path)
    assert GR.RAW in torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    b = mk()
    b.w2log = a.w2log
    b.load_training_state(path)
    ea, eb = a.engine().arena, b.engine().arena
    assert bool(torch.isfinite(ea.param).all())
    assert torch.equal(ea.p(GR.RAW), eb.p(GR.RAW)) and float(ea.p(GR.RAW).abs().max()) > 0
    for w in ('param', 'exp_avg', 'exp_avg_sq', 'avg'):
        assert torch.equal(getattr(ea, w), getattr(eb, w)), w
    sd = a.state_dict()
    assert GR.RAW in sd and torch.equal(sd[GR.RAW], ea.p(GR.RAW))


# ------------------------------------------------------------------------ 5. two ranks on gloo == one process
DP_SW = dict(type_rec='zinb', dispersion='gene', x_transform='log1p', library_size=True)


def _install_refs():
    import drvae_amd.gene_rows as G
    import drvae_amd.kernels as K
    for name in kernel_ref.FUNCTIONS:
        setattr(K, name, getattr(kernel_ref, name))
    G.gene_rows = GR.gene_rows


def _dp_case(kind):
    spec, batch = _case('zinb', kind, 'both')
    n = 12
    batch = {k: v[:n].copy() for k, v in batch.items()}
    pat = 'acbdab' + 'ddcbbb'      # uneven group mix between the two shards
    hy = np.array([ch in 'ac' for ch in pat], np.int64)
    hx = np.array([ch in 'cd' for ch in pat], np.int64)
    batch.update(x2=np.floor(1.3 * batch['x1']).astype(np.float32) * hx[:, None].astype(np.float32), has_x2=hx, has_y=hy)
    noises = [M.make_noise(spec, n, seed=20 + i) for i in range(3)]
    return spec, batch, noises, _ref('zinb', spec, 'off').engine_params()


def _run_steps(spec, params, batch, noises, counts, allreduce, lo=None, hi=None):
    if lo is not None:
        batch = {k: v[lo:hi] for k, v in batch.items()}
        noises = [M.slice_noise(n, lo, hi) for n in noises]
    eng, arena = make_engine(spec, params, **DP_SW)
    t = lambda k: torch.from_numpy(batch[k].copy())
    eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'], counts=counts)
    out = []
    for noise in noises:
        eng.train_step(noise, allreduce=allreduce)
        out.append(arena.loss.clone().numpy())
    return np.stack(out), arena.param.clone().numpy(), arena.grad.clone().numpy(), arena.g(GR.RAW).clone().numpy()


def _worker(rank, world, port, kind, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    _install_refs()
    from drvae_amd import dist as D
    r, w, _ = D.init_from_env(backend='gloo')
    assert (r, w) == (rank, world)
    spec, batch, noises, params = _dp_case(kind)
    n = batch['x1'].shape[0]
    lo, hi = D.shard_rows(n, rank, world)
    counts = D.global_counts(batch['has_x2'][lo:hi], batch['has_y'][lo:hi], kind, spec.semi_supervised)
    res = _run_steps(spec, params, batch, noises, counts, D.allreduce_sum, lo, hi)
    q.put((rank, counts) + res)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_gloo_equal_one_process(monkeypatch):
    """each rank's column sum covers its rows; the existing all-reduce adds them: nothing new in the exchange"""
    from tests.test_dp_gloo import _free_port
    kind = 'drvae'
    GR.install(monkeypatch)
    spec, batch, noises, params = _dp_case(kind)
    single = _run_steps(spec, params, batch, noises, None, None)
    assert GR.CALLS['gene_rows_lib'] > 0 and np.isfinite(single[1]).all() and np.abs(single[3]).max() > 0
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, kind, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, counts, losses, prm, grad, graw in got:
        np.testing.assert_allclose(losses, single[0], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(grad, single[2], rtol=1e-4, atol=1e-6 * np.abs(single[2]).max())
        np.testing.assert_allclose(graw, single[3], rtol=1e-4, atol=1e-6 * np.abs(single[2]).max())
        np.testing.assert_allclose(prm, single[1], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(got[0][3], got[1][3])                          # replicas stay bit-identical


# -------------------------------------------------------------------------------------------------- 6. fit
@pytest.mark.parametrize('family', FAMILIES)
def test_fit_three_epochs_is_finite_and_reports(family, monkeypatch, tmp_path):
    """three epochs on Gamma-Poisson counts with a per-gene theta: finite losses and a finite held-out log-likelihood.
    REPORTED, not asserted: the held-out ``ll`` next to the 'gene-cell' model's and the rank correlation of learned and true
    theta (three epochs of a tiny model decide neither)"""
    import scipy.stats as st
    from tests.test_fit import _loader
    GR.install(monkeypatch)
    zi = family == 'zinb'
    tr, va = GR.gp_dataset('drvae', 64, 1, zero_inflated=zi), GR.gp_dataset('drvae', 32, 2, zero_inflated=zi)
    out = {}
    for disp in ('gene', 'gene-cell'):
        model = tiny_model('drvae', type_rec=family, dispersion=disp, x_transform='log1p', library_size=True, epochs=3)
        model.w2log = lambda *a: None
        model.fit(_loader(tr, 8), _loader(va, 8), add_noise=True, verbose=False, early_stop=True,
                  model_filename=str(tmp_path / ('best_%s.pth' % disp)))
        perf, _ = model.evaluate_performance_on_dataset(va)
        assert np.isfinite(perf['x1_ll']) and np.isfinite(perf['x2_ll']) and np.isfinite(float(perf['losses']['ELBO']))
        out[disp] = (model, perf)
    model, perf = out['gene']
    theta = model.decoder_x.decoder_t.theta().detach().cpu().numpy()
    assert np.all(np.isfinite(theta)) and np.all(theta > 0) and not np.allclose(theta, np.log(2.0) + 1e-3)
    rho = st.spearmanr(theta, GR.gene_theta(13, seed=1)).correlation
    print("%s: held-out x1_ll gene %.4f | gene-cell %.4f; Spearman(learned theta, true theta) = %.3f"
          % (family, perf['x1_ll'], out['gene-cell'][1]['x1_ll'], rho))
    # the evaluation's numbers are the decoder's: ll from the expanded theta
    res = model.forward(va.x1)
    px = model.decoder_x([res['z1']])
    s = model.size_factor(va.x1)
    with torch.no_grad():
        direct = float(model.decoder_x.logp_perx(va.x1, *px, size=s).mean())
    assert perf['x1_ll'] == pytest.approx(direct, rel=1e-6)
