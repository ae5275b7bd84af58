"""``dispersion='gene-batch'`` on the CPU: an inverse dispersion per (nuisance class, gene) -- the launch's emulation against the
float64 reference on the edge grid, its faulty variants, the C-level refusals, construction and refusals of the models, and the
fused step on the stand-ins (``tests/gene_batch_ref.py``) against the model-level float64 reference.  Without a GPU."""
import ctypes as C_
import inspect
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import gene_batch_ref as BR
from tests import gene_disp_ref as GR
from tests import kernel_ref
from tests.golden import cases as C
from tests.test_dropout_cpu import tiny_model
from tests.test_gene_disp_cpu import A, COMBINED, FP32_TOL, SWITCHES, _desc, gene_grid
from tests.test_nb_cpu import LR, close, make_engine, set_batch

FAMILIES = ('nb', 'zinb')
S3 = 3


# ------------------------------------------------------------------------------------- 1. the bound on the edge grid
@pytest.fixture(scope='module', params=[(f, l) for f in FAMILIES for l in (False, True)], ids=lambda p: '%s%s' % (p[0], '-lib' if p[1] else ''))
def grid(request):
    """the edge grid of ``test_gene_disp_cpu`` under three classes: class k's thetas are the grid's rolled by k columns, the rows
    are the decoder rows of a batch of 7 -- sample rows r -> r % 7, then pair rows -> pair_rows[j % 3] -- in five row blocks
    with a short last one; every row reads another row's target"""
    family, library = request.param
    x, mu, raw, logit, coef = gene_grid(family)
    Mr = x.shape[0]
    table = np.stack([np.roll(raw, k) for k in range(S3)])
    cls = np.asarray([0, 1, 2, 1, 0, 2, 1], np.int32)
    pair_from = (2 * Mr // 3) // 7 * 7
    pair_rows = np.asarray([1, 4, 6])
    src = np.concatenate([np.arange(pair_from) % 7, pair_rows[np.arange(Mr - pair_from) % 3]]).astype(np.int32)
    xidx = np.arange(Mr)[::-1].copy()
    rb = 5
    assert GR.blocks(Mr, rb)[-1][1] - GR.blocks(Mr, rb)[-1][0] < GR.blocks(Mr, rb)[0][1] - GR.blocks(Mr, rb)[0][0]
    kw = dict(logit=logit, coef=coef, library=library, xidx=xidx, cls_src=src, row_blocks=rb, pair_from=pair_from)
    careful = BR.emulate(family, x, mu, table, cls, **kw)
    t = torch.from_numpy
    ref = BR.reference(family, t(x[xidx]), t(mu), t(table), careful['cls'], None if logit is None else t(logit), coef=t(coef),
                       library=library, s=careful['size'], row_blocks=rb)
    assert ref['parts'].shape[1] == 2 and set(careful['cls']) == {0, 1, 2}
    return dict(family=family, library=library, x=x, mu=mu, table=table, cls=cls, kw=kw, ref=ref, coef=coef, careful=careful)


def test_careful_emulation_of_the_launch_stays_inside_every_bound(grid):
    e = BR.excess(grid['careful'], grid['ref'], grid['coef'])
    print('%s%s careful emulation, worst |err| / bound: ' % (grid['family'], ' lib' if grid['library'] else '')
          + '  '.join('%s %.3g' % kv for kv in e.items()))
    assert all(v <= 1 for v in e.values()), e


@pytest.mark.parametrize('fault', BR.FAULTS)
def test_each_faulty_emulation_lands_outside(grid, fault):
    bad = BR.emulate(grid['family'], grid['x'], grid['mu'], grid['table'], grid['cls'], fault=fault, **grid['kw'])
    e = BR.excess(bad, grid['ref'], grid['coef'])
    print('%s%s %s, |err| / bound: ' % (grid['family'], ' lib' if grid['library'] else '', fault) + '  '.join('%s %.3g' % kv for kv in e.items()))
    assert max(e.values()) > 1, (fault, e)
    if fault in ('ws_swapped', 'no_clear', 'neighbour_theta'):
        assert e['ws'] > 1, 'a fault of the theta sum shows in the theta sum'
    if fault == 'stale_partial':
        assert e['parts'] > 1 and e['gm'] <= 1 and e['ws'] <= 1


def test_one_class_is_the_gene_emulation_bit_for_bit():
    x, mu, raw, logit, coef = gene_grid('zinb')
    kw = dict(logit=logit, coef=coef, library=True, xidx=np.arange(x.shape[0])[::-1].copy(), row_blocks=5)
    a = GR.emulate('zinb', x, mu, raw, **kw)
    b = BR.emulate('zinb', x, mu, raw[None, :], np.zeros(x.shape[0], np.int32), **kw)
    for k in ('parts', 'size', 'gm', 'gd', 'ws_blocks'):
        assert np.array_equal(a[k], b[k]), k


# --------------------------------------------------------------------- 2. refusals at the C level, without a launch
def _cdesc(kind='nb', M=0, X=2052, grad=True, n_cls=3, **over):
    kw = dict(n_cls=n_cls, cls=A, cls_src=None, ldth=X, ldw=n_cls * X if grad else 0)
    kw.update(over)
    return _desc(kind, M, X=X, grad=grad, **kw)


@pytest.mark.parametrize('M', [0, 4])
def test_the_entry_point_refuses_the_class_operands_before_any_launch(M):
    from drvae_amd import _lib
    lib = _lib.load()
    call = lambda d: lib.dv_gauss_nll_rows_raw_cs(C_.byref(d), None)
    assert [f[0] for f in _lib.NllRawCs._fields_][-4:] == ['n_cls', 'cls', 'cls_src', 'ldth']
    for kind in ('nb', 'nb_lib', 'zinb', 'zinb_lib'):
        if M == 0:      # (nothing to do and nothing wrong: 0, without a launch)
            assert call(_cdesc(kind, M)) == 0 and call(_cdesc(kind, M, grad=False)) == 0
            assert call(_cdesc(kind, M, cls_src=A, ldth=4096, ldw=3 * 2052 + 4)) == 0
            assert call(_cdesc(kind, M, n_cls=1)) == 0 and call(_cdesc(kind, M, n_cls=65535, grad=False)) == 0
        bad = [dict(n_cls=-1), dict(n_cls=65536), dict(cls=None), dict(ldth=2051), dict(ldth=0), dict(ldw=3 * 2052 - 1),
               dict(ldw=2052), dict(n_cls=1, cls=None), dict(n_cls=1, ldth=2051),
               # ... and every refusal of the pass without classes stays
               dict(theta_raw=None), dict(chunks=2), dict(row_blocks=0), dict(row_blocks=max(M, 1) + 1), dict(coef=None),
               dict(ws=None), dict(x=None), dict(mu=None), dict(out_part=None)]
        for over in bad:
            assert call(_cdesc(kind, M, **over)) == -1, (kind, over)
        assert call(_cdesc(kind, M, grad=False, n_cls=-2)) == -1 and call(_cdesc(kind, M, grad=False, cls=None)) == -1
        # without gradients ``ldw`` is not looked at
        assert M != 0 or call(_cdesc(kind, M, grad=False, ldw=0)) == 0
    # classes are for the count kinds: the Gaussian pass (kind == 0) refuses them, and is itself with all four fields zero
    gauss = lambda **o: _lib.NllRawCs(**dict(dict(coef=A, x=A, ldx=8, mu=A, sd=A, ldp=8, M=M, X=8, out_part=A, chunks=1, dmu=A,
                                                  dsd=A, ldd=8, bias_mu=A, bias_sd=A, ws=A, ldw=16, sd_off=8, row_blocks=0), **o))
    assert call(gauss(n_cls=1, cls=A, ldth=8)) == -1 and call(gauss(n_cls=2)) == -1 and call(gauss(n_cls=-1)) == -1
    if M == 0:
        assert call(gauss()) == 0 and call(gauss(cls=A, cls_src=A, ldth=3)) == 0      # (n_cls == 0: the rest is not read)
        assert call(_cdesc('nb', 0, n_cls=0, cls=None, ldth=0, ldw=2052)) == 0
    assert _lib.ABI_VERSION == 13 and len(_lib.SIGNATURES) == 84


def test_the_launcher_module_and_its_stand_in_agree():
    import drvae_amd.gene_batch_rows as GB
    import drvae_amd.gene_rows as G
    public = sorted(n for n, f in vars(GB).items() if inspect.isfunction(f) and f.__module__ == GB.__name__ and not n.startswith('_'))
    assert public == sorted(BR.FUNCTIONS)
    for name in public:
        a, b = inspect.signature(getattr(GB, name)), inspect.signature(getattr(BR, name))
        pos = lambda s: [p.name for p in s.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        kws = lambda s: sorted(p.name for p in s.parameters.values() if p.kind == p.KEYWORD_ONLY)
        assert pos(a) == pos(b) and kws(a) == kws(b), name
    # the keywords of ``gene_rows`` plus ``cls_src``; the constants are ``gene_rows``' own
    kws = lambda f: sorted(p.name for p in inspect.signature(f).parameters.values() if p.kind == p.KEYWORD_ONLY)
    assert kws(GB.gene_batch_rows) == sorted(kws(G.gene_rows) + ['cls_src'])
    assert (GB.CHUNK, GB.TARGET_WORKGROUPS, GB.MIN_ROWS) == (G.CHUNK, G.TARGET_WORKGROUPS, G.MIN_ROWS)
    assert GB.shape(900, 978, 2) == BR.shape(900, 978, 2) and GB.shape(7, 2052, 3, 3) == (3, 3)
    for Mr, X in ((1, 1), (3, 978), (900, 978), (2048, 20000), (8192, 20000), (100000, 978)):
        assert GB.row_blocks_for(Mr, X, 1) == G.row_blocks_for(Mr, X)
        for S in (2, 3, 8):
            rb = GB.row_blocks_for(Mr, X, S)
            assert 1 <= rb <= Mr and rb <= G.row_blocks_for(Mr, X)
            assert rb * S * -(-X // 1024) <= G.TARGET_WORKGROUPS + S * -(-X // 1024)
    with pytest.raises(ValueError, match="'nb' or 'zinb'"):
        GB.gene_batch_rows(torch.zeros(1, 1), torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(2, 4), torch.zeros(1, dtype=torch.int32),
                           kind='poisson')


# ------------------------------------------------------------------------------- 3. construction and refusals
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_build_the_table(kind, family, monkeypatch):
    BR.install(monkeypatch)
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    torch.manual_seed(0)
    model = tiny_model(kind, type_rec=family, dispersion='gene-batch', use_s=True, dim_s=S3)
    dt = model.decoder_x.decoder_t
    assert type(dt) is blk.GeneDispersion and not any(isinstance(m_, torch.nn.Linear) for m_ in dt.modules())
    assert [n for n, _ in dt.named_parameters()] == ['raw_theta'] and tuple(dt.raw_theta.shape) == (S3, 13)
    assert torch.equal(dt.raw_theta.detach().cpu(), torch.zeros(S3, 13))
    keys = [k for k in model.state_dict() if k.startswith('decoder_x.decoder_')]
    want = [GR.RAW, 'decoder_x.decoder_m.linear_m.weight', 'decoder_x.decoder_m.linear_m.bias']
    if family == 'zinb':
        want += ['decoder_x.decoder_d.linear_d.weight', 'decoder_x.decoder_d.linear_d.bias']
    assert keys == want and list(model.state_dict()) == list(E.param_shapes(model._step_config()))
    # no random draw is consumed: every other parameter starts as the 'gene' model's of the same seed
    gene = tiny_model(kind, type_rec=family, dispersion='gene', use_s=True, dim_s=S3)
    sd, sg = model.state_dict(), gene.state_dict()
    assert list(sd) == list(sg) and all(torch.equal(sd[k], sg[k]) for k in sd if k != GR.RAW)
    cfg = model._step_config()
    assert cfg.dispersion == 'gene-batch' and cfg.rec.gene and cfg.rec is gene._step_config().rec
    a, ag = model.engine().arena, gene.engine().arena
    assert a.shapes[GR.RAW] == (S3, 13) and a.p(GR.RAW).data_ptr() == dt.raw_theta.data_ptr()
    assert a.offsets[GR.RAW] == ag.offsets[GR.RAW] and a.offsets[GR.RAW] < a.offsets['decoder_x.decoder_m.linear_m.weight']
    tail = [k for k in a.offsets if a.offsets[k] > a.offsets[GR.RAW]]
    assert all(k.startswith('decoder_x.decoder_m') or k.startswith('decoder_x.decoder_d') for k in tail)
    # inference: every row its class's theta
    with torch.no_grad():
        dt.raw_theta.copy_(torch.arange(S3, dtype=torch.float32)[:, None].expand(S3, 13))
    s = torch.tensor([2, 0, 1, 2])
    res = model.forward(torch.ones(4, 13), s=s)
    assert len(res['px1']) == (3 if family == 'zinb' else 2) and all(tuple(t.shape) == (4, 13) for t in res['px1'])
    want = torch.nn.functional.softplus(s.float()) + 1e-3
    assert torch.allclose(res['px1'][1], want[:, None].expand(4, 13), rtol=1e-6, atol=0)


def test_refusals_on_the_models_the_blocks_and_the_config():
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    for kind in ('drvae', 'pvae', 'vfae'):
        with pytest.raises(ValueError, match='use_s=True'):
            tiny_model(kind, type_rec='nb', dispersion='gene-batch')
        for tr in ('diag_gaussian', 'binary', 'poisson'):
            with pytest.raises(ValueError, match="dispersion='gene-batch' is for"):
                tiny_model(kind, type_rec=tr, dispersion='gene-batch', use_s=True, dim_s=2)
        with pytest.raises(ValueError, match="'gene-cell' or 'gene'"):
            tiny_model(kind, type_rec='nb', dispersion='gene_batch', use_s=True, dim_s=2)
    with pytest.raises(ValueError, match='use_s=True'):
        E.StepConfig(type_rec='nb', dispersion='gene-batch')
    with pytest.raises(ValueError, match="dispersion='gene-batch' is for"):
        E.StepConfig(type_rec='poisson', dispersion='gene-batch', use_s=True)
    with pytest.raises(ValueError, match="'gene-cell' or 'gene'"):
        E.StepConfig(type_rec='nb', dispersion='batch', use_s=True)
    with pytest.raises(ValueError, match='use_s=True'):
        E.check_dispersion('gene-batch', 'zinb')
    assert E.check_dispersion('gene-batch', 'zinb', use_s=True) == 'gene-batch' and 'gene-batch' in E.DISPERSIONS
    cfg = E.StepConfig(type_rec='zinb', dispersion='gene-batch', use_s=True, dim_s=5, dim_x=9, h_en_z1=[4], h_de_x=[4])
    assert E.param_shapes(cfg)[GR.RAW] == (5, 9) and cfg.rec is E.GENE_FAMILIES['zinb']
    for cls in (blk.NegativeBinomialDecoder, blk.ZeroInflatedNegativeBinomialDecoder):
        for dims in ([5], 5):
            with pytest.raises(ValueError, match='last input'):
                cls(dims, [8], 13, dispersion='gene-batch')
        dec = cls([5, 3], [8], 13, dispersion='gene-batch')
        assert dec.decoder_t.raw_theta.shape == (3, 13) and dec.decoder_t.n_classes == 3
        assert tuple(dec._theta(None, None, [torch.zeros(4, 5), torch.eye(3)[[2, 0, 0, 1]]]).shape) == (4, 13)


def test_block_level_path_gathers_theta_and_sums_its_gradient_per_class():
    from drvae_amd import blocks as blk
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.poisson(3.0, (6, 13)).astype(np.float32))
    mu = torch.from_numpy(rs.uniform(0.5, 5, (6, 13)).astype(np.float32))
    cls = np.asarray([1, 0, 2, 1, 1, 0])
    dec = blk.NegativeBinomialDecoder([5, 4], [8], 13, dispersion='gene-batch')       # (class 3: no row)
    with torch.no_grad():
        dec.decoder_t.raw_theta.copy_(torch.from_numpy(rs.normal(0, 1, (4, 13)).astype(np.float32)))
    th = dec.decoder_t(torch.eye(4)[cls])
    assert tuple(th.shape) == (6, 13)
    dec.logp_perx(x, mu, th).sum().backward()
    ref = BR.reference('nb', x, mu, dec.decoder_t.raw_theta.detach(), cls, coef=torch.ones(6))
    close(dec.decoder_t.raw_theta.grad, ref['ws'][0].numpy(), 2e-4, 2e-5)
    assert torch.equal(dec.decoder_t.raw_theta.grad[3], torch.zeros(13))
    close(th.detach(), ref['theta'].numpy()[cls], 2e-7, 0)


@pytest.mark.parametrize('where', ['fit', 'bind'])
def test_a_class_out_of_range_is_refused_once_per_dataset(where, monkeypatch, tmp_path):
    BR.install(monkeypatch)
    from drvae_amd import data as D
    from tests.test_fit import _loader
    good = BR.class_dataset('drvae', 32, 1)
    model = tiny_model('drvae', type_rec='nb', dispersion='gene-batch', use_s=True, dim_s=2, epochs=1)
    model.w2log = lambda *a: None
    for bad_value in (2, -1):
        ds = BR.class_dataset('drvae', 32, 1)
        ds.s[5] = bad_value
        with pytest.raises(ValueError, match='0 <= s < dim_s = 2'):
            if where == 'fit':
                model.fit(_loader(ds, 8), _loader(good, 8), model_filename=str(tmp_path / 'm.pth'))
            else:
                D.DeviceBatcher(ds, torch.ones(32), 8, seed=5, mode='sampler', carry_s='masked').bind(model.engine())
    if where == 'bind':
        D.DeviceBatcher(good, torch.ones(32), 8, seed=5, mode='sampler', carry_s='masked').bind(model.engine())
        assert good._classes_checked == 2
        # other models are not looked at
        other = tiny_model('drvae', type_rec='nb', dispersion='gene', use_s=True, dim_s=2)
        ds = BR.class_dataset('drvae', 32, 1)
        D.require_classes        # (exists)
        D.DeviceBatcher(ds, torch.ones(32), 8, seed=5, mode='sampler', carry_s='masked').bind(other.engine())
        assert not hasattr(ds, '_classes_checked')


# ----------------------------------------------------------------------- 4. the fused step on the stand-ins
def _case(family, kind, sw, dim_s=S3, **over):
    nz = 0.01 if SWITCHES[sw] else 0.0
    spec = C.tiny_spec(kind, add_noise_var=nz, learning_rate=LR, use_s=True, dim_s=dim_s, **over)
    batch = CR.count_batch(spec, 16, seed=3)
    batch['s'] = (np.arange(16) * 7 % dim_s).astype(np.int64) if dim_s > 1 else np.zeros(16, np.int64)
    if dim_s > 2:       # (uneven: class 2 on three rows)
        batch['s'][batch['s'] == 2] = np.where(np.arange((batch['s'] == 2).sum()) < 3, 2, 0)
    if family == 'zinb':
        for k in ('x1', 'x2'):
            batch[k] = batch[k] * (np.random.RandomState(5).rand(*batch[k].shape) > 0.33).astype(np.float32)
    return spec, batch


def _ref(family, spec, sw, **riders):
    kw = dict(SWITCHES[sw])
    if kw.get('x_transform') == 'log1p_norm':
        return BR.ModelRef(family, spec, seed=9, norm=True, library_size=kw['library_size'], **riders)
    return BR.ModelRef(family, spec, seed=9, **kw, **riders)


def _plan_mode(eng, mode):
    """'structure': host-list plans (``s_dec``); 'carried': plans that carry the classes (``s_cls`` + the row map); 'universal':
    the batch-independent plan with the classes carried ('masked')"""
    eng.carry_s = {'structure': False, 'carried': True, 'universal': 'masked'}[mode]
    eng.universal = mode == 'universal'


def run_against_reference(family, kind, mode, sw, dev='cpu', tol=((2e-5, 2e-6), (3e-4, 2e-6), (1e-4, 2e-5)), weight_norm=False,
                          **over):
    """losses and gradients of a train-mode pass with input noise, then three Adam steps at 16 rows in three classes, against
    the model-level float64 reference in which every row reads its class's theta; returns the engine"""
    spec, batch = _case(family, kind, sw, weight_norm=weight_norm, **over)
    ref = _ref(family, spec, sw)
    params = ref.engine_params()
    eng, arena = make_engine(spec, params, dev, type_rec=family, dispersion='gene-batch', **SWITCHES[sw])
    assert arena.p(GR.RAW).is_contiguous() and arena.g(GR.RAW).is_contiguous()
    assert set(arena.shapes) == set(params) and arena.shapes[GR.RAW] == (S3, spec.dim_x)
    _plan_mode(eng, mode)
    set_batch(eng, batch, dev)
    p, X = eng.plan, spec.dim_x
    nh = 2 if family == 'zinb' else 1
    assert p.universal == (mode == 'universal') and bool(p.carry_s) == (mode != 'structure')
    assert p.DPX.shape[1] == nh * X and p.GWS.shape[1] >= S3 * X
    cls, src = p.gene_cls()
    if mode == 'structure':
        assert cls is p.s_dec and src is None
    else:       # the map of decoder row to batch row: r % B, then the pair rows twice over
        L, B = spec.L, p.B
        want = np.concatenate([np.tile(np.arange(B), L), np.tile(p.pair_host, 2 * L)])
        assert cls is p.s_cls and np.array_equal(src.cpu().numpy(), want) and src.dtype == torch.int32
    from drvae_amd.schedule import TRAIN, heads_route
    r = heads_route(eng, p, TRAIN)
    assert r.nll == 'gene' and r.rows == 'NLLG'
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
    graw = np.abs(ref.grads()[GR.RAW])
    assert graw.shape == (S3, X) and all(float(graw[k].max()) > 1e-3 for k in range(S3))
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


CASES = [('structure', 'both'), ('carried', 'off'), ('carried', 'log1p'), ('structure', 'lib'), ('universal', 'both'), ('universal', 'off')]


@pytest.mark.parametrize('mode,sw', CASES)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_matches_the_float64_model_reference(family, kind, mode, sw, monkeypatch):
    BR.install(monkeypatch, exact=True)
    run_against_reference(family, kind, mode, sw)
    lib = bool(SWITCHES[sw].get('library_size'))
    assert (BR.CALLS['gene_batch_rows_lib'] > 0) == lib and (BR.CALLS['gene_batch_rows'] > 0) == (not lib)
    assert GR.CALLS['gene_rows'] == GR.CALLS['gene_rows_lib'] == 0
    assert all(kernel_ref.CALLS[k] == 0 for k in ('nb', 'zinb', 'zinb_lib', 'lib_rows', 'other'))      # no theta-head launch


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('mode', ['structure', 'carried'])
def test_fused_step_with_weight_norm(family, mode, monkeypatch):
    BR.install(monkeypatch, exact=True)
    run_against_reference(family, 'drvae', mode, 'both', weight_norm=True)


@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_at_a_width_whose_weight_rows_are_padded(family, monkeypatch):
    """18 genes: a weight matrix of that width has its rows padded to 16 bytes in the arena; the table does not -- no product
    reads it, and its gradient is ONE contiguous column sum (978 genes is such a width)"""
    from drvae_amd.arena import ParamArena
    a = ParamArena({'w.weight': (3, 978), GR.RAW: (3, 978)}, 'cpu')
    assert a.p('w.weight').stride(0) == 980 and a.p(GR.RAW).is_contiguous() and a.numel(GR.RAW) == 3 * 978 and len(a.pads(a.param)) == 1
    BR.install(monkeypatch, exact=True)
    run_against_reference(family, 'drvae', 'carried', 'both', dim_x=18)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_with_the_depth_normalised_feed(kind, monkeypatch):
    BR.install(monkeypatch, exact=True)
    run_against_reference('nb', kind, 'carried', 'norm')


@pytest.mark.parametrize('family', FAMILIES)
def test_fused_step_on_the_fp32_emulation_of_the_launch(family, monkeypatch):
    BR.install(monkeypatch)
    run_against_reference(family, 'drvae', 'carried', 'both', tol=FP32_TOL)


def combined_against_reference(family, dev='cpu', tol=((2e-5, 2e-6), None, (1e-4, 2e-5))):
    """dropout (column masks), clipping at a norm the gradients exceed, KL annealing and the parameter average TOGETHER with both
    count switches on the universal plan: the table is clipped, decayed and averaged like any parameter"""
    from tests.test_dropout_cpu import column_masks
    spec, batch = _case(family, 'drvae', 'both')
    rid = {k: v for k, v in COMBINED.items() if k != 'dropout_rate'}
    base = _ref(family, spec, 'both').engine_params()
    eng, arena = make_engine(spec, base, dev, type_rec=family, dispersion='gene-batch', **SWITCHES['both'], **COMBINED)
    eng.carry_s = 'masked'
    set_batch(eng, batch, dev)
    sites = eng.dropout_sites()
    assert eng.plan.universal and len(sites) == 4
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (sites[i]['M'], 1)) for i, m in cols.items()})
    ref = _ref(family, spec, 'both', sched=dict(anneal_kl=True, anneal_kl_itermax=rid['anneal_kl_itermax']),
               max_grad_norm=rid['max_grad_norm'], ema_decay=rid['ema_decay'], keep=1.0 - COMBINED['dropout_rate'],
               cols={CR.chain_block(spec, s['chain']): cols[i] for i, s in enumerate(sites)})
    clipped = 0
    for step in range(3):
        nz = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nz)
        eng.train_step(nz)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), *tol[0])
        st = eng.clip_stats()
        assert st['n_skipped'] == 0
        clipped += st['coef'] < 1.0
    assert clipped == 3, 'the threshold is one the gradients exceed'
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    for k, e in ref.averaged().items():
        close(arena.e(k), e, *tol[2])
    assert not torch.equal(arena.e(GR.RAW), arena.p(GR.RAW))


@pytest.mark.parametrize('family', FAMILIES)
def test_combined_riders_match_the_float64_model_reference(family, monkeypatch):
    BR.install(monkeypatch, exact=True)
    combined_against_reference(family)


@pytest.mark.parametrize('optim_alg', ['adam', 'adamax'])
def test_weight_decay_and_the_other_optimisers_reach_the_table(optim_alg, monkeypatch):
    """(coupled weight decay, as the reference's optimisers apply it: the table is decayed like the biases)"""
    BR.install(monkeypatch, exact=True)
    spec, batch = _case('nb', 'vfae', 'off', optim_alg=optim_alg, weight_decay=0.05)
    ref = _ref('nb', spec, 'off')
    eng, arena = make_engine(spec, ref.engine_params(), type_rec='nb', dispersion='gene-batch')
    set_batch(eng, batch)
    for step in range(2):
        nz = M.make_noise(spec, 16, seed=10 + step)
        ref.step(batch, nz)
        eng.train_step(nz)
    for k, prm in ref.params().items():
        close(arena.p(k), prm, 1e-4, 2e-5)


def host_fed_equals_feed(family, kind, dev, extra=None, steps=3, captured=False):
    """two engines from one set of weights: one trains on the graph-resident masked sampler feed, the other on the same rows
    through ``set_batch``: parameters, moments and losses agree bit for bit.  Both count switches on, two classes"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR, use_s=True, dim_s=2)
    ds = BR.class_dataset(kind, 48, 4, dev)
    params = _ref(family, spec, 'off').engine_params()
    kw = dict(type_rec=family, dispersion='gene-batch', x_transform='log1p', library_size=True, **(extra or {}))
    fed, a1 = make_engine(spec, params, dev, **kw)
    twin, a0 = make_engine(spec, params, dev, **kw)
    bat = D.DeviceBatcher(ds, torch.ones(48), 16, seed=5, mode='sampler', carry_s='masked')
    bat.bind(fed)
    bat.begin_epoch()
    twin.universal, twin.carry_s = True, 'masked'
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
                       ds.has_y[i].cpu() if kind != 'pvae' else np.zeros(16, np.int64), s=ds.s[i])
        twin.train_step()
        assert torch.equal(fed.plan.XT, twin.plan.XT) and torch.equal(fed.plan.s_cls, twin.plan.s_cls)
        assert fed.losses() == twin.losses()
        losses.append(fed.losses())
    assert all(torch.equal(getattr(a1, w), getattr(a0, w)) for w in ('param', 'exp_avg', 'exp_avg_sq'))
    assert all(np.isfinite(v) for l in losses for v in l.values())
    moved = (a1.p(GR.RAW) != torch.from_numpy(params[GR.RAW]).to(dev)).any(1)
    assert bool(moved.all()), 'both classes train their row'
    return losses


@pytest.mark.parametrize('family', FAMILIES)
def test_host_fed_step_equals_feed_step_bit_for_bit(family, monkeypatch):
    BR.install(monkeypatch)
    host_fed_equals_feed(family, 'drvae', 'cpu')
    assert BR.CALLS['gene_batch_rows_lib'] >= 6


def test_one_class_is_the_gene_model_bit_for_bit(monkeypatch):
    """dim_s = 1: losses and parameters of the 'gene-batch' step equal the 'gene' step's bit for bit on the fp32 stand-ins, the
    table's one row equal to the vector"""
    BR.install(monkeypatch)
    spec, batch = _case('zinb', 'drvae', 'both', dim_s=1)
    params = GR.ModelRef('zinb', spec, seed=9, **SWITCHES['both']).engine_params()
    one = dict(params)
    one[GR.RAW] = params[GR.RAW][None, :].copy()
    out = {}
    for disp, prm in (('gene', params), ('gene-batch', one)):
        eng, arena = make_engine(spec, prm, type_rec='zinb', dispersion=disp, **SWITCHES['both'])
        set_batch(eng, batch)
        ls = []
        for step in range(3):
            eng.train_step(M.make_noise(spec, 16, seed=10 + step))
            ls.append(eng.losses())
        out[disp] = (ls, {k: arena.p(k).clone() for k in arena.shapes})
    assert out['gene'][0] == out['gene-batch'][0]
    assert BR.CALLS['gene_batch_rows_lib'] == GR.CALLS['gene_rows_lib'] > 0
    for k, v in out['gene'][1].items():
        assert torch.equal(v.reshape(-1), out['gene-batch'][1][k].reshape(-1)), k
    assert tuple(out['gene-batch'][1][GR.RAW].shape) == (1, spec.dim_x)


def test_training_state_round_trip(monkeypatch, tmp_path):
    BR.install(monkeypatch)
    from tests.test_fit import _loader
    mk = lambda: tiny_model('drvae', type_rec='zinb', dispersion='gene-batch', use_s=True, dim_s=2, x_transform='log1p',
                            library_size=True, ema_decay=0.9, epochs=1)
    a = mk()
    a.w2log = lambda *args: None
    tr = BR.class_dataset('drvae', 32, 1)
    a.fit(_loader(tr, 8), _loader(tr, 8), add_noise=True, verbose=False, model_filename=str(tmp_path / 'best.pth'))
    path = str(tmp_path / 'state.pth')
    a.save_training_state(path)
    saved = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    assert tuple(saved[GR.RAW].shape) == (2, 13)
    b = mk()
    b.w2log = a.w2log
    b.load_training_state(path)
    ea, eb = a.engine().arena, b.engine().arena
    assert bool(torch.isfinite(ea.param).all())
    assert torch.equal(ea.p(GR.RAW), eb.p(GR.RAW)) and all(float(ea.p(GR.RAW)[k].abs().max()) > 0 for k in range(2))
    for w in ('param', 'exp_avg', 'exp_avg_sq', 'avg'):
        assert torch.equal(getattr(ea, w), getattr(eb, w)), w
    # a saved model loads, and .to() keeps the table a view of the arena
    c = mk()
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.state_dict()[GR.RAW], a.state_dict()[GR.RAW])
    c.to('cpu')
    assert c.engine().arena.p(GR.RAW).data_ptr() == c.decoder_x.decoder_t.raw_theta.data_ptr()


# ------------------------------------------------------------------------ 5. two ranks on gloo == one process
DP_SW = dict(type_rec='zinb', dispersion='gene-batch', x_transform='log1p', library_size=True)


def _install_refs():
    import drvae_amd.gene_batch_rows as GB
    import drvae_amd.kernels as K
    for name in kernel_ref.FUNCTIONS:
        setattr(K, name, getattr(kernel_ref, name))
    GB.gene_batch_rows = BR.gene_batch_rows


def _dp_case(kind):
    spec, batch = _case('zinb', kind, 'both', dim_s=2)
    n = 12
    batch = {k: v[:n].copy() for k, v in batch.items()}
    pat = 'acbdab' + 'ddcbbb'      # uneven group mix between the two shards
    hy = np.array([ch in 'ac' for ch in pat], np.int64)
    hx = np.array([ch in 'cd' for ch in pat], np.int64)
    batch.update(x2=np.floor(1.3 * batch['x1']).astype(np.float32) * hx[:, None].astype(np.float32), has_x2=hx, has_y=hy,
                 s=np.asarray([0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0], np.int64))       # (uneven class mix, too)
    noises = [M.make_noise(spec, n, seed=20 + i) for i in range(3)]
    return spec, batch, noises, _ref('zinb', spec, 'off').engine_params()


def _run_steps(spec, params, batch, noises, counts, allreduce, lo=None, hi=None, dev='cpu'):
    if lo is not None:
        batch = {k: v[lo:hi] for k, v in batch.items()}
        noises = [M.slice_noise(n, lo, hi) for n in noises]
    eng, arena = make_engine(spec, params, dev, **DP_SW)
    t = lambda k: torch.from_numpy(batch[k].copy()).to(dev)
    eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'], counts=counts, s=batch['s'])
    out = []
    for noise in noises:
        eng.train_step(noise, allreduce=allreduce)
        out.append(arena.loss.clone().cpu().numpy())
    n = lambda a: a.clone().cpu().numpy()
    return np.stack(out), n(arena.param), n(arena.grad), n(arena.g(GR.RAW))


def _worker(rank, world, port, kind, q, dev='cpu'):
    """(``dev`` a GPU: both ranks on that one device, the real launches -- ``tests/test_gpu_gene_batch.py``)"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank) if dev == 'cpu' else '0')
    torch.set_num_threads(1)
    if dev == 'cpu':
        _install_refs()
    else:
        torch.cuda.set_device(0)
    from drvae_amd import dist as D
    r, w, _ = D.init_from_env(backend='gloo')
    assert (r, w) == (rank, world)
    spec, batch, noises, params = _dp_case(kind)
    n = batch['x1'].shape[0]
    lo, hi = D.shard_rows(n, rank, world)
    counts = D.global_counts(batch['has_x2'][lo:hi], batch['has_y'][lo:hi], kind, spec.semi_supervised)
    res = _run_steps(spec, params, batch, noises, counts, D.allreduce_sum, lo, hi, dev=dev)
    q.put((rank, counts) + res)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_gloo_equal_one_process(monkeypatch):
    """each rank's column sum covers its rows of every class; the existing all-reduce adds them: nothing new in the exchange"""
    from tests.test_dp_gloo import _free_port
    kind = 'drvae'
    BR.install(monkeypatch)
    spec, batch, noises, params = _dp_case(kind)
    single = _run_steps(spec, params, batch, noises, None, None)
    assert BR.CALLS['gene_batch_rows_lib'] > 0 and np.isfinite(single[1]).all() and single[3].shape == (2, spec.dim_x)
    assert all(np.abs(single[3][k]).max() > 0 for k in range(2))
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
    """three epochs on Gamma-Poisson counts whose two classes have true theta 0.5 and 20: finite losses, a finite table.
    REPORTED, not asserted: the held-out ``ll`` next to the 'gene' model's and the per-class median of the learned theta"""
    from tests.test_fit import _loader
    BR.install(monkeypatch)
    tr, va = BR.class_dataset('drvae', 64, 1), BR.class_dataset('drvae', 32, 2)
    out = {}
    for disp in ('gene-batch', 'gene'):
        model = tiny_model('drvae', type_rec=family, dispersion=disp, use_s=True, dim_s=2, x_transform='log1p', library_size=True,
                           epochs=3)
        model.w2log = lambda *a: None
        model.fit(_loader(tr, 8), _loader(va, 8), add_noise=True, verbose=False, early_stop=True,
                  model_filename=str(tmp_path / ('best_%s.pth' % disp)))
        perf, _ = model.evaluate_performance_on_dataset(va)
        assert np.isfinite(perf['x1_ll']) and np.isfinite(perf['x2_ll']) and np.isfinite(float(perf['losses']['ELBO']))
        out[disp] = (model, perf)
    model, perf = out['gene-batch']
    theta = model.decoder_x.decoder_t.theta().detach().cpu().numpy()
    assert theta.shape == (2, 13) and np.all(np.isfinite(theta)) and np.all(theta > 0)
    assert all(not np.allclose(theta[k], np.log(2.0) + 1e-3) for k in range(2))
    print("%s: held-out x1_ll gene-batch %.4f | gene %.4f; median learned theta, class 0 (true 0.5): %.3f, class 1 (true 20): %.3f"
          % (family, perf['x1_ll'], out['gene'][1]['x1_ll'], np.median(theta[0]), np.median(theta[1])))
    # the evaluation's numbers are the decoder's: ll from every row's own theta row
    res = model.forward(va.x1, s=va.s)
    px = model.decoder_x([res['z1'], torch.nn.functional.one_hot(va.s.long(), 2).float()])
    sz = model.size_factor(va.x1)
    with torch.no_grad():
        direct = float(model.decoder_x.logp_perx(va.x1, *px, size=sz).mean())
    assert perf['x1_ll'] == pytest.approx(direct, rel=1e-6)
