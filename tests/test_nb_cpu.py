"""CPU: the negative-binomial data decoder (``type_rec='nb'``) -- the float64 reference itself (against scipy and the Poisson
limit), the error bound against fp32 emulations (three faulty ones caught, a careful one inside), model construction, and the
fused step on the plain-PyTorch stand-ins against the model-level float64 reference.  The kernel itself: ``tests/test_gpu_nb.py``."""
import warnings

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests.golden import cases as C
from tests.test_dropout_cpu import tiny_model


def make_engine(spec, params, device='cpu', **over):
    """engine + arena of ``spec`` (a Gaussian-shaped oracle spec) as a negative-binomial model"""
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    kw.update(over)
    cfg = E.StepConfig(**kw)
    arena = ParamArena(E.param_shapes(cfg), device, frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena), arena


def set_batch(eng, batch, dev='cpu'):
    t = lambda k: torch.from_numpy(batch[k].copy()).to(dev)
    kw = dict(s=batch['s']) if eng.cfg.use_s else {}
    return eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'], **kw)


def close(a, b, rtol, atol):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


# ----------------------------------------------------------------------------------------- 1. the reference
def test_reference_equals_scipy_on_the_grid_and_poisson_in_the_limit():
    import scipy.special as sp
    import scipy.stats as st
    x, mu, th, _ = R.edge_grid()
    X_, MU, TH = (ref64.f64(t) for t in (x, mu, th))
    pair, lx, tl, xl = R.logp_terms(X_, MU, TH)
    ll = (pair - lx + tl + xl).numpy()
    want = st.nbinom.logpmf(X_.numpy(), TH.numpy(), (TH / (TH + MU)).numpy())
    # scipy subtracts two float64 lgammas and forms p = theta / (theta + mu) first: a few float64 ulps of each lgamma and of
    # the terms through p (log p and log1p(-p) see p rounded: conditioned by theta/mu and mu/theta at most 1e12 here)
    comps = (pair.abs() + lx + tl.abs() + xl.abs()).numpy()
    e = 2.0 ** -52
    tol = 16 * e * (np.abs(sp.gammaln((X_ + TH).numpy())) + np.abs(sp.gammaln(TH.numpy())) + comps) + \
        8 * e * (X_ * (1 + TH / MU) + TH * (1 + MU / TH)).numpy()
    assert np.all(np.abs(ll - want) <= tol), float(np.max(np.abs(ll - want) / tol))
    # closed-form gradients == float64 autograd
    gm, gt, gm_c, gt_c = R.grads64(X_, MU, TH)
    am, at = R.grads_autograd(X_, MU, TH)
    assert torch.all((gm - am).abs() <= 1e-12 * gm_c + 1e-300)
    # (both subtract two float64 digammas: a few float64 ulps of each -- 1e-9 of the pair at theta = 1e6, against fp32's 6e-8)
    psis = torch.digamma(X_ + TH).abs() + torch.digamma(TH).abs()
    assert torch.all((gt - at).abs() <= 1e-12 * gt_c + 8 * e * psis)
    # theta = 1e12: the Poisson log-pmf to 1e-9 relative.  The two DISTRIBUTIONS differ by ((x - mu)^2 - x) / (2 theta) + O(theta^-2)
    # -- 4.5e-4 at x = 30000, 1.9e-9 of the Poisson term there, more at mu = 1e4 -- so the bound is held with that first-order
    # term of the exact difference taken out, on every grid point; where it is below 1e-10 of the Poisson term, also without
    big = torch.full_like(TH, 1e12)
    nb = R.logp64(X_, MU, big)
    po = X_ * torch.log(MU) - MU - torch.lgamma(X_ + 1)
    gap = ((X_ - MU) ** 2 - X_) / (2 * big)
    assert torch.all((nb - po - gap).abs() <= 1e-9 * po.abs())
    small = gap.abs() <= 1e-10 * po.abs()
    assert int(small.sum()) > small.numel() // 2 and torch.all((nb - po).abs()[small] <= 1e-9 * po.abs()[small])
    # x = 0: the lgamma pair is exactly 0
    assert torch.all(pair[X_ == 0] == 0)


# ------------------------------------------------------------------------------------------ 2. the bound
def _excess(emu, ref):
    ll, gm, gt = (torch.from_numpy(a.astype(np.float64)) for a in emu)
    c = ref64.f64(ref['coef'])[:, None]
    X = ll.shape[1]
    # rows: the per-element bound (one element's share of the row bound) -- the emulations are per element
    e_ll = ref64.excess(ll, ref['ll'], ref64.bound(R.C_ROW, ref['comps']))
    return e_ll, ref64.excess(c * gm, ref['gm'], ref['gm_bound']), ref64.excess(c * gt, ref['gt'], ref['gt_bound'])


@pytest.fixture(scope='module')
def grid():
    x, mu, th, coef = R.edge_grid()
    ref = R.reference(x, mu, th, coef=coef)
    ref['coef'] = coef
    return x.numpy(), mu.numpy(), th.numpy(), ref


def test_careful_fp32_emulation_stays_inside_the_bound(grid):
    x, mu, th, ref = grid
    e_ll, e_gm, e_gt = _excess(R.emulate_fp32(x, mu, th), ref)
    print('careful emulation, worst |err| / bound: rows %.3g  d/da_m %.3g  d/da_t %.3g'
          % (float(e_ll.max()), float(e_gm.max()), float(e_gt.max())))
    assert float(e_ll.max()) <= 1 and float(e_gm.max()) <= 1 and float(e_gt.max()) <= 1


def test_three_faulty_fp32_emulations_are_caught(grid):
    x, mu, th, ref = grid
    at_1e4 = torch.from_numpy(th == np.float32(1e4))
    e_ll, _, _ = _excess(R.emulate_fp32(x, mu, th, pair='lgamma2'), ref)
    assert float(e_ll[at_1e4].max()) >= 10, 'two lgammas subtracted at theta = 1e4: %.3g' % float(e_ll[at_1e4].max())
    ratio = torch.from_numpy((mu.astype(np.float64) / th.astype(np.float64)))
    near = (ratio > 0.5e-6) & (ratio < 2e-6)
    assert bool(near.any())
    e_ll, _, _ = _excess(R.emulate_fp32(x, mu, th, ratio='logdiff'), ref)
    assert float(e_ll[near].max()) >= 10, 'theta (log theta - log(theta + mu)) at mu / theta = 1e-6: %.3g' % float(e_ll[near].max())
    _, _, e_gt = _excess(R.emulate_fp32(x, mu, th, psi='digamma2'), ref)
    assert float(e_gt[at_1e4].max()) >= 10, 'two digammas subtracted at theta = 1e4: %.3g' % float(e_gt[at_1e4].max())


# --------------------------------------------------------------------------------------- 3. construction
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_build_the_negative_binomial_decoder(kind):
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    model = tiny_model(kind, type_rec='nb')
    assert type(model.decoder_x) is blk.NegativeBinomialDecoder
    keys = [k for k in model.state_dict() if k.startswith('decoder_x.')]
    assert keys == ['decoder_x.nnet.model.linear1.weight', 'decoder_x.nnet.model.linear1.bias',
                    'decoder_x.decoder_m.linear_m.weight', 'decoder_x.decoder_m.linear_m.bias',
                    'decoder_x.decoder_t.linear_t.weight', 'decoder_x.decoder_t.linear_t.bias']
    assert list(model.state_dict()) == list(E.param_shapes(model._step_config()))
    gauss = tiny_model(kind, type_rec='diag_gaussian')
    assert [R.nb_name(k) for k in gauss.state_dict()] == list(model.state_dict())
    assert [tuple(v.shape) for v in gauss.state_dict().values()] == [tuple(v.shape) for v in model.state_dict().values()]
    wn = tiny_model(kind, type_rec='nb', weight_norm=True)
    assert 'decoder_x.decoder_t.linear_t.g' in wn.state_dict()
    assert list(wn.state_dict()) == list(E.param_shapes(wn._step_config()))
    with pytest.raises(ValueError, match="'nb'"):
        tiny_model(kind, type_rec='laplace')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        tiny_model(kind, type_rec='nb', dropout_rate=0.25)
        tiny_model(kind, type_rec='poisson', dropout_rate=0.25)
    notes = [str(m.message) for m in w if 'dropout_rate' in str(m.message)]
    assert len(notes) == 2
    shared = lambda s: s.split('ONE keep mask in ')[1].split(';')[0]
    assert 'decoder_x' in shared(notes[0]) and 'decoder_x' not in shared(notes[1])
    drop = tiny_model(kind, type_rec='nb', dropout_rate=0.25)
    assert hasattr(drop.decoder_x.decoder_m, 'dropout') and hasattr(drop.decoder_x.decoder_t, 'dropout')


# ----------------------------------------------------------------------- 4. the fused step on the stand-ins
LR = 2e-4      # (raw counts up to 1e4 enter the encoder: three Adam steps of 5e-3 on its first layer move a hidden unit by 150)


def _case(kind, **over):
    spec = C.tiny_spec(kind, add_noise_var=0.0, learning_rate=LR, **over)
    batch = R.count_batch(spec, 16, seed=3)
    assert batch['x1'].max() >= 1000 and np.all(batch['x1'] == np.floor(batch['x1']))
    return spec, batch


def _use_s_case(kind):
    for sd in range(3, 60):
        spec, _ = _case(kind, use_s=True, dim_s=2)
        batch = R.count_batch(spec, 16, seed=sd)
        hx, hy, s = batch['has_x2'].astype(bool), batch['has_y'].astype(bool), batch['s'].reshape(-1)
        groups = {'drvae': [hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx], 'pvae': [~hx, hx], 'vfae': [hy, ~hy]}[kind]
        if all(len(set(s[g])) == 2 for g in groups):
            return spec, batch
    raise AssertionError('no suitable batch')


VARIANTS = ['plain', 'weight_norm', 'use_s', 'universal']


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_fused_step_matches_the_float64_model_reference(kind, variant, monkeypatch):
    """losses and gradients of a train-mode pass, then three Adam steps at 16 rows: the tolerances of
    ``tests/test_engine_cpu.py::test_bernoulli_poisson_decoders_match_oracle``"""
    kernel_ref.install(monkeypatch)
    if variant == 'use_s':
        spec, batch = _use_s_case(kind)
    else:
        spec, batch = _case(kind, weight_norm=variant == 'weight_norm')
    ref = R.ModelRef(spec, seed=9)
    params = ref.engine_params()
    assert 'decoder_x.decoder_t.linear_t.weight' in params and 'decoder_x.encoder_mu.linear_mu.weight' not in params
    eng, arena = make_engine(spec, params, type_rec='nb')
    assert list(arena.shapes) == list(params)
    if variant == 'universal':
        eng.universal = True
    set_batch(eng, batch)
    assert (eng._plans and list(eng._plans)[0][0] == 'universal') == (variant == 'universal')
    assert eng.plan.DPX.shape[1] == 2 * spec.dim_x
    noise = M.make_noise(spec, 16, seed=4)
    want, _ = ref.loss(batch, noise, True)
    with R.oracle_as_nb():
        want['CMPL'].backward()
    eng.training = True
    eng.set_noise(noise)
    eng.forward()
    eng.backward()
    for k, v in eng.losses().items():
        close(v, float(want[k].detach()), 2e-5, 2e-6)
    for k, g in ref.grads().items():
        close(arena.g(k), g, 3e-4, 2e-6)
    for prm in ref.tr.params.values():
        prm.grad = None
    for step in range(3):
        nz = M.make_noise(spec, 16, seed=10 + step)
        want, _ = ref.step(batch, nz)
        eng.train_step(nz)
        for k, v in eng.losses().items():
            close(v, float(want[k].detach()), 2e-5, 2e-6)
    for k, prm in ref.params().items():
        close(arena.p(k), prm, 1e-4, 2e-5)
    assert kernel_ref.CALLS['nb'] > 0 and kernel_ref.CALLS['other'] == 0


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_two_shards_sum_to_the_whole_batch(kind, monkeypatch):
    """data parallelism needs nothing new: two engines on rows [0, 8) and [8, 16) with the global counts and their rows of the
    noise hold loss scalars and gradients that SUM to the whole batch's (what the all-reduce forms); fp32 sums of 8 + 8
    against 16 terms, compared in float64"""
    kernel_ref.install(monkeypatch)
    spec, batch = _case(kind)
    ref = R.ModelRef(spec, seed=9)
    noise = M.make_noise(spec, 16, seed=4)
    hx, hy = batch['has_x2'].astype(bool), batch['has_y'].astype(bool)
    counts = (16, int(hx.sum()), int(hy.sum()))

    def xchg(lo, hi):
        eng, arena = make_engine(spec, ref.engine_params(), type_rec='nb')
        b = {k: v[lo:hi] for k, v in batch.items()}
        t = lambda k: torch.from_numpy(b[k].copy())
        eng.set_batch(t('x1'), t('x2'), b['y'], b['has_x2'], b['has_y'], counts=counts)
        eng.training = True
        eng.set_noise(M.slice_noise(noise, lo, hi))
        eng.forward()
        eng.backward()
        eng.losses()
        return arena.xchg.clone().double().numpy()
    whole, parts = xchg(0, 16), xchg(0, 8) + xchg(8, 16)
    np.testing.assert_allclose(parts, whole, rtol=2e-5, atol=2e-6 * np.abs(whole).max())
    assert np.abs(whole).max() > 1


# ------------------------------------------------------------------ 5. the other decoders: the step as it was
def _launch_log(mp_ctx, names):
    import drvae_amd.kernels as K
    log = []
    for fn in names:
        real = getattr(K, fn)
        mp_ctx.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append((_n, sorted(k))), _f(*a, **k))[1])
    return log


@pytest.mark.parametrize('type_rec', ['diag_gaussian', 'binary', 'poisson'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_other_decoders_record_the_launches_they_did(kind, type_rec, monkeypatch):
    """the launch list (names and keyword names) and every bit of the result of three train steps: with the stand-ins as they
    were == with this feature's stand-in in place (which is the wrapped one for these kinds, call for call); the row launch is
    the one the decoder had -- the Gaussian step never calls ``rec_nll_rows``, the single-head decoders call it with their own
    kind and the five keywords they always passed, on a buffer as wide as the data"""
    spec = C.tiny_spec(kind, type_rec=type_rec, add_noise_var=0.0)
    batch = M.make_batch(spec, 16, seed=3)
    params = M.init_params(spec, 9, as_numpy=True)
    noises = [M.make_noise(spec, 16, seed=10 + i) for i in range(3)]
    names = sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel', 'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles'})
    out = {}
    for tag, install in (('before', kernel_ref.install), ('after', kernel_ref.install)):
        with pytest.MonkeyPatch.context() as mp_install:
            install(mp_install)
            from tests.test_engine_cpu import make_engine as plain_engine, set_batch as plain_batch
            eng, arena = plain_engine(spec, params)
            plain_batch(eng, batch)
            kinds = []
            with pytest.MonkeyPatch.context() as mpc:
                log = _launch_log(mpc, names)
                import drvae_amd.kernels as K
                real = K.rec_nll_rows
                mpc.setattr(K, 'rec_nll_rows', lambda *a, **k: (kinds.append((k['kind'], tuple(a[2].shape))), real(*a, **k))[1])
                for noise in noises:
                    eng.train_step(noise)
            out[tag] = (log, kinds, arena.param.clone(), arena.exp_avg.clone(), arena.loss.clone(),
                        tuple(eng.plan.DPX.shape))
    a, b = out['before'], out['after']
    assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
    for x, y in zip(a[2:5], b[2:5]):
        assert torch.equal(x, y)
    rec = [kw for n, kw in a[0] if n == 'rec_nll_rows']
    if type_rec == 'diag_gaussian':
        assert not rec and not a[1] and a[5][1] == 2 * spec.dim_x
    else:
        assert len(rec) == 3 and all(kw == ['coef', 'dpre', 'kind', 'shift', 'xidx'] for kw in rec)
        assert all(k == type_rec and shp[1] == spec.dim_x for k, shp in a[1]) and a[5][1] == spec.dim_x
    assert kernel_ref.CALLS['nb'] == 0
