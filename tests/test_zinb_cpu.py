"""CPU: the zero-inflated negative-binomial data decoder (``type_rec='zinb'``) -- the float64 reference itself (autograd, the
naive float64 form where that is well conditioned, the negative-binomial limit), its bound against fp32 emulations (a careful
one inside, five faulty ones caught), construction and refusals, the fused step on the plain-PyTorch stand-ins against the
model-level float64 reference, data parallelism over gloo, the other decoders' steps as they were, and ``fit``.  The kernel
itself: ``tests/test_gpu_zinb.py``."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle import models_ref as M
from tests import counts_ref as CR
from tests import kernel_ref
from tests import nb_ref as R
from tests import ref64
from tests import zinb_ref as Z
from tests.golden import cases as C
from tests.test_dropout_cpu import tiny_model
from tests.test_nb_cpu import LR, close, make_engine, set_batch

SWITCHES = {'off': {}, 'log1p': dict(x_transform='log1p'), 'lib': dict(library_size=True),
            'both': dict(x_transform='log1p', library_size=True)}


# ----------------------------------------------------------------------------------------- 1. the reference
def _small(seed=0, Mr=8, X=12):
    """fp32 heads from random pre-activations, logits over the whole range, half of the counts zero, and the float64
    pre-activations that give exactly those fp32 heads"""
    rs = np.random.RandomState(seed)
    x = rs.poisson(rs.gamma(2.0, 3.0, (Mr, X))).astype(np.float32) * (rs.rand(Mr, X) < 0.5)
    x[1] = 1
    v = (F.softplus(torch.from_numpy(rs.uniform(-6, 4, (Mr, X)))) + R.MU_SHIFT).float()
    th = (F.softplus(torch.from_numpy(rs.uniform(-4, 6, (Mr, X)))) + R.THETA_SHIFT).float()
    a = torch.from_numpy(rs.choice(np.asarray(Z.LOGITS + (-3.0, 2.5)), (Mr, X))).float()
    inv = lambda y: torch.where(y > 30, y, torch.log(torch.expm1(y)))
    a_m, a_t = inv(v.double() - ref64.f32(R.MU_SHIFT)), inv(th.double() - ref64.f32(R.THETA_SHIFT))
    return torch.from_numpy(x.astype(np.float32)), v, th, a, a_m, a_t


@pytest.mark.parametrize('library', [False, True])
def test_reference_equals_autograd_and_the_naive_float64_form(library):
    x, v, th, a, a_m, a_t = _small()
    ones = torch.ones(x.shape[0])
    ref = Z.reference(x, v, th, a, coef=ones, library=library)
    s = ref64.f64(CR.size_factor32(x)) if library else None
    gm, gt, gd = Z.grads_autograd(ref64.f64(x), a_m, a_t, ref64.f64(a), s=s, shift=ref64.f32(R.MU_SHIFT))
    for k, g in (('gm', gm), ('gt', gt), ('gd', gd)):
        # (autograd is the weaker side at |logit| = 30: sigmoid's backward forms 1 - sigmoid, a float64 ulp of 1 absolute)
        np.testing.assert_allclose(ref[k].numpy(), g.numpy(), rtol=1e-9, atol=1e-15, err_msg=k)
    assert float(ref['gd'][~ref['pos']].min()) >= 0 and float(ref['gd'][ref['pos']].max()) <= 0
    # the naive float64 form, where it keeps its digits: |log p| >= 1e-3
    L0 = torch.where(ref['pos'], torch.zeros_like(ref['ll']), ref['nb']['ll'])
    pi = torch.sigmoid(ref64.f64(a))
    naive = torch.log(pi + (1 - pi) * torch.exp(L0))
    ok = ~ref['pos'] & (ref['ll'].abs() >= 1e-3)
    assert int(ok.sum()) > 10
    np.testing.assert_allclose(ref['ll'][ok].numpy(), naive[ok].numpy(), rtol=1e-11)
    # x > 0: the negative-binomial term minus softplus(logit)
    p = ref['pos']
    assert torch.equal(ref['ll'][p], (ref['nb']['ll'] - F.softplus(ref64.f64(a)))[p])


def test_block_logp_perx_equals_the_reference():
    from drvae_amd import blocks as blk
    x, v, th, a, _, _ = _small(seed=2)
    dec = blk.ZeroInflatedNegativeBinomialDecoder([5], [8], x.shape[1])
    got = dec.logp_perx(x, v, th, a)
    ref = Z.reference(x, v, th, a)
    np.testing.assert_allclose(got.numpy(), ref['rows'].numpy(), rtol=2e-5, atol=2e-5)
    s = torch.from_numpy(CR.size_factor32(x))
    lib = Z.reference(x, v, th, a, library=True)
    np.testing.assert_allclose(dec.logp_perx(x, v, th, a, size=s).numpy(), lib['rows'].numpy(), rtol=2e-5, atol=2e-5)
    assert torch.equal(dec.logp(x, v, th, a), got.sum())
    torch.manual_seed(0)
    big = dec.sample(v.expand(400, -1, -1).reshape(-1, x.shape[1]), th.expand(400, -1, -1).reshape(-1, x.shape[1]),
                     torch.zeros(400 * x.shape[0], x.shape[1]))
    torch.manual_seed(0)
    nb = blk.NegativeBinomialDecoder.sample(dec, v.expand(400, -1, -1).reshape(-1, x.shape[1]),
                                            th.expand(400, -1, -1).reshape(-1, x.shape[1]))
    z_nb = float((nb == 0).float().mean())      # (pi = 1/2 zeroes half of the rest: 38400 draws)
    assert float((big == 0).float().mean()) == pytest.approx(z_nb + 0.5 * (1 - z_nb), abs=0.02) and z_nb < 0.9


# ------------------------------------------------------------------------------------------ 2. the bound
@pytest.fixture(scope='module')
def grid():
    x, mu, th, a, coef = Z.edge_grid()
    ref = Z.reference(x, mu, th, a, coef=coef)
    assert float((x == 0).float().mean()) > 0.5
    near1 = (mu < 1.001e-6) & (th == np.float32(1e6)) & (x == 0)      # (a_m = -30: mu = 1e-6 + 9e-14)
    both_tiny = (mu == np.float32(1e4)) & (a == -30) & (x == 0)
    assert bool(near1.any()) and bool(both_tiny.any())
    return dict(x=x.numpy(), mu=mu.numpy(), th=th.numpy(), a=a.numpy(), coef=coef, ref=ref)


def _excess(emu, g, ref=None):
    ref = g['ref'] if ref is None else ref
    ll, gm, gt, gd = (torch.from_numpy(np.asarray(a_, np.float64)) for a_ in emu)
    c = ref64.f64(g['coef'])[:, None]
    return dict(ll=ref64.excess(ll, ref['ll'], ref['ll_bound']), gm=ref64.excess(c * gm, ref['gm'], ref['gm_bound']),
                gt=ref64.excess(c * gt, ref['gt'], ref['gt_bound']), gd=ref64.excess(c * gd, ref['gd'], ref['gd_bound']))


def test_careful_fp32_emulation_stays_inside_the_bound(grid):
    e = _excess(Z.emulate_fp32(grid['x'], grid['mu'], grid['th'], grid['a']), grid)
    print('careful emulation, worst |err| / bound: ' + '  '.join('%s %.3g' % (k, float(v.max())) for k, v in e.items()))
    for k, v in e.items():
        assert float(v.max()) <= 1, k


def _lib_grid(grid):
    """the grid under ``library_size``: size factors 1/4 .. 4 by row (the targets' own totals play no part in an emulation)"""
    s = np.asarray([0.25, 1.0, 4.0, 0.5], np.float32)[np.arange(grid['x'].shape[0]) % 4]
    t = torch.from_numpy
    return s, Z.reference(t(grid['x']), t(grid['mu']), t(grid['th']), t(grid['a']), coef=grid['coef'], library=True, s=s)


def test_five_faulty_fp32_emulations_are_caught(grid):
    args = (grid['x'], grid['mu'], grid['th'], grid['a'])
    worst = {}
    worst['naive log(pi + (1 - pi) exp(L0))'] = float(_excess(Z.emulate_fp32(*args, zero='naive'), grid)['ll'].max())
    worst['softplus(L0 - a) - softplus(-a)'] = float(_excess(Z.emulate_fp32(*args, zero='softplus_pair'), grid)['ll'].max())
    worst['sigmoid(a - L0) - sigmoid(a)'] = float(_excess(Z.emulate_fp32(*args, dlogit='sigdiff'), grid)['gd'].max())
    worst['rho left out of d/da_t at zeros'] = float(_excess(Z.emulate_fp32(*args, rho_in_gt=False), grid)['gt'].max())
    s, lib = _lib_grid(grid)
    ok = _excess(Z.emulate_fp32(*args, s=s), grid, lib)
    print('careful library emulation, worst |err| / bound: ' + '  '.join('%s %.3g' % (k, float(v.max())) for k, v in ok.items()))
    assert all(float(v.max()) <= 1 for v in ok.values())
    worst['library: slope from the scaled mean'] = float(_excess(Z.emulate_fp32(*args, s=s, slope='scaled'), grid, lib)['gm'].max())
    for k, v in worst.items():
        print('faulty emulation %-40s worst |err| / bound: %.3g' % (k, v))
    for k, v in worst.items():
        assert v >= 10, '%s: %.3g' % (k, v)


def test_pi_to_zero_is_the_negative_binomial(grid):
    """logit -30 (pi = 9e-14): where the structural zero's first-order weight pi e^{-L0} is small, the careful emulation of
    the zero-inflated term and its gradients lands on the NEGATIVE-BINOMIAL reference within the bound plus that weight"""
    ref, nb = grid['ref'], grid['ref']['nb']
    a = torch.from_numpy(grid['a'])
    L0 = torch.where(ref['pos'], torch.zeros_like(ref['ll']), nb['ll'])
    dep = 2 * torch.sigmoid(ref64.f64(a)) * torch.exp(-L0)
    sel = (a == -30) & (dep <= 1e-3)
    assert int((sel & ~ref['pos']).sum()) > 1000 and int((sel & ref['pos']).sum()) > 1000
    ll, gm, gt, gd = (torch.from_numpy(np.asarray(v, np.float64)) for v in
                      Z.emulate_fp32(grid['x'], grid['mu'], grid['th'], grid['a']))
    c = ref64.f64(grid['coef'])[:, None]
    assert torch.all(((ll - nb['ll']).abs() <= ref['ll_bound'] + dep)[sel])
    assert torch.all(((c * gm - nb['gm']).abs() <= ref['gm_bound'] + dep * nb['gm'].abs())[sel])
    assert torch.all(((c * gt - nb['gt']).abs() <= ref['gt_bound'] + dep * nb['gt'].abs())[sel])
    assert torch.all(((c * gd).abs() <= ref['gd_bound'] + dep * c.abs())[sel])


# --------------------------------------------------------------------------- 3. construction and refusals
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_build_the_zero_inflated_decoder(kind, monkeypatch):
    kernel_ref.install(monkeypatch)
    from drvae_amd import blocks as blk
    from drvae_amd import engine as E
    model = tiny_model(kind, type_rec='zinb')
    assert type(model.decoder_x) is blk.ZeroInflatedNegativeBinomialDecoder
    keys = [k for k in model.state_dict() if k.startswith('decoder_x.')]
    assert keys == ['decoder_x.nnet.model.linear1.weight', 'decoder_x.nnet.model.linear1.bias',
                    'decoder_x.decoder_m.linear_m.weight', 'decoder_x.decoder_m.linear_m.bias',
                    'decoder_x.decoder_t.linear_t.weight', 'decoder_x.decoder_t.linear_t.bias',
                    'decoder_x.decoder_d.linear_d.weight', 'decoder_x.decoder_d.linear_d.bias']
    assert list(model.state_dict()) == list(E.param_shapes(model._step_config()))
    nb = list(tiny_model(kind, type_rec='nb').state_dict())
    assert list(model.state_dict())[:len(nb)] == nb
    wn = tiny_model(kind, type_rec='zinb', weight_norm=True)
    assert 'decoder_x.decoder_d.linear_d.g' in wn.state_dict()
    assert list(wn.state_dict()) == list(E.param_shapes(wn._step_config()))
    with pytest.raises(ValueError, match="'zinb'"):
        tiny_model(kind, type_rec='laplace')
    # the three heads lie back to back in the arena
    a = model.engine().arena
    q = 'decoder_x.decoder_%s.linear_%s.%s'
    for leaf in ('weight', 'bias'):
        o = [a.offsets[q % (h, h, leaf)] for h in 'mtd']
        assert o[1] == o[0] + a.numel(q % ('m', 'm', leaf)) and o[2] == o[1] + a.numel(q % ('t', 't', leaf))
    # the count switches
    m = tiny_model(kind, type_rec='zinb', x_transform='log1p', library_size=True)
    cfg = m._step_config()
    assert cfg.x_transform == 'log1p' and cfg.library_size is True and cfg.split_x and cfg.type_rec == 'zinb'
    with pytest.raises(ValueError, match='x_transform'):
        tiny_model(kind, type_rec='zinb', x_transform='sqrt')
    with pytest.raises(ValueError, match='count decoders'):
        tiny_model(kind, type_rec='binary', library_size=True)
    assert E.REC_FAMILIES['zinb'].counts
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        drop = tiny_model(kind, type_rec='zinb', dropout_rate=0.25)
    notes = [str(m_.message) for m_ in w if 'dropout_rate' in str(m_.message)]
    assert len(notes) == 1 and 'decoder_x' in notes[0].split('ONE keep mask in ')[1].split(';')[0] and 'all three heads' in notes[0]
    assert all(hasattr(getattr(drop.decoder_x, h), 'dropout') for h in ('decoder_m', 'decoder_t', 'decoder_d'))
    # inference: px1 = (mu, theta, logit), x1_rec the negative-binomial mean
    res = model.forward(torch.ones(4, 13))
    assert len(res['px1']) == 3 and torch.equal(res['x1_rec'], res['px1'][0])
    assert all(tuple(t.shape) == (4, 13) for t in res['px1']) and float(res['px1'][1].min()) > 0


def test_launcher_tables_and_refusals():
    from drvae_amd import _lib
    from drvae_amd import kernels as K
    assert _lib.REC_KIND['zinb'] == 5 and _lib.REC_KIND['zinb_lib'] == 6
    assert _lib.RECON_KIND == {None: 0, 'binary': 1, 'poisson': 2, 'nb': 3}
    with pytest.raises(ValueError, match='library'):
        K.rec_nll_rows(torch.zeros(2), torch.zeros(2, 4), torch.zeros(2, 4), kind='binary', library=True)
    with pytest.raises(AssertionError):
        K.rec_nll_rows(torch.zeros(2), torch.zeros(2, 4), torch.zeros(2, 8), kind='zinb')


# ----------------------------------------------------------------------- 4. the fused step on the stand-ins
def _case(kind, add_noise_var=0.01, **over):
    """(input noise only with a count switch on, where the targets are a buffer of their own: without one the step's targets are
    the encoder's noisy rows, as for every decoder, and a noisy zero is no zero)"""
    spec = C.tiny_spec(kind, add_noise_var=add_noise_var, learning_rate=LR, **over)
    batch = CR.count_batch(spec, 16, seed=3)
    for k in ('x1', 'x2'):      # zero-inflate: a third of the entries
        batch[k] = batch[k] * (np.random.RandomState(5).rand(*batch[k].shape) > 0.33).astype(np.float32)
    assert (batch['x1'] == 0).mean() > 0.3 and batch['x1'].max() >= 1000
    return spec, batch


def _use_s_case(kind, **over):
    for sd in range(3, 60):
        spec, _ = _case(kind, use_s=True, dim_s=2, **over)
        batch = CR.count_batch(spec, 16, seed=sd)
        hx, hy, s = batch['has_x2'].astype(bool), batch['has_y'].astype(bool), batch['s'].reshape(-1)
        groups = {'drvae': [hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx], 'pvae': [~hx, hx], 'vfae': [hy, ~hy]}[kind]
        if all(len(set(s[g])) == 2 for g in groups):
            return spec, batch
    raise AssertionError('no suitable batch')


CASES = [('plain', 'off'), ('plain', 'log1p'), ('plain', 'lib'), ('plain', 'both'), ('weight_norm', 'both'), ('use_s', 'both'),
         ('universal', 'both'), ('universal', 'off')]


def run_against_reference(kind, variant, sw, dev='cpu', tol=((2e-5, 2e-6), (3e-4, 2e-6), (1e-4, 2e-5))):
    """losses and gradients of a train-mode pass with input noise, then three Adam steps at 16 rows, against the model-level
    float64 reference (the tolerances of ``tests/test_counts_cpu.py``); returns the engine"""
    nz = dict(add_noise_var=0.01 if SWITCHES[sw] else 0.0)
    spec, batch = _use_s_case(kind, **nz) if variant == 'use_s' else _case(kind, weight_norm=variant == 'weight_norm', **nz)
    ref = Z.ModelRef(spec, seed=9, **SWITCHES[sw])
    params = ref.engine_params()
    eng, arena = make_engine(spec, params, dev, type_rec='zinb', **SWITCHES[sw])
    assert list(arena.shapes) == list(params) and Z.LOGIT_HEAD + '.weight' in params
    eng.universal = variant == 'universal'
    set_batch(eng, batch, dev)
    p = eng.plan
    assert p.universal == (variant == 'universal') and p.DPX.shape[1] == 3 * spec.dim_x
    assert p.c_decx.out[-1].shape[1] == 3 * spec.dim_x
    from drvae_amd.schedule import TRAIN, heads_route
    r = heads_route(eng, p, TRAIN)      # the ``rec`` route; raw heads, the heads' NLL epilogue and the split-bf16 rungs stay Gaussian-only
    assert r.nll == 'rec' and not r.raw_last and not r.x3 and not r.db_done
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
    assert float(np.abs(ref.grads()[Z.LOGIT_HEAD + '.weight']).max()) > 1e-3
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
def test_fused_step_matches_the_float64_model_reference(kind, variant, sw, monkeypatch):
    kernel_ref.install(monkeypatch)
    run_against_reference(kind, variant, sw)
    lib = bool(SWITCHES[sw].get('library_size'))
    assert (kernel_ref.CALLS['zinb_lib'] > 0) == lib and (kernel_ref.CALLS['zinb'] > 0) == (not lib)
    assert kernel_ref.CALLS['nb'] == 0 and kernel_ref.CALLS['other'] == 0 and kernel_ref.CALLS['lib_rows'] == 0


COMBINED = dict(dropout_rate=0.25, max_grad_norm=1.0, anneal_kl=True, anneal_kl_itermax=10, ema_decay=0.9)


def combined_against_reference(dev='cpu', tol=((2e-5, 2e-6), None, (1e-4, 2e-5)), steps=3):
    """dropout (column masks: the three heads read the one mask), clipping at a norm the gradients exceed, KL annealing and the
    parameter average TOGETHER with both count switches, DrVAE, against ``zinb_ref.ModelRef`` with its riders on"""
    from tests.test_dropout_cpu import column_masks
    spec, batch = _case('drvae')
    rid = {k: v for k, v in COMBINED.items() if k != 'dropout_rate'}
    base = Z.ModelRef(spec, seed=9).engine_params()
    eng, arena = make_engine(spec, base, dev, type_rec='zinb', **SWITCHES['both'], **COMBINED)
    set_batch(eng, batch, dev)
    sites = eng.dropout_sites()
    assert eng.plan.universal and len(sites) == 4 and all(s['layer'] == 1 for s in sites)
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (sites[i]['M'], 1)) for i, m in cols.items()})
    ref = Z.ModelRef(spec, seed=9, **SWITCHES['both'], sched=dict(anneal_kl=True, anneal_kl_itermax=rid['anneal_kl_itermax']),
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
    assert eng.schedule_record()['beta_kl'] == pytest.approx(0.01 + (steps - 1) / 10.0)
    for k, prm in ref.params().items():
        close(arena.p(k), prm, *tol[2])
    for k, e in ref.averaged().items():
        close(arena.e(k), e, *tol[2])
    assert not torch.equal(arena.avg, arena.param)
    return eng


def test_combined_riders_match_the_float64_model_reference(monkeypatch):
    kernel_ref.install(monkeypatch)
    combined_against_reference()
    assert kernel_ref.CALLS['zinb_lib'] > 0


def host_fed_equals_feed(kind, dev, extra=None, steps=3, captured=False):
    """two engines from one set of weights: one trains on the graph-resident feed's batches, the other on the same rows through
    ``set_batch``; same seed, same Philox draws -- parameters, moments and losses agree bit for bit.  Both count switches on"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, add_noise_var=0.01, learning_rate=LR)
    ds = Z.zi_dataset(kind, 48, 4, dev)
    params = Z.ModelRef(spec, seed=9).engine_params()
    kw = dict(type_rec='zinb', x_transform='log1p', library_size=True, **(extra or {}))
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
    return losses


def test_host_fed_step_equals_feed_step_bit_for_bit(monkeypatch):
    kernel_ref.install(monkeypatch)
    host_fed_equals_feed('drvae', 'cpu')
    assert kernel_ref.CALLS['split_feed'] >= 6 and kernel_ref.CALLS['zinb_lib'] >= 6


# ------------------------------------------------------------------------ 5. two ranks on gloo == one process
DP_SW = dict(type_rec='zinb', x_transform='log1p', library_size=True)


def _install_refs():
    import drvae_amd.kernels as K
    for name in kernel_ref.FUNCTIONS:
        setattr(K, name, getattr(kernel_ref, name))


def _dp_case(kind):
    spec, batch = _case(kind)
    n = 12
    batch = {k: v[:n].copy() for k, v in batch.items()}
    pat = 'acbdab' + 'ddcbbb'      # uneven group mix between the two shards
    hy = np.array([ch in 'ac' for ch in pat], np.int64)
    hx = np.array([ch in 'cd' for ch in pat], np.int64)
    batch.update(x2=np.floor(1.3 * batch['x1']).astype(np.float32) * hx[:, None].astype(np.float32), has_x2=hx, has_y=hy)
    noises = [M.make_noise(spec, n, seed=20 + i) for i in range(3)]
    return spec, batch, noises, Z.ModelRef(spec, seed=9).engine_params()


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
    return np.stack(out), arena.param.clone().numpy(), arena.grad.clone().numpy()


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
    from tests.test_dp_gloo import _free_port
    kind = 'drvae'
    kernel_ref.install(monkeypatch)
    spec, batch, noises, params = _dp_case(kind)
    single = _run_steps(spec, params, batch, noises, None, None)
    assert kernel_ref.CALLS['zinb_lib'] > 0 and np.isfinite(single[1]).all()
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
    n = batch['x1'].shape[0]
    for rank, counts, losses, prm, grad in got:
        assert tuple(counts) == (n, int(batch['has_x2'].sum()), int(batch['has_y'].sum()))
        np.testing.assert_allclose(losses, single[0], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(grad, single[2], rtol=1e-4, atol=1e-6 * np.abs(single[2]).max())
        np.testing.assert_allclose(prm, single[1], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(got[0][3], got[1][3])                          # replicas stay bit-identical


# ------------------------------------------------------------------ 6. the other decoders: the step as it was
# launch lists (name, keyword names) of three train steps at 16 rows, recorded on the parent commit with the stand-ins of
# ``tests/kernel_ref.py``: what 'nb', 'poisson' and 'diag_gaussian' steps launched before this decoder existed
def _launch_log(mp_ctx, names):
    import drvae_amd.kernels as K
    log = []
    for fn in names:
        real = getattr(K, fn)
        mp_ctx.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append((_n, sorted(k))), _f(*a, **k))[1])
    return log


def _other_step_log(kind, type_rec, install):
    spec = C.tiny_spec(kind, add_noise_var=0.0, learning_rate=LR, **({} if type_rec == 'nb' else dict(type_rec=type_rec)))
    if type_rec == 'nb':
        batch, params = R.count_batch(spec, 16, seed=3), R.ModelRef(spec, seed=9).engine_params()
    else:
        batch, params = M.make_batch(spec, 16, seed=3), M.init_params(spec, 9, as_numpy=True)
    names = sorted(set(kernel_ref.FUNCTIONS) - {'smalln_ws_numel', 'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles'})
    with pytest.MonkeyPatch.context() as mpi:
        install(mpi)
        eng, arena = make_engine(spec, params, type_rec=type_rec)
        set_batch(eng, batch)
        with pytest.MonkeyPatch.context() as mpc:
            log = _launch_log(mpc, names)
            for i in range(3):
                eng.train_step(M.make_noise(spec, 16, seed=10 + i))
        return log, arena.param.clone(), arena.exp_avg.clone(), arena.loss.clone(), tuple(eng.plan.DPX.shape)


@pytest.mark.parametrize('type_rec', ['nb', 'poisson', 'diag_gaussian'])
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_other_decoders_record_the_launches_they_did(kind, type_rec):
    """the launch list and every bit of three train steps are the same on two fresh installs of ``tests/kernel_ref.py`` (which
    states this decoder's rows too); the list itself is the parent's: its digest is pinned in ``tests/golden/zinb_launches.json``
    (recorded on the parent commit by this very function), and the heads' launches are the ones these decoders always had --
    one ``linear_fwd`` for the decoder's last layer, the row launch with its own kind and its five keywords"""
    import hashlib
    import json
    a = _other_step_log(kind, type_rec, kernel_ref.install)
    b = _other_step_log(kind, type_rec, kernel_ref.install)
    assert a[0] == b[0] and a[4] == b[4] and all(torch.equal(x, y) for x, y in zip(a[1:4], b[1:4]))
    rec = [kw for n, kw in a[0] if n == 'rec_nll_rows']
    X = C.tiny_spec(kind).dim_x
    if type_rec == 'diag_gaussian':
        assert not rec and a[4][1] == 2 * X
    else:
        assert len(rec) == 3 and all(kw == ['coef', 'dpre', 'kind', 'shift', 'xidx'] for kw in rec)
        assert a[4][1] == (2 if type_rec == 'nb' else 1) * X
    digest = hashlib.sha256(json.dumps(a[0]).encode()).hexdigest()
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'zinb_launches.json')) as fh:
        want = json.load(fh)
    assert digest == want['%s/%s' % (kind, type_rec)], 'the launch list of a %s %s step moved' % (kind, type_rec)


# -------------------------------------------------------------------------------------------------- 7. fit
def test_fit_runs_and_evaluates_step_by_step_without_warnings(monkeypatch, tmp_path):
    from tests.test_fit import _loader
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae', type_rec='zinb', x_transform='log1p', library_size=True, epochs=2)
    model.w2log = lambda *a: None
    tr, va = Z.zi_dataset('drvae', 40, 1), Z.zi_dataset('drvae', 24, 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        model.fit(_loader(tr, 8), _loader(va, 8), add_noise=True, verbose=False, early_stop=True,
                  model_filename=str(tmp_path / 'best.pth'))
        perf, _ = model.evaluate_performance_on_dataset(va)
    assert not [str(m.message) for m in w], [str(m.message) for m in w]
    assert np.isfinite(perf['x1_ll']) and np.isfinite(perf['x2_ll']) and np.isfinite(float(perf['losses']['ELBO']))
    res = model.forward(va.x1)
    mu, th, lg = model.decoder_x([res['z1']])
    s = model.size_factor(va.x1)
    assert torch.equal(res['x1_rec'], s[:, None] * mu) and torch.equal(res['px1'][2], lg)
    with torch.no_grad():
        direct = float(model.decoder_x.logp_perx(va.x1, mu, th, lg, size=s).mean())
    assert perf['x1_ll'] == pytest.approx(direct, rel=1e-6)
    assert kernel_ref.CALLS['zinb_lib'] > 0
