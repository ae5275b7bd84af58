"""CPU: hidden-layer dropout in the fused train step -- sites, masks, descriptor rows, the chain's dropped operands and the
schedule decision -- with the HIP launchers replaced by their plain-PyTorch references (tests/kernel_ref.py).
The kernels themselves and the device masks are checked on the GPU (tests/test_gpu_dropout.py)."""
import warnings

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests.golden import cases as C

CHAIN_LAYERS = {'c_enc': 'L_enc', 'c_decx': 'L_decx', 'c_clf': 'L_clf', 'c_top': 'L_top', 'c_dz1': 'L_dz1'}
# the tiny golden cases of the three models and a WeightNorm one
STEP_CASES = ['tiny_drvae', 'tiny_vfae', 'tiny_pvae', 'tiny_drvae_wn']


def make_engine(spec, params, rate=0.0, device='cpu', row0=0):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    cfg = E.StepConfig(dropout_rate=rate, **kw)
    arena = ParamArena(E.param_shapes(cfg), device, frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena, row0=row0), arena


def set_batch(eng, batch, dev='cpu', rows=None):
    sl = slice(None) if rows is None else rows
    t = lambda k: torch.from_numpy(batch[k][sl].copy()).to(dev)
    return eng.set_batch(t('x1'), t('x2'), batch['y'][sl], batch['has_x2'][sl], batch['has_y'][sl])


def column_masks(eng, seed):
    """per site a mask that is the same in every row: column j kept or dropped by a seeded RNG, at least one of each kind"""
    rs, out = np.random.RandomState(seed), {}
    for i, s in enumerate(eng.dropout_sites()):
        m = (rs.rand(s['N']) < 0.6).astype(np.float32)
        m[rs.randint(s['N'])] = 1.0
        m[(int(np.argmax(m)) + 1) % s['N']] = 0.0
        assert 0 < m.sum() < s['N']
        out[i] = m
    return out


def fold_masks_into_weights(eng, ref, cols, keep):
    """the rate-0 engine ``ref`` gets the weights W' = W diag(m / keep) behind every site of ``eng`` (WeightNorm: and the gain
    g' = g |W'| / |W|, so that the effective weight is the dropped engine's times diag(m / keep)); returns what is needed to
    carry its gradients back: [(layer of ref, W, g, d)]"""
    back = []
    for i, s in enumerate(eng.dropout_sites()):
        l = getattr(ref, CHAIN_LAYERS[s['chain']])[s['layer']]
        d = torch.from_numpy(cols[i] / np.float32(keep)).to(l.W.device)
        W0 = l.W.clone()
        g0 = l.g.clone() if l.g is not None else None
        l.W.mul_(d[None, :])
        if l.g is not None:
            l.g.mul_(l.W.double().norm(dim=1).div(W0.double().norm(dim=1)).float())
        back.append((l, W0, g0, d))
    return back


def carry_gradients_back(back):
    """dL/d(W, g) of the dropped engine from dL/d(W', g') of the folded one: the vector-Jacobian product of the map
    (W, g) -> (W diag(d), g |W diag(d)| / |W|), in float64 by autograd.  Without WeightNorm this is dW = dW' diag(m / keep)."""
    for l, W0, g0, d in back:
        W = W0.double().requires_grad_(True)
        Wp = W * d.double()[None, :]
        tot = (Wp * l.dW.double()).sum()
        ins = [W]
        if g0 is not None:
            g = g0.double().requires_grad_(True)
            tot = tot + (g * Wp.norm(dim=1) / W.norm(dim=1) * l.dg.double()).sum()
            ins.append(g)
        grads = torch.autograd.grad(tot, ins)
        l.dW.copy_(grads[0].float())
        if g0 is not None:
            l.dg.copy_(grads[1].float())


def dropped_vs_folded(name, keep, fused, device='cpu', step=None):
    """(losses, gradient arena) of the dropped engine and of the folded rate-0 engine for one golden case; ``step``(eng) runs
    forward + backward (default: eagerly)"""
    case = C.model_case(name)
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    assert spec.L == 2
    eng, arena = make_engine(spec, params, rate=1.0 - keep, device=device)
    ref, rarena = make_engine(spec, params, rate=0.0, device=device)
    for e in (eng, ref):
        set_batch(e, case['batch'], device)
        e.training = True
        e.set_noise(case['noises'][0])
    assert eng.dropout_sites() and not ref.dropout_sites()
    cols = column_masks(eng, 5)
    eng.set_dropout_masks({i: np.tile(m[None, :], (eng.dropout_sites()[i]['M'], 1)) for i, m in cols.items()})
    back = fold_masks_into_weights(eng, ref, cols, keep)
    for e in (eng, ref):
        if step is not None:
            step(e)
        elif fused:
            e._launch_sequence(draw=False, optimizer=False)
        else:
            e.forward()
            e.backward()
    carry_gradients_back(back)
    return eng, ref, arena, rarena


def compare_step(eng, ref, arena, rarena, label):
    worst_l = worst_g = 0.0
    la, lb = eng.losses(), ref.losses()
    for k in la:
        worst_l = max(worst_l, abs(la[k] - lb[k]) / max(abs(lb[k]), 1e-30))
    out = []
    for k in arena.shapes:
        a, b = arena.g(k).detach().cpu().double(), rarena.g(k).detach().cpu().double()
        nb = float(b.norm())
        dev = float((a - b).norm())
        worst_g = max(worst_g, dev / nb if nb > 0 else dev)
        out.append((k, dev, nb))
    print('%s: worst relative loss deviation %.3g, worst norm-wise gradient deviation %.3g' % (label, worst_l, worst_g))
    for k in la:
        np.testing.assert_allclose(la[k], lb[k], rtol=2e-5, atol=2e-6, err_msg=k)
    for k, dev, nb in out:
        assert dev <= 1e-4 * nb, (k, dev, nb)


# ------------------------------------------------------------------------------------------------ 1. construction
def tiny_model(kind, **kw):
    from drvae_amd.DrVAE import DrVAE
    from drvae_amd.PVAE import PVAE
    from drvae_amd.VFAE import VFAE
    common = dict(dim_x=13, dim_s=1, dim_y=2, dim_h_en_z1=[7], dim_h_de_x=[8], dim_z1=5, type_rec='diag_gaussian',
                  nonlinearity='elu', learning_rate=5e-3, L=2, weight_decay=0.01, add_noise_var=0.01, use_MMD=False,
                  random_seed=5, epochs=2, batch_size=8, device='cpu')
    common.update(kw)
    if kind == 'drvae':
        return DrVAE(dim_h_de_z1=[6], dim_h_en_z3=[6], dim_h_clf=[], dim_z3=4, pertloss_rate=0.05, **common)
    if kind == 'pvae':
        return PVAE(pertloss_rate=0.05, **common)
    return VFAE(dim_h_de_z1=[6], dim_h_en_z2=[6], dim_h_clf=[], dim_z2=4, semi_supervised=True, **common)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_construct_with_dropout_and_warn_once(kind):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        model = tiny_model(kind, dropout_rate=0.5)
    notes = [str(x.message) for x in w if 'dropout_rate' in str(x.message)]
    assert len(notes) == 1, notes
    if kind != 'vfae':
        assert 'decoder_z2Fz1' in notes[0]
    assert 'encoder_y' in notes[0] or kind == 'pvae'       # (no hidden layer in the classifier here: not dropped)
    assert 'ONE keep mask' in notes[0] and 'encoder_z1' in notes[0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        plain = tiny_model(kind)
    assert not [x for x in w if 'dropout_rate' in str(x.message)]
    assert list(model.state_dict()) == list(plain.state_dict())
    assert model._step_config().dropout_rate == 0.5 and plain._step_config().dropout_rate == 0.0
    with pytest.raises(ValueError):
        tiny_model(kind, dropout_rate=1.0)


# ------------------------------------------------------------------------------------------------ 2. rate 0
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_pvae', 'tiny_vfae'])
def test_rate_zero_is_untouched(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case = C.model_case(name)
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    eng, _ = make_engine(spec, params)
    drp, _ = make_engine(spec, params, rate=0.5)
    p, q = set_batch(eng, case['batch']), set_batch(drp, case['batch'])
    assert p.drop_sites == [] and eng.dropout_sites() == [] and 'dropout' not in str(p.key)
    assert all(c.masks is None and c.outd is None for c in (getattr(p, n, None) for n in CHAIN_LAYERS) if c is not None)
    # the arena and the table are what they were: the sizes written out ...
    cfg, L, B, Np = eng.cfg, eng.cfg.L, p.B, p.Np
    numel = (B + Np) * cfg.dim_x + L * B * cfg.dim_z1 + L * Np * cfg.dim_z1 + (L * B * cfg.dim_z1 if cfg.has_pert else 0) \
        + (p.Mf * cfg.dim_z3 if cfg.has_y else 0)
    rows = (B + Np) + L * B + L * Np + (L * B if cfg.has_pert else 0) + (p.Mf if cfg.has_y else 0)
    assert p.noise.numel() == numel and tuple(p.noise_desc.shape) == (rows, 4) and p.n_normal_rows == rows
    # ... and a plan WITH sites keeps exactly this layout in front of its keep rows
    assert q.n_normal_rows == rows and torch.equal(q.noise_desc[:rows], p.noise_desc)
    assert p.noise_table[-1].tolist()[0] == 0 and q.noise_table[-1].tolist()[0] == len(q.noise_desc) - rows
    assert q.drop_sites[0]['mask'].storage_offset() - q.noise.storage_offset() == numel
    assert int(q.noise_desc[rows:, 0].min()) == numel
    # a step that draws its noise never calls the new launcher
    eng.train_step()
    eng.training = False
    eng.draw_noise()
    eng.forward()
    assert kernel_ref.CALLS['fill_noise_rows'] == 0 and kernel_ref.CALLS['mask_scale'] == 0
    drp.train_step()
    assert kernel_ref.CALLS['fill_noise_rows'] == 1 and kernel_ref.CALLS['mask_scale'] == 2 * len(q.drop_sites)


# ------------------------------------------------------------------------------------------------ 3. column-constant masks
@pytest.mark.parametrize('fused', [True, False], ids=['step', 'loss+backward'])
@pytest.mark.parametrize('keep', [0.5, 0.8])
@pytest.mark.parametrize('name', STEP_CASES)
def test_column_constant_masks_reduce_to_the_undropped_step(name, keep, fused, monkeypatch):
    """a mask that is the same in every row is a diagonal scaling of the next layer's weight: losses and every gradient of
    the dropped step equal those of a rate-0 engine with W' = W diag(m / keep) behind each site (dW = dW' diag(m / keep))"""
    kernel_ref.install(monkeypatch)
    eng, ref, arena, rarena = dropped_vs_folded(name, keep, fused)
    assert kernel_ref.CALLS['fill_noise_rows'] == 0, 'injected noise and injected masks: nothing is drawn'
    assert kernel_ref.CALLS['mask_scale'] == 2 * len(eng.dropout_sites())
    compare_step(eng, ref, arena, rarena, '%s keep %.1f' % (name, keep))


# ------------------------------------------------------------------------------------------------ 4. row keying
def _row_keys(p, row0):
    """per chain the identity of every stacked row, from the plan's POSITIONS (not from its descriptors)"""
    L, B, Np = p._cfg.L, p.B, p.Np
    g = row0 + np.asarray(p.rows)
    gp = g[p.pair_host]
    keys = {'c_enc': [('x1', int(r)) for r in g] + [('x2', int(r)) for r in gp],
            'c_decx': [('z1', l, int(r)) for l in range(L) for r in g] + [('z2', l, int(r)) for l in range(L) for r in gp]
            + [('z2F', l, int(r)) for l in range(L) for r in gp],
            'c_clf': [(l, int(r)) for l in range(L) for r in g]}
    if p._cfg.has_y:
        fp = [(int(l), int(s), int(g[i])) for l, s, i in zip(p.fp_l_host, p.fp_slot_host, p.fp_i_host)]
        keys['c_top'] = keys['c_dz1'] = fp
    return keys


def test_masks_are_keyed_by_global_row(monkeypatch):
    """two plans over the two halves of a batch (``row0`` = 0 and k) draw, row for row, the masks of the single plan"""
    kernel_ref.install(monkeypatch)
    spec = C.tiny_spec('drvae', dim_y=3, h_clf=[3], h_de_x=[8, 5])
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 12, seed=4)
    batch['has_y'], batch['has_x2'] = C._flags('acbdabcdbdca')
    k, seed = 5, 12345
    ctr = torch.tensor([7, 0], dtype=torch.int32)
    drawn = []
    for row0, rows in ((0, None), (0, slice(0, k)), (k, slice(k, 12))):
        eng, _ = make_engine(spec, params, rate=0.3, row0=row0)
        p = set_batch(eng, batch, rows=rows)
        eng.rng_ctr.copy_(ctr)
        eng.draw_noise()
        desc = p.noise_desc.numpy()
        nn = p.n_normal_rows
        # draw ids: keep rows one past every normal id, one block per site, one id per replica within it
        assert desc[nn:, 2].min() > desc[:nn, 2].max() and len(desc) > nn
        keys, r0, table = _row_keys(p, row0), nn, {}
        seen = set()
        for s in p.drop_sites:
            d = desc[r0:r0 + s['M']]
            r0 += s['M']
            ids = set(d[:, 2].tolist())
            assert not (ids & seen), 'two sites share a draw id'
            seen |= ids
            assert len({(a, b) for a, b in d[:, 2:4].tolist()}) == s['M'], 'two rows of a site share (draw id, global row)'
            kk = keys[s['chain']]
            assert len(kk) == s['M'] and len(set(kk)) == s['M']
            # one draw id per replica: rows with the same identity up to the global row share it, others do not
            rep = {}
            for key, (did, grow) in zip(kk, d[:, 2:4].tolist()):
                assert grow == key[-1]
                assert rep.setdefault(key[:-1], did) == did
            assert len(set(rep.values())) == len(rep)
            assert set(np.unique(s['mask'].numpy())) <= {0.0, 1.0}
            table[(s['chain'], s['layer'])] = dict(zip(kk, s['mask'].numpy().copy()))
        assert r0 == len(desc)
        drawn.append(table)
    full, lo, hi = drawn
    assert set(full) == set(lo) == set(hi) and len(full) == 6
    for site, rows in full.items():
        halves = dict(lo[site])
        assert not (set(halves) & set(hi[site]))
        halves.update(hi[site])
        assert set(halves) == set(rows), site
        for key, m in rows.items():
            assert np.array_equal(m, halves[key]), (site, key)
        kept = np.mean([m.mean() for m in rows.values()])
        assert 0.4 < kept < 0.95            # (rate 0.3: a mask, not a constant)


# ------------------------------------------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_vfae', 'tiny_pvae'])
def test_evaluation_drops_nothing(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case = C.model_case(name)
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    out = []
    for rate in (0.5, 0.0):
        eng, _ = make_engine(spec, params, rate=rate)
        set_batch(eng, case['batch'])
        eng.training = False
        eng.set_noise(case['noises'][0])
        eng.forward()
        out.append(eng.losses())
        eng.draw_noise()              # an evaluation draw skips the keep rows as it skips the input noise
        eng.forward()
    assert kernel_ref.CALLS['fill_noise_rows'] == 0 and kernel_ref.CALLS['mask_scale'] == 0
    assert list(out[0].values()) == list(out[1].values())          # bit-equal


# ------------------------------------------------------------------------------------------------ 6. schedule
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_vfae', 'tiny_pvae'])
def test_a_plan_with_sites_never_draws_ahead(name, monkeypatch):
    """the side chain's draw-ahead is released when the encoder backward starts; with sites that backward reads its masks:
    every tail the schedule builds for such a plan has ``noise_ahead`` off, and the recorded step draws at its head"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    case = C.model_case(name)
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    ahead = {}
    for rate in (0.0, 0.5):
        for universal in (False, True):
            eng, _ = make_engine(spec, params, rate=rate)
            eng.universal = universal
            set_batch(eng, case['batch'])
            eng.set_noise(case['noises'][0])
            for split in (False, True, 'overlap', 'captured'):
                tail = eng._step_tail(split, on_gpu=True)
                ahead[(rate, universal, split)] = tail.noise_ahead
                if rate and tail.dual:
                    names = {}
                    for chain in ('main', 'side'):
                        log = names[chain] = []
                        with pytest.MonkeyPatch.context() as mp:
                            for fn in ('fill_noise_rows', 'fill_normal_rows', 'mask_scale', 'rows_gather'):
                                real = getattr(K, fn)
                                mp.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append(_n), _f(*a, **k))[1])
                            with eng._recording(chain, tail):
                                eng._launch_sequence(draw=chain == 'main', optimizer=False)
                    assert names['main'][0] == 'fill_noise_rows' and names['main'].count('fill_noise_rows') == 1
                    assert 'fill_noise_rows' not in names['side'] and 'fill_normal_rows' not in names['main'] + names['side']
    assert not any(v for (rate, _, _), v in ahead.items() if rate), ahead
    assert any(v for (rate, _, _), v in ahead.items() if not rate), 'the rate-0 step still draws ahead'
