"""-m gpu: hidden-layer dropout of the fused train step on the device -- ``dv_fill_noise_rows`` element by element against the
numpy Philox reference, one chain with device-drawn masks against float64, the model step with column-constant masks
(tests/test_dropout_cpu.py on the device, eager and captured), finite differences, fresh masks per step, and the rate-0 step's
launch list."""
import gc
import math

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import gemm_contract as G
from tests import kernel_ref
from tests import ref64
from tests.golden import cases as C
from tests.ref64 import U
from tests.test_dropout_cpu import (STEP_CASES, compare_step, dropped_vs_folded, make_engine, set_batch, tiny_model)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
NOISE = 'dv_fill_noise_rows'        # the draw of a step with keep rows in the launch lists


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def thr_of(rate):
    return min(int(math.floor((1.0 - rate) * 4294967296.0)), 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ 1. the keep-row draw
WIDTHS = (1, 3, 4, 5, 64, 67, 200)
TINY_RATE = 5e-8               # keep_thr = 2^32 - 214: within a few hundred units of 2^32


def table(n_rows):
    """rows of every width, at offsets that are and are not 16-byte aligned, with sentinel gaps between them"""
    rows, off = [], 0
    for r in range(n_rows):
        w = WIDTHS[(r + r // 7) % len(WIDTHS)]
        off += (0, 1, 4, 2)[r % 4]
        rows.append((off, w, 100 + r % 5, 1000 + 7 * r))
        off += w
    d = np.asarray(rows, np.int64)
    assert {int(o) % 4 for o in d[:, 0]} == ({0} if n_rows == 1 else {0, 1, 2, 3})
    return d, off + 8


@pytest.mark.parametrize('n_normal', ['none', 'all', 'between'])
@pytest.mark.parametrize('n_rows', [1, 300])
def test_fill_noise_rows_matches_the_reference_exactly(K, dev, n_rows, n_normal):
    assert 0 < 2 ** 32 - thr_of(TINY_RATE) < 500 and K.keep_threshold(TINY_RATE) == thr_of(TINY_RATE)
    assert K.keep_threshold(0.5) == 2 ** 31 and K.keep_threshold(0.0) == 0xFFFFFFFF
    d, size = table(n_rows)
    nn = {'none': 0, 'all': n_rows, 'between': n_rows // 3}[n_normal]
    desc = torch.as_tensor(d, dtype=torch.int32, device=dev)
    described = np.zeros(size, bool)
    for o, w, _, _ in d:
        assert not described[o:o + w].any()
        described[o:o + w] = True
    seed = 0x1234ABCD5678
    for event in ((0, 0), (5, 3)):              # (the second: a non-zero high word, folded into the key)
        ctr = torch.tensor(event, dtype=torch.int32, device=dev)
        ev = event[1] << 32 | event[0]
        want_n = torch.full((size,), SENTINEL, device=dev)
        if nn:
            K.fill_normal_rows(want_n, desc[:nn], seed, ctr)
        for rate in (0.5, 0.2, TINY_RATE):
            thr = thr_of(rate)
            got = torch.full((size,), SENTINEL, device=dev)
            K.fill_noise_rows(got, K.noise_table(desc, nn, thr), seed, ctr)
            torch.cuda.synchronize()
            g = got.cpu().numpy()
            assert (g[~described] == np.float32(SENTINEL)).all(), 'written outside the described elements'
            # the normal rows: what dv_fill_normal_rows writes for the same rows, bit for bit
            nmask = np.zeros(size, bool)
            for o, w, _, _ in d[:nn]:
                nmask[o:o + w] = True
            assert np.array_equal(g[nmask].view(np.int32), want_n.cpu().numpy()[nmask].view(np.int32))
            # the keep rows: the reference mask element for element, exactly 0.0 or 1.0
            offs, vals = kernel_ref.keep_rows(d[nn:], thr, seed, ev)
            assert len(offs) == int(d[nn:, 1].sum())
            assert np.array_equal(g[offs], vals) and set(np.unique(g[offs])) <= {0.0, 1.0}
            if rate == TINY_RATE and len(offs) > 1000:
                assert vals.mean() > 0.999


def test_fill_noise_rows_keeps_the_stated_fraction(K, dev):
    """8192 rows x 256 columns, seed 1234, event 0, draw id 100: the kept fraction lies within 4 sigma of keep_thr / 2^32 (the
    numpy reference alone: +0.20, -0.98, -1.66 sigma).  The mask is compared exactly above: this guards the specification."""
    R, W = 8192, 256
    d = np.stack([np.arange(R) * W, np.full(R, W), np.full(R, 100), np.arange(R)], 1)
    desc = torch.as_tensor(d, dtype=torch.int32, device=dev)
    for rate in (0.5, 0.3, 0.1):
        thr = thr_of(rate)
        got = torch.zeros(R * W, device=dev)
        K.fill_noise_rows(got, K.noise_table(desc, 0, thr), 1234, None)
        keep, n = thr / 2.0 ** 32, R * W
        z = (float(got.double().mean()) - keep) / math.sqrt(keep * (1 - keep) / n)
        print('rate %.1f: kept fraction %+.2f sigma from keep_thr / 2^32' % (rate, z))
        assert abs(z) <= 4.0
        offs, vals = kernel_ref.keep_rows(d, thr, 1234, 0)
        assert np.array_equal(got.cpu().numpy()[offs], vals)


# ------------------------------------------------------------------------------------------ 2. one chain against float64
def _fwd_check(site, got, x, W, b, scale, act0, act1, split, shift1):
    """a layer's forward against float64 on the inputs the launch read, bound as the FWD epilogue of
    ``gemm_contract.expected``: the accumulator's bound through scale and bias (three roundings), the activation by the rule of
    tests/ref64.py with C = 8 (its derivative is at most 1 for identity, elu and softplus), the shift once"""
    c64, dacc = G.acc_bound(x, W.t())
    s = scale.double() if scale is not None else torch.ones(W.shape[0], dtype=torch.float64)
    lin = c64 * s
    pre = lin + b.double()
    dpre = dacc * s.abs() + U * (2 * lin.abs() + pre.abs())
    cols = [(act0, slice(0, split), 0.0), (act1, slice(split, W.shape[0]), shift1)]
    y = torch.cat([ref64.act(a, pre[:, c]) + sh for a, c, sh in cols], 1)
    extra = torch.cat([ref64.act_exp_extra(a, pre[:, c]) for a, c, _ in cols], 1)
    bound = 1.01 * dpre + ref64.bound(8, y.abs(), extra) + U * y.abs()
    return ref64.check(site, got, y, bound), bound


def _wn_grads(raw, draw, W, g):
    """float64 autograd through W_eff = g W / |W| of the device's raw gradient, and its bound: the raw gradient's own bound
    ``draw`` carried through the (linear) map, plus the rule of tests/ref64.py with C = 32 on the terms' magnitudes (a row dot
    of at most 13 products, the norm, the combination)"""
    W64, g64 = W.double().requires_grad_(True), g.double().requires_grad_(True)
    n = W64.norm(dim=1, keepdim=True)
    ((g64[:, None] * W64 / n) * raw.double()).sum().backward()
    Wd, nd = W.double(), W.double().norm(dim=1, keepdim=True)
    s = (g.double()[:, None] / nd).abs()
    dot = (raw.double().abs() * Wd.abs()).sum(1, keepdim=True)
    ddot = (draw * Wd.abs()).sum(1, keepdim=True)
    bW = s * (draw + Wd.abs() * ddot / nd ** 2) + ref64.bound(32, s * (raw.double().abs() + Wd.abs() * dot / nd ** 2))
    bg = (ddot / nd + ref64.bound(32, dot / nd)).reshape(-1)
    return W64.grad, g64.grad, bW, bg


@pytest.mark.parametrize('wn', [False, True], ids=['plain', 'weightnorm'])
def test_one_chain_with_device_masks_against_float64(K, dev, wn):
    """a three-layer chain (sources 9 + 4 -> 11 -> 6 -> two heads of 5; 37 rows; elu, softplus on the second head), masks drawn
    on the device at rate 0.5.  Every launch of the pass against float64 on what the launch read -- the dropped buffers and the
    read-back masks included --, element by element within the fp32 contract of tests/gemm_contract.py (``acc_bound`` /
    ``expected`` / ``colsum_bound``); then the whole pass against a float64 torch-autograd MLP with the same masks, element by
    element too: every launch's contract bound plus what its operands' errors can move it by, carried through the layers."""
    from collections import OrderedDict
    from drvae_amd.arena import ParamArena
    from drvae_amd.chain import _Chain, _Lin
    Mr, keep = 37, 0.5
    shapes = OrderedDict()
    for name, (n_out, n_in) in (('b.nnet.model.linear1', (11, 13)), ('b.nnet.model.linear2', (6, 11)),
                                ('b.encoder_mu.linear_mu', (5, 6)), ('b.encoder_sg.linear_sg', (5, 6))):
        shapes[name + '.weight'], shapes[name + '.bias'] = (n_out, n_in), (n_out,)
        if wn:
            shapes[name + '.g'] = (n_out,)
    arena = ParamArena(shapes, dev)
    gen = torch.Generator().manual_seed(5)
    arena.load({k: (torch.randn(*s, generator=gen) * (0.4 if k.endswith('weight') else 0.2)
                    + (1.0 if k.endswith('.g') else 0.0)).numpy() for k, s in shapes.items()})
    gname = (lambda p: p + '.g') if wn else (lambda p: None)
    layers = [_Lin(arena, p + '.weight', p + '.bias', gname(p), act='elu') for p in ('b.nnet.model.linear1', 'b.nnet.model.linear2')]
    m, s = 'b.encoder_mu.linear_mu', 'b.encoder_sg.linear_sg'
    layers.append(_Lin(arena, m + '.weight', m + '.bias', gname(m), second=(s + '.weight', s + '.bias', gname(s)),
                       act='identity', act1='softplus', shift1=1e-3))
    chain = _Chain(layers, Mr, dev)
    # masks: two segments of an arena, drawn by the device
    sizes = [Mr * 11, Mr * 6]
    noise = torch.zeros(sum(sizes), device=dev)
    masks = [noise[:sizes[0]].view(Mr, 11), noise[sizes[0]:].view(Mr, 6)]
    rows = np.arange(Mr)
    desc = np.concatenate([np.stack([rows * 11, np.full(Mr, 11), np.full(Mr, 40), 300 + rows], 1),
                           np.stack([sizes[0] + rows * 6, np.full(Mr, 6), np.full(Mr, 41), 300 + rows], 1)])
    K.fill_noise_rows(noise, K.noise_table(torch.as_tensor(desc, dtype=torch.int32, device=dev), 0, thr_of(1 - keep)), 77, None)
    chain.add_dropout(masks, keep)
    pad = lambda r, c: torch.zeros(r, (c + 3) // 4 * 4, device=dev)[:, :c]
    x1, x2, d1, d2 = pad(Mr, 9), pad(Mr, 4), pad(Mr, 9), pad(Mr, 4)
    x1.copy_(torch.randn(Mr, 9, generator=gen))
    x2.copy_(torch.randn(Mr, 4, generator=gen))
    dlast = pad(Mr, 10)
    dlast.copy_(torch.randn(Mr, 10, generator=gen))
    chain.forward([x1, x2], drop=True)
    chain.backward(dlast, [x1, x2], [[(d1, 1.0, 0.0)], [(d2, 1.0, 0.0)]], drop=True)
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu()
    mk = [c(t) for t in masks]
    assert all(set(np.unique(t.numpy())) == {0.0, 1.0} for t in mk)
    worst = 0.0
    # the dropped buffers: exactly out * mask / keep, zero pads
    for li in range(2):
        assert torch.equal(c(chain.outd[li]), c(chain.out[li]) * mk[li] / keep)
        base = chain.outd[li]._base
        assert not bool(base[:, chain.outd[li].shape[1]:].any()), 'pad columns of outd'
    ins = [torch.cat([c(x1), c(x2)], 1), c(chain.outd[0]), c(chain.outd[1])]
    B = {}          # the per-launch bounds, kept: the end-to-end comparison below carries them from launch to launch
    for li, l in enumerate(layers):
        W, b = c(l.W), c(l.b)
        scale = c(l.scale) if wn else None
        if wn:      # the scale the launch multiplies by: g / |W|, a row norm of <= 13 terms (rule of tests/ref64.py, C = 32)
            s64 = c(l.g).double() / W.double().norm(dim=1)
            worst = max(worst, ref64.check('wn scale %d' % li, scale, s64, ref64.bound(32, s64.abs())))
        if li == 2:     # identity | softplus + shift: the FWD epilogue of ``gemm_contract.expected`` as it stands
            e = dict(kind='fwd', alpha=1.0, beta=0.0, C0=None, h=l.split, scale=scale if wn else torch.ones(l.N), bias=b,
                     resid=torch.zeros(Mr, l.split), act1=l.act1, shift1=ref64.f32(l.shift1))
            want, B['out', li], _ = G.expected(ins[li], W.t().contiguous(), e)
            worst = max(worst, ref64.check('forward %d' % li, c(chain.out[li]), want, B['out', li]))
        else:           # elu, which that helper does not know: its formula with elu's terms (``_fwd_check``)
            w_, B['out', li] = _fwd_check('forward %d' % li, c(chain.out[li]), ins[li], W, b, scale, l.act0, l.act1, l.split, l.shift1)
            worst = max(worst, w_)
    # backward, layer by layer from the top: the launch's upstream gradient is what the device holds
    ups = [c(chain.dpre[0]), c(chain.dpre[1]), c(dlast)]
    plain = dict(kind='plain', alpha=1.0, beta=0.0, h=0, C0=None)
    for li in (2, 1, 0):
        l, dy, x = layers[li], ups[li], ins[li]
        W = c(l.W)
        want_db, b_db = G.colsum_bound(dy)
        B['db', li] = b_db + U * want_db.abs()
        worst = max(worst, ref64.check('db %d' % li, c(l.db), want_db, B['db', li]))
        want_raw, b_raw, _ = G.expected(dy.t().contiguous(), x, dict(plain, h=x.shape[1]))
        B['raw', li] = b_raw
        if wn:
            raw = c(l.raw)
            worst = max(worst, ref64.check('raw dW %d' % li, raw, want_raw, b_raw))
            gW, gg, bW, bg = _wn_grads(raw, torch.zeros_like(b_raw), W, c(l.g))
            worst = max(worst, ref64.check('dW %d' % li, c(l.dW), gW, bW), ref64.check('dg %d' % li, c(l.dg), gg, bg))
            A = dy * c(l.scale)[None, :]           # (the data-gradient launch scales its operand: one fp32 rounding, as here)
        else:
            worst = max(worst, ref64.check('dW %d' % li, c(l.dW), want_raw, b_raw))
            A = dy
        if li > 0:      # (dy W) * act'(out) through the BWD epilogue's bound, then the mask: factors 0 and 2, exact
            prev = layers[li - 1]
            e = dict(kind='bwd', alpha=1.0, beta=0.0, h=prev.N, yref=c(chain.out[li - 1]), C0=None)
            want, bound, _ = G.expected(A, W, e)
            f = (mk[li - 1] / keep).double()
            B['dpre', li - 1] = bound * f
            worst = max(worst, ref64.check('dpre %d' % (li - 1), ups[li - 1], want * f, bound * f))
            assert bool((ups[li - 1][mk[li - 1] == 0] == 0).all())
        else:
            bs = []
            for dst, cols in ((d1, slice(0, 9)), (d2, slice(9, 13))):
                want, bound, _ = G.expected(A, W[:, cols].contiguous(), dict(plain, h=0))
                bs.append(bound)
                worst = max(worst, ref64.check('dx', c(dst), want, bound))
            B['dx'] = torch.cat(bs, 1)
    print('one chain (%s): worst error %.3f of the bound, launch by launch' % ('weightnorm' if wn else 'plain', worst))

    # ---- end to end: a float64 torch-autograd MLP with the read-back masks, from the chain's inputs alone, ELEMENT BY ELEMENT.
    # The bound of a quantity is its launch's contract bound (above, B) plus what the errors of the launch's operands can
    # move its float64 value by, carried from launch to launch with the exact magnitudes:
    #   forward   pre = s (x W^T) + b:   E_pre <= |s| (E_x |W|^T) + E_s |x W^T|;  identity, elu, softplus are 1-Lipschitz;
    #             the mask multiplies values and errors by 0 or 1 / keep
    #   backward  raw = G^T x:           E_raw <= E_G^T |x| + |G|^T E_x           (db: column sums of E_G)
    #             dpre' = ((G s) W) act'(y) f:  E <= (E_A |W|) |act'| + |(G s) W| E_y,  E_A = E_G |s| + |G| E_s
    #             (act' is taken from the stored output y, elu: |d act'/dy| <= 1, the error of y is the forward's E_y)
    #   WeightNorm maps raw to (dW, dg) linearly: ``_wn_grads`` carries E_raw through it
    # 1.01 covers the products of two errors, as in ``gemm_contract.acc_bound``.
    leaf = lambda t: c(t).double().requires_grad_(True)
    xin = leaf(torch.cat([x1, x2], 1))
    prm = [(leaf(l.W), leaf(l.b), leaf(l.g) if wn else None) for l in layers]
    h, outs, pres, hs = xin, [], [], []
    for li, (l, (W, b, g)) in enumerate(zip(layers, prm)):
        Weff = g[:, None] * W / W.norm(dim=1, keepdim=True) if wn else W
        hs.append(h.detach())
        pre = h @ Weff.t() + b
        pre.retain_grad()
        pres.append(pre)
        y = torch.cat([ref64.act(l.act0, pre[:, :l.split]), ref64.act(l.act1, pre[:, l.split:]) + l.shift1], 1)
        outs.append(y.detach())
        if li < 2:
            h = y * mk[li].double() / keep
    (pre * c(dlast).double()).sum().backward()
    Gref = [p_.grad for p_ in pres]
    W64 = [c(l.W).double() for l in layers]
    sdev = [c(l.scale).double() if wn else torch.ones(l.N, dtype=torch.float64) for l in layers]
    sref = [c(l.g).double() / w.norm(dim=1) if wn else torch.ones(l.N, dtype=torch.float64) for l, w in zip(layers, W64)]
    Es = [ref64.bound(32, s_.abs()) if wn else torch.zeros_like(s_) for s_ in sref]
    e2e = 0.0
    Ex, Exs, Ey = torch.zeros(Mr, 13, dtype=torch.float64), [], []
    for li, l in enumerate(layers):
        Exs.append(Ex)
        Epre = sdev[li].abs() * (Ex @ W64[li].abs().t()) + Es[li] * (hs[li] @ W64[li].t()).abs()
        Ey.append(B['out', li] + 1.01 * Epre)
        e2e = max(e2e, ref64.check('out %d end to end' % li, c(chain.out[li]), outs[li], Ey[li]))
        if li < 2:
            Ex = Ey[li] * mk[li].double() / keep
    EG = torch.zeros(Mr, 10, dtype=torch.float64)
    for li in (2, 1, 0):
        l, (W, b, g), Gr = layers[li], prm[li], Gref[li]
        e2e = max(e2e, ref64.check('db %d end to end' % li, c(l.db), b.grad, B['db', li] + 1.01 * EG.sum(0)))
        Eraw = B['raw', li] + 1.01 * (EG.t() @ ins[li].double().abs() + Gr.abs().t() @ Exs[li])
        if wn:
            _, _, bW, bg = _wn_grads(Gr.t() @ hs[li], Eraw, c(l.W), c(l.g))
            e2e = max(e2e, ref64.check('dW %d end to end' % li, c(l.dW), W.grad, 1.01 * bW),
                      ref64.check('dg %d end to end' % li, c(l.dg), g.grad, 1.01 * bg))
        else:
            e2e = max(e2e, ref64.check('dW %d end to end' % li, c(l.dW), W.grad, Eraw))
        Aref = Gr * sref[li]
        EA = EG * sdev[li].abs() + Gr.abs() * Es[li] + (U * Aref.abs() if wn else 0.0)
        if li > 0:
            dprime = ref64.dact_from_y('elu', c(chain.out[li - 1])).abs()
            f = mk[li - 1].double() / keep
            EG = B['dpre', li - 1] + 1.01 * ((EA @ W64[li].abs()) * dprime + (Aref @ W64[li]).abs() * Ey[li - 1]) * f
            e2e = max(e2e, ref64.check('dpre %d end to end' % (li - 1), ups[li - 1], Gref[li - 1], EG))
        else:
            e2e = max(e2e, ref64.check('dx end to end', torch.cat([c(d1), c(d2)], 1), xin.grad,
                                       B['dx'] + 1.01 * (EA @ W64[li].abs())))
    print('one chain (%s): worst error %.3f of the carried bound, end to end' % ('weightnorm' if wn else 'plain', e2e))


# ------------------------------------------------------------------------------------------ 3. the model step
def _zero_grads(e):
    e.arena.grad.zero_()
    e.arena.loss.zero_()


def _captured(e):
    """the pass (forward + backward on the injected noise and masks) as ONE captured graph, replayed once"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e._launch_sequence(draw=False, optimizer=False)          # warm-up: loads code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e.step_dev.zero_()
    _zero_grads(e)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            e._launch_sequence(draw=False, optimizer=False)
    finally:
        if on:
            gc.enable()
    _zero_grads(e)
    e.step_dev.zero_()
    g.replay()
    torch.cuda.synchronize()
    e._graph_keepalive = g


@pytest.mark.parametrize('keep', [0.5, 0.8])
@pytest.mark.parametrize('name', STEP_CASES)
def test_column_constant_masks_on_the_device(dev, name, keep):
    """tests/test_dropout_cpu.py's reduction to the undropped step on the device, eagerly and as a captured graph; the captured
    replay equals the eager pass bit for bit"""
    eng, ref, arena, rarena = dropped_vs_folded(name, keep, True, device=dev)
    torch.cuda.synchronize()
    compare_step(eng, ref, arena, rarena, '%s keep %.1f eager' % (name, keep))
    eager = (arena.grad.clone(), arena.loss.clone())
    ceng, cref, carena, crarena = dropped_vs_folded(name, keep, True, device=dev, step=_captured)
    compare_step(ceng, cref, carena, crarena, '%s keep %.1f captured' % (name, keep))
    assert torch.equal(carena.grad, eager[0]) and torch.equal(carena.loss, eager[1])


def test_captured_step_with_philox_masks_replays_like_the_eager_one(dev):
    case = C.model_case('tiny_drvae')
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    eng, arena = make_engine(spec, params, rate=0.5, device=dev)
    set_batch(eng, case['batch'], dev)
    eng.train_step()
    eng.capture()
    assert not eng.noise_ahead
    for _ in range(3):
        eng.replay()
    eng.check_sync()
    losses = eng.losses()
    eng2, arena2 = make_engine(spec, params, rate=0.5, device=dev)
    set_batch(eng2, case['batch'], dev)
    for _ in range(4):
        eng2.train_step()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses.values())
    assert eng2.losses() == losses and torch.equal(arena2.param, arena.param)
    assert all(torch.equal(a['mask'], b['mask']) for a, b in zip(eng.dropout_sites(), eng2.dropout_sites()))


# ------------------------------------------------------------------------------------------ 4. finite differences
def test_backward_matches_finite_differences_with_held_masks(dev):
    """<grad, d> == (f(theta + e d) - f(theta - e d)) / 2e along 8 random relative directions, noise and masks held by
    injection; f is the objective the hand-written backward differentiates (CMPL, minus the ELBO plus the label term), step
    size and bound as tests/test_gpu_properties.py"""
    case = C.model_case('tiny_drvae')
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    eng, arena = make_engine(spec, params, rate=0.5, device=dev)
    set_batch(eng, case['batch'], dev)
    eng.training = True
    eng.set_noise(case['noises'][0])
    rs = np.random.RandomState(2)
    eng.set_dropout_masks({i: (rs.rand(s['M'], s['N']) < 0.5).astype(np.float32) for i, s in enumerate(eng.dropout_sites())})
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    n = arena.n_params
    grad, theta = arena.grad[:n].clone(), arena.param.clone()

    def cmpl(t):
        arena.param.copy_(t)
        eng.forward()
        return float(arena.loss[6])
    g = torch.Generator().manual_seed(0)
    eps = 1e-2
    for k in range(8):
        d = torch.randn(n, generator=g).to(dev) * theta.abs().clamp(min=1e-3)
        lin = float((grad.double() * d.double()).sum())
        fd = (cmpl(theta + eps * d) - cmpl(theta - eps * d)) / (2 * eps)
        print('direction %d: finite difference %.6g, gradient %.6g' % (k, fd, lin))
        assert abs(fd - lin) <= 3e-2 * max(1.0, abs(lin)), (k, fd, lin)
    arena.param.copy_(theta)


# ------------------------------------------------------------------------------------------ 5. fresh masks, same masks
def test_fresh_masks_per_step_and_one_mask_per_step(dev):
    case = C.model_case('tiny_drvae')
    spec, params = case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)
    eng, arena = make_engine(spec, params, rate=0.5, device=dev)
    p = set_batch(eng, case['batch'], dev)
    eng.train_step()
    eng.capture()
    seen = []
    for _ in range(2):
        eng.replay()
        torch.cuda.synchronize()
        eng.check_sync()
        sites = eng.dropout_sites()
        seen.append([s['mask'].clone() for s in sites])
        for s in sites:
            ch = getattr(p, s['chain'])
            li = s['layer'] - 1
            m = s['mask']
            # forward and backward of the step used THIS mask: the dropped activation and the gradient vanish where it does
            assert torch.equal(ch.outd[li], ch.out[li] * m * 2.0)
            assert bool((ch.dpre[li][m == 0] == 0).all())
            # ... and only there, in every row that carries a gradient at all (a row whose KL terms sit at their free-bits
            # floor carries none: q(z2|x2) rows of the encoder, fprop rows)
            live = (ch.dpre[li] != 0).any(1)
            assert bool(live.any()) and torch.equal(ch.dpre[li][live] == 0, m[live] == 0)
            if s['chain'] == 'c_decx':                  # (every reconstruction row carries one)
                assert bool(live.all())
            assert 0.2 < float(m.mean()) < 0.8
    assert len(seen[0]) == 4
    for a, b in zip(*seen):
        assert not torch.equal(a, b)


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_fit_with_dropout_trains_and_evaluates_undropped(dev, kind, tmp_path, monkeypatch):
    from drvae_amd import _lib
    from tests.test_fit import _loader, _tiny_dataset
    with pytest.warns(UserWarning, match='dropout_rate'):
        model = tiny_model(kind, dropout_rate=0.5, device=dev)
    model.w2log = lambda *a: None
    tr, va = _tiny_dataset(kind, 40, 1, dev), _tiny_dataset(kind, 24, 2, dev)
    names = {'train': [], 'eval': []}
    state = {'in': 'train'}
    real = _lib.check
    monkeypatch.setattr(_lib, 'check', lambda code, what: (names[state['in']].append(what), real(code, what))[1])
    real_eval = model.evaluate_performance_on_dataset

    def evaluating(*a, **k):
        state['in'] = 'eval'
        try:
            return real_eval(*a, **k)
        finally:
            state['in'] = 'train'
    monkeypatch.setattr(model, 'evaluate_performance_on_dataset', evaluating)
    model.fit(_loader(tr, 8), _loader(va, 8), add_noise=True, verbose=False, early_stop=False,
              model_filename=str(tmp_path / 'b.pth'))
    assert model.finished_training_iters == 2 * 5
    perf, _ = model.evaluate_performance_on_dataset(va)
    assert all(np.isfinite(float(v)) for v in perf['losses'].values())
    assert bool(torch.isfinite(model.engine().arena.param).all())
    assert names['eval'] and 'dv_mask_scale' not in names['eval'] and NOISE not in names['eval']
    assert 'dv_mask_scale' in names['train'] and NOISE in names['train']


# ------------------------------------------------------------------------------------------ 6. rate 0
def _captured_launch_names(eng, monkeypatch):
    from drvae_amd import _lib
    log, on = [], {'on': False}
    real = _lib.check
    real_main = eng._capture_main

    def check(code, what):
        if on['on'] and not what.startswith('dv_gemm_set_option'):
            log.append(what)
        return real(code, what)

    def capture_main(*a, **k):          # (the warm-up pass in front of the capture is not part of the step)
        on['on'] = True
        return real_main(*a, **k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, 'check', check)
        mp.setattr(eng, '_capture_main', capture_main)
        eng.capture()
    return log


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_rate_zero_step_launches_what_it_always_did(dev, kind, monkeypatch):
    """the captured step at the benchmark's batch shape: at rate 0 no launch of the feature appears (its count is guarded by
    tests/test_gpu_engine.py); in the one-graph schedule, where both steps draw at their head, the dropped step IS the rate-0
    step plus one ``dv_mask_scale`` per site and pass, with ``dv_fill_noise_rows`` in the draw's place"""
    from tests.test_gpu_x3 import tuned
    spec = M.ModelSpec(kind=kind, L=1 if kind == 'pvae' else 2)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    lists = {}
    for tune in ('', 'sched=3'):
        with tuned(tune):
            for rate in (0.0, 0.5):
                eng, _ = make_engine(spec, params, rate=rate, device=dev)
                set_batch(eng, batch, dev)
                eng.train_step()
                lists[(tune, rate)] = _captured_launch_names(eng, monkeypatch)
                eng.replay()
                torch.cuda.synchronize()
                eng.check_sync()
                n_sites = len(eng.dropout_sites())
    for tune in ('', 'sched=3'):
        plain = lists[(tune, 0.0)]
        assert plain and NOISE not in plain and 'dv_mask_scale' not in plain
    assert lists[('', 0.0)].count('dv_fill_normal_rows') == 1
    plain, dropped = lists[('sched=3', 0.0)], lists[('sched=3', 0.5)]
    assert dropped.count('dv_mask_scale') == 2 * n_sites and dropped.count(NOISE) == 1
    folded = ['dv_fill_normal_rows' if w == NOISE else w for w in dropped if w != 'dv_mask_scale']
    assert folded == plain
    print('%s: %d launches at rate 0, %d at rate 0.5 (%d sites)' % (kind, len(plain), len(dropped), n_sites))
