"""The two folded launches of ``Tail.fold_rows`` below model level: their cases, a staged float64 reference and faulty host
emulations that show the checks have teeth.  Plain torch on the host, no library call; ``tests/test_fold_rows_cpu.py`` runs
it without a device, ``tests/test_gpu_fold_rows.py`` holds the kernels to it.

``z2f_post_bwd`` with ``kl_out`` / ``seg`` / ``z1_dz2f`` computes, per batch row i (pair slot jp or -1) and sample l
(r = l*B + i, kr = l*Np + jp):

    raw[kr], kl[kr]     the KL(q2[jp] || p2[r]) row sum and its free-bits value max(raw, kl_min)
    dp2[r]              reparam backward of the z2Fz1 sample + the gated KL gradient w.r.t. p2
    dq2[jp]             sum over l of the gated KL gradient w.r.t. q2
    dz1[r]             += dp2[r].mu + ((dz1b[r] + seg_beta * sum_t seg_src[t]) + z1_dz2f * dz2f[r])

``smalln_fwd`` with ``dgrad`` writes dst_t[r] = beta_t dst_t[r] + dlogit[r] . (alpha_t W[:, col0_t:] + alpha2_t W[:, col1_t:])
from the ``dqy`` / ``probs`` the same launch stored.

The reference is STAGED (the rule of ``tests/clf_launch_ref.py`` / ``tests/ref64.py``): every stage takes as exact inputs
the fp32 values the stage in front of it stored -- the gate reads the stored raw, dz1 the stored dp2 -- so each bound stays
componentwise, C * 2^-24 * sum |components| with the constants the suite uses for the same expressions."""
import math
import os

import torch

from tests import kernel_ref
from tests.ref64 import bound, excess, f32, f64, row_sum_bound

SENTINEL = 7.0
PAD_COLS, PAD_ROWS = 3, 2

C_KL = 16       # KL forward and backward: two exps, a division and a sum of four terms per element (test_gpu_numerics)
C_SUM = 8       # a handful of additions of stored values (the d/dz1 shares: at most 3 fprop rows + 4 terms)
C_DLOGIT = 8    # clamp + softmax backward: a dot product of Y terms, a difference and a product (softmax_clamp_bwd)
C_DOT = 2       # a dot product's terms and the scaling, per term (clf_launch_ref)

Z2F_OUT = ('raw', 'kl', 'dp2', 'dq2', 'dz1')


def _wide(t, junk=1e3):
    buf = torch.full((t.shape[0] + PAD_ROWS, t.shape[1] + PAD_COLS), junk, dtype=torch.float32)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf


# ---------------------------------------------------------------------------------------------- z2f_post_bwd
def make_z2f_case(Z, L, B, Np, seg=True, dz2f=True, tie=True, seed=0):
    """one case: fp32 host operands, every matrix a view into a wider buffer with junk pads (row strides larger than the
    widths).  Pairs sit on the odd rows first (mixed singletons), then wherever rows are left.  The raw KL terms spread over
    1.5 decades; ``kl_min`` is chosen between them -- and, with ``tie``, is exactly one row's computed raw value (set by
    the caller from a first launch: ``with_tie``)"""
    g = torch.Generator().manual_seed(1009 * seed + 7 * Z + 3 * L + Np)
    rn = lambda *s: torch.randn(*s, generator=g)              # noqa: E731
    order = [i for i in range(B) if i % 2] + [i for i in range(B) if not i % 2]
    slot = torch.full((B,), -1, dtype=torch.int32)
    for jp, i in enumerate(order[:Np]):
        slot[i] = jp
    R = L * B
    spread = torch.exp(torch.rand(R, 1, generator=g) * math.log(30.0) + math.log(0.05))
    q2 = rn(max(Np, 1), 2 * Z) * 0.5
    p2 = rn(R, 2 * Z) * 0.5
    for l in range(L):
        for i in range(B):
            if slot[i] >= 0:
                p2[l * B + i] = q2[slot[i]] + spread[l * B + i] * rn(2 * Z) * 0.5
    nseg = torch.tensor([(r % 3) + 1 for r in range(R)])      # segments of 1, 2 and 3 fprop rows
    seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), nseg.cumsum(0)]).to(torch.int32)
    mats = dict(p2=p2, q2=q2, eps=rn(R, Z), dz1=rn(R, Z), dz1b=rn(R, Z), pert=rn(max(L * Np, 1), Z),
                seg_src=rn(int(seg_ptr[-1]), Z + 2))
    if dz2f:
        mats['dz2f'] = rn(R, Z)
    case = dict(name='Z%d-L%d-B%d-Np%d%s%s' % (Z, L, B, Np, '' if seg else '-noseg', '' if dz2f else '-nodz2f'),
                shape=(Z, L, B, Np), seg=seg, has_dz2f=dz2f, tie=tie, slot=slot, seg_ptr=seg_ptr,
                coef=rn(max(L * Np, 1)), bufs={k: _wide(v.float()) for k, v in mats.items()},
                dims={k: tuple(v.shape) for k, v in mats.items()}, kl_min=0.0)
    raw = f64(z2f_reference(case, None)['raw'][0]) if Np else torch.zeros(0, dtype=torch.float64)
    if Np:
        srt = torch.sort(raw)[0]
        mid = srt.numel() // 2
        case['kl_min'] = f32(0.5 * float(srt[max(mid - 1, 0)] + srt[mid])) if srt.numel() > 1 else f32(float(srt[0]) - 1.0)
    return case


def with_tie(case, stored_raw):
    """the case with ``kl_min`` set to a raw value a launch computed (the middle one): that row's gate is the tie"""
    c = dict(case)
    srt = torch.sort(stored_raw.reshape(-1))[0]
    c['kl_min'] = float(srt[srt.numel() // 2])
    return c


def z2f_operands(case, dev=None):
    Z, L, B, Np = case['shape']
    o = {}
    for k, buf in case['bufs'].items():
        b = buf if dev is None else buf.to(dev)
        r, c = case['dims'][k]
        o[k] = b[:r, :c]
    for k in ('slot', 'seg_ptr', 'coef'):
        o[k] = case[k] if dev is None else case[k].to(dev)
    o.setdefault('dz2f', None)
    return o


def z2f_alloc(case, o, dev=None):
    """{name: (buffer, view)}: outputs prefilled with the sentinel inside wider buffers; dz1 (in/out) starts from its operand"""
    Z, L, B, Np = case['shape']
    dev = dev or torch.device('cpu')
    out = {}
    for k, (rows, cols) in (('dp2', (L * B, 2 * Z)), ('dq2', (max(Np, 1), 2 * Z)), ('dz1', (L * B, Z))):
        buf = torch.full((rows + PAD_ROWS, cols + PAD_COLS), SENTINEL, device=dev)
        out[k] = (buf, buf[:rows, :cols])
    for k in ('raw', 'kl'):
        buf = torch.full((max(L * Np, 1) + PAD_COLS,), SENTINEL, device=dev)
        out[k] = (buf, buf[:max(L * Np, 1)])
    out['dz1'][1].copy_(o['dz1'])
    return out


def z2f_launch(mod, case, o, out, fold_kl=True, raw_in=None):
    """the launch through ``mod`` (drvae_amd.kernels, tests.kernel_ref or a faulty emulation).  ``fold_kl`` False:
    the KL rows are an input (``raw_in``), the old form of the same launcher"""
    Z, L, B, Np = case['shape']
    v = {k: b[1] for k, b in out.items()}
    kw = dict(seg=(o['seg_src'], o['seg_ptr'], 1.0) if case['seg'] else None, z1_dz2f=-1.0 if case['has_dz2f'] else 0.0)
    if fold_kl and Np:
        kw['kl_out'] = v['kl'][:L * Np]
    raw = v['raw'][:L * Np] if (fold_kl or raw_in is None) else raw_in
    mod.z2f_post_bwd(v['dp2'], v['dz1'], v['dq2'][:Np] if Np else None, o['dz2f'], o['pert'][:L * Np] if Np else None,
                     o['slot'], o['eps'], o['p2'], o['q2'][:Np] if Np else None, o['coef'][:L * Np], raw, case['kl_min'],
                     o['dz1b'], L, B, Np, **kw)


def to_host(out):
    res = {}
    for k, (b, v) in out.items():
        hb = b.detach().cpu().clone()
        res[k] = (hb, torch.as_strided(hb, v.size(), v.stride(), v.storage_offset()))
    return res


def z2f_reference(case, stored):
    """{stage: (ref, bound)} in float64; ``stored`` (None: the raw stage alone): the fp32 values a launch left, by name"""
    Z, L, B, Np = case['shape']
    o = z2f_operands(case)
    slot = o['slot'].long()
    pair = slot >= 0
    ii = torch.arange(B)[pair]
    jp = slot[pair]
    p2, q2 = f64(o['p2']), f64(o['q2'])
    ref = {}
    R = L * B
    rows = (torch.arange(L)[:, None] * B + ii[None, :]).reshape(-1)          # p row of KL row l*Np' + k (pairs in row order)
    krow = (torch.arange(L)[:, None] * Np + jp[None, :]).reshape(-1)
    mq, lq = q2[jp.repeat(L), :Z], q2[jp.repeat(L), Z:]
    mp, lp = p2[rows, :Z], p2[rows, Z:]
    dm, ivp, vq = mq - mp, torch.exp(-lp), torch.exp(lq)
    raw = torch.zeros(max(L * Np, 1), dtype=torch.float64)
    braw = torch.zeros_like(raw)
    if Np:
        comps = 1 + lp.abs() + lq.abs() + (dm * dm + vq) * ivp
        raw[krow] = -0.5 * (1 - lp + lq - (dm * dm + vq) * ivp).sum(1)
        braw[krow] = 0.5 * (bound(C_KL, comps).sum(1) + row_sum_bound(comps, Z))
    ref['raw'] = (raw, braw)
    if stored is None:
        return ref
    m = f64(f32(case['kl_min']))
    sr = f64(stored['raw'])
    ref['kl'] = (torch.clamp(sr, min=m), torch.zeros_like(sr))             # (a selection: exact)
    gate = torch.where(sr > m, 1.0, torch.where(sr == m, 0.5, 0.0)).double()
    c = (f64(o['coef']) * gate)[krow][:, None] if Np else None
    g = f64(o['dz2f']) if o['dz2f'] is not None else torch.zeros(R, Z, dtype=torch.float64)
    gc = g.abs().clone()
    if Np:
        pert = f64(o['pert'])[krow]
        g = g.clone()
        g[rows] = g[rows] + pert
        gc[rows] = gc[rows] + pert.abs()
    P2m, P2l = p2[:, :Z], p2[:, Z:]
    e = f64(o['eps'])
    dmu, dlv = g.clone(), g * e * 0.5 * torch.exp(0.5 * P2l)
    dmu_c, dlv_c = gc.clone(), gc * e.abs() * 0.5 * torch.exp(0.5 * P2l)
    dq = torch.zeros(max(Np, 1), 2 * Z, dtype=torch.float64)
    dq_c = torch.zeros_like(dq)
    if Np:
        gm, gl = c * dm * ivp, c * (-0.5 * (1 - vq * ivp))
        dmu[rows] = dmu[rows] - gm
        dlv[rows] = dlv[rows] + c * (-0.5 * (-1 + (dm * dm + vq) * ivp))
        dmu_c[rows] = dmu_c[rows] + gm.abs()
        dlv_c[rows] = dlv_c[rows] + 0.5 * c.abs() * (1 + (dm * dm + vq) * ivp)
        jj = jp.repeat(L)
        dq.index_add_(0, jj, torch.cat([gm, gl], 1))
        dq_c.index_add_(0, jj, torch.cat([gm.abs(), 0.5 * c.abs() * (1 + vq * ivp)], 1))
    ref['dp2'] = (torch.cat([dmu, dlv], 1), bound(C_KL, torch.cat([dmu_c, dlv_c], 1)))
    ref['dq2'] = (dq, bound(C_KL, dq_c))
    # d/dz1 on the STORED dp2 means: a few additions of fp32 values
    sm = f64(stored['dp2'])[:, :Z]
    share = f64(o['dz1b'])
    share_c = share.abs()
    if case['seg']:
        ptr = o['seg_ptr'].long()
        own = torch.repeat_interleave(torch.arange(R), ptr[1:] - ptr[:-1])
        src = f64(o['seg_src'])[:, :Z]
        share = share.index_add(0, own, src)
        share_c = share_c.index_add(0, own, src.abs())
    if case['has_dz2f']:
        share = share - f64(o['dz2f'])
        share_c = share_c + f64(o['dz2f']).abs()
    z0 = f64(o['dz1'])
    ref['dz1'] = (z0 + sm + share, bound(C_SUM, z0.abs() + sm.abs() + share_c))
    return ref


def _memory(host, inside):
    """(pads untouched, views written): ``inside`` = {name: boolean mask of the view's elements the launch must write}"""
    untouched = written = True
    for k, (buf, view) in host.items():
        outside = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(outside, view.size(), view.stride(), view.storage_offset()).fill_(False)
        untouched &= bool((buf[outside] == SENTINEL).all())
        mask = inside.get(k)
        if mask is None:
            untouched &= bool((view == SENTINEL).all())
        else:
            written &= bool((view[mask] != SENTINEL).all())
            untouched &= bool((view[~mask] == SENTINEL).all())
    return untouched, written


def z2f_verify(case, host, raises=True, site=''):
    """hold what a launch left to the reference, stage by stage, and to the memory contract: {check: worst excess}"""
    Z, L, B, Np = case['shape']
    stored = {k: v for k, (_, v) in host.items()}
    ref = z2f_reference(case, stored)
    ones = lambda k: torch.ones_like(stored[k], dtype=torch.bool)        # noqa: E731
    inside = dict(dp2=ones('dp2'), dz1=ones('dz1'))
    if Np:
        inside.update(raw=ones('raw'), kl=ones('kl'), dq2=ones('dq2'))
    untouched, written = _memory(host, inside)
    worst = {'pads': 0.0 if untouched else math.inf, 'written': 0.0 if written else math.inf}
    if raises:
        assert untouched, '%s pads: an element outside the outputs\' extent lost the sentinel' % site
        assert written, '%s written: an element inside the outputs\' extent still holds the sentinel' % site
    for k in Z2F_OUT:
        if not Np and k in ('raw', 'kl', 'dq2'):
            continue
        r, b = ref[k]
        e = excess(stored[k], r, b)
        worst[k] = float(e.max()) if e.numel() else 0.0
        if raises:
            assert worst[k] <= 1.0, '%s %s: worst %.3g x bound' % (site, k, worst[k])
    return worst


def kl_rows_separate(mod, case, o, dev=None):
    """(kl, raw) of the separate launch ``mod.kl_rows_fwd`` on the case's operands: what the folded launch must equal bit
    for bit"""
    Z, L, B, Np = case['shape']
    kl, raw = torch.zeros(L * Np, device=dev), torch.zeros(L * Np, device=dev)
    q2, p2 = o['q2'][:Np], o['p2']
    mod.kl_rows_fwd(kl, raw, q2[:, :Z], q2[:, Z:], p2[:, :Z], p2[:, Z:], pidx=kernel_ref.pair_rows(o['slot'], L, B, Np).to(torch.int32),
                    reps=L, free_bits=True, kl_min=case['kl_min'])
    return kl, raw


class FaultyZ2F:
    """the folded launch on the host in fp32 -- ``kernel_ref.z2f_post_bwd`` -- with ONE defect (None: bitwise that)"""

    def __init__(self, fault=None):
        self.fault = fault

    def z2f_post_bwd(self, dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, raw, kl_min, dz1b, L, B, Np,
                     park=None, prior=None, kl_out=None, seg=None, z1_dz2f=0.0):
        fault = self.fault
        Z = dp2.shape[1] // 2
        if kl_out is not None and Np:
            pidx = kernel_ref.pair_rows(pair_slot, L, B, Np)
            if fault == 'sum_in_another_order':     # the dims summed back to front, in fp32
                mq, lq = q2[:, :Z].repeat(L, 1), q2[:, Z:2 * Z].repeat(L, 1)
                mp, lp = p2[pidx, :Z], p2[pidx, Z:2 * Z]
                t = 1 - lp + lq - ((mq - mp) ** 2 + lq.exp()) / lp.exp()
                acc = torch.zeros(L * Np)
                for d in reversed(range(Z)):
                    acc = acc + t[:, d]
                raw.copy_(-0.5 * acc)                            # (inside the float64 bound: the BIT comparison catches it)
                kl_out.copy_(torch.clamp(raw, min=kl_min))
            else:
                kernel_ref.kl_rows_fwd(kl_out, raw, q2[:, :Z], q2[:, Z:2 * Z], p2[:, :Z], p2[:, Z:2 * Z], pidx=pidx, reps=L,
                                       free_bits=True, kl_min=kl_min)
        share = dz1b.clone()
        if seg is not None:
            ptr = seg[1].long()
            s = torch.zeros(L * B, Z)
            for r in range(L * B):
                hi = int(ptr[r + 1]) - (1 if (fault == 'segment_drops_its_last_row' and ptr[r + 1] - ptr[r] > 1) else 0)
                s[r] = seg[0][int(ptr[r]):hi, :Z].sum(0)
            share = share + s
        if z1_dz2f != 0.0 and dz2f is not None:
            share = share + z1_dz2f * dz2f
        gate_raw = raw
        if fault == 'tie_weighted_1' and Np:
            gate_raw = torch.where(raw == kl_min, raw + 1.0, raw)      # a tie takes the full gradient
        kernel_ref.z2f_post_bwd(dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, gate_raw, kl_min, share, L, B,
                                Np, prior=prior)
        if fault == 'pad_column_written':
            torch.as_strided(dp2, (L * B, 2 * Z + 1), dp2.stride(), dp2.storage_offset())[:, -1] = 0.0


# fault -> the check meant to catch it
Z2F_FAULTS = {'sum_in_another_order': 'kl_bits', 'tie_weighted_1': 'dp2', 'segment_drops_its_last_row': 'dz1',
              'pad_column_written': 'pads'}

# Z: below one lane stride, exactly one, ragged second stride, third stride (the walk-twice kernel); L 1 and 2;
# B = 7 with no pairs, mixed singletons, all pairs
Z2F_CASES = tuple(make_z2f_case(Z, L, 7, Np, seed=s) for s, (Z, L, Np) in enumerate(
    [(6, 1, 3), (6, 2, 0), (64, 2, 7), (64, 1, 0), (100, 2, 3), (100, 1, 7), (130, 2, 3), (130, 1, 7), (130, 2, 0)])) + (
    make_z2f_case(100, 2, 7, 3, seg=False, seed=20), make_z2f_case(64, 2, 7, 3, dz2f=False, seed=21),
    make_z2f_case(130, 2, 7, 7, seg=False, dz2f=False, seed=22))


# -------------------------------------------------------------------------------------- the classifier rider
def dgrad_reference(dqy, probs, W, dsts, old):
    """[(ref, bound)] per destination (dst, col0, alpha, beta[, col1, alpha2]) in float64 on the STORED dqy / probs;
    ``old``: the destinations' contents before the launch"""
    g, p, W = f64(dqy), f64(probs), f64(W)
    live = p > f32(1e-10)
    gm = torch.where(live, g, torch.zeros_like(g))
    dot = (gm * p).sum(1, keepdim=True)
    dl = p * (gm - dot)
    dl_c = p * (gm.abs() + (gm.abs() * p).sum(1, keepdim=True))
    out = []
    for d, o in zip(dsts, old):
        w = d[0].shape[1]
        Wt = d[2] * W[:, d[1]:d[1] + w]
        Wc = abs(d[2]) * W[:, d[1]:d[1] + w].abs()
        if len(d) > 5 and d[5] != 0.0:
            Wt = Wt + d[5] * W[:, d[4]:d[4] + w]
            Wc = Wc + abs(d[5]) * W[:, d[4]:d[4] + w].abs()
        base = d[3] * f64(o)
        out.append((base + dl @ Wt, bound(C_DLOGIT + C_DOT + W.shape[0], dl_c @ Wc) + bound(2, base.abs())))
    return out


def report(path, title, rows):
    """append the worst excess per output (``rows``: {case: {check: excess}}) to the checks file"""
    have = open(path).read() if os.path.exists(path) else ''
    with open(path, 'a') as f:
        if title not in have:
            f.write('%s\n' % title)
        for name, w in rows.items():
            f.write('  %-28s %s\n' % (name, '  '.join('%s %.3g' % (k, v) for k, v in sorted(w.items()))))
