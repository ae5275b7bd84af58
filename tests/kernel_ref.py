"""Plain-PyTorch reference of every launcher in ``drvae_amd.kernels`` that reaches the library (same names, same
signatures with every keyword of today, writes into the same output tensors; works on CPU or GPU tensors) -- ONE module:
``FUNCTIONS`` names them all, ``tests/test_engine_cpu.py`` holds the list to the launchers' signatures.

Two uses, both test-only:
  * ``-m gpu`` tests run each HIP kernel next to its reference here;
  * CPU tests install these as a stand-in for ``drvae_amd.kernels`` (see
    ``install``) to check the host-side orchestration (autograd wrappers, the fused
    step engine's hand-written backward, data-parallel sharding) against the oracle
    without a GPU.  The product never imports this module.

The arithmetic is fp32 in the launchers' own operation order, except where a launcher is SPECIFIED in float64 with one
rounding, and the stand-in states that specification: the negative-binomial, zero-inflated and library-size rows
(``tests/nb_ref.py``, ``tests/zinb_ref.py``, ``tests/counts_ref.py``), the count kinds of ``recon_rows``
(``tests/eval_counts_ref.py``), the noise (``tests/philox_ref.py``), the split-bf16 products (``tests/x3_ref.py``), the schedule
record, the rate / decay / average factors of the sweeps and the clip record.  ``CALLS`` counts what the step tests ask
about (reset by ``install``); ``FAULT`` makes one stand-in wrong on purpose.
"""
import math

import numpy as np

import torch
import torch.nn.functional as F

from drvae_amd._lib import ACT, EPI_BWD, EPI_FWD, EPI_PLAIN, GAUSS_LOGVAR, GAUSS_SIGMA  # noqa: F401
from tests import counts_ref, eval_counts_ref, nb_ref, philox_ref, x3_ref, zinb_ref

LOG_2PI = 1.8378770664093453
_ACT_NAME = {v: k for k, v in ACT.items()}

CALLS = dict.fromkeys(['batch_masks', 'batch_feed', 'lr_scaled_sweeps', 'decoupled_sweeps', 'averaged_sweeps', 'clip_norm',
                       'adam_l2_clip', 'adamax_l2_clip', 'split_feed', 'plain_feed', 'lib_rows', 'plain_rows',
                       'fill_noise_rows', 'mask_scale', 'z2f_post_bwd', 'smalln_fwd', 'folded_kl', 'folded_dgrad', 'nb',
                       'other', 'zinb', 'zinb_lib', 'norm_feed'], 0)
FAULT = {'name': None}          # tests only: 'moved_on_skipped_step' makes the averaged sweeps wrong on purpose


def _name(a):
    return a if isinstance(a, str) else _ACT_NAME[int(a)]


def act_fwd(a, x):
    a = _name(a)
    if a == 'identity':
        return x
    if a == 'elu':
        return F.elu(x)
    if a == 'softplus':
        return F.softplus(x)
    if a == 'sigmoid':
        return torch.sigmoid(x)
    if a == 'tanh':
        return torch.tanh(x)
    if a == 'relu':
        return torch.relu(x)
    if a == 'leaky_relu':
        return F.leaky_relu(x, 0.1)
    if a == 'selu':
        return F.selu(x)
    if a == 'softsign':
        return F.softsign(x)
    if a == 'cos':
        return torch.cos(x)
    raise KeyError(a)


def dact_from_y(a, y):
    a = _name(a)
    one = torch.ones_like(y)
    if a == 'identity':
        return one
    if a == 'elu':
        return torch.where(y > 0, one, y + 1)
    if a == 'softplus':
        return -torch.expm1(-y)
    if a == 'sigmoid':
        return y * (1 - y)
    if a == 'tanh':
        return 1 - y * y
    if a == 'relu':
        return (y > 0).float()
    if a == 'leaky_relu':
        return torch.where(y > 0, one, 0.1 * one)
    if a == 'selu':
        l_, a_ = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
        return torch.where(y > 0, l_ * one, y + l_ * a_)
    if a == 'softsign':
        return (1 - y.abs()) ** 2
    raise KeyError(a)


def _acc(out, val, beta):
    if beta != 0.0:
        out.copy_(beta * out + val)
    else:
        out.copy_(val)


def _seg(N, split, a0, a1, v0, v1, dev):
    """per-column selection helper for the dual-head epilogues"""
    first = (torch.arange(N, device=dev) < split)
    return first


def _ldr(t):
    """leading dimension as ``drvae_amd.kernels._ld`` sees it"""
    if t is None:
        return 0
    if t.dim() == 1:
        return t.numel()
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _widen(t, cols):
    """the (rows, cols) view over the SAME rows of a row-padded buffer (what a kernel sees when it runs over padded K / N)"""
    return torch.as_strided(t, (t.shape[0], cols), (_ldr(t), 1), t.storage_offset())


RUNG_TERMS = {3: x3_ref.TERMS, 2: ((0, 0), (0, 1), (1, 0)), 1: ((0, 0),)}     # bf16 part products of a split-bf16 rung


def routed_product(Cm, A, B, a_kc, b_kc, parts, *, a_colsum=None, colsum_beta=0.0, **kw):
    """one product routed with ``x3=True``: the rung's contract (``x3_ref.matmul`` with its terms: float64 sums, rounded to
    fp32 once), its epilogue by the fp32 stand-in (through an exact product with the identity)"""
    Aop, Bop = (A if a_kc else A.t()), (B.t() if b_kc else B)
    prod = x3_ref.matmul(Aop.contiguous(), Bop.contiguous(), RUNG_TERMS[parts]).float()
    gemm(Cm, prod, torch.eye(Cm.shape[1]), True, False, **kw)
    if a_colsum is not None:
        _acc(a_colsum, Aop.sum(1), colsum_beta)


def gemm(Cm, A, B, a_kc, b_kc, x3=False, parts=3, *, A2=None, a_kscale=None, alpha=1.0, beta=0.0, epi=EPI_PLAIN, scale=None,
         bias=None, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0, resid=None, resid_cols=0, yref=None,
         a_colsum=None, colsum_beta=0.0, overread=False, publish=None, kpad=False, npad=False):
    """mirrors ``kernels._gemm_desc`` INCLUDING its padded forms (round 5, advisor): with ``kpad`` the product runs over
    K rounded up to 4 and so reads the operands' pad columns; with ``npad`` it runs over N rounded up and WRITES C's pad
    columns -- a pad that is not zero shows up in the CPU suite exactly as it would on the device.  ``x3``: the product is
    ``routed_product`` (no second source, no per-k scale, and its pads are not run over)"""
    if x3:
        assert A2 is None and a_kscale is None
        return routed_product(Cm, A, B, a_kc, b_kc, parts, alpha=alpha, beta=beta, epi=epi, scale=scale, bias=bias,
                              split=split, act0=act0, act1=act1, shift0=shift0, shift1=shift1, resid=resid,
                              resid_cols=resid_cols, yref=yref, a_colsum=a_colsum, colsum_beta=colsum_beta, publish=publish)
    if parts != 3:
        raise ValueError('gemm(parts=%r) without x3=True: the fp32 product has no parts' % (parts,))
    if publish is not None:
        flag_publish(publish[0], publish[1], publish[2])
    M, N = Cm.shape
    K_ = (A.shape[1] + (A2.shape[1] if A2 is not None else 0)) if a_kc else A.shape[0]
    Kp, Np = (K_ + 3) & ~3, (N + 3) & ~3
    if kpad and a_kc and b_kc and A2 is None and (K_ & 3) and min(_ldr(A), _ldr(B)) >= Kp and not ((_ldr(A) | _ldr(B)) & 3):
        A, B = _widen(A, Kp), _widen(B, Kp)
    if npad and not b_kc and (N & 3) and min(_ldr(B), _ldr(Cm)) >= Np and not ((_ldr(B) | _ldr(Cm)) & 3) and resid is None \
            and scale is None and bias is None and (yref is None or _ldr(yref) >= Np):
        B, Cm = _widen(B, Np), _widen(Cm, Np)
        if yref is not None:
            yref = _widen(yref, Np)
        split = N if split is None else split
        N = Np
    Aop = (torch.cat([A, A2], 1) if A2 is not None else A) if a_kc else A.t()
    if a_kscale is not None:
        Aop = Aop * a_kscale[None, :]
    Bop = B.t() if b_kc else B
    v = alpha * (Aop @ Bop)
    split = N if split is None else split
    first = _seg(N, split, act0, act1, shift0, shift1, Cm.device)[None, :]
    if epi == EPI_FWD:
        if scale is not None:
            v = v * scale[None, :]
        if bias is not None:
            v = v + bias[None, :]
        v = torch.where(first, act_fwd(act0, v) + shift0, act_fwd(act1, v) + shift1)
        if resid is not None and resid_cols > 0:
            v = torch.cat([v[:, :resid_cols] + resid[:, :resid_cols], v[:, resid_cols:]], 1)
    elif epi == EPI_BWD:
        d = torch.where(first, dact_from_y(act0, yref - shift0), dact_from_y(act1, yref - shift1))
        v = v * d
    _acc(Cm, v, beta)
    if a_colsum is not None:
        _acc(a_colsum, Aop.sum(1), colsum_beta)


def linear_fwd(out, x, W, bias=None, *, x2=None, scale=None, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0,
               resid=None, resid_cols=0, overread=False, publish=None, kpad=False):
    gemm(out, x, W, True, True, A2=x2, epi=EPI_FWD, scale=scale, bias=bias, split=split, act0=act0, act1=act1,
         shift0=shift0, shift1=shift1, resid=resid, resid_cols=resid_cols, publish=publish, kpad=kpad)


def heads_tiles(split):
    return (split + 15) // 16


def linear_heads(out, x, W, bias=None, *, split, x2=None, scale=None, act0=0, act1=0, shift0=0.0, shift1=0.0,
                 resid=None, resid_cols=0, overread=False, publish=None, sample=None, nll=None, kpad=False):
    """the unfused sequence ``dv_gemm_heads`` replaces: heads GEMM, then reparam_fwd / nll_rows_fwdbwd"""
    M, N = out.shape
    heads = torch.zeros(M, N, device=out.device) if nll is not None else out
    # (the NLL epilogue of a softplus sigma head takes its slope from the pre-activation: the heads' raw form below)
    sp = nll is not None and _name(act1) == 'softplus'
    linear_fwd(heads, x, W, bias, x2=x2, scale=scale, split=split, act0=act0, act1=0 if sp else act1, shift0=shift0,
               shift1=0.0 if sp else shift1, resid=resid, resid_cols=resid_cols, publish=publish, kpad=kpad)
    mu, sd = heads[:, :split], heads[:, split:]
    if sample is not None:
        g = sample.get
        n_src, eps, dst = sample['n_src'], sample['eps'], sample['out']
        for r in range(n_src):
            rows = [r] if g('seg_ptr') is None else \
                g('seg_rows')[int(g('seg_ptr')[r]):int(g('seg_ptr')[r + 1])].long().tolist()
            for s_ in rows:
                z = eps[s_] * torch.exp(0.5 * sd[r]) + mu[r]
                dst[s_] = z
                if g('out2') is not None:
                    g('out2')[s_] = z - g('sub')[s_]
                if g('out3') is not None and int(g('out3_idx')[s_]) >= 0:
                    g('out3')[int(g('out3_idx')[s_])] = z
                if g('out4') is not None:
                    g('out4')[int(g('out4_ptr')[s_]):int(g('out4_ptr')[s_ + 1])] = z
    else:
        rows = torch.zeros(M, device=out.device)
        zero = torch.zeros(split, device=out.device)
        nll_rows_fwdbwd(rows, out[:, :split], out[:, split:], nll['coef'], nll['x'], mu, sd, mode=GAUSS_SIGMA,
                        xidx=nll.get('xidx'), sd_act=act1, sd_shift=shift1, bias=(zero, zero) if sp else None)
        nll['part'].zero_()
        nll['part'][:, 0] = rows              # (any split of a row's sum over the tiles is as good)


def linear_bwd_data(dx, dpre, W, *, kscale=None, alpha=1.0, beta=0.0, yref=None, act=0, shift=0.0, overread=False,
                    npad=False):
    if yref is None:
        gemm(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta, npad=npad)
    else:
        gemm(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta, epi=EPI_BWD, yref=yref, act0=act,
             act1=act, shift0=shift, shift1=shift, npad=npad)


def linear_bwd_weight(dW, dpre, x, *, beta=0.0, dbias=None, overread=False, npad=False):
    gemm(dW, dpre, x, False, False, beta=beta, a_colsum=dbias, colsum_beta=beta, npad=npad)


def bn_fwd(y, x, w, b, mean, rstd, running_mean, running_var, eps=1e-5, momentum=0.1, training=True):
    """dv_bn_fwd: nn.BatchNorm1d(affine=True) over the rows of x; ``mean`` / ``rstd`` keep what ``bn_bwd`` needs"""
    M = x.shape[0]
    if training:
        mu, var = x.mean(0), x.var(0, unbiased=False)
        if running_mean is not None:
            running_mean.mul_(1 - momentum).add_(momentum * mu)
            running_var.mul_(1 - momentum).add_(momentum * var * (M / max(M - 1, 1)))
    else:
        mu, var = running_mean, running_var
    mean.copy_(mu)
    rstd.copy_(torch.rsqrt(var + eps))
    y.copy_((x - mean) * rstd * w + b)


def bn_bwd(dx, dw, db, dy, x, mean, rstd, w, training=True):
    """dv_bn_bwd; dx, dw, db optional"""
    M = x.shape[0]
    xhat = (x - mean) * rstd
    sw, sb = (dy * xhat).sum(0), dy.sum(0)
    if dw is not None:
        dw.copy_(sw)
    if db is not None:
        db.copy_(sb)
    if dx is not None:
        dx.copy_(w * rstd * (dy - sb / M - xhat * sw / M) if training else dy * w * rstd)


def mask_scale(y, x, mask, scale):
    """dv_mask_scale: y = x * mask * scale in fp32, in that order (y may be x)"""
    CALLS['mask_scale'] += 1
    y.copy_(x * mask * torch.tensor(scale, dtype=x.dtype, device=x.device))


def linear_bwd_pair(dW, dbias, dx, dpre, x, W, x3=False, parts=3, *, kscale=None, alpha=1.0, beta_x=0.0, yref=None, act=0,
                    shift=0.0, overread=False, publish=None, npad=False, npad_x=False, klq=None):
    if x3:                     # both products routed (``routed_product``)
        assert kscale is None and beta_x == 0.0 and klq is None
        routed_product(dW, dpre, x, False, False, parts, a_colsum=dbias, publish=publish)
        e = {} if yref is None else dict(epi=EPI_BWD, yref=yref, act0=act, act1=act, shift0=shift, shift1=shift)
        return routed_product(dx, dpre, W, True, False, parts, alpha=alpha, **e)
    if parts != 3:
        raise ValueError('linear_bwd_pair(parts=%r) without x3=True: the fp32 products have no parts' % (parts,))
    if publish is not None:
        flag_publish(publish[0], publish[1], publish[2])
    linear_bwd_weight(dW, dpre, x, dbias=dbias, npad=npad)
    if klq is not None:        # DV_EPI_KLQ: d/d(mu | logvar) of the sampled q rows instead of dx
        Z, q, out = klq['Z'], klq['q'], klq['out']
        v = alpha * (dpre @ W)[:, :Z]
        gm, gs = _prior_kl_grad(klq['coef'], klq['raw'], klq['kl_min'], q[:, :Z], q[:, Z:2 * Z])
        out[:, :Z] = gm + v
        out[:, Z:2 * Z] = gs + v * klq['eps'] * 0.5 * torch.exp(0.5 * q[:, Z:2 * Z])
        return
    linear_bwd_data(dx, dpre, W, kscale=kscale, alpha=alpha, beta=beta_x, yref=yref, act=act, shift=shift, npad=npad_x)


def colsum(out, X, beta=0.0):
    _acc(out, X.sum(0), beta)


def act_bwd_(dY, Y, *, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0):
    N = Y.shape[1]
    first = _seg(N, N if split is None else split, 0, 0, 0, 0, Y.device)[None, :]
    dY.mul_(torch.where(first, dact_from_y(act0, Y - shift0), dact_from_y(act1, Y - shift1)))


def wn_scale(scale, norm, W, g):
    nrm = torch.norm(W, 2, 1)
    if norm is not None:
        norm.copy_(nrm)
    scale.copy_(g / nrm)


def wn_bwd(dW, dg, dWraw, W, g, norm, beta=0.0):
    dot = (W * dWraw).sum(1)
    _acc(dW, (g / norm)[:, None] * dWraw - (dot * g / norm ** 3)[:, None] * W, beta)
    _acc(dg, dot / norm, beta)


def _std(sd, mode):
    return torch.exp(0.5 * sd) if mode == GAUSS_LOGVAR else sd


def _qrows(n, reps, idx, dev):
    j = torch.arange(n * reps, device=dev) % n
    return idx.long()[j] if idx is not None else j


def reparam_fwd(out, mu, sd, eps, *, mode=GAUSS_LOGVAR, src_idx=None, reps=1, sub=None, out2=None, out3=None,
                out3_idx=None):
    R = out.shape[0]
    q = _qrows(R // reps, reps, src_idx, out.device)
    z = mu[q] + eps * _std(sd[q], mode)
    out.copy_(z)
    if out2 is not None:
        out2.copy_(z - sub)
    if out3 is not None:
        sel = out3_idx.long() >= 0
        out3[out3_idx.long()[sel]] = z[sel]


def reparam_bwd(dmu, dsd, dz, eps, sd, *, mode=GAUSS_LOGVAR, src_idx=None, reps=1, beta=0.0):
    R, Z = dz.shape
    n = R // reps
    a = dz.reshape(reps, n, Z).sum(0)
    b = (dz * eps).reshape(reps, n, Z).sum(0)
    q = src_idx.long() if src_idx is not None else torch.arange(n, device=dz.device)
    if mode == GAUSS_LOGVAR:
        b = b * 0.5 * torch.exp(0.5 * sd[q])
    if beta != 0.0:
        dmu[q] = beta * dmu[q] + a
        dsd[q] = beta * dsd[q] + b
    else:
        dmu[q] = a
        dsd[q] = b


def _prior_kl_grad(coef, raw, kl_min, mu, lv):
    c = (coef * torch.where(raw > kl_min, torch.ones_like(raw), torch.where(raw == kl_min, 0.5 * torch.ones_like(raw),
                                                                           torch.zeros_like(raw))))[:, None]
    return c * mu, c * (-0.5 * (1 - torch.exp(lv)))


def reparam_bwd_seg(dmu, dsd, dz, eps, sd, seg_ptr, seg_rows, *, mode=GAUSS_LOGVAR, extra=None, ex_ptr=None,
                    ex_rows=None, beta=0.0, bump=None, dz_add=None, park=None, prior=None):
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    for (c, inc) in (bump or ()):
        if c is not None:
            counter_add(c, inc)
    if dz_add is not None:
        dz = dz.clone()
        dz[:dz_add.shape[0]] += dz_add
    nq, Z = seg_ptr.numel() - 1, dz.shape[1]
    for i in range(nq):
        rows = seg_rows[int(seg_ptr[i]):int(seg_ptr[i + 1])].long()
        a = dz[rows].sum(0)
        b = (dz[rows] * eps[rows]).sum(0)
        if mode == GAUSS_LOGVAR:
            b = b * 0.5 * torch.exp(0.5 * sd[i])
        if extra is not None:
            er = ex_rows[int(ex_ptr[i]):int(ex_ptr[i + 1])].long()
            a = a + extra[er][:, :Z].sum(0)
            b = b + extra[er][:, Z:2 * Z].sum(0)
        dmu[i] = (beta * dmu[i] if beta != 0.0 else 0) + a
        dsd[i] = (beta * dsd[i] if beta != 0.0 else 0) + b
    if prior is not None:
        gm, gs = _prior_kl_grad(prior[0][:nq], prior[1][:nq], prior[2], prior[3][:nq], sd[:nq])
        dmu[:nq] += gm
        dsd[:nq] += gs


def pair_rows(pair_slot, L, B, Np):
    """p row l*B + i of every KL row l*Np + jp (pair_slot[i] == jp): the ``pidx`` of the separate launch"""
    slot = pair_slot.long()
    i_of = torch.empty(Np, dtype=torch.long, device=slot.device)
    i_of[slot[slot >= 0]] = torch.arange(B, device=slot.device)[slot >= 0]
    return (torch.arange(L, device=slot.device)[:, None] * B + i_of[None, :]).reshape(-1)


def z2f_post_bwd(dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, raw, kl_min, dz1b, L, B, Np,
                 park=None, prior=None, kl_out=None, seg=None, z1_dz2f=0.0):
    """the folded forms (``Tail.fold_rows``) as the unfolded sequences they replace: ``kl_out``: the pairs' KL rows are
    formed here first; ``seg`` / ``z1_dz2f``: the fprop rows' d/dz1 and the classifier's share join ``dz1b``"""
    CALLS['z2f_post_bwd'] += 1
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)                  # single-threaded stand-in: the producer has run already
    Z = dp2.shape[1] // 2
    dev = dp2.device
    if kl_out is not None and Np:
        CALLS['folded_kl'] += 1
        kl_rows_fwd(kl_out, raw, q2[:, :Z], q2[:, Z:2 * Z], p2[:, :Z], p2[:, Z:2 * Z], pidx=pair_rows(pair_slot, L, B, Np),
                    reps=L, free_bits=True, kl_min=kl_min)
    if seg is not None:
        s = torch.zeros(L * B, Z, device=dev)
        rows_segment_sum(s, seg[0], seg_ptr=seg[1], beta=0.0, width=Z)
        s = s * (seg[2] if len(seg) > 2 else 1.0)
        dz1b = s if dz1b is None else dz1b + s
    if z1_dz2f != 0.0 and dz2f is not None:
        dz1b = z1_dz2f * dz2f if dz1b is None else dz1b + z1_dz2f * dz2f
    if dz2f is None:
        dz2f = torch.zeros(L * B, Z, device=dev)
    slot = pair_slot.long() if (pair_slot is not None and Np) else torch.full((B,), -1, dtype=torch.long, device=dev)
    is_pair = slot >= 0
    if Np and dq2 is not None:
        dq2.zero_()
    for l in range(L):
        rs = slice(l * B, (l + 1) * B)
        mp, lp = p2[rs, :Z], p2[rs, Z:2 * Z]
        g = dz2f[rs].clone()
        if Np and dzdec_pert is not None:
            g[is_pair] = g[is_pair] + dzdec_pert[l * Np + slot[is_pair]]
        dmu = g.clone()
        dlv = g * eps[rs] * 0.5 * torch.exp(0.5 * lp)
        if Np:
            kr = l * Np + slot[is_pair]
            rv = raw[kr]
            c = (coef[kr] * torch.where(rv > kl_min, torch.ones_like(rv),
                                        torch.where(rv == kl_min, 0.5 * torch.ones_like(rv), torch.zeros_like(rv))))[:, None]
            mq, lq = q2[slot[is_pair], :Z], q2[slot[is_pair], Z:2 * Z]
            dm, ivp, vq = mq - mp[is_pair], torch.exp(-lp[is_pair]), torch.exp(lq)
            if dq2 is not None:
                dq2[slot[is_pair], :Z] += c * dm * ivp
                dq2[slot[is_pair], Z:2 * Z] += c * (-0.5 * (1 - vq * ivp))
            dmu[is_pair] = dmu[is_pair] - c * dm * ivp
            dlv[is_pair] = dlv[is_pair] + c * (-0.5 * (-1 + (dm * dm + vq) * ivp))
        dp2[rs, :Z] = dmu
        dp2[rs, Z:2 * Z] = dlv
        dz1[rs] = dz1[rs] + dmu + (dz1b[rs] if dz1b is not None else 0)
    if prior is not None and Np and dq2 is not None:
        gm, gs = _prior_kl_grad(prior[0][:Np], prior[1][:Np], kl_min, q2[:Np, :Z], q2[:Np, Z:2 * Z])
        dq2[:Np, :Z] += gm
        dq2[:Np, Z:2 * Z] += gs


def _kl_operands(mu_q, sd_q, mu_p, sd_p, prior, qidx, pidx, R, reps):
    q = _qrows(R // reps, reps, qidx, mu_q.device)
    mq, sq = mu_q[q], sd_q[q]
    if mu_p is None:
        mp, sp = torch.full_like(mq, prior[0]), torch.full_like(sq, prior[1])
    else:
        p = pidx.long() if pidx is not None else torch.arange(R, device=mu_q.device)
        mp, sp = mu_p[p], sd_p[p]
    return mq, sq, mp, sp


def kl_rows_fwd(out, raw, mu_q, sd_q, mu_p=None, sd_p=None, *, prior=(0.0, 0.0), mode=GAUSS_LOGVAR, qidx=None,
                pidx=None, reps=1, free_bits=False, kl_min=0.0, add=None, eps=None, zout=None, park=None, second=None):
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    R = out.numel()
    mq, sq, mp, sp = _kl_operands(mu_q, sd_q, mu_p, sd_p, prior, qidx, pidx, R, reps)
    if zout is not None:
        zout.copy_(mq + eps * _std(sq, mode))
    if mode == GAUSS_LOGVAR:
        t = 1 - sp + sq - ((mq - mp) ** 2 + sq.exp()) / sp.exp()
    else:
        t = 1 - torch.log(sp ** 2) + torch.log(sq ** 2) - ((mq - mp) ** 2 + sq ** 2) / sp ** 2
    r = -0.5 * t.sum(1)
    if raw is not None:
        raw.copy_(r)
    v = torch.clamp(r, min=kl_min) if free_bits else r
    if add is not None:
        v = v + add
    if second is not None:
        m2, s2, raw2 = second
        pm, ps = torch.full_like(m2, prior[0]), torch.full_like(s2, prior[1])
        if mode == GAUSS_LOGVAR:
            t2 = 1 - ps + s2 - ((m2 - pm) ** 2 + s2.exp()) / ps.exp()
        else:
            t2 = 1 - torch.log(ps ** 2) + torch.log(s2 ** 2) - ((m2 - pm) ** 2 + s2 ** 2) / ps ** 2
        r2 = -0.5 * t2.sum(1)
        if raw2 is not None:
            raw2.copy_(r2)
        v = v + (torch.clamp(r2, min=kl_min) if free_bits else r2)
    out.copy_(v)


def kl_rows_fwd_pair(first, second):
    kl_rows_fwd(*first[0], **first[1])
    kl_rows_fwd(*second[0], **second[1])


def kl_rows_bwd(dq_mu, dq_sd, dp_mu, dp_sd, coef, raw, mu_q, sd_q, mu_p=None, sd_p=None, *, prior=(0.0, 0.0),
                mode=GAUSS_LOGVAR, qidx=None, pidx=None, reps=1, free_bits=False, kl_min=0.0, beta=0.0, dz=None,
                eps=None):
    R = coef.numel()
    mq, sq, mp, sp = _kl_operands(mu_q, sd_q, mu_p, sd_p, prior, qidx, pidx, R, reps)
    c = coef.clone()
    if free_bits:
        c = c * torch.where(raw > kl_min, torch.ones_like(raw),
                            torch.where(raw == kl_min, 0.5 * torch.ones_like(raw), torch.zeros_like(raw)))
    c = c[:, None]
    dm = mq - mp
    if mode == GAUSS_LOGVAR:
        ivp, vq = torch.exp(-sp), torch.exp(sq)
        gmq, gsq = dm * ivp, -0.5 * (1 - vq * ivp)
        gsp = -0.5 * (-1 + (dm * dm + vq) * ivp)
    else:
        vp = sp * sp
        gmq, gsq = dm / vp, -1 / sq + sq / vp
        gsp = 1 / sp - (dm * dm + sq * sq) / (vp * sp)
    tq_mu, tq_sd = c * gmq, c * gsq
    if dz is not None:
        tq_mu = tq_mu + dz
        tq_sd = tq_sd + dz * eps * (0.5 * torch.exp(0.5 * sq) if mode == GAUSS_LOGVAR else 1.0)
    _acc(dq_mu, tq_mu, beta)
    _acc(dq_sd, tq_sd, beta)
    if dp_mu is not None:
        _acc(dp_mu, -c * gmq, beta)
        _acc(dp_sd, c * gsp, beta)


def nll_rows_fwd(out, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, bias=None, sd_shift=1e-3):
    if bias is not None:          # raw heads: finished here
        mu = mu + bias[0]
        sd = F.softplus(sd + bias[1]) + sd_shift
    xr = x[xidx.long()] if xidx is not None else x
    if mode == GAUSS_SIGMA:
        t = LOG_2PI + torch.log(sd ** 2) + (xr - mu) ** 2 / sd ** 2
    else:
        t = LOG_2PI + sd + (xr - mu) ** 2 / sd.exp()
    out.copy_(-0.5 * t.sum(1))


def nll_rows_bwd(dmu, dsd, coef, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, sd_act=0, sd_shift=0.0, dx=None,
                 beta=0.0):
    xr = x[xidx.long()] if xidx is not None else x
    d = xr - mu
    c = coef[:, None]
    if mode == GAUSS_SIGMA:
        gm, gs = d / sd ** 2, -1 / sd + d * d / sd ** 3
    else:
        gm, gs = d * torch.exp(-sd), -0.5 * (1 - d * d * torch.exp(-sd))
    if _name(sd_act) != 'identity':
        gs = gs * dact_from_y(sd_act, sd - sd_shift)
    _acc(dmu, c * gm, beta)
    _acc(dsd, c * gs, beta)
    if dx is not None:
        _acc(dx, -c * gm, beta)


def rec_nll_rows(out, x, v, *, kind, shift=0.0, xidx=None, coef=None, dpre=None, library=False):
    """``kind='nb'`` (``v`` = [mu | theta], ``dpre`` = [d/da_m | d/da_t]) and ``library=True`` (the mean scaled by the size
    factor the kernel forms, an fp32 quotient) state the header's formulas: float64 on the fp32 values handed in, rounded
    once (``tests/nb_ref.py``, ``tests/counts_ref.py``); so does ``kind='zinb'`` (``v`` = [mu | theta | logit], ``dpre`` 3X wide;
    ``tests/zinb_ref.py``), counted on its own"""
    xs = x[xidx.long()] if xidx is not None else x
    X = x.shape[1]
    if kind == 'zinb':
        CALLS['zinb_lib' if library else 'zinb'] += 1
        assert v.shape[1] == 3 * X and (dpre is None or dpre.shape[1] == 3 * X)
        ref = zinb_ref.reference(xs, v[:, :X], v[:, X:2 * X], v[:, 2 * X:], coef=coef, shift=shift, library=library)
        out.copy_(ref['rows'].to(out.dtype))
        if coef is not None:
            for i, k in enumerate(('gm', 'gt', 'gd')):
                dpre[:, i * X:(i + 1) * X] = ref[k].to(dpre.dtype)
        return
    CALLS['lib_rows' if library else 'plain_rows'] += 1
    if library:
        assert kind in ('poisson', 'nb')
        ref = counts_ref.reference(kind, xs, v[:, :X], v[:, X:] if kind == 'nb' else None, coef=coef, shift=shift)
        out.copy_(ref['rows'].to(out.dtype))
        if coef is not None:
            dpre[:, :X] = ref['gm'].to(dpre.dtype)
            if kind == 'nb':
                dpre[:, X:] = ref['gt'].to(dpre.dtype)
        return
    CALLS['nb' if kind == 'nb' else 'other'] += 1
    if kind == 'nb':
        assert v.shape[1] == 2 * X
        xs, mu, th = xs.double(), v[:, :X].double(), v[:, X:].double()
        out.copy_(nb_ref.logp64(xs, mu, th).sum(1).to(out.dtype))
        if coef is not None:
            gm, gt, _, _ = nb_ref.grads64(xs, mu, th)
            sm = -torch.expm1(-(mu - nb_ref.ref64.f32(shift)))
            st = -torch.expm1(-(th - nb_ref.ref64.f32(nb_ref.THETA_SHIFT)))
            c = coef.double()[:, None]
            dpre[:, :X] = (c * gm * sm).to(dpre.dtype)
            dpre[:, X:] = (c * gt * st).to(dpre.dtype)
        return
    if kind == 'binary':
        lo, hi = 1e-10, float(np.float32(1.0 - 1e-10))
        pc = v.clamp(lo, hi)
        out.copy_((xs * pc.log() + (1 - xs) * (1 - pc).log()).sum(1))
        g = torch.where((v > lo) & (v < hi), xs - v, torch.zeros_like(v))
    else:
        out.copy_((xs * v.log() - v - torch.lgamma(xs + 1)).sum(1))
        g = (xs / v - 1) * -torch.expm1(-(v - shift))
    if coef is not None:
        dpre.copy_(coef[:, None] * g)


def nll_rows_fwdbwd(out, dmu, dsd, coef, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, sd_act=0, sd_shift=0.0, bias=None):
    if bias is None:
        nll_rows_fwd(out, x, mu, sd, mode=mode, xidx=xidx)
        nll_rows_bwd(dmu, dsd, coef, x, mu, sd, mode=mode, xidx=xidx, sd_act=sd_act, sd_shift=sd_shift)
        return
    # raw heads: finished here; the softplus slope is taken from the pre-activation (sigmoid), the others' from the output
    pre = sd + bias[1]
    mu = mu + bias[0]
    sd = act_fwd(sd_act, pre) + sd_shift
    nll_rows_fwd(out, x, mu, sd, mode=mode, xidx=xidx)
    if _name(sd_act) != 'softplus':
        nll_rows_bwd(dmu, dsd, coef, x, mu, sd, mode=mode, xidx=xidx, sd_act=sd_act, sd_shift=sd_shift)
        return
    nll_rows_bwd(dmu, dsd, coef, x, mu, sd, mode=mode, xidx=xidx)
    dsd.mul_(torch.sigmoid(pre))


P_MIN = 1e-10


def softmax_clamp_fwd(probs, logits, sigmoid1=False):
    if sigmoid1:
        s = torch.sigmoid(logits[:, :1])
        p = torch.cat([1 - s, s], 1)
    else:
        p = torch.softmax(logits, -1)
    probs.copy_(torch.clamp(p, min=P_MIN, max=1. - 1e-10))


def softmax_clamp_bwd(dlogits, dprobs, probs, sigmoid1=False, beta=0.0):
    g = torch.where(probs > P_MIN, dprobs, torch.zeros_like(dprobs))
    if sigmoid1:
        s = probs[:, 1:2]
        _acc(dlogits, (g[:, 1:2] - g[:, 0:1]) * s * (1 - s), beta)
    else:
        dot = (g * probs).sum(1, keepdim=True)
        _acc(dlogits, probs * (g - dot), beta)


def cat_terms_fwd(probs, *, labels=None, prior=None, logp=None, kl=None, ent=None, best=None):
    lp = probs.log()
    if logp is not None:
        logp.copy_(lp.gather(1, labels.long()[:, None])[:, 0])
    if kl is not None:
        kl.copy_(-probs * (prior.log() - lp))
    if ent is not None:
        ent.copy_(-(probs * lp).sum(1))
    if best is not None:
        best.copy_(torch.max(probs, 1)[1].to(best.dtype))


def cat_terms_bwd(dprobs, probs, *, labels=None, prior=None, c_logp=None, g_kl=None, c_ent=None, beta=0.0):
    lp = probs.log()
    v = torch.zeros_like(probs)
    if c_logp is not None:
        oh = F.one_hot(labels.long(), probs.shape[1]).to(probs.dtype)
        v = v + oh * (c_logp[:, None] / probs)
    if g_kl is not None:
        v = v + g_kl * (lp - prior.log() + 1)
    if c_ent is not None:
        v = v - c_ent[:, None] * (lp + 1)
    _acc(dprobs, v, beta)


def _dlogits(dprobs, probs):
    if probs is None:
        return dprobs
    g = torch.where(probs > P_MIN, dprobs, torch.zeros_like(dprobs))
    return probs * (g - (g * probs).sum(1, keepdim=True))


def smalln_fwd(probs, logits, a1, W, bias=None, a2=None, ymarg=None, park=None, fprop_kl=None, dgrad=None):
    """``dgrad`` (the folded form, ``Tail.fold_rows``): the classifier's data gradient leaves the launch too"""
    CALLS['smalln_fwd'] += 1
    _smalln_fwd(probs, logits, a1, W, bias, a2, ymarg, park, fprop_kl)
    if dgrad:
        CALLS['folded_dgrad'] += 1
        assert ymarg is not None and len(dgrad) <= 2
        smalln_bwd_data(list(dgrad), ymarg[3], probs, W)


def _smalln_fwd(probs, logits, a1, W, bias=None, a2=None, ymarg=None, park=None, fprop_kl=None):
    if park is not None:
        flag_wait(*park)
    if ymarg is not None:
        yl, kld, cfp, dqy, label, fp_ptr, klfp, log_prior, c_kld, c_yl = ymarg
        f = fprop_kl
        if f is not None:      # the unfused sequence the fused launch replaces
            Z1, Z3 = f['Z1'], f['Z3']
            kl_rows_fwd(klfp, f['raw1'], f['Q'][:, :Z1], f['Q'][:, Z1:], f['P'][:, :Z1], f['P'][:, Z1:], qidx=f['qidx'],
                        free_bits=True, kl_min=f['kl_min'], prior=(0.0, 0.0),
                        second=(f['Q3'][:, :Z3], f['Q3'][:, Z3:], f['raw3']))
        _smalln_fwd(probs, logits, a1, W, bias, a2)
        ymarg_fwdbwd(yl, kld, cfp, dqy, probs, label, fp_ptr, klfp, log_prior, c_kld, c_yl)
        if f is not None:
            kl_rows_bwd(f['dq'][:, :Z1], f['dq'][:, Z1:], f['dp'][:, :Z1], f['dp'][:, Z1:], cfp, f['raw1'],
                        f['Q'][:, :Z1], f['Q'][:, Z1:], f['P'][:, :Z1], f['P'][:, Z1:], qidx=f['qidx'], free_bits=True,
                        kl_min=f['kl_min'])
        return
    x = torch.cat([a1, a2], 1) if a2 is not None else a1
    z = x @ W.t() + (bias if bias is not None else 0)
    if logits is not None:
        logits.copy_(z)
    if probs is not None:
        probs.copy_(torch.clamp(torch.softmax(z, -1), min=P_MIN, max=1. - 1e-10))


def smalln_bwd_data(dsts, dprobs, probs, W, seg=None):
    dl = _dlogits(dprobs, probs)
    for di, d in enumerate(dsts):
        dst, col0, alpha, beta = d[:4]
        w = dst.shape[1]
        if di == 0 and seg is not None:
            rows_segment_sum(dst, seg[0], seg_ptr=seg[1], beta=0.0, width=w)
            beta = 1.0
        v = alpha * (dl @ W[:, col0:col0 + w])
        if len(d) > 5 and d[5] != 0.0:
            v = v + d[5] * (dl @ W[:, d[4]:d[4] + w])
        _acc(dst, v, beta)


def smalln_ws_numel(N, K):
    return 16 * N * (K + 1)


def smalln_bwd_weight(dW, db, dprobs, probs, a1, a2=None, beta=0.0, publish=None, ws=None):
    if publish is not None:
        flag_publish(*publish)
    dl = _dlogits(dprobs, probs)
    x = torch.cat([a1, a2], 1) if a2 is not None else a1
    _acc(dW, dl.t() @ x, beta)
    if db is not None:
        _acc(db, dl.sum(0), beta)


def ymarg_fwd(yl, kld, qy, label, fp_ptr, klfp, log_prior):
    R, Y = qy.shape
    f0 = fp_ptr[:-1].long()
    nf = (fp_ptr[1:] - fp_ptr[:-1]).long()
    lab = nf == 1
    slot = label.long() <= -2                 # labeled row with all Y class slots materialised (universal plan)
    cls = torch.where(slot, -2 - label.long(), label.long().clamp(min=0))
    j = torch.arange(Y, device=qy.device)[None, :]
    fidx = torch.where(lab[:, None], f0[:, None].expand(R, Y), f0[:, None] + j).clamp(max=max(klfp.numel() - 1, 0))
    kf = klfp[fidx]
    lq = qy.log()
    yl.copy_(torch.where(lab | slot, lq.gather(1, cls[:, None])[:, 0], torch.zeros_like(yl)))
    marg = (qy * kf).sum(1) + (-qy * (log_prior - lq)).sum(1)
    kld.copy_(torch.where(lab, kf[:, 0], torch.where(slot, kf.gather(1, cls[:, None])[:, 0], marg)))


def ymarg_fwdbwd(yl, kld, cfp, dqy, qy, label, fp_ptr, klfp, log_prior, c_kld, c_yl):
    ymarg_fwd(yl, kld, qy, label, fp_ptr, klfp, log_prior)
    ymarg_bwd(cfp, dqy, qy, label, fp_ptr, klfp, log_prior, c_kld, c_yl)


def ymarg_bwd(cfp, dqy, qy, label, fp_ptr, klfp, log_prior, c_kld, c_yl):
    R, Y = qy.shape
    f0 = fp_ptr[:-1].long()
    nf = (fp_ptr[1:] - fp_ptr[:-1]).long()
    for r in range(R):       # small R in tests; clarity over speed
        if int(nf[r]) == 1:
            dqy[r].zero_()
            dqy[r, int(label[r])] = c_yl[r] / qy[r, int(label[r])]
            cfp[int(f0[r])] = c_kld[r]
        elif int(label[r]) <= -2:
            c = -2 - int(label[r])
            dqy[r].zero_()
            dqy[r, c] = c_yl[r] / qy[r, c]
            cfp[int(f0[r]):int(f0[r]) + Y] = 0
            cfp[int(f0[r]) + c] = c_kld[r]
        else:
            sl = slice(int(f0[r]), int(f0[r]) + Y)
            cfp[sl] = c_kld[r] * qy[r]
            dqy[r] = c_kld[r] * (klfp[sl] + qy[r].log() - log_prior + 1)


def ycont_fwd(yl, fpin_y, z3in_y, mu, ylab, has_y, eps, logvar, B, sqerr=False):
    R, Y = mu.shape
    i = torch.arange(R, device=mu.device) % B
    lab = has_y[i].bool()
    yv = torch.where(lab[:, None], ylab[i], mu + math.exp(0.5 * logvar) * eps[:, :Y])
    ll = -((ylab[i] - mu) ** 2).sum(1) if sqerr else \
        -0.5 * (LOG_2PI + logvar + (ylab[i] - mu) ** 2 / math.exp(logvar)).sum(1)
    yl.copy_(torch.where(lab, ll, torch.zeros_like(ll)))
    fpin_y[:, :Y] = yv
    z3in_y[:, :Y] = yv


def ycont_bwd(dlogit, cfp, mu, ylab, has_y, logvar, c_yl, c_kld, dfpin_y, dz3in_y, B, sqerr=False):
    R, Y = mu.shape
    if dlogit is None:
        cfp[:R] = c_kld[:R]
        return
    i = torch.arange(R, device=mu.device) % B
    lab = has_y[i].bool()
    dmu = torch.where(lab[:, None], c_yl[:, None] * (ylab[i] - mu) * (2.0 if sqerr else 1.0 / math.exp(logvar)),
                      dfpin_y[:, :Y] + dz3in_y[:, :Y])
    dlogit[:, :Y] = dmu * mu * (1 - mu)


def mmd_rff_fwd(diff, mmd2, th1, th2, c):
    d = c * (torch.cos(th1).mean(0) - torch.cos(th2).mean(0))
    diff.copy_(d)
    mmd2[0] = (d ** 2).sum()


def mmd_rff_bwd(G, th, diff, gout, coef):
    G.copy_(-coef * gout.reshape(-1)[0] * diff[None, :] * torch.sin(th))


def mmd_identity_fwd(diff, out, x1, x2):
    d = x1.mean(0) - x2.mean(0)
    diff.copy_(d)
    out[0] = (d ** 2).sum()


def mmd_identity_bwd(dx, diff, gout, coef):
    dx.copy_((coef * gout.reshape(-1)[0] * diff)[None, :].expand_as(dx))


def nuisance_feed(sohe, sohd, cls, s32, *, table=None, n_batches=0, ctr=None, base=None, pair_rows=None, L=1):
    B, S = cls.numel(), sohe.shape[1]
    if table is not None:
        b = min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)
        c = s32[table[b].long()]
    else:
        c = s32.reshape(-1)
    c = c.to(torch.int32)
    cp = c[pair_rows.long()] if (pair_rows is not None and pair_rows.numel()) else c[:0]
    cls.copy_(c)
    sohe.copy_(F.one_hot(torch.cat([c, cp]).long(), S).to(sohe.dtype))
    sohd.copy_(F.one_hot(torch.cat([c.repeat(L), cp.repeat(L), cp.repeat(L)]).long(), S).to(sohd.dtype))


def _grouped_terms(g, count):
    """(term, class k, theta rows, rows of z, class of every row) of every term of the grouped penalty (``_Plan``'s table);
    ``count`` (the forward launch): ``cnt`` is written on the way"""
    Kc, E = (1 if g['S'] == 2 else g['S']), g['rows'].numel()
    ptr = g['grp_ptr'].tolist()
    for tg in range(len(ptr) - 1):
        e = slice(ptr[tg], ptr[tg + 1])
        rows = g['rows'][e].long()
        c = g['cls'][g['src'][e].long()]
        for k in range(Kc):
            if count:
                g['cnt'][tg, k] = int((c == k).sum())
                if g['S'] == 2:
                    g['cnt'][tg, 1] = c.numel() - int((c == k).sum())
            yield tg * Kc + k, k, slice(k * E + e.start, k * E + e.stop), rows, c


_MASKED_GROUPS = {'drvae': 4, 'pvae': 2, 'vfae': 2}


def _masked_terms(g, count):
    """the same of the masked penalty (a batch-independent plan: data groups and classes read as data); ``count``:
    ``members`` and ``cnt`` are written on the way"""
    cls, S = g['cls'], g['S']
    B, Np, L, model, n_z = cls.numel(), g['Np'], g['L'], g['model'], g['z'].shape[0]
    table = g.get('table')
    if table is not None:
        b = min(max(int(g['ctr'][0]) - int(g['base'][0]), 0), g['n_batches'] - 1)
        r = table[b].long()
    else:
        r = torch.arange(B, device=cls.device)
    zero = torch.zeros(B, dtype=torch.bool, device=cls.device)
    hx = g['hx'][r] != 0 if g.get('hx') is not None else zero
    hy = g['hy'][r] != 0 if g.get('hy') is not None else zero
    if model == 'drvae':
        grp = torch.where(hx, torch.where(hy, 2, 3), torch.where(hy, 0, 1))
    elif model == 'pvae':
        grp = hx.long()
    else:
        grp = 1 - hy.long()
    G, Kc = _MASKED_GROUPS[model], (1 if S == 2 else S)
    lists = [(l * B, B, False) for l in range(L)] + ([(L * B + l * Np, Np, True) for l in range(L)] if Np else [])
    for q, (z0, n, z2) in enumerate(lists):
        for gi in range(G):
            m = grp[:n] == gi
            if z2:
                m = m & hx[:n]
            mem = torch.nonzero(m).reshape(-1)
            tg, c = q * G + gi, cls[mem]
            if count:
                g['members'][tg, :mem.numel()] = mem.to(torch.int32)
                for k in range(S):
                    g['cnt'][tg, k] = int((c == k).sum())
                g['cnt'][tg, S] = mem.numel()
            for k in range(Kc):
                yield tg * Kc + k, k, k * n_z + z0 + mem, z0 + mem, c


def _mmd_fwd(g, terms, zero_theta):
    z, rff = g['z'], g['kind'] == 'rbf_fourier'
    for t, k, th_rows, rows, c in terms:
        n0 = int((c == k).sum())
        n1 = c.numel() - n0
        if n0 == 0 or n1 == 0:
            g['diff'][t].zero_()
            if rff and zero_theta:
                g['theta'][th_rows].zero_()
            continue
        u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
        if rff:
            th = g['a'] * (z[rows] @ g['W'][t]) + 2 * math.pi * g['b'][t]
            g['theta'][th_rows] = th
            g['diff'][t] = g['c'] * (u[:, None] * torch.cos(th)).sum(0)
        else:
            g['diff'][t] = (u[:, None] * z[rows]).sum(0)


def _mmd_bwd(g, terms):
    z, rff = g['z'], g['kind'] == 'rbf_fourier'
    dz = torch.zeros_like(g['dz'])
    val = z.new_zeros(())
    for t, k, th_rows, rows, c in terms:
        diff = g['diff'][t]
        m2 = (diff * diff).sum()
        g['m2'][t] = m2
        n0 = int((c == k).sum())
        n1 = c.numel() - n0
        if float(m2) <= 0.0 or n0 == 0 or n1 == 0:
            continue
        val = val - g['w'] * torch.sqrt(m2)
        coef = -g['fac'] * g['w'] / torch.sqrt(m2)
        u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
        if rff:
            G = -diff[None, :] * torch.sin(g['theta'][th_rows])
            dz[rows] += (coef * g['c'] * g['a']) * u[:, None] * (G @ g['W'][t].t())
        else:
            dz[rows] += coef * u[:, None] * diff[None, :]
    g['dz'].copy_(dz)
    g['value'].copy_(val.reshape(1))


def mmd_grouped_fwd(g):
    _mmd_fwd(g, _grouped_terms(g, True), zero_theta=True)       # (a term with an empty side leaves zeros in its theta rows)


def mmd_grouped_bwd(g):
    _mmd_bwd(g, _grouped_terms(g, False))


def mmd_masked_fwd(g):
    g['cnt'].zero_()
    _mmd_fwd(g, _masked_terms(g, True), zero_theta=False)


def mmd_masked_bwd(g):
    _mmd_bwd(g, _masked_terms(g, False))


def _mix(G, kind, gammas, sa, sb):
    """the kernel mixture on a Gram matrix and its derivative w.r.t. G (poly) / the squared distance (rbf): dv_mmd_mix_*"""
    gam = [float(g) for g in gammas]
    if kind == 'poly':
        v = sum((g * G + 1.0) ** 2 for g in gam) / len(gam)
        dv = sum(2.0 * g * (g * G + 1.0) for g in gam) / len(gam)
    else:
        d2 = (sa.diagonal()[:, None] + sb.diagonal()[None, :] - 2.0 * G).clamp_min(0.0)
        v = sum(torch.exp(-g * d2) for g in gam) / len(gam)
        dv = sum(-g * torch.exp(-g * d2) for g in gam) / len(gam)
    return v, dv


def mmd_mix_fwd(part, G, kind, gammas, sa=None, sb=None):
    part.copy_(_mix(G, kind, gammas, sa, sb)[0].sum(1))


def mmd_mix_bwd(W, rs, G, kind, gammas, gout, coef, sa=None, sb=None):
    W.copy_(coef * gout.reshape(-1)[0] * _mix(G, kind, gammas, sa, sb)[1])
    rs.copy_(W.sum(1))


def mmd_mix_combine(out4, p11, p12, p22, c11, c12, c22):
    c11, c12, c22 = (float(np.float32(c)) for c in (c11, c12, c22))       # (the launch receives the counts as fp32)
    m11, m12, m22 = p11.double().sum() / c11, p12.double().sum() / c12, p22.double().sum() / c22
    out4.copy_(torch.stack([m11 - 2.0 * m12 + m22, m11, m12, m22]).float())


def rows_gather(out, src, idx=None, *, noise=None, sigma=0.0, onehot_cls=None, n_classes=0, width=None, park=None):
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    n = out.shape[0]
    W = (src.shape[1] if src is not None else 0) if width is None else width
    if W > 0:
        v = src[idx.long()][:, :W] if idx is not None else src[:n, :W]
        if noise is not None:
            v = v + sigma * noise[:n, :W]
        out[:, :W] = v
    if onehot_cls is not None:
        out[:, W:W + n_classes] = F.one_hot(onehot_cls.long(), n_classes).to(out.dtype)


def batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, *, pair_rows=None, noise=None, sigma=0.0, has_y=None,
               L=1, label_r=None, fp_i=None, fp_lab=None, fp_slot=None, fp_cls=None, onehot=None, n_classes=0, yf=None,
               ylab=None, onehot2=None, masks=None, park=None, xt=None, transform=None):
    """``xt`` (the split form, raw-count inputs): the gathered rows go to ``xt`` and ``xin`` = T(xt) + sigma * noise;
    ``transform='log1p_norm'``: T = log1p(xt / s), s in fp32 from the gathered row itself"""
    CALLS['batch_feed'] += 1
    CALLS['plain_feed' if xt is None else 'split_feed'] += 1
    CALLS['norm_feed'] += transform == 'log1p_norm'
    assert transform is None if xt is None else (transform in (None, 'log1p', 'log1p_norm') and
                                                 tuple(xt.shape) == tuple(xin.shape))
    rows = xin if xt is None else xt
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    if masks is not None:
        _batch_masks(table.shape[1], L, table=table, n_batches=n_batches, ctr=ctr, base=base, **masks)
    if ylab is not None:
        bb = min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)
        ylab.copy_(yf.reshape(-1, ylab.shape[1])[table[bb].long()])
    b = min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)
    tb = table[b].long()
    B = tb.numel()
    rows[:B] = x1[tb]
    if pair_rows is not None and pair_rows.numel():
        rows[B:] = x2[tb[pair_rows.long()]]
    if xt is not None:
        if transform == 'log1p_norm':
            t = torch.log1p(xt / (torch.clamp(xt.sum(1), min=1.0) / float(xt.shape[1]))[:, None])
        else:
            t = torch.log1p(xt) if transform == 'log1p' else xt
        xin.copy_(t + sigma * noise if noise is not None else t)
    elif noise is not None:
        xin += sigma * noise
    if label_r is not None:
        label_r.copy_(torch.where(has_y.bool(), y32[tb], torch.zeros_like(y32[tb])).repeat(L))
    if fp_cls is not None and fp_cls.numel():
        cls = torch.where(fp_lab.bool(), y32[tb[fp_i.long()]], fp_slot)
        fp_cls.copy_(cls)
        if onehot is not None:
            onehot.copy_(torch.nn.functional.one_hot(cls.long(), n_classes).to(onehot.dtype))
        if onehot2 is not None:
            onehot2.copy_(torch.nn.functional.one_hot(cls.long(), n_classes).to(onehot2.dtype))


def rows_segment_sum(dst, src, *, seg_ptr=None, seg_rows=None, w=None, n=None, dst_idx=None, beta=0.0, width=None,
                     park=None):
    if park is not None:
        flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    if n is None:
        n = seg_ptr.numel() - 1 if seg_ptr is not None else (seg_rows.numel() if seg_rows is not None else
                                                              src.shape[0])
    W = dst.shape[1] if width is None else width
    for i in range(n):
        if seg_ptr is not None:
            ts = range(int(seg_ptr[i]), int(seg_ptr[i + 1]))
        else:
            ts = [i]
        s = torch.zeros(W, device=dst.device)
        for t in ts:
            row = int(seg_rows[t]) if seg_rows is not None else t
            s = s + (float(w[t]) if w is not None else 1.0) * src[row, :W]
        di = int(dst_idx[i]) if dst_idx is not None else i
        dst[di, :W] = (beta * dst[di, :W] if beta != 0.0 else 0) + s


def weighted_sum(out, x, w=None, idx=None, scale=1.0, beta=0.0, n=None):
    if n is None:
        n = idx.numel() if idx is not None else x.numel()
    xv = x.reshape(-1)[idx.long()[:n]] if idx is not None else x.reshape(-1)[:n]
    s = (xv * w.reshape(-1)[:n]).sum() if w is not None else xv.sum()
    out.reshape(-1)[0] = (beta * out.reshape(-1)[0] if beta != 0.0 else 0) + scale * s


def recon_row_stats(out, x, r):
    mx, mr = x.mean(1, keepdim=True), r.mean(1, keepdim=True)
    out.copy_(torch.stack([((x - r) ** 2).sum(1), mx[:, 0], mr[:, 0], ((x - mx) ** 2).sum(1), ((r - mr) ** 2).sum(1),
                           ((x - mx) * (r - mr)).sum(1)], 1))


def col_moment_blocks(M):
    return max(1, min(64, max(min(16, (M + 255) // 256), (M + 511) // 512)))


def col_moments(out, x, r, sel=None, part=None, r_bias=None):
    if r_bias is not None:
        r = r + r_bias
    if sel is not None:
        x, r = x[sel.long()], r[sel.long()]
    xd, rd = x.double(), r.double()
    tot = torch.stack([xd.sum(0), (xd * xd).sum(0), ((xd - rd) ** 2).sum(0)], 0)
    if part is not None:
        part.zero_()
        part[0].copy_(tot)
    if out is not None:
        out.copy_(tot)


RECON_ROWS_MAX_X = 1024


def recon_rows(rows, ll, x, mu, sd, *, bias=None, sd_shift=1e-3, kind=None, size_from=None, rec_out=None):
    """the count kinds (``kind`` / ``size_from`` / ``rec_out``): the header's formulas in float64 on the fp32 values handed in,
    rounded once (``tests/eval_counts_ref.py``; the refusals of the launcher / the entry point as assertions)"""
    if kind is not None:
        assert kind in eval_counts_ref.KINDS and bias is None and (sd is not None) == (kind == 'nb')
        assert not (kind == 'binary' and size_from is not None) and (rec_out is None or size_from is not None)
        ref = eval_counts_ref.reference(kind, x, mu, sd, size_from)
        rows.copy_(ref['rows'].to(rows.dtype))
        if ll is not None:
            ll.copy_(ref['ll'].to(ll.dtype))
        if rec_out is not None:
            rec_out.copy_(ref['rec'].to(rec_out.dtype))
        return
    assert size_from is None and rec_out is None
    if bias is not None:          # raw heads: finished here
        mu = mu + bias[0]
        sd = F.softplus(sd + bias[1]) + sd_shift
    recon_row_stats(rows, x, mu)
    if ll is not None:
        nll_rows_fwd(ll, x, mu, sd, mode=GAUSS_SIGMA)


def recon_finalize(out4, rows, part, X, *, sel=None, n=None, ll=None):
    n = (sel.numel() if sel is not None else rows.shape[0]) if n is None else n
    idx = sel.long()[:n] if sel is not None else torch.arange(n, device=rows.device)      # (sel NULL: rows 0..n-1)
    r = rows[idx].double()
    cols = part.sum(0)
    out4[0] = torch.sqrt(r[:, 0].sum() / (n * X)) if n else float('nan')
    out4[1] = 1.0 - cols[2].sum() / (cols[1] - cols[0] ** 2 / n).sum()
    out4[2] = (r[:, 5] / torch.sqrt(r[:, 3] * r[:, 4])).mean() if n else float('nan')
    out4[3] = ll[idx].double().mean() if (ll is not None and n) else float('nan')


RANK_MAX_ROWS = 32768


def rank_metrics(out, counts, proba, y32, *, pred32=None, sel=None, c0=1, n_cls=1, binary=True):
    from drvae_amd import metrics as MET
    idx = sel.long() if sel is not None else torch.arange(proba.shape[0])
    y, pr = y32[idx], proba[idx]
    for c in range(n_cls):
        pos = (y > 0) if binary else (y == c0 + c)
        out[2 * c] = MET.roc_auc(pos, pr[:, c0 + c])
        out[2 * c + 1] = MET.average_precision(pos, pr[:, c0 + c])
    out[2 * n_cls] = float((pred32[idx] == y).float().sum() / max(len(idx), 1)) if (pred32 is not None and len(idx)) else float('nan')


def _halted(halt):
    return halt is not None and bool((halt.reshape(-1)[0::2] != 0).any())


def reg_metrics64(pred, y, sel=None, n=None):
    """numpy float64 restatement of ``dv_reg_metrics`` (include/drvae_hip.h): the regression metrics of a continuous target
    in the kernel's TWO-PASS arithmetic -- the means first, then the centred sums -- with its defined edge cases.
    -> float64 array [rmse, r2, pearr] over the rows ``sel`` (None: the first ``n`` rows, default all) x all columns of
    ``pred`` / ``y`` ((rows, Y) or (rows,)), flattened"""
    pred = np.asarray(pred, np.float64).reshape(len(pred), -1)
    y = np.asarray(y, np.float64).reshape(len(y), -1)
    if sel is not None:
        sel = np.asarray(sel, np.int64)
        pred, y = pred[sel], y[sel]
    elif n is not None:
        pred, y = pred[:n], y[:n]
    p, t = pred.reshape(-1), y.reshape(-1)
    nan = float('nan')
    if t.size == 0:
        return np.array([nan, nan, nan])
    my, mp = t.sum() / t.size, p.sum() / p.size          # pass 1
    d, yc, pc = t - p, t - my, p - mp                    # pass 2
    sse, syy, spp, syp = (d * d).sum(), (yc * yc).sum(), (pc * pc).sum(), (yc * pc).sum()
    den = np.sqrt(syy * spp)
    return np.array([np.sqrt(sse / t.size), 1.0 - sse / syy if syy > 0 else nan, syp / den if den > 0 else nan])


def reg_metrics(out3, pred, y, *, sel=None, n=None):
    """the launcher's form of ``reg_metrics64``: tensors in, ``out3`` (3 float64) written"""
    v = reg_metrics64(pred.detach().cpu().numpy(), y.detach().cpu().numpy(), None if sel is None else sel.cpu().numpy(), n)
    out3[:3] = torch.from_numpy(v).to(out3.device)


def loss_assemble(loss, terms, w_elbo, w_cmpl, after=None, bump=(), halt=None, accum=None):
    if after is not None:
        flag_wait(after[0], after[1], after[2], after[3], after[4])
    for (c, inc) in bump:
        if c is not None:
            counter_add(c, inc)
    if after is not None and not terms:
        return
    acc = torch.zeros(8, device=loss.device)
    for term in terms:
        x, w, scale, out = term[:4]
        row_len = term[4] if len(term) > 4 else 1
        v = x.reshape(-1)
        if w is not None and row_len > 1:
            w = w.reshape(-1).repeat_interleave(row_len)
        acc[out] = acc[out] + scale * ((v * w.reshape(-1)).sum() if w is not None else v.sum())
    acc[5] = (w_elbo[:3] * acc[:3]).sum()
    acc[6] = (w_cmpl[:8] * acc[:8]).sum()
    loss[:8] = torch.full_like(acc, float('nan')) if _halted(halt) else acc
    if accum is not None:
        accum[:8] += loss[:8]


def axpby(y, x, a=1.0, b=0.0):
    y.copy_(a * x + (b * y if b != 0.0 else 0))


def lr_effective(lr, lr_scale):
    """the rate a sweep with ``lr_scale`` runs at: (float)((double)lr * (double)lr_scale[0]) of the fp32 ``lr`` it is handed"""
    return float(np.float32(np.float64(np.float32(lr)) * np.float64(np.float32(float(lr_scale.reshape(-1)[0])))))


def _sweep(adamax, p, g, m, v, step_dev, state, *, lr, beta1, beta2, eps, weight_decay, gscale, gate=None, halt=None,
           lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    """the one body of the four sweeps.  ``state`` (the ``_clip`` forms): the clip state, whose first word is the step.  A
    sweep is TAKEN unless a halt word is set (behind the gate's wait, where there is one) or the clip record says skip; a
    sweep that is not taken touches nothing, the average included.  Clipping: the gradient scaled by fl32(gscale * coef),
    t = step - n_skipped.  ``lr_scale``: ``lr_effective``.  Decoupled decay: p *= fl32(1 - lr_eff wd) first (the factor in
    double from the fp32 rate the sweep runs at), then the sweep at weight_decay = 0.  The average: e += fl32(1 - avg_decay)
    (p_new - e) behind the sweep."""
    if decoupled and adamax:
        raise RuntimeError('drvae_amd: dv_adamax_l2 failed: invalid argument (-1)')       # (as ``_lib.check`` raises)
    if avg is not None:
        if avg_decay is None:
            raise ValueError('an average needs its avg_decay')
        if not 0.0 < float(np.float32(avg_decay)) < 1.0:
            raise RuntimeError('drvae_amd: dv_adam_l2 failed: invalid argument (-1)')
        assert avg.shape == p.shape
    if state is not None:
        import drvae_amd.kernels as K
        CALLS['adamax_l2_clip' if adamax else 'adam_l2_clip'] += 1
        clip, step_dev = K.clip_record(state), state[0:1]
    CALLS['lr_scaled_sweeps'] += lr_scale is not None
    CALLS['decoupled_sweeps'] += bool(decoupled)
    CALLS['averaged_sweeps'] += avg is not None
    if gate is not None:
        flag_wait(gate[0], gate[1], gate[3], gate[2])
    taken = not _halted(halt) and not (state is not None and int(clip[2]))
    if taken:
        t = int(step_dev.reshape(-1)[0])
        if state is not None:
            gscale = float(np.float32(gscale) * np.float32(float(clip.view(torch.float32)[1])))
            t -= int(clip[3])
        if lr_scale is not None:
            lr = lr_effective(lr, lr_scale)
        if decoupled:
            p.mul_(float(np.float32(1.0 - np.float64(np.float32(lr)) * np.float64(np.float32(weight_decay)))))
            weight_decay = 0.0
        gg = g * gscale
        if weight_decay != 0.0:
            gg = gg + weight_decay * p
        m.lerp_(gg, 1 - beta1)
        if adamax:
            torch.maximum(v.mul_(beta2), gg.abs().add_(eps), out=v)
            p.addcdiv_(m, v, value=-(lr / (1 - beta1 ** t)))
        else:
            v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
            bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
            denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
            p.addcdiv_(m, denom, value=-(lr / bc1))
    if avg is not None and (taken or FAULT['name'] == 'moved_on_skipped_step'):
        avg.add_((p - avg) * float(np.float32(1.0 - np.float64(np.float32(avg_decay)))))


def adam_l2(p, g, m, v, step_dev, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, gate=None,
            halt=None, lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep(False, p, g, m, v, step_dev, None, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
           gscale=gscale, gate=gate, halt=halt, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def adamax_l2(p, g, m, u, step_dev, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
              lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep(True, p, g, m, u, step_dev, None, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
           gscale=gscale, halt=halt, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def adam_l2_clip(p, g, m, v, state, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
                 lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep(False, p, g, m, v, None, state, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
           gscale=gscale, halt=halt, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def adamax_l2_clip(p, g, m, u, state, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
                   lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep(True, p, g, m, u, None, state, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
           gscale=gscale, halt=halt, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def clip_norm(g, state, *, gscale=1.0):
    """dv_grad_norm_clip on the clip state of ``kernels.clip_state`` (word 0 the step, max_norm a double, the record {norm,
    coef (fp32 bits), skip, n_skipped}, then the workspace): the whole double sum goes into the first partial (one per
    8192-element share would do), the partials are summed in index order, the record is written"""
    import drvae_amd.kernels as K
    CALLS['clip_norm'] += 1
    part, rec = K.clip_partials(state), K.clip_record(state)
    n_part = K.sumsq_partials(g.numel())
    assert part.numel() >= n_part
    max_norm = float(state[K._CLIP_MAX_NORM:K._CLIP_MAX_NORM + 2].view(torch.float64)[0])
    assert max_norm > 0
    part.zero_()
    part[0] = (g.reshape(-1).double() ** 2).sum()
    s = 0.0
    for v in part[:n_part].tolist():        # index order
        s = s + v
    skip = not math.isfinite(s)
    norm = abs(float(np.float32(gscale))) * math.sqrt(s) if s == s else float('nan')
    coef = 0.0 if skip else min(1.0, max_norm / (norm + 1e-6))
    f = rec.view(torch.float32)
    f[0], f[1] = float(np.float32(norm)), float(np.float32(coef))
    rec[2] = int(skip)
    rec[3] += int(skip)


def flag_publish(flag, ctr, add=1):
    flag[0] = int(ctr[0]) + add


def flag_wait(flag, ctr, err, add=1, max_spins=None, publish=None):
    if publish is not None:
        flag_publish(*publish)
    if int(flag[0]) < int(ctr[0]) + add:      # single-threaded stand-in: the producer must have run already
        err[0] = 1                            # (err[1], the parked-time statistic, stays 0)


def counters_add2(c1, inc1, c2, inc2, publish=None):
    if publish is not None:
        flag_publish(*publish)
    counter_add(c1, inc1)
    counter_add(c2, inc2)


def counter_add(counter, inc=1):
    if counter.numel() == 1:
        counter += inc
    else:
        v = (int(counter[1]) & 0xffffffff) << 32 | (int(counter[0]) & 0xffffffff)
        v = (v + inc) & 0xffffffffffffffff
        lo, hi = v & 0xffffffff, v >> 32
        counter[0] = lo - (1 << 32) if lo >= (1 << 31) else lo
        counter[1] = hi - (1 << 32) if hi >= (1 << 31) else hi


def _coef64(it, itermax, offset):
    if itermax <= 0:
        return 1.0
    d = it - offset
    if d <= 0:
        return 0.01
    return min(1.0, 0.01 + float(d) / float(itermax))


def record(it, pert, kl, yl, lr):
    """the schedule record {beta_pert, beta_kl, beta_yr, lr_scale} as ``dv_batch_masks`` evaluates it: in double from the
    integer step counter and the integer schedule parameters, one rounding to fp32 per coefficient.  ``pert`` / ``yl`` =
    (itermax, offset), ``kl`` / ``lr`` = itermax; an itermax <= 0 switches that schedule off (value 1)"""
    lr_s = max(0.01, 1.0 - _coef64(it, lr, 0)) if lr > 0 else 1.0
    return np.array([np.float32(_coef64(it, pert[0], pert[1])), np.float32(_coef64(it, kl, 0)),
                     np.float32(_coef64(it, yl[0], yl[1])), np.float32(lr_s)], np.float32)


def _coef32(it, itermax, offset):
    f = np.float32
    if itermax <= 0:
        return f(1.0)
    d = it - offset
    if d <= 0:
        return f(0.01)
    return min(f(1.0), f(f(0.01) + f(f(d) / f(itermax))))


def record_fp32(it, pert, kl, yl, lr):
    """FAULTY on purpose: the same record with every operation rounded to fp32 (what a kernel evaluating the schedule in
    single precision would store)"""
    f = np.float32
    lr_s = max(f(0.01), f(f(1.0) - _coef32(it, lr, 0))) if lr > 0 else f(1.0)
    return np.array([_coef32(it, pert[0], pert[1]), _coef32(it, kl, 0), _coef32(it, yl[0], yl[1]), lr_s], np.float32)


def _apply_schedule(B, L, an, m, rec):
    """what the annealed launch does behind the plain masks: the record, beta_kl / beta_yr folded into the coefficients, the
    copies without beta_kl, the ELBO / CMPL weights (fp32 arithmetic on the fp32 record, like the kernel)"""
    dev = m['c_nll'].device
    r = torch.from_numpy(rec).to(dev)
    an['sched'].copy_(r)
    b_kl, b_yr = r[1], r[2]
    if m.get('c_klz2') is not None and m.get('hx') is not None:
        if an.get('w_klz2') is not None:
            an['w_klz2'].copy_(m['c_klz2'])
        m['c_klz2'].mul_(b_kl)
    if m.get('c_klp') is not None:
        if an.get('w_klp') is not None:
            an['w_klp'].copy_(m['c_klp'])
        m['c_klp'].mul_(b_kl)
    if m.get('hy') is not None:
        m['c_yl'].mul_(b_yr)
    if an.get('c_kld') is not None:
        c_tot = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(L), dtype=torch.float32) * torch.tensor(m['n_tot'], dtype=torch.float32))
        an['c_kld'][:L * B] = (b_kl.cpu() * c_tot).to(dev)
    has_pert, has_y = m.get('hx') is not None, m.get('hy') is not None
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    an['w_elbo'][:3] = torch.stack([f(1.0), -r[1].cpu(), r[0].cpu() * f(m['pert_rate']) if has_pert else f(0.0)]).to(dev)
    w = torch.zeros(8)
    w[3] = -(r[2].cpu() * f(m['yl_rate'])) if has_y else 0.0
    mmd = float(an.get('mmd_rate', 0.0))
    w[4] = -float(np.float32(mmd)) if mmd != 0.0 else 0.0
    w[5] = -1.0
    an['w_cmpl'][:8] = w.to(dev)


def batch_masks(B, L, **masks):
    CALLS['batch_masks'] += 1
    _batch_masks(B, L, **masks)


def _batch_masks(B, L, *, anneal=None, **m):
    """``anneal`` (the annealing schedules): the launch evaluates its OWN beta_pert -- ``beta`` is not read -- and applies
    the schedule behind the plain masks"""
    if anneal is None:
        return _plain_masks(B, L, **m)
    rec = record(int(anneal['step'].reshape(-1)[0]), anneal['pert'], anneal['kl'], anneal['yl'], anneal['lr'])
    if m.get('gcounts') is not None:      # (an explicit batch's one pair of global counts: ``_plain_masks`` indexes rows)
        m = dict(m, gcounts=m['gcounts'].reshape(-1, 2))
    _plain_masks(B, L, **dict(m, beta=torch.from_numpy(rec[0:1].copy()).to(m['c_nll'].device)))
    _apply_schedule(B, L, anneal, m, rec)


def _plain_masks(B, L, *, n_tot, kl_rate, pert_rate, yl_rate, beta, c_nll, w_recl, hx=None, hy=None, y=None, c_klz2=None,
                 c_yl=None, w_pert=None, w_yl=None, label=None, c_klp=None, table=None, n_batches=0, ctr=None, base=None,
                 Np=None, one_slot=None, gcounts=None):
    Np = B if Np is None else Np
    gc = None
    if gcounts is not None:       # data parallelism: the GLOBAL (N_pairs, N_labeled) of the batch are table data
        gc = gcounts[min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1) if table is not None else 0]
    if c_klp is not None:
        s_ = table[min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)].long() if table is not None else \
            torch.arange(B, device=c_nll.device)
        c_klp[:B] = 1.0 / n_tot
        c_klp[B:B + Np] = torch.where(hx[s_[:Np]] != 0, 1.0 / n_tot, 0.0) if hx is not None else 0.0
    if table is not None:
        b = min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)
        src = table[b].long()
    else:
        src = torch.arange(B, device=c_nll.device)
    LB, ct, bt = L * B, 1.0 / (L * n_tot), float(beta[0]) if beta is not None else 1.0
    c_nll[:LB] = -ct
    w_recl[:LB] = ct
    if hx is not None:
        LP = L * Np
        px = (hx[src[:Np]] != 0).repeat(L)
        npair = max(float((hx[src] != 0).sum()) if gc is None else float(gc[0]), 1.0)
        c_nll[LB:LB + LP] = torch.where(px, -ct, 0.0)
        w_recl[LB:LB + LP] = torch.where(px, ct, 0.0)
        c_nll[LB + LP:LB + 2 * LP] = torch.where(px, -bt * pert_rate / (L * npair), 0.0)
        w_pert[:LP] = torch.where(px, 1.0 / (L * npair), 0.0)
        c_klz2[:LP] = torch.where(px, bt * kl_rate * ct, 0.0)
    if hy is not None:
        py = (hy[src] != 0).repeat(L)
        nlab = max(float((hy[src] != 0).sum()) if gc is None else float(gc[1]), 1.0)
        c_yl[:LB] = torch.where(py, -yl_rate / (L * nlab), 0.0)
        w_yl[:LB] = 1.0 / (L * nlab)
        label[:LB] = torch.where(py, -2 - y[src].to(label.dtype).repeat(L), torch.zeros_like(label[:LB]))
        if one_slot is not None:
            label[:LB] = torch.where(one_slot.repeat(L) != 0, y[src].to(label.dtype).repeat(L), label[:LB])


def _event(ctr_dev):
    return 0 if ctr_dev is None else ((int(ctr_dev[1]) & 0xffffffff) << 32 | (int(ctr_dev[0]) & 0xffffffff))


def fill_normal_rows(arena, desc, seed, ctr_dev=None, park=None):
    """dv_fill_normal_rows as specified (tests/philox_ref.py, float32 of its float64 value): the device's numbers up to
    the fp32 rounding of its Box-Muller transform"""
    if park is not None:
        flag_wait(*park)
    offsets, z, _, _ = philox_ref.rows_table(desc.cpu().numpy(), seed, _event(ctr_dev))
    arena.view(-1)[torch.from_numpy(offsets).to(arena.device)] = torch.from_numpy(z.astype(np.float32)).to(arena.device)


def keep_rows(desc, keep_thr, seed, event):
    """(offsets, mask) flat over every element the KEEP rows ``desc`` (n x {offset, width, draw id, global row}) describe:
    mask = 1.0 where word col % 4 of Philox4x32-10(counter = (col // 4, global row, draw id, event_lo),
    key = (seed_lo, seed_hi ^ event_hi)) is < keep_thr, else 0.0 (integer Philox words against the threshold: no float
    uniform, so a conforming kernel writes exactly these masks)"""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    s_lo, s_hi = philox_ref._split(seed)
    e_lo, e_hi = philox_ref._split(event)
    offs, vals = [], []
    for w in np.unique(desc[:, 1]):
        if w <= 0:
            continue
        d = desc[desc[:, 1] == w]
        blk = np.arange((int(w) + 3) // 4, dtype=np.uint64).reshape(1, -1)
        words = philox_ref.philox4x32_10(blk, d[:, 3].reshape(-1, 1), d[:, 2].reshape(-1, 1), e_lo, s_lo, s_hi ^ e_hi)
        words = np.stack(words, -1).reshape(len(d), -1)[:, :int(w)]              # (rows, width): word col % 4 of block col // 4
        offs.append((d[:, 0][:, None] + np.arange(int(w))[None, :]).reshape(-1))
        vals.append((words.astype(np.uint64) < np.uint64(keep_thr)).astype(np.float32).reshape(-1))
    if not offs:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(offs), np.concatenate(vals)


def fill_noise_rows(arena, table, seed, ctr_dev=None, park=None):
    """dv_fill_noise_rows as specified: ``table`` = descriptor rows + the trailer row {number of keep
    rows at the end, keep_thr's bits, 0, 0}; the rows in front as ``fill_normal_rows``, the rest keep masks"""
    CALLS['fill_noise_rows'] += 1
    desc, tr = table[:-1], table[-1].tolist()
    n_normal, keep_thr = desc.shape[0] - tr[0], tr[1] & 0xFFFFFFFF
    assert 0 <= n_normal <= desc.shape[0] and tr[2] == tr[3] == 0
    if park is not None:
        flag_wait(*park)
    d = desc.cpu().numpy()
    if n_normal:
        fill_normal_rows(arena, desc[:n_normal], seed, ctr_dev)
    offs, vals = keep_rows(d[n_normal:], keep_thr, seed, _event(ctr_dev))
    arena.view(-1)[torch.from_numpy(offs).to(arena.device)] = torch.from_numpy(vals).to(arena.device)


def fill_normal(out, seed, ctr_dev=None):
    """dv_fill_normal as specified (tests/philox_ref.py, float32 of its float64 value)"""
    z = philox_ref.flat(out.numel(), seed, _event(ctr_dev))[0]
    out.copy_(torch.from_numpy(z.astype(np.float32)).view(out.shape).to(out.device))


def nll_raw_cs_shape(M, X):
    return ((X >> 2) + 255) // 256, (M + 63) // 64


def nll_rows_raw_cs(out_part, dmu, dsd, ws, coef, x, mu, sd, bias, *, xidx=None, sd_shift=1e-3):
    """stand-in of dv_gauss_nll_rows_raw_cs: per-chunk row partials (1024 genes per chunk), per-block (64 rows) column sums;
    dmu is None: forward only"""
    M, X = mu.shape
    chunks, rbs = nll_raw_cs_shape(M, X)
    if dmu is not None:
        full = torch.zeros(M, dtype=mu.dtype, device=mu.device)
        nll_rows_fwdbwd(full, dmu, dsd, coef, x, mu, sd, mode=GAUSS_SIGMA, xidx=xidx, sd_act='softplus', sd_shift=sd_shift, bias=bias)
    xs = x[xidx.long()] if xidx is not None else x
    m = mu + bias[0]
    s_ = F.softplus(sd + bias[1]) + sd_shift
    el = -0.5 * (math.log(2 * math.pi) + 2 * torch.log(s_) + ((xs - m) / s_) ** 2)
    for c in range(chunks):
        out_part[:, c] = el[:, c * 1024:(c + 1) * 1024].sum(1)
    if dmu is not None:
        for b in range(rbs):
            ws[b, :X] = dmu[b * 64:(b + 1) * 64].sum(0)
            ws[b, X:2 * X] = dsd[b * 64:(b + 1) * 64].sum(0)


# the host-side helpers of ``drvae_amd.kernels`` (``clip_state``, ``noise_table``, ``x3_refusal``, ...) are plain python and
# are used as they are
FUNCTIONS = sorted(
    'gemm linear_fwd heads_tiles linear_heads linear_bwd_data linear_bwd_weight linear_bwd_pair bn_fwd bn_bwd mask_scale '
    'colsum act_bwd_ wn_scale wn_bwd reparam_fwd reparam_bwd reparam_bwd_seg z2f_post_bwd kl_rows_fwd kl_rows_fwd_pair '
    'kl_rows_bwd nll_rows_fwd nll_rows_bwd nll_rows_fwdbwd nll_raw_cs_shape nll_rows_raw_cs rec_nll_rows softmax_clamp_fwd '
    'softmax_clamp_bwd cat_terms_fwd cat_terms_bwd smalln_fwd smalln_bwd_data smalln_ws_numel smalln_bwd_weight ymarg_fwd '
    'ymarg_bwd ymarg_fwdbwd ycont_fwd ycont_bwd mmd_rff_fwd mmd_rff_bwd mmd_identity_fwd mmd_identity_bwd mmd_mix_fwd '
    'mmd_mix_bwd mmd_mix_combine nuisance_feed mmd_grouped_fwd mmd_grouped_bwd mmd_masked_fwd mmd_masked_bwd rows_gather '
    'batch_feed batch_masks rows_segment_sum weighted_sum recon_row_stats recon_rows col_moments col_moment_blocks '
    'recon_finalize rank_metrics reg_metrics loss_assemble axpby adam_l2 adamax_l2 clip_norm adam_l2_clip adamax_l2_clip '
    'flag_publish flag_wait counter_add counters_add2 fill_normal_rows fill_noise_rows fill_normal'.split())


def install(monkeypatch):
    """Replace the HIP launchers by these references for one CPU test (pytest monkeypatch); resets ``CALLS`` and ``FAULT``."""
    import drvae_amd.kernels as K
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
    for name in CALLS:
        CALLS[name] = 0
    FAULT['name'] = None


assert nb_ref.MU_SHIFT == 1e-6
