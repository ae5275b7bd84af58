"""Tensor-level launchers for the C-ABI kernels (device fp32 tensors in, enqueue on the
current HIP stream, nothing returned that needs a sync).

Every function writes into caller-provided output tensors (``out=``-style), so the
callers own all memory and the sequence is hipGraph-capturable.  2-D tensors may be
row-strided views (``stride(1) == 1``); the row stride is passed as the leading
dimension.  There is no CPU path here: tensors must live on the GPU.
"""
import ctypes as C
import math
import os
from typing import Any, NamedTuple, Optional

import torch

from . import _lib
from ._lib import ACT, EPI_BWD, EPI_FWD, EPI_KLQ, EPI_PLAIN, GAUSS_LOGVAR, GAUSS_SIGMA, GemmDesc  # noqa: F401
from .sparse_rows import CsrRows


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name='tensor', any_device=False):
    """``any_device``: the address goes into a descriptor that is looked at, never launched (``x3_refusal``)"""
    if t is None:
        return None
    if not ((t.is_cuda or any_device) and t.dtype == torch.float32):
        raise RuntimeError('drvae_amd kernels need CUDA/HIP float32 tensors (%s is %s on %s); there is no CPU '
                           'fallback' % (name, t.dtype, t.device))
    if t.dim() >= 1 and t.numel() > 0 and t.stride(-1) != 1 and t.size(-1) != 1:
        raise RuntimeError('%s must have unit inner stride' % name)
    return t.data_ptr()


def _i32(t, name='index'):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise RuntimeError('%s must be a contiguous CUDA int32 tensor' % name)
    return t.data_ptr()


def _ld(t):
    if t is None:
        return 0
    if t.dim() == 1:
        return t.numel()
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _act(a):
    return ACT[a] if isinstance(a, str) else int(a)


# ------------------------------------------------------------------------------ GEMM
# Steering of the GEMM dispatcher for tests and tools: the state lives HERE, on the caller's side, and travels with every
# descriptor (``dv_gemm_desc.tune``); the library itself keeps none.
_TUNE = _lib.GemmTune()
_TUNE.opt[0] = -1


def gemm_force_tiling(t):
    """run every GEMM-family call on tiling code ``t`` (0: the dispatcher's heuristics); returns 0, or a non-zero status
    when this build of the library does not carry the tiling (lab tilings: ``python -m drvae_amd.build --lab``)"""
    if not _lib.load().dv_gemm_has_tiling(int(t)):
        return _lib.DV_ERR_UNSUPPORTED if hasattr(_lib, 'DV_ERR_UNSUPPORTED') else 4
    _TUNE.tiling = int(t)
    return 0


def gemm_set_option(key, value):
    """dispatcher option ``key`` (see ``dv_gemm_tune`` in include/drvae_hip.h)"""
    if not 0 <= int(key) < 10:
        return 1
    _TUNE.opt[int(key)] = int(value)
    return 0


def _tune_ptr():
    t = _TUNE
    if t.tiling == 0 and t.opt[0] == -1 and not any(t.opt[i] for i in range(1, 10)):
        return None
    return C.addressof(t)


def _gemm_desc(Cm, A, B, a_kc, b_kc, *, A2=None, a_kscale=None, alpha=1.0, beta=0.0, epi=EPI_PLAIN, scale=None,
               bias=None, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0, resid=None, resid_cols=0, yref=None,
               a_colsum=None, colsum_beta=0.0, overread=False, publish=None, kpad=False, npad=False, _any_device=False):
    f32 = lambda t, name: _f32(t, name, _any_device)
    M, N = Cm.shape
    if a_kc:
        K = A.shape[1] + (A2.shape[1] if A2 is not None else 0)
        assert A.shape[0] == M
    else:
        K = A.shape[0]
        assert A.shape[1] == M and A2 is None
    if b_kc:
        assert tuple(B.shape) == (N, K), (tuple(B.shape), N, K)
    else:
        assert tuple(B.shape) == (K, N), (tuple(B.shape), K, N)
    d = GemmDesc()
    d.M, d.N, d.K, d.a_kcontig, d.b_kcontig = M, N, K, int(bool(a_kc)), int(bool(b_kc))
    d.A, d.lda = f32(A, 'A'), _ld(A)
    if kpad and a_kc and b_kc and A2 is None and (K & 3) and min(_ld(A), _ld(B)) >= ((K + 3) & ~3) \
            and not ((A.data_ptr() | B.data_ptr()) & 15) and not ((_ld(A) | _ld(B)) & 3):
        # ``kpad``: the caller guarantees that the rows of both operands are ZERO from K up to the next multiple of 4
        # (row-padded activation buffers, the arena's row-padded weights): the product over the padded K is the same
        # number, and its operands qualify for the LDS-DMA kernels (16-B chunks along k)
        d.K = K = (K + 3) & ~3
    if npad and not b_kc and (N & 3) and min(_ld(B), _ld(Cm)) >= ((N + 3) & ~3) and not ((B.data_ptr() | Cm.data_ptr()) & 15) \
            and not ((_ld(B) | _ld(Cm)) & 3) and resid is None and scale is None and bias is None \
            and (yref is None or _ld(yref) >= ((N + 3) & ~3)):
        # ``npad``: the caller guarantees that the rows of B are ZERO from N up to the next multiple of 4 and that C's rows
        # are padded the same way: the product over the padded N writes zeros into C's pad columns (they are zero
        # anyway) and every output row ends on a 16-B store
        d.N = N = (N + 3) & ~3
    d.A2, d.lda2, d.K1 = f32(A2, 'A2'), _ld(A2), (A.shape[1] if A2 is not None else K)
    d.a_kscale = f32(a_kscale, 'a_kscale')
    d.B, d.ldb = f32(B, 'B'), _ld(B)
    d.C, d.ldc = f32(Cm, 'C'), _ld(Cm)
    d.alpha, d.beta, d.epilogue = alpha, beta, epi
    d.scale, d.bias = f32(scale, 'scale'), f32(bias, 'bias')
    d.split = N if split is None else split
    d.act0, d.act1, d.shift0, d.shift1 = _act(act0), _act(act1), shift0, shift1
    d.resid, d.ldr, d.resid_cols = f32(resid, 'resid'), _ld(resid), resid_cols
    d.yref, d.ldy = f32(yref, 'yref'), _ld(yref)
    d.a_colsum, d.colsum_beta = f32(a_colsum, 'a_colsum'), colsum_beta
    d.flags = 3 if overread else 0
    if publish is not None:                 # ``Publish``: on kernel entry, see dv_flag_publish
        publish = Publish(*publish)
        d.pub_flag, d.pub_ctr, d.pub_add = _i32(publish.flag), _i32(publish.ctr), publish.add
    d.tune = _tune_ptr()
    return d


def _x3_refusal(d, parts=3):
    """why ``dv_gemm_x3`` (``parts`` < 3: ``dv_gemm_split``) does not run descriptor ``d`` (None: it does).  The verdict is
    the library's (``dv_gemm_x3_ok`` / ``dv_gemm_split_ok``, pure host functions); this only puts a name to it."""
    lib = _lib.load()
    if parts not in (1, 2, 3):
        return 'parts = %r (the split-bf16 rungs have 1, 2 or 3 parts)' % (parts,)
    if lib.dv_gemm_x3_ok(C.byref(d)) if parts == 3 else lib.dv_gemm_split_ok(C.byref(d), parts):
        return None
    why = []
    if d.A2:
        why.append('a second A source (A2)')
    if d.a_kscale:
        why.append('a per-k scale (a_kscale)')
    if d.epilogue not in (EPI_PLAIN, EPI_BWD):
        why.append('epilogue %d (only DV_EPI_PLAIN and DV_EPI_BWD)' % d.epilogue)
    if d.pub_flag:
        why.append('a publish on entry (pub_flag)')
    if (d.K & 3) and ((d.a_kcontig and not d.flags & 1) or (d.b_kcontig and not d.flags & 2)):
        why.append('K = %d is no multiple of 4 and the rows of a k-contiguous operand may not be over-read' % d.K)
    if ((d.A or 0) | (d.B or 0)) & 15 or (d.lda | d.ldb) & 3:
        why.append('operand rows that are not 16-B aligned')
    if not d.a_kcontig and d.b_kcontig:
        why.append('the layout (a_kcontig, b_kcontig) = (0, 1)')
    if d.a_colsum and (d.a_kcontig or d.b_kcontig):
        why.append('a_colsum outside the dy^T x layout')
    return ', '.join(why) or 'dv_gemm_x3_ok refuses the descriptor'


def _launch_x3(descs, what, parts=3):
    """split-bf16 routing decides up front: every descriptor of the call must be one the rung's entry point runs
    (``dv_gemm_x3``: three parts; ``dv_gemm_split``: two or one) -- no silent fallback"""
    for d in descs:
        why = _x3_refusal(d, parts)
        if why is not None:
            raise RuntimeError('%s(x3=True%s): the split-bf16 kernels do not run this %d x %d x %d product: %s'
                               % (what, '' if parts == 3 else ', parts=%r' % (parts,), d.M, d.N, d.K, why))
    lib = _lib.load()
    for d in descs:
        if parts == 3:
            _lib.check(lib.dv_gemm_x3(C.byref(d), _stream()), 'dv_gemm_x3')
        else:
            _lib.check(lib.dv_gemm_split(C.byref(d), parts, _stream()), 'dv_gemm_split')


def gemm(Cm, A, B, a_kc, b_kc, x3=False, parts=3, **kw):
    """C[M,N] = epilogue(alpha * Aop @ Bop) + beta*C, see ``dv_gemm`` in include/drvae_hip.h.
    ``overread``: rows of A and B may be over-read by up to 3 floats (padded / arena buffers).
    ``x3`` (opt-in): the product runs as a split-bf16 product (``dv_gemm_x3``; dtype bf16x3) -- raises where that entry
    point does not take the descriptor.  ``parts`` (with ``x3``; 3 by default): 2 or 1 bf16 parts per operand, the cheaper
    rungs of the ladder (``dv_gemm_split``; dtype bf16x2 / bf16x1 -- the latter is a bf16 product, not an fp32 one)."""
    d = _gemm_desc(Cm, A, B, a_kc, b_kc, **kw)
    if x3:
        return _launch_x3([d], 'gemm', parts)
    if parts != 3:
        raise ValueError('gemm(parts=%r) without x3=True: the fp32 product has no parts' % (parts,))
    _lib.check(_lib.load().dv_gemm(C.byref(d), _stream()), 'dv_gemm')


def x3_refusal(Cm, A, B, a_kc, b_kc, parts=3, **kw):
    """plan-time question: would ``gemm(..., x3=True[, parts=...])`` with these operands run?  None, or the reason why not.
    Shapes, strides and addresses only -- nothing is launched, so the operands may live on any device"""
    return _x3_refusal(_gemm_desc(Cm, A, B, a_kc, b_kc, _any_device=True, **kw), parts)


def _pair_descs(dW, dbias, dx, dpre, x, W, *, kscale=None, alpha=1.0, beta_x=0.0, yref=None, act=0, shift=0.0,
                overread=False, publish=None, npad=False, npad_x=False, klq=None, _any_device=False):
    """the two descriptors of ``linear_bwd_pair``: dW = dpre^T x (+ dbias) | dx (or the KLQ rows)"""
    dev = dict(_any_device=_any_device)
    d1 = _gemm_desc(dW, dpre, x, False, False, a_colsum=dbias, overread=overread, publish=publish, npad=npad, **dev)
    if klq is not None:
        assert yref is None and kscale is None and beta_x == 0.0
        Z, out = klq['Z'], klq['out']
        assert out.shape[1] == 2 * Z and W.shape[1] >= Z and W.shape[1] <= 2 * Z
        d2 = _gemm_desc(out[:, :W.shape[1]], dpre, W, True, False, alpha=alpha, epi=EPI_KLQ, split=Z, yref=klq['q'],
                        resid=klq['eps'], bias=klq['coef'], scale=klq['raw'], shift0=klq['kl_min'], overread=overread, **dev)
    elif yref is None:
        d2 = _gemm_desc(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta_x, overread=overread, npad=npad_x,
                        **dev)
    else:
        d2 = _gemm_desc(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta_x, epi=EPI_BWD, yref=yref,
                        act0=act, act1=act, shift0=shift, shift1=shift, overread=overread, npad=npad_x, **dev)
    return d1, d2


def linear_bwd_pair(dW, dbias, dx, dpre, x, W, x3=False, parts=3, **kw):
    """dW = dpre^T x (+ dbias) and dx = beta_x*dx + alpha*(dpre W) * act'(yref) in ONE launch when both fit
    the fused form of ``dv_gemm_pair`` (otherwise two launches).  Keywords: kscale, alpha, beta_x, yref, act, shift,
    overread, publish, npad, npad_x, klq (``_pair_descs``).
    ``x3`` (opt-in): both products as split-bf16 products (``dv_gemm_x3``, two launches -- what a chip-filling pair is
    anyway); raises where that entry point does not take one of the two descriptors.  ``parts`` as in ``gemm``.
    ``klq`` = dict(out, q, eps, coef, raw, kl_min, Z): the layer's input was [a sample z of the q rows | ...]: instead of
    dx the launch writes d/d(mu | logvar) of those rows incl. their prior term into ``out`` (M, 2Z) -- the epilogue
    DV_EPI_KLQ of include/drvae_hip.h; ``dx`` is not written (pass None)"""
    d1, d2 = _pair_descs(dW, dbias, dx, dpre, x, W, **kw)
    if x3:
        return _launch_x3([d1, d2], 'linear_bwd_pair', parts)
    if parts != 3:
        raise ValueError('linear_bwd_pair(parts=%r) without x3=True: the fp32 products have no parts' % (parts,))
    _lib.check(_lib.load().dv_gemm_pair(C.byref(d1), C.byref(d2), _stream()), 'dv_gemm_pair')


def x3_pair_refusal(dW, dbias, dx, dpre, x, W, parts=3, **kw):
    """plan-time question, as ``x3_refusal``: would ``linear_bwd_pair(..., x3=True[, parts=...])`` with these operands run?"""
    d1, d2 = _pair_descs(dW, dbias, dx, dpre, x, W, _any_device=True, **kw)
    return _x3_refusal(d1, parts) or _x3_refusal(d2, parts)


def linear_fwd(out, x, W, bias=None, *, x2=None, scale=None, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0,
               resid=None, resid_cols=0, overread=False, publish=None, kpad=False):
    """out = act([x|x2] W^T * scale + bias) + shift (+ resid) -- one Linear (or two heads) forward."""
    gemm(out, x, W, True, True, A2=x2, epi=EPI_FWD, scale=scale, bias=bias, split=split, act0=act0, act1=act1,
         shift0=shift0, shift1=shift1, resid=resid, resid_cols=resid_cols, overread=overread, publish=publish, kpad=kpad)


def heads_tiles(split):
    """column tiles of ``linear_heads`` (= floats per row of the NLL partial-sum buffer)"""
    return _lib.load().dv_gemm_heads_tiles(split)


def linear_heads(out, x, W, bias=None, *, split, x2=None, scale=None, act0=0, act1=0, shift0=0.0, shift1=0.0,
                 resid=None, resid_cols=0, overread=False, publish=None, sample=None, nll=None, kpad=False):
    """Dual-head Linear with the row work on both heads fused into its epilogue (``dv_gemm_heads``).
    ``sample`` = dict(eps, out, n_src[, seg_ptr, seg_rows, sub, out2, out3, out3_idx, out4, out4_ptr]): ``out`` =
    (mu | logvar) is written and the reparameterised samples of every source row leave the same launch (``out4``:
    sample row s is also copied to rows [out4_ptr[s], out4_ptr[s+1]) of out4);
    ``nll`` = dict(x, coef, part[, xidx]): ``out`` receives d/d(mu | pre-activation of std) of the Gaussian
    log-likelihood rows, ``part`` (M, heads_tiles(split)) their per-tile partial sums."""
    assert (sample is None) != (nll is None)
    d = _gemm_desc(out, x, W, True, True, A2=x2, epi=EPI_FWD, scale=scale, bias=bias, split=split, act0=act0, act1=act1,
                   shift0=shift0, shift1=shift1, resid=resid, resid_cols=resid_cols, overread=overread, publish=publish,
                   kpad=kpad)
    e = _lib.HeadsEpi()
    if sample is not None:
        g = sample.get
        e.mode = _lib.HEADS_SAMPLE
        e.seg_ptr, e.seg_rows, e.n_src = _i32(g('seg_ptr')), _i32(g('seg_rows')), sample['n_src']
        e.eps, e.lde = _f32(sample['eps'], 'eps'), _ld(sample['eps'])
        e.out, e.ldo = _f32(sample['out'], 'out'), _ld(sample['out'])
        e.sub, e.lds = _f32(g('sub'), 'sub'), _ld(g('sub'))
        e.out2, e.ldo2 = _f32(g('out2'), 'out2'), _ld(g('out2'))
        e.out3, e.ldo3, e.out3_idx = _f32(g('out3'), 'out3'), _ld(g('out3')), _i32(g('out3_idx'))
        e.out4, e.ldo4, e.out4_ptr = _f32(g('out4'), 'out4'), _ld(g('out4')), _i32(g('out4_ptr'))
    else:
        e.mode = _lib.HEADS_NLL
        e.x, e.ldx, e.xidx = _f32(nll['x'], 'x'), _ld(nll['x']), _i32(nll.get('xidx'))
        e.coef, e.part = _f32(nll['coef'], 'coef'), _f32(nll['part'], 'part')
        assert nll['part'].is_contiguous() and tuple(nll['part'].shape) == (out.shape[0], heads_tiles(split))
    _lib.check(_lib.load().dv_gemm_heads(C.byref(d), C.byref(e), _stream()), 'dv_gemm_heads')


def linear_bwd_data(dx, dpre, W, *, kscale=None, alpha=1.0, beta=0.0, yref=None, act=0, shift=0.0, overread=False,
                    npad=False):
    """dx = beta*dx + alpha*((dpre*kscale) W) * act'(yref)   (W may be a column slice view)."""
    if yref is None:
        gemm(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta, overread=overread, npad=npad)
    else:
        gemm(dx, dpre, W, True, False, a_kscale=kscale, alpha=alpha, beta=beta, epi=EPI_BWD, yref=yref, act0=act,
             act1=act, shift0=shift, shift1=shift, overread=overread, npad=npad)


def linear_bwd_weight(dW, dpre, x, *, beta=0.0, dbias=None, overread=False, npad=False):
    """dW = beta*dW + dpre^T x ;  dbias = beta*dbias + colsum(dpre) fused in the same launch."""
    gemm(dW, dpre, x, False, False, beta=beta, a_colsum=dbias, colsum_beta=beta, overread=overread, npad=npad)


def bn_fwd(y, x, w, b, mean, rstd, running_mean, running_var, eps=1e-5, momentum=0.1, training=True):
    """nn.BatchNorm1d forward over the rows of x, see ``dv_bn_fwd`` (mean / rstd: saved for the backward pass)"""
    M, N = x.shape
    _lib.check(_lib.load().dv_bn_fwd(_f32(x), _ld(x), M, N, _f32(w), _f32(b), eps, _f32(mean), _f32(rstd), _f32(y), _ld(y),
                                     _f32(running_mean), _f32(running_var), momentum, int(bool(training)), _stream()),
               'dv_bn_fwd')


def bn_bwd(dx, dw, db, dy, x, mean, rstd, w, training=True):
    M, N = x.shape
    _lib.check(_lib.load().dv_bn_bwd(_f32(dy), _ld(dy), _f32(x), _ld(x), _f32(mean), _f32(rstd), _f32(w), M, N, _f32(dx),
                                     _ld(dx), _f32(dw), _f32(db), int(bool(training)), _stream()), 'dv_bn_bwd')


def mask_scale(y, x, mask, scale):
    M, N = x.shape
    _lib.check(_lib.load().dv_mask_scale(_f32(x), _ld(x), _f32(mask), _ld(mask), scale, M, N, _f32(y), _ld(y), _stream()),
               'dv_mask_scale')


def colsum(out, X, beta=0.0):
    M, N = X.shape
    _lib.check(_lib.load().dv_colsum(_f32(X), _ld(X), M, N, _f32(out), beta, _stream()), 'dv_colsum')


def act_bwd_(dY, Y, *, split=None, act0=0, act1=0, shift0=0.0, shift1=0.0):
    M, N = Y.shape
    _lib.check(_lib.load().dv_act_bwd(_f32(dY), _ld(dY), _f32(Y), _ld(Y), M, N, N if split is None else split,
                                      _act(act0), _act(act1), shift0, shift1, _stream()), 'dv_act_bwd')


def wn_scale(scale, norm, W, g):
    N, K = W.shape
    _lib.check(_lib.load().dv_wn_scale(_f32(W), _ld(W), _f32(g), N, K, _f32(scale), _f32(norm), _stream()),
               'dv_wn_scale')


def wn_bwd(dW, dg, dWraw, W, g, norm, beta=0.0):
    N, K = W.shape
    _lib.check(_lib.load().dv_wn_bwd(_f32(dWraw), _ld(dWraw), _f32(W), _ld(W), _f32(g), _f32(norm), N, K, _f32(dW),
                                     _ld(dW), _f32(dg), beta, _stream()), 'dv_wn_bwd')


# --------------------------------------------------------------------------- reparam
def reparam_fwd(out, mu, sd, eps, *, mode=GAUSS_LOGVAR, src_idx=None, reps=1, sub=None, out2=None, out3=None,
                out3_idx=None):
    """out[l*n+j] = mu[q] + eps[l*n+j]*std(sd[q]), q = src_idx[j] or j; out2 = out - sub;
    out3[out3_idx[r]] = out[r] where out3_idx[r] >= 0."""
    R, Z = out.shape
    n = R // reps
    assert n * reps == R and eps.shape[0] == R
    assert _ld(mu) == _ld(sd)
    _lib.check(_lib.load().dv_reparam_fwd(_f32(mu), _f32(sd), _ld(mu), _i32(src_idx), n, reps, Z, _f32(eps),
                                          _ld(eps), mode, _f32(out), _ld(out), _f32(sub), _ld(sub), _f32(out2),
                                          _ld(out2), _f32(out3), _ld(out3), _i32(out3_idx), _stream()),
               'dv_reparam_fwd')


def reparam_bwd(dmu, dsd, dz, eps, sd, *, mode=GAUSS_LOGVAR, src_idx=None, reps=1, beta=0.0):
    R, Z = dz.shape
    n = R // reps
    assert _ld(dmu) == _ld(dsd)
    _lib.check(_lib.load().dv_reparam_bwd(_f32(dz), _ld(dz), _f32(eps), _ld(eps), _f32(sd), _ld(sd), _i32(src_idx),
                                          n, reps, Z, mode, _f32(dmu), _f32(dsd), _ld(dmu), beta, _stream()),
               'dv_reparam_bwd')


# The arguments that order one launch against the other chain (``schedule.StepSync`` builds them by name).  A plain
# tuple in the same field order is accepted wherever one of them is.
class Wait(NamedTuple):        # park until ``flag`` >= ``ctr`` + ``add``, at most ``max_spins`` polls (None: WAIT_SPINS);
    # a time-out sets ``err``
    flag: Any
    ctr: Any
    err: Any
    add: int = 1
    max_spins: Optional[int] = None


class Publish(NamedTuple):     # ``flag`` = ``ctr`` + ``add``, on entry of the launch
    flag: Any
    ctr: Any
    add: int = 1


class Gate(NamedTuple):        # the optimiser sweep's elements [``lo``, ``hi``) wait like a ``Wait`` (mind ``add`` / ``err``)
    flag: Any
    ctr: Any
    add: int
    err: Any
    lo: int
    hi: int


def _wait(park):
    """``Wait`` -> dv_wait (None: no wait)"""
    if park is None:
        return None
    park = Wait(*park)
    w = _lib.Wait()
    w.flag, w.ctr, w.err, w.add = _i32(park.flag), _i32(park.ctr), _i32(park.err), park.add
    w.max_spins = WAIT_SPINS if park.max_spins is None else park.max_spins
    return C.byref(w)


def _publish(pub):
    """``Publish`` -> dv_publish (None: nothing published)"""
    if pub is None:
        return None
    pub = Publish(*pub)
    w = _lib.Publish()
    w.flag, w.ctr, w.add = _i32(pub.flag), _i32(pub.ctr), pub.add
    return C.byref(w)


def _bump(counters):
    """up to two (counter, inc) -> dv_bump (None / empty: nothing)"""
    cs = [c for c in (counters or ()) if c[0] is not None]
    if not cs:
        return None
    assert len(cs) <= 2
    b = _lib.Bump()
    for i, (c, inc) in enumerate(cs):
        b.c[i], b.n[i], b.inc[i] = _i32(c), c.numel(), inc
    return C.byref(b)


def _halt(halt):
    """the (err, ticks) pairs of a step's device-side waits -> (pointer, number of pairs)"""
    if halt is None:
        return None, 0
    assert halt.numel() % 2 == 0
    return _i32(halt), halt.numel() // 2


def reparam_bwd_seg(dmu, dsd, dz, eps, sd, seg_ptr, seg_rows, *, mode=GAUSS_LOGVAR, extra=None, ex_ptr=None,
                    ex_rows=None, beta=0.0, bump=None, dz_add=None, park=None, prior=None):
    """CSR backward of the reparameterisation (+ row-aligned extra (dmu|dsd) rows), see dv_reparam_bwd_seg.
    ``bump``: up to two (counter, inc) the launch advances as well; ``dz_add``: a second gradient source for the first
    ``dz_add.shape[0]`` sample rows; ``park`` = (flag, ctr, err[, add[, max_spins]]): the launch parks on another chain's flag;
    ``prior`` = (coef, raw, kl_min, mu): the gradient of coef * max(KL(q_i || N(0,I)), kl_min) is added to row i (dv_prior_kl)"""
    nq, Z = seg_ptr.numel() - 1, dz.shape[1]
    assert _ld(dmu) == _ld(dsd)
    add = None
    if dz_add is not None:
        add = _lib.SegAdd(_f32(dz_add), _ld(dz_add), dz_add.shape[0])
    pk = None
    if prior is not None:
        pk = C.byref(_lib.PriorKl(coef=_f32(prior[0]), raw=_f32(prior[1]), kl_min=prior[2], mu=_f32(prior[3]), ld=_ld(prior[3])))
    _lib.check(_lib.load().dv_reparam_bwd_seg(_f32(dz), _ld(dz), _f32(eps), _ld(eps), _f32(sd), _ld(sd),
                                              _i32(seg_ptr), _i32(seg_rows), nq, Z, mode, _f32(extra), _ld(extra),
                                              _i32(ex_ptr), _i32(ex_rows), _f32(dmu), _f32(dsd), _ld(dmu), beta,
                                              _bump(bump), C.byref(add) if add is not None else None, _wait(park), pk,
                                              _stream()), 'dv_reparam_bwd_seg')


def z2f_post_bwd(dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, raw, kl_min, dz1b, L, B, Np,
                 park=None, prior=None, kl_out=None, seg=None, z1_dz2f=0.0):
    """fused backward of the z2Fz1 sample / KL(q(z2|x2)||p(z2|z1)) / residual block, see dv_z2f_post_bwd.
    ``park`` = (flag, ctr, err[, add[, max_spins]]): the launch first parks on another chain's flag.
    ``prior`` = (coef, raw) of the Np q2 rows: their prior-KL gradient (same kl_min) is added to dq2 (dv_prior_kl).
    ``kl_out``: the launch forms the pairs' KL rows itself -- ``kl_out`` and ``raw`` are then OUTPUTS, what
    ``kl_rows_fwd(kl_out, raw, ..., free_bits=True)`` in front of it wrote.  ``seg`` = (src, seg_ptr[, beta]): sample row r
    also adds beta * the sum of ``src`` rows [seg_ptr[r], seg_ptr[r+1]) (their first Z columns) to dz1, and
    ``z1_dz2f`` * dz2f[r] (a classifier on [z1, z2Fz1 - z1]: -1)."""
    Z = dp2.shape[1] // 2
    d = _lib.Z2F(dz2f=_f32(dz2f), ld_dz2f=_ld(dz2f), dzdec_pert=_f32(dzdec_pert), ld_pert=_ld(dzdec_pert),
                 pair_slot=_i32(pair_slot), eps=_f32(eps), lde=_ld(eps), p2=_f32(p2), ldp2=_ld(p2), q2=_f32(q2),
                 ldq2=_ld(q2), coef=_f32(coef), raw=_f32(raw), kl_min=kl_min, dz1b=_f32(dz1b), ld_dz1b=_ld(dz1b),
                 dp2=_f32(dp2), ld_dp2=_ld(dp2), dz1=_f32(dz1), ld_dz1=_ld(dz1), dq2=_f32(dq2), ld_dq2=_ld(dq2),
                 L=L, B=B, Np=Np, Z=Z, prior_coef=_f32(prior[0]) if prior is not None else None,
                 prior_raw=_f32(prior[1]) if prior is not None else None)
    if kl_out is not None:
        d.kl_out, d.raw_out, d.raw = _f32(kl_out), _f32(raw), None
    d.z1_dz2f = z1_dz2f
    if seg is not None:
        d.seg_src, d.ld_seg, d.seg_ptr, d.seg_beta = _f32(seg[0]), _ld(seg[0]), _i32(seg[1]), seg[2] if len(seg) > 2 else 1.0
    _lib.check(_lib.load().dv_z2f_post_bwd(C.byref(d), _wait(park), _stream()), 'dv_z2f_post_bwd')


# --------------------------------------------------------------------------- KL rows
def _kl_desc(out, raw, mu_q, sd_q, mu_p=None, sd_p=None, *, prior=(0.0, 0.0), mode=GAUSS_LOGVAR, qidx=None, pidx=None,
             reps=1, free_bits=False, kl_min=0.0, add=None):
    R = out.numel()
    assert _ld(mu_q) == _ld(sd_q) and (mu_p is None or _ld(mu_p) == _ld(sd_p))
    return _lib.KlRows(mu_q=_f32(mu_q), sd_q=_f32(sd_q), ldq=_ld(mu_q), qidx=_i32(qidx), mu_p=_f32(mu_p), sd_p=_f32(sd_p),
                       ldp=_ld(mu_p), pidx=_i32(pidx), prior_mu=prior[0], prior_sd=prior[1], n=R // reps, reps=reps,
                       Z=mu_q.shape[1], mode=mode, free_bits=int(free_bits), kl_min=kl_min, raw_out=_f32(raw), out=_f32(out),
                       add=_f32(add))


def kl_rows_fwd_pair(first, second):
    """two independent sets of plain KL rows in one launch; ``first`` / ``second`` = (args, kwargs) of ``kl_rows_fwd``
    (no fused sample, no second term, no park)"""
    d1, d2 = _kl_desc(*first[0], **first[1]), _kl_desc(*second[0], **second[1])
    _lib.check(_lib.load().dv_kl_rows_fwd_pair(C.byref(d1), C.byref(d2), _stream()), 'dv_kl_rows_fwd_pair')


def kl_rows_fwd(out, raw, mu_q, sd_q, mu_p=None, sd_p=None, *, prior=(0.0, 0.0), mode=GAUSS_LOGVAR, qidx=None,
                pidx=None, reps=1, free_bits=False, kl_min=0.0, add=None, eps=None, zout=None, park=None, second=None):
    """``second`` = (mu2, sd2, raw2): a second, row-aligned term KL(N(mu2, sd2) || N(prior)) with its own free bits is
    added to ``out`` and its raw value written to ``raw2`` (same launch)"""
    R = out.numel()
    n = R // reps
    Z = mu_q.shape[1]
    assert _ld(mu_q) == _ld(sd_q) and (mu_p is None or _ld(mu_p) == _ld(sd_p))
    assert second is None or (_ld(second[0]) == _ld(second[1]) and second[0].shape[0] == R)
    d = _lib.KlRows(_f32(mu_q), _f32(sd_q), _ld(mu_q), _i32(qidx), _f32(mu_p), _f32(sd_p), _ld(mu_p), _i32(pidx),
                    prior[0], prior[1], n, reps, Z, mode, int(free_bits), kl_min, _f32(raw), _f32(out), _f32(add),
                    _f32(eps), _ld(eps), _f32(zout), _ld(zout),
                    _f32(second[0]) if second else None, _f32(second[1]) if second else None,
                    _ld(second[0]) if second else 0, second[0].shape[1] if second else 0,
                    _f32(second[2]) if second else None)
    _lib.check(_lib.load().dv_kl_rows_fwd(C.byref(d), _wait(park), _stream()), 'dv_kl_rows_fwd')


def kl_rows_bwd(dq_mu, dq_sd, dp_mu, dp_sd, coef, raw, mu_q, sd_q, mu_p=None, sd_p=None, *, prior=(0.0, 0.0),
                mode=GAUSS_LOGVAR, qidx=None, pidx=None, reps=1, free_bits=False, kl_min=0.0, beta=0.0, dz=None,
                eps=None):
    R = coef.numel()
    n = R // reps
    Z = mu_q.shape[1]
    assert _ld(dq_mu) == _ld(dq_sd) and (dp_mu is None or _ld(dp_mu) == _ld(dp_sd))
    d = _lib.KlRows(mu_q=_f32(mu_q), sd_q=_f32(sd_q), ldq=_ld(mu_q), qidx=_i32(qidx), mu_p=_f32(mu_p), sd_p=_f32(sd_p),
                    ldp=_ld(mu_p), pidx=_i32(pidx), prior_mu=prior[0], prior_sd=prior[1], n=n, reps=reps, Z=Z, mode=mode,
                    free_bits=int(free_bits), kl_min=kl_min, raw_out=_f32(raw), eps=_f32(eps), lde=_ld(eps))
    g = _lib.KlRowsGrad(coef=_f32(coef), dq_mu=_f32(dq_mu), dq_sd=_f32(dq_sd), lddq=_ld(dq_mu), dp_mu=_f32(dp_mu),
                        dp_sd=_f32(dp_sd), lddp=_ld(dp_mu), beta=beta, dz=_f32(dz), ldz=_ld(dz))
    _lib.check(_lib.load().dv_kl_rows_bwd(C.byref(d), C.byref(g), _stream()), 'dv_kl_rows_bwd')


# ------------------------------------------------------------------------- NLL rows
def nll_rows_fwd(out, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, bias=None, sd_shift=1e-3):
    """``bias`` = (bias_mu, bias_sd): ``mu`` / ``sd`` are the heads' raw products, finished by the pass (mu + bias_mu,
    softplus(sd + bias_sd) + sd_shift): evaluation passes behind a plain heads product"""
    M, X = mu.shape
    assert _ld(mu) == _ld(sd)
    _lib.check(_lib.load().dv_gauss_nll_rows_fwd(_f32(x), _ld(x), _i32(xidx), _f32(mu), _f32(sd), _ld(mu), M, X,
                                                 mode, _f32(out), _f32(bias[0]) if bias is not None else None,
                                                 _f32(bias[1]) if bias is not None else None, sd_shift, _stream()),
               'dv_gauss_nll_rows_fwd')


def nll_rows_fwdbwd(out, dmu, dsd, coef, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, sd_act=0, sd_shift=0.0, bias=None):
    """row log-likelihoods AND coef-weighted gradients w.r.t. (mu, pre-activation of sd) in one pass; ``bias`` =
    (bias_mu, bias_sd): ``mu`` / ``sd`` are the heads' raw products, finished here (+ bias, activation of sd, shift)"""
    M, X = mu.shape
    assert _ld(mu) == _ld(sd) and _ld(dmu) == _ld(dsd)
    _lib.check(_lib.load().dv_gauss_nll_rows_fwdbwd(_f32(coef), _f32(x), _ld(x), _i32(xidx), _f32(mu), _f32(sd),
                                                    _ld(mu), M, X, mode, _act(sd_act), sd_shift, _f32(out),
                                                    _f32(dmu), _f32(dsd), _ld(dmu),
                                                    _f32(bias[0]) if bias is not None else None,
                                                    _f32(bias[1]) if bias is not None else None, _stream()),
               'dv_gauss_nll_rows_fwdbwd')


def nll_raw_cs_shape(M, X):
    """(chunks, row_blocks) of ``nll_rows_raw_cs`` for M rows of X genes"""
    lib = _lib.load()
    return lib.dv_nll_raw_cs_chunks(X), lib.dv_nll_raw_cs_row_blocks(M)


def nll_rows_raw_cs(out_part, dmu, dsd, ws, coef, x, mu, sd, bias, *, xidx=None, sd_shift=1e-3):
    """the raw-heads NLL forward + backward pass with the heads' bias gradient folded in (``dv_gauss_nll_rows_raw_cs``):
    ``out_part`` (M, chunks) partial row log-likelihoods, ``ws`` (row_blocks, ld) per-block column sums of (dmu | dsd) --
    dsd's at the column offset dsd has behind dmu; the caller sums the blocks (``colsum``).  ``dmu = dsd = ws = coef =
    None``: forward only (evaluation)."""
    M, X = mu.shape
    chunks, rbs = nll_raw_cs_shape(M, X)
    fwd_only = dmu is None
    assert _ld(mu) == _ld(sd) and tuple(out_part.shape) == (M, chunks) and out_part.is_contiguous()
    off = 0
    if not fwd_only:
        assert _ld(dmu) == _ld(dsd) and dmu.untyped_storage().data_ptr() == dsd.untyped_storage().data_ptr()
        off = dsd.storage_offset() - dmu.storage_offset()
        assert ws.shape[0] == rbs and ws.dim() == 2
    else:
        assert dsd is None and ws is None
    d = _lib.NllRawCs(coef=_f32(coef), x=_f32(x), ldx=_ld(x), xidx=_i32(xidx), mu=_f32(mu), sd=_f32(sd), ldp=_ld(mu), M=M,
                      X=X, shift=sd_shift, out_part=_f32(out_part), chunks=chunks, dmu=_f32(dmu), dsd=_f32(dsd),
                      ldd=_ld(dmu), bias_mu=_f32(bias[0]), bias_sd=_f32(bias[1]), ws=_f32(ws),
                      ldw=ws.stride(0) if ws is not None else 0, sd_off=off, row_blocks=rbs)
    _lib.check(_lib.load().dv_gauss_nll_rows_raw_cs(C.byref(d), _stream()), 'dv_gauss_nll_rows_raw_cs')


def rec_nll_rows(out, x, v, *, kind, shift=0.0, xidx=None, coef=None, dpre=None, library=False):
    """log-likelihood rows of the Bernoulli ('binary') / Poisson decoders from the head's post-activation output
    ``v``; with ``coef`` also the gradient w.r.t. the head's pre-activation (``dv_rec_nll_rows``).  ``kind='nb'`` (negative
    binomial): ``v`` = [mu | theta] and ``dpre`` = [d/da_m | d/da_t], 2X columns each; ``shift`` is the mean's, theta's is
    ``DV_NB_THETA_SHIFT``.  ``kind='zinb'`` (zero-inflated negative binomial): ``v`` = [mu | theta | dropout logit] (the
    logit RAW) and ``dpre`` = [d/da_m | d/da_t | d/da_d], 3X columns each.  ``library`` ('poisson' / 'nb' / 'zinb' only): the
    library-scaled kind -- the mean of row r is s * v with s = max(sum_g x[xidx[r], g], 1) / X, the size factor the kernel
    forms from the target row it reads"""
    from .engine import REC_FAMILIES          # (the engine imports this module: looked up at call time)
    fam = REC_FAMILIES[kind]
    code = fam.rows_kind_lib if library else fam.rows_kind
    if library and code is None:
        raise ValueError("rec_nll_rows: library= is for kind 'poisson' / 'nb' / 'zinb', not %r" % (kind,))
    M, X = v.shape
    if len(fam.heads) > 1:
        X, w = x.shape[1], len(fam.heads)
        assert v.shape[1] == w * X and (dpre is None or tuple(dpre.shape) == (M, w * X))
    _lib.check(_lib.load().dv_rec_nll_rows(code, shift, _f32(coef), _f32(x), _ld(x), _i32(xidx), _f32(v),
                                           _ld(v), M, X, _f32(out), _f32(dpre), _ld(dpre), _stream()), 'dv_rec_nll_rows')


def nll_rows_bwd(dmu, dsd, coef, x, mu, sd, *, mode=GAUSS_SIGMA, xidx=None, sd_act=0, sd_shift=0.0, dx=None,
                 beta=0.0):
    M, X = mu.shape
    assert _ld(mu) == _ld(sd) and _ld(dmu) == _ld(dsd)
    _lib.check(_lib.load().dv_gauss_nll_rows_bwd(_f32(coef), _f32(x), _ld(x), _i32(xidx), _f32(mu), _f32(sd),
                                                 _ld(mu), M, X, mode, _act(sd_act), sd_shift, _f32(dmu), _f32(dsd),
                                                 _ld(dmu), _f32(dx), _ld(dx), beta, _stream()),
               'dv_gauss_nll_rows_bwd')


# ----------------------------------------------------------------------- categorical
def softmax_clamp_fwd(probs, logits, sigmoid1=False):
    M, Y = probs.shape
    _lib.check(_lib.load().dv_softmax_clamp_fwd(_f32(logits), _ld(logits), M, Y, int(sigmoid1), _f32(probs),
                                                _ld(probs), _stream()), 'dv_softmax_clamp_fwd')


def softmax_clamp_bwd(dlogits, dprobs, probs, sigmoid1=False, beta=0.0):
    M, Y = probs.shape
    _lib.check(_lib.load().dv_softmax_clamp_bwd(_f32(dprobs), _ld(dprobs), _f32(probs), _ld(probs), M, Y,
                                                int(sigmoid1), _f32(dlogits), _ld(dlogits), beta, _stream()),
               'dv_softmax_clamp_bwd')


def cat_terms_fwd(probs, *, labels=None, prior=None, logp=None, kl=None, ent=None, best=None):
    M, Y = probs.shape
    _lib.check(_lib.load().dv_cat_terms_fwd(_f32(probs), _ld(probs), M, Y, _i32(labels), _f32(prior), _ld(prior),
                                            _f32(logp), _f32(kl), _ld(kl), _f32(ent), _i32(best), _stream()),
               'dv_cat_terms_fwd')


def cat_terms_bwd(dprobs, probs, *, labels=None, prior=None, c_logp=None, g_kl=None, c_ent=None, beta=0.0):
    M, Y = probs.shape
    _lib.check(_lib.load().dv_cat_terms_bwd(_f32(probs), _ld(probs), M, Y, _i32(labels), _f32(prior), _ld(prior),
                                            _f32(c_logp), _f32(g_kl), _ld(g_kl), _f32(c_ent), _f32(dprobs),
                                            _ld(dprobs), beta, _stream()), 'dv_cat_terms_bwd')


def smalln_fwd(probs, logits, a1, W, bias=None, a2=None, ymarg=None, park=None, fprop_kl=None, dgrad=None):
    """probs = clamp(softmax([a1|a2] W^T + b)) for N <= 8 outputs (either output may be None).
    ``ymarg`` = (yl, kld, cfp, dqy, label, fp_ptr, klfp, log_prior, c_kld, c_yl): the y-marginalisation of every row
    (the arguments of ``ymarg_fwdbwd``) rides on the same launch.  ``park`` = (flag, ctr, err[, add[, max_spins]]): every
    workgroup first parks on another chain's flag (see ``flag_wait``).  ``fprop_kl`` = dict(Q, qidx, P, Q3, Z1, Z3,
    kl_min, raw1, raw3, dq, dp) with ``ymarg``: the KL rows of the fprop rows (forward in front of the
    y-marginalisation, the z1 term's backward behind it) ride on the same launch (``dv_fprop_kl``).  ``dgrad`` (with
    ``ymarg``) = up to two (dst, col0, alpha, beta[, col1, alpha2]) of ``smalln_bwd_data``: the classifier's data gradient
    from the ``dqy`` the launch has just stored leaves it too (``dv_clf_dgrad``)."""
    M = a1.shape[0]
    N = W.shape[0]
    K1, K2 = a1.shape[1], (a2.shape[1] if a2 is not None else 0)
    ym = None
    if ymarg is not None:
        yl, kld, cfp, dqy, label, fp_ptr, klfp, log_prior, c_kld, c_yl = ymarg
        vec = log_prior if torch.is_tensor(log_prior) else None
        y = _lib.Ymarg()
        y.label, y.fp_ptr, y.klfp = _i32(label), _i32(fp_ptr), _f32(klfp)
        y.log_prior, y.log_prior_v = (0.0 if vec is not None else log_prior), _f32(vec)
        y.c_kld, y.c_yl, y.yl, y.kld, y.cfp = _f32(c_kld), _f32(c_yl), _f32(yl), _f32(kld), _f32(cfp)
        y.dqy, y.lddq = _f32(dqy), _ld(dqy)
        ym = C.byref(y)
    kf = None
    if fprop_kl is not None:
        assert ymarg is not None
        f = _lib.FpropKl()
        Q, P, Q3 = fprop_kl['Q'], fprop_kl['P'], fprop_kl['Q3']
        f.Z1, f.Z3, f.kl_min = fprop_kl['Z1'], fprop_kl['Z3'], fprop_kl['kl_min']
        assert Q.shape[1] == 2 * f.Z1 and P.shape[1] == 2 * f.Z1 and Q3.shape[1] == 2 * f.Z3
        f.mu_q, f.ldq, f.qidx = _f32(Q), _ld(Q), _i32(fprop_kl['qidx'])
        f.mu_p, f.ldp, f.mu3, f.ld3 = _f32(P), _ld(P), _f32(Q3), _ld(Q3)
        f.klfp, f.raw1, f.raw3 = _f32(ymarg[6]), _f32(fprop_kl['raw1']), _f32(fprop_kl['raw3'])
        f.dq, f.lddq, f.dp, f.lddp = _f32(fprop_kl['dq']), _ld(fprop_kl['dq']), _f32(fprop_kl['dp']), _ld(fprop_kl['dp'])
        kf = C.byref(f)
    dg = None
    if dgrad:
        assert ymarg is not None and len(dgrad) <= 2
        g = _lib.ClfDgrad(n=len(dgrad))
        for t, d in enumerate(dgrad):
            g.dst[t], g.ld[t], g.col0[t], g.ncol[t], g.alpha[t], g.beta[t] = _f32(d[0]), _ld(d[0]), d[1], d[0].shape[1], d[2], d[3]
            g.col1[t], g.alpha2[t] = (d[4], d[5]) if len(d) > 5 else (0, 0.0)
        dg = C.byref(g)
    _lib.check(_lib.load().dv_smalln_linear_fwd(_f32(a1), _ld(a1), K1, _f32(a2), _ld(a2), K2, _f32(W), _ld(W),
                                                _f32(bias), M, N, _f32(logits), _ld(logits), _f32(probs),
                                                _ld(probs), ym, _wait(park), kf, dg, _stream()), 'dv_smalln_linear_fwd')


def smalln_bwd_data(dsts, dprobs, probs, W, seg=None):
    """dsts: list of (dst, col0, alpha, beta[, col1, alpha2]);
    dst = beta*dst + dlogit @ (alpha*W[:, col0:col0+w] + alpha2*W[:, col1:col1+w]), w = dst.shape[1].
    ``seg`` = (src, seg_ptr): the FIRST destination starts from the segment sum of ``src`` rows
    [seg_ptr[r], seg_ptr[r+1]) (its first w columns) instead of beta*dst."""
    M, N = dprobs.shape
    n = len(dsts)
    P = (C.c_void_p * n)(*[_f32(d[0]) for d in dsts])
    LD = (C.c_int64 * n)(*[_ld(d[0]) for d in dsts])
    C0 = (C.c_int32 * n)(*[d[1] for d in dsts])
    NC = (C.c_int32 * n)(*[d[0].shape[1] for d in dsts])
    AL = (C.c_float * n)(*[d[2] for d in dsts])
    BE = (C.c_float * n)(*[d[3] for d in dsts])
    C1 = (C.c_int32 * n)(*[(d[4] if len(d) > 4 else 0) for d in dsts])
    A2 = (C.c_float * n)(*[(d[5] if len(d) > 5 else 0.0) for d in dsts])
    _lib.check(_lib.load().dv_smalln_linear_bwd_data(_f32(dprobs), _ld(dprobs), _f32(probs), _ld(probs), _f32(W),
                                                     _ld(W), M, N, n, P, LD, C0, NC, AL, BE, C1, A2,
                                                     _f32(seg[0]) if seg else None, _ld(seg[0]) if seg else 0,
                                                     _i32(seg[1]) if seg else None, _stream()),
               'dv_smalln_linear_bwd_data')


SMALLN_WS_SPLITS = 16


def smalln_ws_numel(N, K):
    """floats of the optional row-split workspace of ``smalln_bwd_weight`` for N classes and K = K1 + K2 inputs"""
    return SMALLN_WS_SPLITS * N * (K + 1)


def smalln_bwd_weight(dW, db, dprobs, probs, a1, a2=None, beta=0.0, publish=None, ws=None):
    """``publish`` = (flag, ctr[, add]): the launch publishes on entry that everything in front of it is complete;
    ``ws`` (``smalln_ws_numel`` floats): lets many-row products (>= 1024 rows) split the rows over workgroups"""
    M, N = dprobs.shape
    K1, K2 = a1.shape[1], (a2.shape[1] if a2 is not None else 0)
    assert ws is None or (ws.is_contiguous() and ws.numel() >= smalln_ws_numel(N, K1 + K2))
    _lib.check(_lib.load().dv_smalln_linear_bwd_weight(_f32(dprobs), _ld(dprobs), _f32(probs), _ld(probs), _f32(a1),
                                                       _ld(a1), K1, _f32(a2), _ld(a2), K2, M, N, _f32(dW), _ld(dW),
                                                       _f32(db), beta, _publish(publish), _f32(ws),
                                                       SMALLN_WS_SPLITS if ws is not None else 0, _stream()),
               'dv_smalln_linear_bwd_weight')


def ymarg_fwd(yl, kld, qy, label, fp_ptr, klfp, log_prior):
    """``log_prior``: python float (uniform prior) or a device vector of Y log-probabilities"""
    R, Y = qy.shape
    vec = log_prior if torch.is_tensor(log_prior) else None
    _lib.check(_lib.load().dv_ymarg_fwd(_f32(qy), _ld(qy), _i32(label), _i32(fp_ptr), _f32(klfp),
                                        0.0 if vec is not None else log_prior, _f32(vec), R, Y, _f32(yl), _f32(kld),
                                        _stream()), 'dv_ymarg_fwd')


def ymarg_fwdbwd(yl, kld, cfp, dqy, qy, label, fp_ptr, klfp, log_prior, c_kld, c_yl):
    R, Y = qy.shape
    vec = log_prior if torch.is_tensor(log_prior) else None
    _lib.check(_lib.load().dv_ymarg_fwdbwd(_f32(qy), _ld(qy), _i32(label), _i32(fp_ptr), _f32(klfp),
                                           0.0 if vec is not None else log_prior, _f32(vec), _f32(c_kld), _f32(c_yl),
                                           R, Y, _f32(yl), _f32(kld), _f32(cfp), _f32(dqy), _ld(dqy), _stream()),
               'dv_ymarg_fwdbwd')


def ymarg_bwd(cfp, dqy, qy, label, fp_ptr, klfp, log_prior, c_kld, c_yl):
    R, Y = qy.shape
    vec = log_prior if torch.is_tensor(log_prior) else None
    _lib.check(_lib.load().dv_ymarg_bwd(_f32(qy), _ld(qy), _i32(label), _i32(fp_ptr), _f32(klfp),
                                        0.0 if vec is not None else log_prior, _f32(vec), _f32(c_kld), _f32(c_yl), R, Y,
                                        _f32(cfp), _f32(dqy), _ld(dqy), _stream()), 'dv_ymarg_bwd')


def ycont_fwd(yl, fpin_y, z3in_y, mu, ylab, has_y, eps, logvar, B, sqerr=False):
    """regression head forward, see ``dv_ycont_fwd``"""
    R, Y = mu.shape
    _lib.check(_lib.load().dv_ycont_fwd(_f32(mu), _ld(mu), _f32(ylab), _i32(has_y), _f32(eps), _ld(eps), logvar, int(sqerr), R, B,
                                        Y, _f32(yl), _f32(fpin_y), _ld(fpin_y), _f32(z3in_y), _ld(z3in_y), _stream()),
               'dv_ycont_fwd')


def ycont_bwd(dlogit, cfp, mu, ylab, has_y, logvar, c_yl, c_kld, dfpin_y, dz3in_y, B, sqerr=False):
    """``dlogit`` None: only cfp[r] = c_kld[r]; else the gradient w.r.t. the head's pre-sigmoid output"""
    R, Y = mu.shape
    _lib.check(_lib.load().dv_ycont_bwd(_f32(mu), _ld(mu), _f32(ylab), _i32(has_y), logvar, int(sqerr), _f32(c_yl),
                                        _f32(c_kld),
                                        _f32(dfpin_y), _ld(dfpin_y), _f32(dz3in_y), _ld(dz3in_y), R, B, Y,
                                        _f32(dlogit), _ld(dlogit), _f32(cfp), _stream()), 'dv_ycont_bwd')


def mmd_rff_fwd(diff, mmd2, th1, th2, c):
    """finish the random-Fourier-feature MMD^2 from the projections theta, see ``dv_mmd_rff_fwd``"""
    R = th1.shape[1]
    _lib.check(_lib.load().dv_mmd_rff_fwd(_f32(th1), _ld(th1), th1.shape[0], _f32(th2), _ld(th2), th2.shape[0], R, c,
                                          _f32(diff), _f32(mmd2), _stream()), 'dv_mmd_rff_fwd')


def mmd_rff_bwd(G, th, diff, gout, coef):
    n, R = th.shape
    _lib.check(_lib.load().dv_mmd_rff_bwd(_f32(th), _ld(th), n, R, _f32(diff), _f32(gout), coef, _f32(G), _ld(G),
                                          _stream()), 'dv_mmd_rff_bwd')


MMD_KIND = {'poly': 0, 'rbf': 1}


def _gammas(gammas):
    arr = (C.c_float * len(gammas))(*[float(g) for g in gammas])
    return arr, len(gammas)


def mmd_mix_fwd(part, G, kind, gammas, sa=None, sb=None):
    """part[i] = sum_j of the kernel mixture on the Gram matrix ``G`` (``dv_mmd_mix_fwd``); ``sa`` / ``sb``: the self
    products whose diagonals are the squared row norms (rbf)"""
    arr, nb = _gammas(gammas)
    M, N = G.shape
    _lib.check(_lib.load().dv_mmd_mix_fwd(_f32(G), _ld(G), M, N, MMD_KIND[kind], arr, nb, _f32(sa), (_ld(sa) + 1) if sa is not None else 0,
                                          _f32(sb), (_ld(sb) + 1) if sb is not None else 0, _f32(part), _stream()), 'dv_mmd_mix_fwd')


def mmd_mix_bwd(W, rs, G, kind, gammas, gout, coef, sa=None, sb=None):
    arr, nb = _gammas(gammas)
    M, N = G.shape
    _lib.check(_lib.load().dv_mmd_mix_bwd(_f32(G), _ld(G), M, N, MMD_KIND[kind], arr, nb, _f32(sa), (_ld(sa) + 1) if sa is not None else 0,
                                          _f32(sb), (_ld(sb) + 1) if sb is not None else 0, _f32(gout), coef, _f32(W), _ld(W),
                                          _f32(rs), _stream()), 'dv_mmd_mix_bwd')


def mmd_mix_combine(out4, p11, p12, p22, c11, c12, c22):
    _lib.check(_lib.load().dv_mmd_mix_combine(_f32(p11), p11.numel(), c11, _f32(p12), p12.numel(), c12, _f32(p22), p22.numel(),
                                              c22, _f32(out4), _stream()), 'dv_mmd_mix_combine')


def mmd_identity_fwd(diff, out, x1, x2):
    _lib.check(_lib.load().dv_mmd_identity_fwd(_f32(x1), _ld(x1), x1.shape[0], _f32(x2), _ld(x2), x2.shape[0], x1.shape[1],
                                               _f32(diff), _f32(out), _stream()), 'dv_mmd_identity_fwd')


def mmd_identity_bwd(dx, diff, gout, coef):
    _lib.check(_lib.load().dv_mmd_identity_bwd(_f32(diff), _f32(gout), coef, dx.shape[0], dx.shape[1], _f32(dx), _ld(dx),
                                               _stream()), 'dv_mmd_identity_bwd')


def nuisance_feed(sohe, sohd, cls, s32, *, table=None, n_batches=0, ctr=None, base=None, pair_rows=None, L=1):
    """classes of a batch's rows -> one-hot columns of the stacked encoder (``sohe``) / decoder (``sohd``) rows and the
    class vector ``cls`` (B, int32); ``s32``: the dataset's column read through batch (ctr - base) of ``table``, or
    (``table`` None) the batch's own B classes.  See ``dv_nuisance_feed``"""
    B, S = cls.numel(), sohe.shape[1]
    Np = pair_rows.numel() if pair_rows is not None else 0
    assert sohe.shape[0] == B + Np and sohd.shape[0] == L * B + 2 * L * Np and sohd.shape[1] == S
    assert table is None or (tuple(table.shape) == (n_batches, B) and table.is_contiguous())
    assert table is not None or s32.numel() == B
    _lib.check(_lib.load().dv_nuisance_feed(_i32(s32), _i32(table), n_batches, _i32(ctr), _i32(base), B, _i32(pair_rows), Np,
                                            L, S, _f32(sohe), _ld(sohe), _f32(sohd), _ld(sohd), _i32(cls), _stream()),
               'dv_nuisance_feed')


MMD_GROUPED_KIND = {'identity': 0, 'rbf_fourier': 1}
MMD_MAX_CLASSES = 8         # DV_MMD_MAX_CLASSES


def _mmd_grouped_desc(g):
    """``g``: the operands of the grouped MMD penalty by name (``_Plan``'s term table, see ``dv_mmd_grouped_desc``)"""
    z, dz, rff = g['z'], g['dz'], g['kind'] == 'rbf_fourier'
    n_groups, E, Kc = g['grp_ptr'].numel() - 1, g['rows'].numel(), (1 if g['S'] == 2 else g['S'])
    D = g['R'] if rff else z.shape[1]
    assert g['src'].numel() == E and tuple(g['diff'].shape) == (n_groups * Kc, D) and g['diff'].is_contiguous()
    assert tuple(g['cnt'].shape) == (n_groups, g['S']) and g['m2'].numel() == n_groups * Kc and dz.shape == z.shape
    if rff:
        assert tuple(g['W'].shape) == (n_groups * Kc, z.shape[1], g['R']) and g['W'].is_contiguous()
        assert tuple(g['b'].shape) == (n_groups * Kc, g['R']) and g['b'].is_contiguous()
        assert tuple(g['theta'].shape) == (Kc * E, g['R']) and g['theta'].is_contiguous()
    return _lib.MmdGrouped(z=_f32(z), ldz=_ld(z), n_z=z.shape[0], Z=z.shape[1], kind=MMD_GROUPED_KIND[g['kind']],
                           R=g['R'] if rff else 0, n_groups=n_groups, n_entries=E, max_rows=g['max_rows'], S=g['S'],
                           B=g['cls'].numel(), grp_ptr=_i32(g['grp_ptr']), rows=_i32(g['rows']), src=_i32(g['src']),
                           cls=_i32(g['cls']), W=_f32(g['W']) if rff else None, b=_f32(g['b']) if rff else None, a=g['a'],
                           c=g['c'], w=g['w'], fac=g['fac'], theta=_f32(g['theta']) if rff else None, diff=_f32(g['diff']),
                           cnt=_i32(g['cnt']), m2=_f32(g['m2']), value=_f32(g['value']), dz=_f32(dz), ldd=_ld(dz))


def mmd_grouped_fwd(g):
    """feature-mean differences of every MMD term of a step, one launch (``dv_mmd_grouped_fwd``)"""
    d = _mmd_grouped_desc(g)
    _lib.check(_lib.load().dv_mmd_grouped_fwd(C.byref(d), _stream()), 'dv_mmd_grouped_fwd')


def mmd_grouped_bwd(g):
    """the penalty's value and its gradient w.r.t. the sample rows, one launch (``dv_mmd_grouped_bwd``)"""
    d = _mmd_grouped_desc(g)
    _lib.check(_lib.load().dv_mmd_grouped_bwd(C.byref(d), _stream()), 'dv_mmd_grouped_bwd')


MMD_MASKED_MODEL = {'drvae': 0, 'pvae': 1, 'vfae': 2}       # DV_MMD_GROUPS_*: (data groups, their order)
MMD_MASKED_GROUPS = {'drvae': 4, 'pvae': 2, 'vfae': 2}


def mmd_masked_shapes(model, B, Np, L, S):
    """(row lists, data groups, classes looped, terms, rows of z) of the masked penalty of a universal plan"""
    n_lists, G, Kc = L * (2 if Np else 1), MMD_MASKED_GROUPS[model], (1 if S == 2 else S)
    return n_lists, G, Kc, n_lists * G * Kc, L * (B + Np)


def _mmd_masked_desc(g):
    """``g``: the operands of the masked MMD penalty by name (``_Plan.carry_nuisance`` on a universal plan, see
    ``dv_mmd_masked_desc``); ``hx`` / ``hy`` (and ``table`` / ``n_batches`` / ``ctr`` / ``base``) are the batch's flags"""
    z, dz, rff, S = g['z'], g['dz'], g['kind'] == 'rbf_fourier', g['S']
    B, Np, L = g['cls'].numel(), g['Np'], g['L']
    n_lists, G, Kc, T, n_z = mmd_masked_shapes(g['model'], B, Np, L, S)
    D = g['R'] if rff else z.shape[1]
    assert z.shape[0] == n_z and dz.shape == z.shape and tuple(g['diff'].shape) == (T, D) and g['diff'].is_contiguous()
    assert tuple(g['cnt'].shape) == (n_lists * G, S + 1) and tuple(g['members'].shape) == (n_lists * G, B)
    assert g['cnt'].is_contiguous() and g['members'].is_contiguous() and g['m2'].numel() == T
    if rff:
        assert tuple(g['W'].shape) == (T, z.shape[1], g['R']) and g['W'].is_contiguous()
        assert tuple(g['b'].shape) == (T, g['R']) and g['b'].is_contiguous()
        assert tuple(g['theta'].shape) == (Kc * n_z, g['R']) and g['theta'].is_contiguous()
    hx, hy, table = g.get('hx'), g.get('hy'), g.get('table')
    flags = [f for f in (hx, hy) if f is not None]
    assert all(f.dtype == torch.int32 and f.is_contiguous() for f in flags)
    assert len({f.numel() for f in flags}) <= 1 and (table is not None or all(f.numel() == B for f in flags))
    assert table is None or (tuple(table.shape) == (g['n_batches'], B) and table.is_contiguous())
    return _lib.MmdMasked(z=_f32(z), ldz=_ld(z), Z=z.shape[1], kind=MMD_GROUPED_KIND[g['kind']], R=g['R'] if rff else 0, S=S,
                          B=B, Np=Np, L=L, model=MMD_MASKED_MODEL[g['model']], cls=_i32(g['cls']), hx=_i32(hx), hy=_i32(hy),
                          n_flags=flags[0].numel() if flags else 1, table=_i32(table),
                          n_batches=g.get('n_batches', 0) if table is not None else 0,
                          ctr=_i32(g.get('ctr')) if table is not None else None,
                          base=_i32(g.get('base')) if table is not None else None,
                          W=_f32(g['W']) if rff else None, b=_f32(g['b']) if rff else None, a=g['a'], c=g['c'], w=g['w'],
                          fac=g['fac'], theta=_f32(g['theta']) if rff else None, diff=_f32(g['diff']), cnt=_i32(g['cnt']),
                          members=_i32(g['members']), m2=_f32(g['m2']), value=_f32(g['value']), dz=_f32(dz), ldd=_ld(dz))


def mmd_masked_fwd(g):
    """feature-mean differences of every MMD term of a step on a universal plan, one launch (``dv_mmd_masked_fwd``)"""
    d = _mmd_masked_desc(g)
    _lib.check(_lib.load().dv_mmd_masked_fwd(C.byref(d), _stream()), 'dv_mmd_masked_fwd')


def mmd_masked_bwd(g):
    """the penalty's value and its gradient w.r.t. every sample row, one launch (``dv_mmd_masked_bwd``)"""
    d = _mmd_masked_desc(g)
    _lib.check(_lib.load().dv_mmd_masked_bwd(C.byref(d), _stream()), 'dv_mmd_masked_bwd')


def rows_gather(out, src, idx=None, *, noise=None, sigma=0.0, onehot_cls=None, n_classes=0, width=None, park=None):
    n = out.shape[0]
    W = (src.shape[1] if src is not None else 0) if width is None else width
    _lib.check(_lib.load().dv_rows_gather(_f32(src), _ld(src), _i32(idx), n, W, _f32(noise), _ld(noise), sigma,
                                          _i32(onehot_cls), n_classes, _f32(out), _ld(out), _wait(park), _stream()),
               'dv_rows_gather')


def _masks_desc(m, B):
    """keyword arguments of ``batch_masks`` -> dv_batch_masks_desc"""
    d = dict(hx=None, hy=None, y=None, c_klz2=None, c_yl=None, w_pert=None, w_yl=None, label=None, c_klp=None, Np=None,
             one_slot=None, gcounts=None, anneal=None)
    d.update(m)
    assert d['gcounts'] is None or (d['gcounts'].dtype == torch.int32 and d['gcounts'].is_contiguous())
    md = _lib.BatchMasks(_i32(d['hx']), _i32(d['hy']), _i32(d['y']), B if d['Np'] is None else d['Np'],
                         d['n_tot'], d['kl_rate'], d['pert_rate'], d['yl_rate'], _f32(d['beta']), _f32(d['c_nll']),
                         _f32(d['c_klz2']), _f32(d['c_yl']), _f32(d['w_recl']), _f32(d['w_pert']), _f32(d['w_yl']),
                         _i32(d['label']), _f32(d['c_klp']), _i32(d['one_slot']), _i32(d['gcounts']))
    an = d['anneal']
    if an is not None:      # the annealing schedules: the descriptor's trailing fields (left zero: the launch as it was)
        sched, w_elbo, w_cmpl = an['sched'], an['w_elbo'], an['w_cmpl']
        assert sched.numel() == 4 and w_elbo.numel() >= 3 and w_cmpl.numel() >= 8 and an['step'].dtype == torch.int32
        assert all(t is None or t.is_contiguous() for t in (sched, w_elbo, w_cmpl, an.get('c_kld'), an.get('w_klz2'),
                                                            an.get('w_klp')))
        md.sched_step = _i32(an['step'])
        md.pert_itermax, md.pert_offset = int(an['pert'][0]), int(an['pert'][1])
        md.kl_itermax = int(an['kl'])
        md.yl_itermax, md.yl_offset = int(an['yl'][0]), int(an['yl'][1])
        md.lr_itermax = int(an['lr'])
        md.mmd_rate = float(an.get('mmd_rate', 0.0))
        md.sched, md.w_elbo, md.w_cmpl = _f32(sched), _f32(w_elbo), _f32(w_cmpl)
        md.c_kld, md.w_klz2, md.w_klp = _f32(an.get('c_kld')), _f32(an.get('w_klz2')), _f32(an.get('w_klp'))
    return md


FEED_TRANSFORM = {None: 0, 'log1p': 1, 'log1p_norm': 3}      # dv_batch_feed_desc.transform (2 is no code: refused)


def _csr_fields(m):
    """``CsrRows`` -> the (ptr, idx, val) addresses of dv_batch_feed_desc's csr1_* / csr2_* fields"""
    if not (m.ptr.is_cuda and m.ptr.dtype == torch.int64 and m.ptr.is_contiguous()):
        raise RuntimeError('CsrRows.ptr must be a contiguous CUDA int64 tensor (CsrRows.to(device))')
    if m.nnz == 0:      # (no entry is ever read: any address completes the triple -- an empty tensor has none of its own)
        return m.ptr.data_ptr(), m.ptr.data_ptr(), m.ptr.data_ptr()
    return m.ptr.data_ptr(), _i32(m.idx, 'CsrRows.idx'), _f32(m.val, 'CsrRows.val')


def batch_feed(xin, x1, x2, y32, table, n_batches, ctr, base, *, pair_rows=None, noise=None, sigma=0.0, has_y=None,
               L=1, label_r=None, fp_i=None, fp_lab=None, fp_slot=None, fp_cls=None, onehot=None, n_classes=0, yf=None,
               ylab=None, onehot2=None, masks=None, park=None, xt=None, transform=None):
    """graph-resident minibatch feed: see dv_batch_feed in include/drvae_hip.h; ``masks``: keyword arguments of
    ``batch_masks`` (minus table / ctr / base / B / L): the batch's masks written by the same launch.  ``xt`` (split form,
    raw-count inputs): the raw rows go to ``xt`` and ``xin`` gets T(x) + sigma * noise, T = log1p with ``transform='log1p'``,
    log1p(x / s) with ``'log1p_norm'`` -- s = max(sum_g x_g, 1) / X of the same source row, summed by the launch itself"""
    B = table.shape[1]
    md = _masks_desc(masks, B) if masks is not None else None
    assert masks is None or masks.get('gcounts') is None or masks['gcounts'].shape[0] == n_batches
    Np = pair_rows.numel() if pair_rows is not None else 0
    assert xin.shape[0] == B + Np and table.shape[0] == n_batches and table.is_contiguous()
    Mf = fp_cls.numel() if fp_cls is not None else 0
    # (a ``CsrRows`` for x1 / x2: the matrix goes in as its CSR triple -- the descriptor's trailing fields -- not as a dense pointer)
    csr1, csr2 = (x1 if isinstance(x1, CsrRows) else None), (x2 if (isinstance(x2, CsrRows) and Np) else None)
    x1, x2 = (None if csr1 is not None else x1), (None if isinstance(x2, CsrRows) else x2)
    assert all(c is None or c.shape[1] == xin.shape[1] for c in (csr1, csr2))
    d = _lib.BatchFeed(x1=_f32(x1), ld1=_ld(x1), x2=_f32(x2) if Np else None, ld2=_ld(x2) if Np else 0, y=_i32(y32),
                       table=_i32(table), n_batches=n_batches, ctr=_i32(ctr), base=_i32(base), B=B,
                       pair_rows=_i32(pair_rows), Np=Np, X=xin.shape[1], noise=_f32(noise), ldn=_ld(noise), sigma=sigma,
                       xin=_f32(xin), ldo=_ld(xin), has_y=_i32(has_y), L=L, label_r=_i32(label_r), fp_i=_i32(fp_i),
                       fp_lab=_i32(fp_lab), fp_slot=_i32(fp_slot), Mf=Mf, fp_cls=_i32(fp_cls), onehot=_f32(onehot),
                       ldh=_ld(onehot), Y=n_classes, yf=_f32(yf), ylab=_f32(ylab),
                       Yc=ylab.shape[1] if ylab is not None else 0, onehot2=_f32(onehot2), ldh2=_ld(onehot2))
    if xt is not None or transform is not None:
        assert xt is None or tuple(xt.shape) == tuple(xin.shape)
        d.xt, d.ldt, d.transform = _f32(xt), _ld(xt), FEED_TRANSFORM[transform]
    if csr1 is not None:
        d.csr1_ptr, d.csr1_idx, d.csr1_val = _csr_fields(csr1)
    if csr2 is not None:
        d.csr2_ptr, d.csr2_idx, d.csr2_val = _csr_fields(csr2)
    _lib.check(_lib.load().dv_batch_feed(C.byref(d), C.byref(md) if md is not None else None, _wait(park), _stream()),
               'dv_batch_feed')


def batch_masks(B, L, *, table=None, n_batches=0, ctr=None, base=None, **masks):
    """per-batch coefficient / weight vectors of a batch-independent step plan from the batch's pair / label flags
    (``dv_batch_masks``); ``hx`` / ``hy`` / ``y``: int32 device arrays indexed by dataset row (``table`` given) or by
    batch row; ``beta``: 1-element device float; ``Np``: rows [0, Np) have pair slots (default: all B); ``gcounts``
    (int32, (n_batches | 1, 2)): the GLOBAL (N_pairs, N_labeled) per batch under data parallelism.
    ``anneal`` (the annealing schedules, "annealing schedules" in include/drvae_hip.h): dict(step=<int32 device scalar: finished
    iterations>, pert=(itermax, offset), kl=itermax, yl=(itermax, offset), lr=itermax -- an itermax <= 0 switches that schedule
    off --, mmd_rate, sched=<4 floats: the record>, w_elbo, w_cmpl[, c_kld, w_klz2, w_klp]); ``beta`` is then not read"""
    md = _masks_desc(masks, B)
    _lib.check(_lib.load().dv_batch_masks(C.byref(md), _i32(table), n_batches, _i32(ctr), _i32(base), B, L, _stream()),
               'dv_batch_masks')


def rows_segment_sum(dst, src, *, seg_ptr=None, seg_rows=None, w=None, n=None, dst_idx=None, beta=0.0, width=None,
                     park=None):
    if n is None:
        n = seg_ptr.numel() - 1 if seg_ptr is not None else (seg_rows.numel() if seg_rows is not None else
                                                              src.shape[0])
    W = dst.shape[1] if width is None else width
    _lib.check(_lib.load().dv_rows_segment_sum(_f32(src), _ld(src), _i32(seg_ptr), _i32(seg_rows), _f32(w), n, W,
                                               _i32(dst_idx), _f32(dst), _ld(dst), beta, _wait(park), _stream()),
               'dv_rows_segment_sum')


def weighted_sum(out, x, w=None, idx=None, scale=1.0, beta=0.0, n=None):
    if n is None:
        n = idx.numel() if idx is not None else x.numel()
    _lib.check(_lib.load().dv_weighted_sum(_f32(x), _f32(w), _i32(idx), n, scale, _f32(out), beta, _stream()),
               'dv_weighted_sum')


def recon_row_stats(out, x, r):
    """out (M,6): per-row {SSE, mean x, mean r, centred sums xx, rr, xr} (evaluation metrics)."""
    M, X = x.shape
    assert out.is_contiguous() and tuple(out.shape) == (M, 6)
    _lib.check(_lib.load().dv_recon_row_stats(_f32(x), _ld(x), _f32(r), _ld(r), M, X, _f32(out), _stream()),
               'dv_recon_row_stats')


def col_moments(out, x, r, sel=None, part=None, r_bias=None):
    """out (3,X) float64: per-column sum x, sum x^2, sum (x-r)^2 over the rows (``sel``: int32 list of the rows that
    count).  ``part`` (row_blocks, 3, X) float64: leave the per-block partials there instead (``recon_finalize`` adds
    them up); out may then be None.  ``r_bias`` (X): r is a raw heads product, r + r_bias the reconstruction."""
    M = sel.numel() if sel is not None else x.shape[0]
    X = x.shape[1]
    if part is not None:
        nb = part.shape[0]
        assert part.dtype == torch.float64 and part.is_cuda and part.is_contiguous() and tuple(part.shape[1:]) == (3, X)
    else:
        assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (3, X)
        nb = col_moment_blocks(M)      # row blocks: partial sums per block, added up here in a fixed order
        part = out.unsqueeze(0) if nb == 1 else torch.empty(nb, 3, X, dtype=torch.float64, device=out.device)
    _lib.check(_lib.load().dv_col_moments(_f32(x), _ld(x), _f32(r), _ld(r), M, X, part.data_ptr(), nb, _i32(sel), _f32(r_bias), _stream()),
               'dv_col_moments')
    if out is not None and part.data_ptr() != out.data_ptr():
        torch.sum(part, 0, out=out)


def col_moment_blocks(M):
    """row blocks of ``col_moments`` (16-wave workgroups): 256 rows up to 16 blocks, then 512 rows, at most 64 --
    ``recon_finalize``, one workgroup, walks every block's partials"""
    return max(1, min(64, max(min(16, (M + 255) // 256), (M + 511) // 512)))


RECON_ROWS_MAX_X = 1024


def recon_rows(rows, ll, x, mu, sd, *, bias=None, sd_shift=1e-3, kind=None, size_from=None, rec_out=None):
    """row statistics (M, 6) and log-likelihood rows (M; may be None) of a reconstruction in ONE pass over (x, mu, sd),
    X <= RECON_ROWS_MAX_X -- ``recon_row_stats`` + ``nll_rows_fwd``.  ``bias`` = (bias_mu, bias_sd): mu / sd are the
    heads' raw products, finished on the way.

    The count decoders: ``kind='binary' | 'poisson' | 'nb' | 'zinb'``, any X.  ``mu`` is the mean head's finished output, ``sd`` the
    theta head for 'nb', the (M, 2X) pair [theta | raw dropout logit] for 'zinb' (the decoder's heads buffer from column X on; the
    statistics and ``rec_out`` are 'nb''s, at the negative-binomial mean) and None otherwise.  ``size_from`` (M, X;
    'poisson' / 'nb' / 'zinb'): the statistics and the log-likelihood are taken at r = s * mu, s the size factor of ``size_from``'s rows
    (the target itself or another matrix); ``rec_out`` (M, X; with ``size_from`` only, may be ``mu`` itself) receives r."""
    M, X = x.shape
    if kind is not None:
        assert kind in ('binary', 'poisson', 'nb', 'zinb') and bias is None
        assert tuple(mu.shape) == (M, X) and rows.is_contiguous() and tuple(rows.shape) == (M, 6)
        if kind == 'zinb':
            assert sd is not None and tuple(sd.shape) == (M, 2 * X)
        else:
            assert (sd is not None and tuple(sd.shape) == (M, X)) if kind == 'nb' else sd is None
        assert size_from is None or tuple(size_from.shape) == (M, X)
        assert rec_out is None or tuple(rec_out.shape) == (M, X)
        assert ll is None or (ll.is_contiguous() and ll.numel() == M)
        d = _lib.ReconRows(x=_f32(x), ldx=_ld(x), mu=_f32(mu), sd=_f32(sd), ldp=_ld(mu), M=M, X=X, rows=_f32(rows),
                           ll=_f32(ll), kind=_lib.RECON_ZINB if kind == 'zinb' else _lib.RECON_KIND[kind], ldt=_ld(sd) if sd is not None else 0,
                           size_x=_f32(size_from), size_ld=_ld(size_from) if size_from is not None else 0,
                           rec_out=_f32(rec_out), rec_ld=_ld(rec_out) if rec_out is not None else 0)
        _lib.check(_lib.load().dv_recon_rows(C.byref(d), _stream()), 'dv_recon_rows')
        return
    assert size_from is None and rec_out is None, 'size_from / rec_out: the count kinds'
    assert tuple(mu.shape) == (M, X) and tuple(sd.shape) == (M, X) and _ld(mu) == _ld(sd)
    assert rows.is_contiguous() and tuple(rows.shape) == (M, 6)
    d = _lib.ReconRows(x=_f32(x), ldx=_ld(x), mu=_f32(mu), sd=_f32(sd), ldp=_ld(mu),
                       bias_mu=_f32(bias[0]) if bias is not None else None,
                       bias_sd=_f32(bias[1]) if bias is not None else None, sd_shift=sd_shift, M=M, X=X,
                       rows=_f32(rows), ll=_f32(ll))
    _lib.check(_lib.load().dv_recon_rows(C.byref(d), _stream()), 'dv_recon_rows')


def recon_finalize(out4, rows, part, X, *, sel=None, n=None, ll=None):
    """out4 (4 float64) = rmse, variance-weighted R^2, mean per-row Pearson r, mean log-likelihood from the partials of
    ``recon_row_stats`` / ``col_moments(part=...)`` (+ the per-row log-likelihoods): ``dv_recon_finalize``"""
    n = (sel.numel() if sel is not None else rows.shape[0]) if n is None else n
    assert out4.dtype == torch.float64 and out4.is_cuda and out4.numel() >= 4 and out4.is_contiguous()
    assert part.dtype == torch.float64 and part.is_contiguous() and rows.is_contiguous() and rows.shape[1] == 6
    _lib.check(_lib.load().dv_recon_finalize(_f32(rows), _i32(sel), n, X, part.data_ptr(), part.shape[0], _f32(ll),
                                             out4.data_ptr(), _stream()), 'dv_recon_finalize')


RANK_MAX_ROWS = 32768       # DV_RANK_MAX_ROWS


def rank_metrics(out, counts, proba, y32, *, pred32=None, sel=None, c0=1, n_cls=1, binary=True):
    """ROC-AUC / average precision per class and the accuracy (``dv_rank_metrics``): out (2 n_cls + 1 float64), counts
    (n_cls, n, 4) int32 zeros (left zeroed)"""
    n = sel.numel() if sel is not None else proba.shape[0]
    assert out.dtype == torch.float64 and out.is_cuda and out.numel() >= 2 * n_cls + 1 and out.is_contiguous()
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= n_cls * n * 4
    _lib.check(_lib.load().dv_rank_metrics(_f32(proba), _ld(proba), _i32(y32), _i32(pred32), _i32(sel), n, c0, n_cls,
                                           int(bool(binary)), counts.data_ptr(), out.data_ptr(), _stream()), 'dv_rank_metrics')


def reg_metrics(out3, pred, y, *, sel=None, n=None):
    """out3 (3 float64) = rmse, R^2, Pearson r of a continuous target over the rows ``sel`` (int32; None: the first ``n``
    rows, default all) x the Y columns of ``pred`` / ``y`` ((rows, Y) fp32, row strides free), both flattened; two-pass
    float64 sums in a fixed order (``dv_reg_metrics``)"""
    pred = pred.reshape(-1, 1) if pred.dim() == 1 else pred
    y = y.reshape(-1, 1) if y.dim() == 1 else y
    n = (sel.numel() if sel is not None else pred.shape[0]) if n is None else n
    assert pred.dim() == 2 and y.dim() == 2 and pred.shape[1] == y.shape[1]
    assert sel is not None or (n <= pred.shape[0] and n <= y.shape[0])
    assert out3.dtype == torch.float64 and out3.is_cuda and out3.numel() >= 3 and out3.is_contiguous()
    _lib.check(_lib.load().dv_reg_metrics(_f32(pred), _ld(pred), _f32(y), _ld(y), _i32(sel), n, pred.shape[1],
                                          out3.data_ptr(), _stream()), 'dv_reg_metrics')


def loss_assemble(loss, terms, w_elbo, w_cmpl, after=None, bump=(), halt=None, accum=None):
    """terms: list of (x, w_or_None, scale, out_index); see ``dv_loss_assemble``.  ``after`` =
    a ``Wait``: park like ``flag_wait`` inside the same launch first;
    ``bump`` = up to two (counter, inc): advanced at the end of the launch;
    ``halt``: the (err, ticks) pairs of the step's waits -- any error set: the scalars come out NaN;
    ``accum`` (8 floats): running sums, ``accum += loss`` in the same launch."""
    hp, hn = _halt(halt)
    arr = (_lib.LossTerm * max(len(terms), 1))()
    for i, term in enumerate(terms):      # (x, w, scale, out[, row_len]): row_len > 1 = one weight per row of x
        x, w, scale, out = term[:4]
        arr[i].x, arr[i].w, arr[i].n, arr[i].scale, arr[i].out = _f32(x), _f32(w), x.numel(), scale, out
        arr[i].row_len = term[4] if len(term) > 4 else 1
    if after is None and not bump:
        _lib.check(_lib.load().dv_loss_assemble(arr, len(terms), _f32(w_elbo), _f32(w_cmpl), _f32(loss), hp, hn,
                                                _f32(accum), _stream()), 'dv_loss_assemble')
    else:
        # (``after`` None: no wait, only the counters ride on the launch)
        _lib.check(_lib.load().dv_loss_assemble_after(_wait(after), arr, len(terms), _f32(w_elbo), _f32(w_cmpl), _f32(loss),
                                                      _bump(bump), hp, hn, _f32(accum), _stream()), 'dv_loss_assemble_after')


def axpby(y, x, a=1.0, b=0.0):
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    _lib.check(_lib.load().dv_axpby(_f32(x), a, _f32(y), b, x.numel(), _stream()), 'dv_axpby')


# ------------------------------------------------------------------------- optimiser
def _hyper(lr, beta1, beta2, eps, weight_decay, gscale, lr_scale, p=None, decoupled=False, avg=None, avg_decay=None):
    """dv_adam_hyper; ``lr_scale``: None or a 1-element fp32 device tensor the sweep multiplies the rate by (in double, one
    rounding: learning-rate annealing); ``decoupled``: AdamW's weight decay (p *= 1 - lr * wd, no wd * p in the gradient);
    ``avg`` / ``avg_decay``: the parameter average riding on the sweep, laid out like ``p`` -- e += (1 - avg_decay)(p_new - e).
    The three defaults leave the trailing fields zero: the sweep as it was"""
    assert lr_scale is None or (lr_scale.dtype == torch.float32 and lr_scale.numel() == 1)
    h = _lib.AdamHyper(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, gscale=gscale,
                       lr_scale=_f32(lr_scale))
    if decoupled:
        h.decoupled = 1
    if avg is not None:
        if avg_decay is None:
            raise ValueError('an average needs its avg_decay')
        assert avg.dtype == torch.float32 and avg.is_contiguous() and avg.numel() == p.numel() and avg.device == p.device
        h.avg, h.avg_decay = _f32(avg), avg_decay
    return h


def _sweep(symbol, p, g, m, v, step_or_state, *, gate=None, halt=None, **hyper):
    """one optimiser sweep through entry point ``symbol`` -- what the four public wrappers are: they differ in the symbol and in
    whether the int32 tensor behind the moments is the step counter or a clip state (its first word is the step).
    ``gate`` = a ``Gate``: elements [lo, hi) wait for the flag (the symbol's ``_gated`` form);
    ``halt``: the (err, ticks) pairs of the step's waits -- any error set: nothing is updated;
    ``hyper``: ``_hyper``'s arguments -- ``lr_scale``: a device scalar the rate is multiplied by; ``decoupled``, ``avg``,
    ``avg_decay``: AdamW's decay and the parameter average (Adamax takes the average only)"""
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    hp, hn = _halt(halt)
    h = _hyper(p=p, **hyper)
    args = (_f32(p), _f32(g), _f32(m), _f32(v), p.numel(), C.byref(h), _i32(step_or_state))
    if gate is not None:
        gate, symbol = Gate(*gate), symbol + '_gated'
        args += (_wait(Wait(gate.flag, gate.ctr, gate.err, gate.add)), gate.lo, gate.hi)
    _lib.check(getattr(_lib.load(), symbol)(*args, hp, hn, _stream()), symbol)


def adam_l2(p, g, m, v, step_dev, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, gate=None,
            halt=None, lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    """torch.optim.Adam with coupled L2 (AdamW: ``decoupled``) over the flat range; ``gate``: ``dv_adam_l2_gated`` (``_sweep``)"""
    _sweep('dv_adam_l2', p, g, m, v, step_dev, gate=gate, halt=halt, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
           weight_decay=weight_decay, gscale=gscale, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def adamax_l2(p, g, m, u, step_dev, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
              lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep('dv_adamax_l2', p, g, m, u, step_dev, halt=halt, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
           weight_decay=weight_decay, gscale=gscale, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


# gradient-norm clipping (``StepConfig.max_grad_norm``): ``dv_grad_norm_clip`` and the ``_clipped`` sweeps of include/drvae_hip.h.
# The clip STATE of an engine is one int32 device buffer laid out as ``dv_clip_state`` (``_lib.ClipState``) + workspace: the
# optimiser step (the engine's ``step_dev`` is this word), max_norm (a double), the record {norm, coef (fp32 bits), skip,
# n_skipped}, then ``sumsq_partials(n)`` doubles
CLIP_STATE_WORDS = C.sizeof(_lib.ClipState) // 4
_CLIP_STEP, _CLIP_MAX_NORM, _CLIP_REC = (getattr(_lib.ClipState, f).offset // 4 for f in ('step', 'max_norm', 'rec'))
assert _CLIP_STEP == 0 and CLIP_STATE_WORDS % 2 == 0 and _CLIP_MAX_NORM % 2 == 0


def sumsq_partials(n):
    """number of double partials the norm pass writes for ``n`` elements (DV_SUMSQ_PARTIALS: a function of n alone)"""
    per, cap = _lib.SUMSQ_PER_BLOCK, _lib.SUMSQ_MAX_BLOCKS
    return int(min(max((int(n) + per - 1) // per, 1), cap))


def clip_state(device, n, max_norm):
    st = torch.zeros(CLIP_STATE_WORDS + 2 * sumsq_partials(n), dtype=torch.int32, device=device)
    clip_set_max_norm(st, max_norm)
    return st


def clip_set_max_norm(state, max_norm):
    state[_CLIP_MAX_NORM:_CLIP_MAX_NORM + 2].copy_(torch.tensor([float(max_norm)], dtype=torch.float64).view(torch.int32))


def clip_record(state):
    """the record words {norm, coef, skip, n_skipped} of a clip state (a view)"""
    return state[_CLIP_REC:_CLIP_REC + C.sizeof(_lib.ClipRecord) // 4]


def clip_partials(state):
    """the workspace of a clip state as doubles (a view)"""
    return state[CLIP_STATE_WORDS:].view(torch.float64)


def clip_record_values(record):
    """dict(norm, coef, skipped_last, n_skipped) of a clip record, as python numbers (one small copy)"""
    r = record.detach().cpu()
    f = r.view(torch.float32)
    return dict(norm=float(f[0]), coef=float(f[1]), skipped_last=bool(int(r[2])), n_skipped=int(r[3]))


def clip_norm(g, state, *, gscale=1.0):
    """the norm pass over the contiguous fp32 range ``g`` into ``state``: the sum of squares in double (one partial per
    workgroup), then the record: norm = |gscale| sqrt(sumsq), coef = min(1, max_norm / (norm + 1e-6)), skip (a non-finite sum)
    and the running count of skipped steps.  Two launches (``dv_grad_norm_clip``)"""
    assert g.is_contiguous() and state.numel() >= CLIP_STATE_WORDS + 2 * sumsq_partials(g.numel())
    _lib.check(_lib.load().dv_grad_norm_clip(_f32(g), g.numel(), gscale, _i32(state), _stream()), 'dv_grad_norm_clip')


def adam_l2_clip(p, g, m, v, state, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
                 lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    """``adam_l2`` reading the record of the clip state (whose first word is the step): skipped when the record says so, else
    the gradient scaled by fl32(gscale * coef) and t = step - n_skipped.  No gated form."""
    _sweep('dv_adam_l2_clipped', p, g, m, v, state, halt=halt, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
           weight_decay=weight_decay, gscale=gscale, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def adamax_l2_clip(p, g, m, u, state, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0, halt=None,
                   lr_scale=None, decoupled=False, avg=None, avg_decay=None):
    _sweep('dv_adamax_l2_clipped', p, g, m, u, state, halt=halt, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
           weight_decay=weight_decay, gscale=gscale, lr_scale=lr_scale, decoupled=decoupled, avg=avg, avg_decay=avg_decay)


def flag_publish(flag, ctr, add=1):
    _lib.check(_lib.load().dv_flag_publish(_i32(flag), _i32(ctr), add, _stream()), 'dv_flag_publish')


# Bound of a device-side wait, in polls (~1 us each: an agent-scope load + s_sleep).  Inside one process
# the chains are at most a step (~0.3 ms) apart; under data parallelism a chain may also sit out the skew
# between the ranks (the next step's first publish follows the previous step's gradient exchange), hence
# seconds rather than milliseconds.  A wait that still times out is reported (see ``check_sync``), never hung.
WAIT_SPINS = int(os.environ.get('DRVAE_WAIT_SPINS', '4000000'))


def flag_wait(flag, ctr, err, add=1, max_spins=None, publish=None):
    """the arguments of a ``Wait``; ``publish`` = a ``Publish``: goes out on entry of the wait launch"""
    max_spins = WAIT_SPINS if max_spins is None else max_spins
    _lib.check(_lib.load().dv_flag_wait(_i32(flag), _i32(ctr), add, _i32(err), max_spins, _publish(publish), _stream()),
               'dv_flag_wait')


def counter_add(counter, inc=1):
    _lib.check(_lib.load().dv_counter_add(_i32(counter), counter.numel(), inc, _stream()), 'dv_counter_add')


def counters_add2(c1, inc1, c2, inc2, publish=None):
    """``publish`` = a ``Publish``: goes out on entry, before the counters move (ctr may be one of them)"""
    _lib.check(_lib.load().dv_counters_add2(_i32(c1), c1.numel(), inc1, _i32(c2), c2.numel(), inc2, _publish(publish),
                                            _stream()), 'dv_counters_add2')


def fill_normal_rows(arena, desc, seed, ctr_dev=None, park=None):
    """row-keyed N(0,1) draws of a train step's noise arena: ``desc`` (R,4) int32 = {offset, width, draw id,
    global row}; ``ctr_dev`` counts draw events (see ``dv_fill_normal_rows``)"""
    assert arena.is_contiguous() and desc.dim() == 2 and desc.shape[1] == 4
    _lib.check(_lib.load().dv_fill_normal_rows(_f32(arena), _i32(desc), desc.shape[0], seed, _i32(ctr_dev), _wait(park),
                                               _stream()), 'dv_fill_normal_rows')


def keep_threshold(dropout_rate):
    """``keep_thr`` of the keep rows (``dv_fill_noise_rows``): floor((1 - dropout_rate) * 2^32) in double, as
    uint32; the keep probability of a hidden unit is exactly ``keep_threshold(rate) / 2**32``"""
    assert 0.0 <= dropout_rate < 1.0
    return min(int(math.floor((1.0 - float(dropout_rate)) * 4294967296.0)), 0xFFFFFFFF)


def noise_table(desc, n_normal, keep_thr):
    """the table ``fill_noise_rows`` takes: the (R, 4) descriptor rows ``desc`` -- N(0,1) rows [0, n_normal), KEEP rows behind
    them -- plus the trailer row {number of keep rows, keep_thr's bits, 0, 0}; any ``table[lo:]`` is such a table too"""
    assert desc.dim() == 2 and desc.shape[1] == 4 and 0 <= n_normal <= desc.shape[0] and 0 <= keep_thr <= 0xFFFFFFFF
    thr = keep_thr - (1 << 32) if keep_thr >= (1 << 31) else keep_thr
    tr = torch.tensor([[desc.shape[0] - n_normal, thr, 0, 0]], dtype=torch.int32, device=desc.device)
    return torch.cat([desc.to(torch.int32), tr])


def fill_noise_rows(arena, table, seed, ctr_dev=None, park=None):
    """``fill_normal_rows`` over a ``noise_table``: the same N(0,1) values in its normal rows, 1.0 / 0.0 keep masks with keep
    probability ``keep_thr / 2**32`` in its keep rows -- ``dv_fill_noise_rows``, a kernel of its own"""
    assert arena.is_contiguous() and table.dim() == 2 and table.shape[1] == 4 and table.shape[0] >= 1 and table.is_contiguous()
    _lib.check(_lib.load().dv_fill_noise_rows(_f32(arena), _i32(table), table.shape[0] - 1, seed, _i32(ctr_dev), _wait(park),
                                              _stream()), 'dv_fill_noise_rows')


def fill_normal(out, seed, ctr_dev=None):
    assert out.is_contiguous()
    _lib.check(_lib.load().dv_fill_normal(_f32(out), out.numel(), seed, _i32(ctr_dev), _stream(), None),
               'dv_fill_normal')      # (no draw descriptor: ``count_sample.draw`` is the launch with one)
