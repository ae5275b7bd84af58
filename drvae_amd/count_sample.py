"""Posterior-predictive draws from finished decoder heads: the launcher of the SAMPLER form of ``dv_fill_normal`` (its
trailing ``dv_draw_desc``; include/drvae_hip.h, "THE SAMPLER", is the specification) and the seed rule of the model-level
interface (``ELBOModel.sample_x`` / ``posterior_predictive``).

Every element is a function of (seed, event, sample index, GLOBAL row, gene) and its own operands: a whole-set draw, a draw
in row chunks and a draw of shuffled rows (``grow``) give the same bits.  Like ``drvae_amd.kernels`` there is no CPU path here
(the float64 statement of the same specification is ``tests/count_sample_ref.py``).
"""
import ctypes as C

import torch

from . import _lib
from .kernels import _f32, _i32, _stream

KIND = {'diag_gaussian': 0, 'binary': 1, 'poisson': 2, 'nb': 3, 'zinb': 4}      # type_rec -> DV_RECON_*
CHUNK = 1024            # genes per workgroup (256 threads x 4 genes)
SEED_SALT = 0x5AD0C0DE9E3779B9      # ``default_seed``: what separates a model's draws from its train step's noise


def default_seed(random_seed):
    """the seed of ``sample_x(seed=None)``: the model's ``random_seed`` spread over 64 bits and salted, so that it is not the
    seed of the train step's row-keyed noise (whose blocks the sampler's would otherwise be: see the header)"""
    return ((int(random_seed) & 0xFFFFFFFFFFFFFFFF) * 0x9E3779B97F4A7C15 + SEED_SALT) & 0xFFFFFFFFFFFFFFFF


def event_words(event, device):
    """the draw EVENT as the two int32 device words ``dv_fill_normal`` reads (None for event 0: no words, no copy)"""
    event = 0 if event is None else int(event) & 0xFFFFFFFFFFFFFFFF
    if event == 0:
        return None
    lo, hi = event & 0xFFFFFFFF, event >> 32
    return torch.tensor([lo - (1 << 32) if lo >= 1 << 31 else lo, hi - (1 << 32) if hi >= 1 << 31 else hi],
                        dtype=torch.int32, device=device)


def _row_stride(t, X, name, shared_ok=False):
    """the row stride of a (M, X) operand with unit inner stride; a row expanded over the rows (stride 0) where allowed"""
    if t is None:
        return 0
    if t.dim() != 2 or t.shape[1] != X:
        raise ValueError('count_sample.draw: %s must be (rows, %d), not %r' % (name, X, tuple(t.shape)))
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), X)
    if ld == 0 and not shared_ok:
        raise ValueError('count_sample.draw: %s is a row expanded over the rows; only theta may be one' % name)
    return ld


def draw(out, mu, *, kind, sd=None, theta=None, logit=None, size=None, seed, event=None, row0=0, grow=None, sample0=0):
    """``out`` (S, M, X) float32 <- S samples of the M rows of finished heads: ``mu`` (M, X) always; ``sd`` (Gaussian),
    ``theta`` ('nb' / 'zinb'; a (1, X) row expanded over M rows -- stride 0 -- is read as the one shared row it is), ``logit``
    ('zinb', raw), ``size`` ((M,) size factors, count kinds).  ``kind``: a ``type_rec`` name.  ``seed``: 64 bits; ``event``:
    None, an int, or the two int32 device words of a 64-bit event.  Global rows: ``row0 + r``, or the int32 device array
    ``grow``.  ``sample0``: the sample index of ``out[0]`` (sample k of a launch is sample k of any other launch).  Rows may
    be strided views with unit inner stride; the launch picks 16-byte accesses where every row allows."""
    if kind not in KIND:
        raise ValueError('count_sample.draw: kind is one of %s, not %r' % (sorted(KIND), kind))
    if out.dim() != 3 or mu.dim() != 2:
        raise ValueError('count_sample.draw: out is (samples, rows, genes) and mu (rows, genes)')
    S, M, X = out.shape
    if tuple(mu.shape) != (M, X):
        raise ValueError('count_sample.draw: mu %r does not match out %r' % (tuple(mu.shape), tuple(out.shape)))
    if size is not None and not (size.dim() == 1 and size.numel() == M and size.is_contiguous()):
        raise ValueError('count_sample.draw: size must be a contiguous (rows,) tensor')
    if grow is not None and grow.numel() != M:
        raise ValueError('count_sample.draw: grow must hold one global row per row')
    if torch.is_tensor(event):
        ev = _i32(event, 'event')
    else:
        ev = _i32(event_words(event, out.device), 'event')
    d = _lib.DrawDesc(kind=KIND[kind], M=M, X=X, S=S, mu=_f32(mu, 'mu'), ldm=_row_stride(mu, X, 'mu'),
                      sd=_f32(sd, 'sd'), lds=_row_stride(sd, X, 'sd'),
                      theta=_f32(theta, 'theta'), ldt=_row_stride(theta, X, 'theta', shared_ok=True),
                      logit=_f32(logit, 'logit'), ldl=_row_stride(logit, X, 'logit'), size=_f32(size, 'size'),
                      out=_f32(out, 'out'), ldo=out.stride(1) if M > 1 else max(out.stride(1), X),
                      sso=out.stride(0) if S > 1 else max(out.stride(0), 0), row0=int(row0), grow=_i32(grow, 'grow'),
                      k0=int(sample0))
    _lib.check(_lib.load().dv_fill_normal(None, 0, int(seed) & 0xFFFFFFFFFFFFFFFF, ev, _stream(), C.byref(d)),
               'dv_fill_normal (sampler)')
    return out


# ------------------------------------------------------------------------------------------------ model level
LATENTS = ('mean', 'sample')
X2_SEED_XOR = 0x243F6A8885A308D3         # x2_samp is drawn under seed ^ this: its own stream, not x1_samp's numbers again
LATENT_SEED_XOR = 0x13198A2E03707344     # the row-keyed normals of latent='sample' are drawn under seed ^ this


def _head_operands(model, px, size):
    """the operands of ``draw`` from a decoder_x output ``px`` (UNSCALED heads) and the rows' size factors"""
    tr = model.type_rec
    if tr == 'diag_gaussian':
        return dict(kind=tr, sd=px[1])
    if tr == 'binary':
        return dict(kind=tr)
    kw = dict(kind=tr, size=size)
    if tr in ('nb', 'zinb'):
        kw['theta'] = px[1]
    if tr == 'zinb':
        kw['logit'] = px[2]
    return kw


def check_sample_args(model, n_samples, latent):
    if latent not in LATENTS:
        raise ValueError("latent must be 'mean' (the heads of forward(): observation noise only) or 'sample' (the full "
                         "posterior predictive), not %r" % (latent,))
    if (isinstance(n_samples, bool) or not isinstance(n_samples, (int, float)) or int(n_samples) != n_samples
            or int(n_samples) < 1 or int(n_samples) > _lib.DRAW_MAX_SAMPLES):
        raise ValueError('n_samples must be an integer in 1 .. %d, not %r' % (_lib.DRAW_MAX_SAMPLES, n_samples))
    return int(n_samples)


def _latent_noise(model, S, rows, grow_i32, row0, seed, ev, dev):
    """(S, 2, rows, Z1) row-keyed N(0,1) draws: [k, 0] the z1 noise of sample k (draw id 2k), [k, 1] its z2 noise (draw id
    2k + 1), of the global rows, under seed ^ LATENT_SEED_XOR at the draw's event -- ONE ``fill_normal_rows`` launch"""
    from . import kernels as K
    Z = model.dim_z1
    g = grow_i32.long() if grow_i32 is not None else torch.arange(row0, row0 + rows, device=dev)
    n = S * 2 * rows
    if n * Z >= 1 << 31:       # (the table's offsets are int32)
        raise ValueError("latent='sample': %d samples x 2 x %d rows x %d latent dimensions of noise do not fit one table (2^31 "
                         "elements); sample fewer rows at a time (posterior_predictive: chunk_rows=)" % (S, rows, Z))
    eps = torch.empty(S, 2, rows, Z, device=dev)
    desc = torch.empty(n, 4, dtype=torch.int64, device=dev)
    desc[:, 0] = torch.arange(n, device=dev) * Z
    desc[:, 1] = Z
    desc[:, 2] = torch.arange(S * 2, device=dev).repeat_interleave(rows)
    desc[:, 3] = g.repeat(S * 2)
    K.fill_normal_rows(eps.view(-1), desc.to(torch.int32).contiguous(), (seed ^ LATENT_SEED_XOR) & 0xFFFFFFFFFFFFFFFF, ev)
    return eps


def head_passes(model, x1, s, *, n_samples, latent, seed, ev, row0=0, grow=None, second=True):
    """the latent and decoder passes of ``sample_x``, shared by the sampler (``sample_rows``) and the effect reduction
    (``effect.perturbation_effect``): yields ``(k, which, z, px)`` per sample k in order -- ``which`` 1: z = z1 and the UNSCALED
    heads ``decoder_x([z1] + cond)``; then, with ``second``, ``which`` 2: z = z2 = F(z1) and its heads.  ``latent='mean'``: one
    pass (k = 0) at the means, the heads of ``forward()``.  ``'sample'``: z1 ~ q(z1|x1), z2 ~ p(z2|z1) from the row-keyed normals
    of ``_latent_noise`` (``seed``: the resolved 64-bit seed, ``ev``: the event's device words or None).  The consumer works
    between two yields: nothing of the next pass is launched before it asks for it."""
    cond = model._s_inputs(s, x1)
    qz1 = model.encoder_z1([model._enc_x(x1)] + cond)
    if latent == 'mean':
        z1 = qz1[0]
        yield 0, 1, z1, model.decoder_x([z1] + cond)
        if second:
            z2 = model.decoder_z2Fz1([z1])[0]
            yield 0, 2, z2, model.decoder_x([z2] + cond)
        return
    eps = _latent_noise(model, n_samples, x1.shape[0], grow, row0, seed, ev, x1.device)
    sd1 = torch.exp(0.5 * qz1[1])
    for k in range(n_samples):
        z1 = qz1[0] + sd1 * eps[k, 0]
        yield k, 1, z1, model.decoder_x([z1] + cond)
        if second:
            pz2 = model.decoder_z2Fz1([z1])
            z2 = pz2[0] + torch.exp(0.5 * pz2[1]) * eps[k, 1]
            yield k, 2, z2, model.decoder_x([z2] + cond)


@torch.no_grad()
def sample_rows(model, x1, s, *, n_samples, latent, size_factor, seed, event, row0=0, grow=None, out1=None, want_x2=True,
                latents_out=None):
    """the draws behind ``ELBOModel.sample_x`` for the rows ``x1`` (device, fp32): -> (x1_samp, x2_samp or None).  ``out1``:
    where x1_samp goes ((S, rows, X) float32 device; default a new tensor).  ``latents_out``: a dict that receives z1_samp /
    z2_samp of ``latent='sample'``"""
    S = n_samples
    dev = x1.device
    rows, X = x1.shape
    has2 = want_x2 and model.kind in ('drvae', 'pvae')
    size = model._chosen_size(size_factor, x1)
    if getattr(model, 'library_size', False):
        size = (model.size_factor(x1) if size is None else size).to(torch.float32).contiguous()
    seed = default_seed(model.random_seed) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    ev = event if torch.is_tensor(event) else event_words(event, dev)
    new = lambda: torch.empty(S, rows, X, device=dev)
    out1 = new() if out1 is None else out1
    out2 = new() if has2 else None
    where = dict(event=ev, row0=row0, grow=grow)
    sampled = latent != 'mean'
    if sampled and latents_out is not None:
        latents_out['z1_samp'] = torch.empty(S, rows, model.dim_z1, device=dev)
        if has2:
            latents_out['z2_samp'] = torch.empty(S, rows, model.dim_z1, device=dev)
    for k, which, z, px in head_passes(model, x1, s, n_samples=S, latent=latent, seed=seed, ev=ev, row0=row0, grow=grow,
                                       second=has2):
        out, sd = (out1, seed) if which == 1 else (out2, seed ^ X2_SEED_XOR)
        if sampled:       # one decoder pass per sample: sample k of the launch is sample k of the result
            draw(out[k:k + 1], px[0], seed=sd, sample0=k, **where, **_head_operands(model, px, size))
            if latents_out is not None:
                latents_out['z%d_samp' % which][k] = z
        else:             # the heads of forward(): every sample from the one pass
            draw(out, px[0], seed=sd, **where, **_head_operands(model, px, size))
    return out1, out2


def check_out(out, shape):
    """``posterior_predictive``'s ``out=``: a float32 tensor of ``shape`` on the device, or pinned on the host"""
    if not torch.is_tensor(out) or out.dtype != torch.float32:
        raise ValueError('out must be a float32 tensor, not %s' % (out.dtype if torch.is_tensor(out) else type(out).__name__))
    if tuple(out.shape) != tuple(shape):
        raise ValueError('out must be (n_samples, rows, dim_x) = %r, not %r' % (tuple(shape), tuple(out.shape)))
    if not out.is_contiguous():
        raise ValueError('out must be contiguous')
    if not out.is_cuda and not out.is_pinned():
        raise ValueError('out on the host must be pinned memory (it is filled chunk by chunk from the device)')


@torch.no_grad()
def posterior_predictive(model, ds, n_samples=1, *, chunk_rows=None, out=None, latent='mean', seed=None, event=0):
    """the draws behind ``ELBOModel.posterior_predictive``"""
    from .sparse_rows import CsrRows
    S = check_sample_args(model, n_samples, latent)
    if getattr(model, '_dp', None) is not None:
        raise NotImplementedError('posterior_predictive under data parallelism is not built: sample on one rank')
    if chunk_rows is not None and (int(chunk_rows) != chunk_rows or int(chunk_rows) < 1):
        raise ValueError('chunk_rows must be a positive integer or None, not %r' % (chunk_rows,))
    x1 = ds.x1
    N, X = int(x1.shape[0]), int(x1.shape[1])
    if out is not None:
        check_out(out, (S, N, X))
    if not ((torch.is_tensor(x1) or isinstance(x1, CsrRows)) and x1.is_cuda):
        raise ValueError('posterior_predictive samples a DEVICE-resident set (ds.to(device)); this one lives on the host')
    dev = x1.device
    model.eval()
    C_ = N if chunk_rows is None else min(int(chunk_rows), max(N, 1))
    result = torch.empty(S, N, X, device=dev) if out is None else out
    on_host = not result.is_cuda
    buf = torch.empty(S, C_, X, device=dev) if on_host else None
    dense = torch.empty(C_, X, device=dev) if isinstance(x1, CsrRows) else None
    ev = event_words(event, dev)
    seed = default_seed(model.random_seed) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    for c0 in range(0, N, max(C_, 1)):
        c1 = min(c0 + C_, N)
        if dense is not None:       # sparse rows: one chunk at a time through the feed launch, never the whole matrix
            rows = x1.gather_rows(dense[:c1 - c0], torch.arange(c0, c1, dtype=torch.int32, device=dev))
        else:
            rows = x1[c0:c1].to(torch.float32)
        dst = buf[:, :c1 - c0] if on_host else result[:, c0:c1]
        sample_rows(model, rows, ds.s[c0:c1], n_samples=S, latent=latent, size_factor=None, seed=seed, event=ev, row0=c0,
                    out1=dst, want_x2=False)
        if on_host:
            result[:, c0:c1].copy_(dst, non_blocking=True)
            torch.cuda.current_stream().synchronize()      # (the staging buffer is drawn into again by the next chunk)
    return result
