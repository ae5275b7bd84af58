"""Per-gene perturbation effects: the launcher of the EFFECT REDUCTION (``dv_draw_desc.fx`` behind ``dv_fill_normal``;
include/drvae_hip.h, "THE EFFECT REDUCTION", is the specification) and the model-level summary on top
(``DrVAE.perturbation_effect`` / ``PVAE.perturbation_effect``).

The launch reads two finished mean-head matrices -- a decoded from z1, b from z2 = F(z1) -- and leaves, per (row block, group,
gene), seven float64 sums of the effect e = log2(b + c) - log2(a + c) (count decoders) or b - a (Gaussian): nothing of size
samples x rows x genes exists at any time.  Like ``drvae_amd.kernels`` there is no CPU path here (the float64 statement of the
same specification is ``tests/effect_ref.py``).
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _lib
from .kernels import _f32, _i32, _stream

STATS = _lib.EFFECT_STATS
N_STATS = len(STATS)
MODE = {'diag_gaussian': _lib.EFFECT_DIFF, 'poisson': _lib.EFFECT_LFC, 'nb': _lib.EFFECT_LFC, 'zinb': _lib.EFFECT_LFC}
CHUNK = 64                  # genes per workgroup
TARGET_WORKGROUPS = 1024    # four per compute unit
MIN_ROWS = 32               # rows per block from which the blocks' partials (56 bytes per group and gene) stay under a
#                             quarter of the bytes read (8 per row and gene) for one group


def row_blocks_for(M, X, n_groups=1):
    """the row-block rule: as many blocks as bring the grid (gene chunks x blocks x groups) to ``TARGET_WORKGROUPS``, but no
    block of fewer than ``MIN_ROWS`` rows -- the partials are written once per block and read again by ``fold``"""
    chunks = -(-int(X) // CHUNK)
    return max(1, min(TARGET_WORKGROUPS // (chunks * int(n_groups)), int(M) // MIN_ROWS, 65535))


def _rows(t, M, X, name):
    if t.dim() != 2 or tuple(t.shape) != (M, X):
        raise ValueError('effect_cols: %s must be (%d, %d), not %r' % (name, M, X, tuple(t.shape)))
    ld = t.stride(0) if M > 1 else max(t.stride(0), X)
    if ld < X:
        raise ValueError('effect_cols: the rows of %s overlap (row stride %d < %d genes)' % (name, ld, X))
    return ld


def effect_cols(out, a, b, *, grp=None, n_groups=1, mode, delta, pseudocount=0.0, row_blocks=None):
    """``out`` (row_blocks, n_groups, 7, X) float64 <- the statistics ``STATS`` of the effect between the finished mean heads
    ``a`` and ``b`` ((M, X) float32; views with unit inner stride, e.g. columns of a wider heads buffer; they may be one
    tensor), per row block and group.  ``grp``: (M,) int32 group of every row (None: all in group 0; a value outside [0,
    n_groups) leaves the row out).  ``mode``: ``_lib.EFFECT_LFC`` or ``_lib.EFFECT_DIFF``.  ``row_blocks``: default
    ``out.shape[0]``.  Every element of ``out`` is written; at M == 0 with zeros, here."""
    if a.dim() != 2:
        raise ValueError('effect_cols: a is (rows, genes)')
    M, X = a.shape
    rb = int(out.shape[0]) if row_blocks is None else int(row_blocks)
    if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (rb, n_groups, N_STATS, X)):
        raise ValueError('effect_cols: out must be a contiguous float64 device tensor of shape %r, not %s %r'
                         % ((rb, n_groups, N_STATS, X), out.dtype, tuple(out.shape)))
    if grp is not None and not (grp.dim() == 1 and grp.numel() == M):
        raise ValueError('effect_cols: grp must hold one group per row')
    fx = _lib.EffectDesc(a=_f32(a, 'a'), lda=_rows(a, M, X, 'a'), b=_f32(b, 'b'), ldb=_rows(b, M, X, 'b'), mode=int(mode),
                         delta=float(delta), pseudo=float(pseudocount), out=out.data_ptr(), row_blocks=rb, n_grp=int(n_groups),
                         grp=_i32(grp, 'grp'))
    d = _lib.DrawDesc(M=M, X=X, fx=C.addressof(fx))
    _lib.check(_lib.load().dv_fill_normal(None, 0, 0, None, _stream(), C.byref(d)), 'dv_fill_normal (effect reduction)')
    if M == 0:
        out.zero_()
    return out


def fold(acc, part):
    """the (G, 7, X) float64 accumulator ``acc`` += the blocks of ``part`` (row_blocks, G, 7, X), added up over the leading
    dimension -- the sibling of ``evaluate.fold_col_blocks``: one fixed order for a given shape, chunks and samples in the order
    they arrive"""
    assert acc.dtype == part.dtype == torch.float64 and tuple(acc.shape) == tuple(part.shape[1:])
    return acc.add_(part.sum(0))


def summarize(raw):
    """the (G, 7, X) sums -> the result of ``perturbation_effect``: (G, X) float64 tensors; a gene without a valid element
    (n == 0) has NaN ratios"""
    n, s1, s2, up, dn, sa, sb = raw.unbind(1)
    mean = s1 / n
    return OrderedDict(n=n, lfc_mean=mean, lfc_sd=(s2 / n - mean * mean).clamp_min(0.0).sqrt(), p_up=up / n, p_down=dn / n,
                       mean_base=sa / n, mean_pert=sb / n, raw=raw)


@torch.no_grad()
def perturbation_effect(model, ds, *, n_samples=1, latent='mean', groups=None, n_groups=None, delta=0.25, pseudocount=0.0,
                        chunk_rows=None, seed=None, event=0):
    """the work behind ``ELBOModel.perturbation_effect``"""
    from . import count_sample as CS
    from .sparse_rows import CsrRows
    S = CS.check_sample_args(model, n_samples, latent)
    if latent == 'mean' and S != 1:
        raise ValueError("n_samples must be 1 with latent='mean' (the heads of forward() are one pass); latent='sample' draws more")
    if model.type_rec not in MODE:
        raise ValueError("perturbation_effect: type_rec=%r has no effect scale (the count decoders give a log2 fold change, "
                         "'diag_gaussian' a difference)" % (model.type_rec,))
    mode = MODE[model.type_rec]
    pseudocount, delta = float(pseudocount), float(delta)
    if not (0.0 <= pseudocount < float('inf')):
        raise ValueError('pseudocount must be a finite number >= 0, not %r' % (pseudocount,))
    if mode == _lib.EFFECT_DIFF and pseudocount != 0.0:
        raise ValueError("pseudocount belongs to the log2 fold change of a count decoder; a 'diag_gaussian' model's effect is "
                         "the difference of the means (pseudocount=0)")
    if not delta >= 0.0:
        raise ValueError('delta must be >= 0, not %r' % (delta,))
    if getattr(model, '_dp', None) is not None:
        raise NotImplementedError('perturbation_effect under data parallelism is not built: summarise on one rank')
    if chunk_rows is not None and (int(chunk_rows) != chunk_rows or int(chunk_rows) < 1):
        raise ValueError('chunk_rows must be a positive integer or None, not %r' % (chunk_rows,))
    x1 = ds.x1
    N, X = int(x1.shape[0]), int(x1.shape[1])
    if not ((torch.is_tensor(x1) or isinstance(x1, CsrRows)) and x1.is_cuda):
        raise ValueError('perturbation_effect summarises a DEVICE-resident set (ds.to(device)); this one lives on the host')
    dev = x1.device
    if groups is None:
        G, grp = 1 if n_groups is None else int(n_groups), None
    else:
        if n_groups is None:
            raise ValueError('groups= needs n_groups=: the number of groups is not read back from the device')
        G = int(n_groups)
        groups = torch.as_tensor(groups)
        if groups.dim() != 1 or groups.numel() != N or groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise ValueError('groups must be an integer tensor of shape (%d,)' % N)
        groups = groups.to(dev)
        if N and bool((groups >= G).any()):       # (the one host synchronisation, in front of the passes)
            raise ValueError('groups holds a value >= n_groups=%d (a negative value leaves a row out)' % G)
        grp = groups.clamp_min(-1).to(torch.int32).contiguous()
    if not 1 <= G <= 65535:
        raise ValueError('n_groups must be in 1 .. 65535, not %r' % (n_groups,))
    model.eval()
    C_ = max(N, 1) if chunk_rows is None else min(int(chunk_rows), max(N, 1))
    dense = torch.empty(C_, X, device=dev) if isinstance(x1, CsrRows) else None
    ev = CS.event_words(event, dev)
    seed = CS.default_seed(model.random_seed) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    acc = torch.zeros(G, N_STATS, X, dtype=torch.float64, device=dev)
    parts = {}        # row blocks -> the launch's partials (a full chunk and the tail chunk: at most two)
    for c0 in range(0, N, C_):
        c1 = min(c0 + C_, N)
        if dense is not None:       # sparse rows: one chunk at a time through the feed launch, never the whole matrix
            rows = x1.gather_rows(dense[:c1 - c0], torch.arange(c0, c1, dtype=torch.int32, device=dev))
        else:
            rows = x1[c0:c1].to(torch.float32)
        rb = row_blocks_for(c1 - c0, X, G)
        if rb not in parts:
            parts[rb] = torch.empty(rb, G, N_STATS, X, dtype=torch.float64, device=dev)
        base = None
        for k, which, z, px in CS.head_passes(model, rows, ds.s[c0:c1], n_samples=S, latent=latent, seed=seed, ev=ev, row0=c0):
            if which == 1:
                base = px[0]
                continue
            effect_cols(parts[rb], base, px[0], grp=None if grp is None else grp[c0:c1], n_groups=G, mode=mode, delta=delta,
                        pseudocount=pseudocount)
            fold(acc, parts[rb])
    return summarize(acc)
