"""The count rows with an inverse dispersion PER (NUISANCE CLASS, GENE) (``dispersion='gene-batch'``): the launcher of the count
kinds of ``dv_gauss_nll_rows_raw_cs`` with the class operands, the rule that picks its row blocks and the shape helper.

theta is an ``(S, X)`` pre-activation table, ``theta[k, g] = softplus(raw[k, g]) + 1e-3``; a row of class k reads row k.  The
class is the launch's third grid dimension: a workgroup owns one gene chunk, one row block and one class, and skips its
block's rows of other classes.  The gradient of the table is ONE column sum -- ``ws`` holds a segment of X columns per
class, ``kernels.colsum(grad.view(-1), ws[:, :S * X])``.  Like ``drvae_amd.gene_rows`` there is no CPU path here (the CPU
stand-in of these functions is ``tests/gene_batch_ref.py``).
"""
import ctypes as C

from . import _lib
from .gene_rows import _KIND, CHUNK, MIN_ROWS, TARGET_WORKGROUPS
from .kernels import _f32, _i32, _ld, _stream


# the row-block rule.  The launch has S workgroups per (chunk, block), so the 'gene' rule's workgroup target is shared among the
# classes: ceil(TARGET_WORKGROUPS / (chunks S)) blocks.  The rows a workgroup TAKES are its class's share of the block -- a S-th
# of it with balanced classes, nearly all of it for the majority class of an uneven mix -- and its time is linear in them, so
# the least rows a block do NOT grow with S: the first form of this rule (at least MIN_ROWS S rows a block) gave 16 rows a block
# at 900 x 978 with 8 classes, 66 us balanced and 151 us at 90/10 against 59 and 48 us at 4 rows.  Twice MIN_ROWS from two classes
# on is fastest or within 4 % of it at 2 and 8 classes, balanced and 90/10 (profiles/r29_gene_batch.md)
MIN_ROWS_CLASSES = 2 * MIN_ROWS


def row_blocks_for(M, X, S):
    """the number of row blocks the host asks for at M rows of X genes in S classes: ceil(TARGET_WORKGROUPS / (chunks S))
    blocks, at least MIN_ROWS rows each with one class (the rule of ``gene_rows.row_blocks_for``) and MIN_ROWS_CLASSES with
    more, within [1, M]"""
    chunks = -(-X // CHUNK)
    S = max(int(S), 1)
    least = MIN_ROWS if S == 1 else MIN_ROWS_CLASSES
    return max(1, min(-(-TARGET_WORKGROUPS // (chunks * S)), -(-M // least), M))


def shape(M, X, S, row_blocks=None):
    """(chunks, row_blocks) of ``gene_batch_rows`` for M rows of X genes in S classes: ``out_part`` is (M, chunks), ``ws``
    (row_blocks, >= S X)"""
    return -(-X // CHUNK), row_blocks_for(M, X, S) if row_blocks is None else int(row_blocks)


def gene_batch_rows(out_part, x, mu, theta_raw, cls, *, kind, cls_src=None, shift=0.0, logit=None, xidx=None, coef=None,
                    dmu=None, dlogit=None, ws=None, library=False, size=None, row_blocks=None):
    """``gene_rows.gene_rows`` with a theta per (class, gene): ``theta_raw`` the (S, X) pre-activation table, ``cls`` int32
    class values, ``cls_src`` (M int32, optional) the entry of ``cls`` a row reads -- the class of row r is
    ``cls[cls_src[r]]``, without ``cls_src`` ``cls[r]``.  ``ws`` (row_blocks, >= S X): per-block sums of coef[r] * d/d raw_theta
    over the block's rows of class k in its columns [k X, (k + 1) X).  Everything else as ``gene_rows``.  A class outside
    [0, S) is the caller's error (no row of it is written)."""
    if (kind, bool(library)) not in _KIND:
        raise ValueError("gene_batch_rows: kind is 'nb' or 'zinb', not %r" % (kind,))
    M, X = mu.shape
    assert theta_raw.dim() == 2 and theta_raw.shape[1] == X and theta_raw.stride(1) == 1
    S = theta_raw.shape[0]
    grad = dmu is not None
    if row_blocks is None:
        row_blocks = ws.shape[0] if grad else None
    chunks, rbs = shape(M, X, S, row_blocks)
    assert tuple(out_part.shape) == (M, chunks) and out_part.is_contiguous()
    assert cls.is_contiguous() and (cls_src.numel() >= M and cls_src.is_contiguous() if cls_src is not None
                                    else cls.numel() >= M)
    assert logit is None or _ld(logit) == _ld(mu)
    assert size is None or (size.numel() >= M and size.is_contiguous())
    if grad:
        assert ws is not None and ws.dim() == 2 and ws.shape[0] == rbs and ws.shape[1] >= S * X
        assert dlogit is None or _ld(dlogit) == _ld(dmu)
    d = _lib.NllRawCs(coef=_f32(coef), x=_f32(x), ldx=_ld(x), xidx=_i32(xidx), mu=_f32(mu), sd=_f32(logit), ldp=_ld(mu), M=M,
                      X=X, shift=shift, out_part=_f32(out_part), chunks=chunks, dmu=_f32(dmu), dsd=_f32(dlogit),
                      ldd=_ld(dmu), ws=_f32(ws), ldw=_ld(ws), row_blocks=rbs,
                      kind=_lib.REC_KIND[_KIND[kind, bool(library)]], theta_raw=_f32(theta_raw), size=_f32(size),
                      n_cls=S, cls=_i32(cls), cls_src=_i32(cls_src), ldth=_ld(theta_raw))
    _lib.check(_lib.load().dv_gauss_nll_rows_raw_cs(C.byref(d), _stream()), 'dv_gauss_nll_rows_raw_cs (theta per class)')
