"""The count rows with a GENE-WISE inverse dispersion (``dispersion='gene'``): the launcher of the count kinds of
``dv_gauss_nll_rows_raw_cs``, the rule that picks its row blocks and the shape helper.

theta is one ``(X,)`` pre-activation vector shared by all rows (``theta_g = softplus(raw_g) + 1e-3``), not a decoder head: the
pass reads it from the vector, and the gradient of the vector is a column sum -- per-row-block partials ``ws`` from the launch,
summed over the blocks by ``kernels.colsum``.  Like ``drvae_amd.kernels`` there is no CPU path here (the CPU stand-in of these
functions is ``tests/gene_disp_ref.py``).
"""
import ctypes as C

from . import _lib
from .kernels import _f32, _i32, _ld, _stream

CHUNK = 1024            # genes per workgroup (256 threads x 4 genes)
# the row-block rule.  A workgroup's time is linear in its rows (a row is four dependent term evaluations per thread: ~12 us
# a row at one wave per SIMD), so the launch wants MANY workgroups -- the chip holds 256 CUs x 4 to 6 of them, and 8192 keeps
# its tail short -- but never fewer than MIN_ROWS rows per block: a block forms its thetas once (in double) and writes one row
# of ``ws``, both paid per block.  Measured (profiles/r28_gene_dispersion.md): 900 x 978 is fastest at 2 rows a block, 2048 x
# 20000 at 4 to 8; the first form of this rule (2048 workgroups, 4 rows) gave 4 and 20
TARGET_WORKGROUPS = 8192
MIN_ROWS = 2

_KIND = {('nb', False): 'nb', ('nb', True): 'nb_lib', ('zinb', False): 'zinb', ('zinb', True): 'zinb_lib'}


def row_blocks_for(M, X):
    """the number of row blocks the host asks for at M rows of X genes: ceil(TARGET_WORKGROUPS / chunks) blocks, at least
    MIN_ROWS rows each, within [1, M]"""
    chunks = -(-X // CHUNK)
    return max(1, min(-(-TARGET_WORKGROUPS // chunks), -(-M // MIN_ROWS), M))


def shape(M, X, row_blocks=None):
    """(chunks, row_blocks) of ``gene_rows`` for M rows of X genes: ``out_part`` is (M, chunks), ``ws`` (row_blocks, >= X)"""
    return -(-X // CHUNK), row_blocks_for(M, X) if row_blocks is None else int(row_blocks)


def gene_rows(out_part, x, mu, theta_raw, *, kind, shift=0.0, logit=None, xidx=None, coef=None, dmu=None, dlogit=None,
              ws=None, library=False, size=None, row_blocks=None):
    """row partials of the 'nb' / 'zinb' log-likelihood with a gene-wise theta, and with ``coef`` the gradients: ``mu`` the
    FINISHED mean head (M, X), ``theta_raw`` the (X,) pre-activation vector, ``logit`` the RAW dropout logit ('zinb' only), ``x``
    the targets (rows ``xidx``).  ``out_part`` (M, chunks); ``dmu`` / ``dlogit`` = coef[r] * d/da_m, d/da_d; ``ws`` (row_blocks,
    >= X): per-block sums of coef[r] * d/d raw_theta -- ``kernels.colsum(grad, ws[:, :X])`` is the vector's gradient.
    ``library``: the mean of row r is s * mu with the size factor of its target row; ``size`` (M floats) is scratch the pass
    needs with more than one chunk (and fills either way when given).  ``row_blocks``: ``ws.shape[0]`` with gradients, else
    the rule's.  ``coef = dmu = dlogit = ws = None``: forward only."""
    if (kind, bool(library)) not in _KIND:
        raise ValueError("gene_rows: kind is 'nb' or 'zinb', not %r" % (kind,))
    M, X = mu.shape
    grad = dmu is not None
    if row_blocks is None:
        row_blocks = ws.shape[0] if grad else None
    chunks, rbs = shape(M, X, row_blocks)
    assert tuple(out_part.shape) == (M, chunks) and out_part.is_contiguous()
    assert theta_raw.numel() == X and theta_raw.is_contiguous()
    assert logit is None or _ld(logit) == _ld(mu)
    assert size is None or (size.numel() >= M and size.is_contiguous())
    if grad:
        assert ws is not None and ws.dim() == 2 and ws.shape[0] == rbs
        assert dlogit is None or _ld(dlogit) == _ld(dmu)
    d = _lib.NllRawCs(coef=_f32(coef), x=_f32(x), ldx=_ld(x), xidx=_i32(xidx), mu=_f32(mu), sd=_f32(logit), ldp=_ld(mu), M=M,
                      X=X, shift=shift, out_part=_f32(out_part), chunks=chunks, dmu=_f32(dmu), dsd=_f32(dlogit),
                      ldd=_ld(dmu), ws=_f32(ws), ldw=_ld(ws), row_blocks=rbs,
                      kind=_lib.REC_KIND[_KIND[kind, bool(library)]], theta_raw=_f32(theta_raw), size=_f32(size))
    _lib.check(_lib.load().dv_gauss_nll_rows_raw_cs(C.byref(d), _stream()), 'dv_gauss_nll_rows_raw_cs (gene-wise theta)')
