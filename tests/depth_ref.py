"""Float64 reference of the depth-normalised encoder feed (``x_transform='log1p_norm'``: ``dv_batch_feed`` with ``xt`` and
``transform`` == 3), the bound it is held to, fp32 emulations -- a careful one and five faulty ones the bound catches -- and
a model-level float64 reference of one step (the feed's CPU stand-in: ``tests/kernel_ref.py``).  Test-only; builds on
``tests/counts_ref.py``.

The feed.  ``xt`` is the source row, bit for bit.  The encoder's row is fmaf(sigma, eps, log1p(x / s)) with
s = max(sum_g x_g, 1) / X of that same source row.  For integer counts with a row total below 2^24 every partial sum is an
integer below 2^24, exact in fp32 in any order, so the kernel's s is ONE correctly rounded fp32 quotient whatever the path:
``counts_ref.size_factor32`` forms the same number on the host and the reference takes it as data,

    T64 = log1p(x / s32)        in float64.

The bound.  Behind s the kernel forms q = fl(x / s): K_DIV roundings (1 for a true division -- what the kernel does --, 2 for
a reciprocal and a product), in front of what ``counts_ref`` counts for the 'log1p' feed (C_ENC = 4: log1p 3, the fused
product-sum 1).  A relative perturbation d of q moves log1p(q) by

    q / (1 + q) * d  <=  log1p(q) * d        (log1p(q) >= q / (1 + q) for q >= 0: equal at 0, derivative 1/(1+q) >= 1/(1+q)^2),

so each rounding of q costs at most one U of |T64| itself: C = C_ENC + K_DIV on the components |T64| + |sigma eps|."""
import contextlib

import numpy as np
import torch

from tests import counts_ref as CR
from tests import ref64
from tests.ref64 import bound, f64

K_DIV = 1                           # the kernel divides (v_div_*: correctly rounded); a reciprocal and a product would be 2
C_NORM = CR.C_ENC + K_DIV


# ---------------------------------------------------------------------------------------------------- the feed
def feed_reference(src, noise=None, sigma=0.0):
    """``src``: the gathered source rows (fp32, integer counts, totals < 2^24).  Returns (xt, xin64, xin_bound): the targets (the
    rows themselves), the encoder's rows in float64 and their bound"""
    x = f64(src)
    s = f64(CR.size_factor32(src))[:, None]
    t = torch.log1p(x / s)
    e = f64(ref64.f32(sigma)) * f64(noise) if noise is not None else torch.zeros_like(x)
    return src.clone(), t + e, bound(C_NORM, t.abs() + e.abs())


FAULTS = ('log_1_plus_q', 'no_guard', 'noisy_sum', 'x1_total', 'targets_too')


def emulate_fp32(src, noise=None, sigma=0.0, fault=None, other=None):
    """the feed in numpy float32, operation by operation: (xt, xin).  Careful (``fault=None``) = the kernel's construction:
    s = fl(max(tot, 1) / X) from the exact total of the source row, q = fl(x / s), fl(log1p(q)), one fused product-sum.
    FAULTY on purpose: ``'log_1_plus_q'`` (logf(1 + q): 1 + q rounds the small quotients away); ``'no_guard'`` (s = tot / X
    without max(., 1): an all-zero row divides 0 by 0); ``'noisy_sum'`` (s from the row AFTER the noise); ``'x1_total'`` (every
    row normalised by the total of the same row of ``other``, as if the pairs' x2 rows took x1's); ``'targets_too'`` (the
    normalised row written to the targets as well)"""
    f = np.float32
    x = np.asarray(src, f)
    X = x.shape[1]
    e = (f(sigma) * np.asarray(noise, f)).astype(f) if noise is not None else np.zeros_like(x)
    summed = (x + e).astype(f) if fault == 'noisy_sum' else (np.asarray(other, f) if fault == 'x1_total' else x)
    tot = summed.astype(np.float64).sum(1).astype(f)
    with np.errstate(all='ignore'):
        s = ((tot if fault == 'no_guard' else np.maximum(tot, f(1))) / f(X)).astype(f)
        q = (x / s[:, None]).astype(f)
        t = np.log(f(1) + q).astype(f) if fault == 'log_1_plus_q' else np.log1p(q).astype(f)
        xin = t if noise is None else (f64(f(sigma)).numpy() * np.asarray(noise, np.float64) + t.astype(np.float64)).astype(f)
    assert xin.dtype == f and q.dtype == f and s.dtype == f
    return (q if fault == 'targets_too' else x), xin


def edge_rows(X=16):
    """the edge grid of the feed, one case per row (integer counts, totals < 2^24): all zero; a single 1; total exactly X
    (s = 1); one count of 1 in a total near 1e7 (q ~ 1e-6 X); total 2^24 - 1; counts up to 30000"""
    assert X >= 8
    x = np.zeros((6, X), np.float32)
    x[1, 3] = 1.0
    x[2] = 1.0
    x[2, 0], x[2, 1] = 0.0, 2.0                     # (total still X, not every entry alike)
    x[3, 0], x[3, 1:5] = 1.0, 2500000.0             # total 1e7 + 1
    x[4, :] = np.float32((2 ** 24 - 1) // X)
    x[4, 0] += np.float32((2 ** 24 - 1) % X)
    x[5] = np.random.RandomState(X).randint(0, 30001, X).astype(np.float32)
    x[5, 2], x[5, 5] = 30000.0, 0.0
    tot = x.astype(np.float64).sum(1)
    assert tot[2] == X and tot[3] == 1e7 + 1 and tot[4] == 2 ** 24 - 1 and tot.max() < 2 ** 24
    return x


# ------------------------------------------------------------------------------- model-level float64 reference
@contextlib.contextmanager
def normalised_encoder():
    """inside ``counts_ref.oracle_as_counts(spec, x_transform=None, ...)``: the encoder's first input becomes log1p(x / s) of the
    raw rows it is handed, s = max(sum, 1) / X of the same row in float64 -- IN FRONT of ``counts_ref``'s substitution, which
    (without a transform of its own) adds sigma * eps to what it receives: T(x) + sigma * eps, the noise never in the sum"""
    from oracle import blocks_ref as B
    inner = B.diag_gaussian

    def diag_gaussian(inputs, p, prefix, *a, **k):
        if prefix == 'encoder_z1':
            x = inputs[0]
            inputs = [torch.log1p(x / CR.size_factor64(x)[:, None])] + list(inputs[1:])
        return inner(inputs, p, prefix, *a, **k)
    B.diag_gaussian = diag_gaussian
    try:
        yield
    finally:
        B.diag_gaussian = inner


class ModelRef(CR.RidersRef):
    """``counts_ref.RidersRef`` (the negative-binomial model with ``library_size`` and the step's riders, all off by default)
    whose encoder reads the depth-normalised rows: every call inside ``normalised_encoder`` inside ``counts_ref``'s context"""

    def __init__(self, spec, seed=9, library_size=False, **riders):
        super().__init__(spec, seed, None, library_size, **riders)

    @contextlib.contextmanager
    def context(self):
        with super().context():
            with normalised_encoder():
                yield
