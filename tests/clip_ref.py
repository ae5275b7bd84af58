"""Global-norm gradient clipping of the fused step (the norm pass, ``dv_grad_norm_clip``; drvae_amd/csrc/optim.hip) below
model level: the float64 reference of the clip record, its bound, the value classes of the device test and two faulty
emulations the CPU file (tests/test_clip_cpu.py) proves the checks against.  tests/test_gpu_clip.py holds the device to the
same reference.  Plain numpy on the host: no device, no library.

The semantics (include/drvae_hip.h).  For the fp32 elements g_i of a contiguous range and the host scale gscale:

    sumsq = sum_i g_i^2      norm = |gscale| sqrt(sumsq)      coef = min(1, max_norm / (norm + 1e-6))
    skip  = sumsq is not finite  (some g_i is inf or NaN: finite fp32 inputs cannot overflow a double sum; then coef = 0)

sumsq is accumulated in double from the square on, every element widened first; norm and coef are evaluated in double and
stored as fp32.

The bound (derived, not chosen).  The square of a widened fp32 element has 48 significant bits: exact in double.  The terms
are non-negative, so ANY order of double additions of n of them is within (n - 1) u64 of the exact sum, relatively (u64 =
2^-53; no cancellation, the classical bound of recursive summation holds with the sum itself on the right-hand side).  With
n <= 2^25 that is 2^-28 = U / 16 (U = 2^-24).  The square root halves a relative error and adds one double rounding, the
product with |gscale| another; the store rounds to fp32 once: U.  Together U (1 + 1/32) + 2 u64 for the kernel, the same
without the final U for this reference (numpy's pairwise double sum) -- below 2 U.  coef is computed from the DOUBLE norm:
x -> max_norm / (x + 1e-6) has relative sensitivity x / (x + 1e-6) <= 1 and min(1, .) moves nothing further, so coef carries
the double stage's U / 32, a division's and an addition's double rounding, and its own fp32 store: below 2 U as well.  Both
are multiplied by SLACK = 1.01 for the second-order terms, as in tests/optim_ref.py, and ETA = 2^-149 is added for a result
among the fp32 subnormals.  A kernel that accumulates in fp32, in whatever order, is outside this bound from a few thousand
elements on (``sumsq_fp32`` below, measured in tests/test_clip_cpu.py); that is the point of the bound.
"""
import math

import numpy as np

from tests.optim_ref import ETA, SLACK, U

F32 = np.float32
GUARD = 64
SIZES = (1, 3, 4, 5, 255, 256, 257, 4099, (1 << 20) + 3, (16 << 20) + 5)      # the last: the streaming path
CLASSES = ('normal', 'one_huge', 'zeros', 'spread')
N_MAX = 1 << 25                 # the bound's derivation holds up to here


def values(cls, n, seed=0):
    """the four value classes, as fp32"""
    rs = np.random.RandomState(seed + n % 1000)
    if cls == 'normal':
        return rs.standard_normal(n).astype(F32)
    if cls == 'one_huge':       # squares of 1e36 and 1e-36: both ends of the fp32 range, 72 decades apart
        g = np.full(n, 1e-18, F32)
        g[n // 2] = F32(1e18)
        return g
    if cls == 'zeros':
        return np.zeros(n, F32)
    if cls == 'spread':         # magnitudes 2^-60 .. 2^60, random signs
        e = rs.uniform(-60.0, 60.0, n)
        return (np.exp2(e) * rs.choice([-1.0, 1.0], n)).astype(F32)
    raise ValueError(cls)


def sumsq64(*arrays):
    """sum of squares of fp32 arrays in float64 (pairwise: log2(n) u64, far inside the bound)"""
    s = 0.0
    for a in arrays:
        a = np.asarray(a)
        assert a.dtype == F32
        d = a.reshape(-1).astype(np.float64)
        with np.errstate(over='ignore', invalid='ignore'):
            s = s + float(np.sum(d * d))
    return s


def record(sumsq, gscale, max_norm):
    """dict(norm, coef, skip) in float64 from a float64 sum of squares"""
    skip = not math.isfinite(sumsq)
    norm = abs(float(F32(gscale))) * math.sqrt(sumsq) if not (skip and sumsq != sumsq) else float('nan')
    if skip:
        return dict(norm=norm, coef=0.0, skip=1)
    return dict(norm=norm, coef=min(1.0, float(max_norm) / (norm + 1e-6)), skip=0)


def ref(arrays, gscale=1.0, max_norm=float('inf')):
    if isinstance(arrays, np.ndarray):
        arrays = [arrays]
    n = sum(int(np.asarray(a).size) for a in arrays)
    assert n <= N_MAX
    return record(sumsq64(*arrays), gscale, max_norm)


def bound(x):
    """what an fp32 ``norm`` or ``coef`` may differ from its float64 reference ``x`` by"""
    return SLACK * 2.0 * U * abs(x) + ETA


def check(got, want, what=''):
    """assert the kernel's {norm, coef, skip} (python numbers) against the reference's; returns the worst error / bound"""
    assert int(got['skip']) == int(want['skip']), (what, got, want)
    if want['skip']:
        assert not math.isfinite(got['norm']) and got['coef'] == 0.0, (what, got)
        return 0.0
    worst = 0.0
    for k in ('norm', 'coef'):
        err, b = abs(float(got[k]) - want[k]), bound(want[k])
        assert err <= b, (what, k, got[k], want[k], err, b)
        worst = max(worst, err / b)
    assert 0.0 <= got['coef'] <= 1.0
    return worst


# ---------------------------------------------------------------------------------------------- faulty emulations
def sumsq_fp32(a):
    """FAULTY: squares and running sum in fp32, in index order"""
    a = np.asarray(a, F32).reshape(-1)
    return float(np.cumsum(a * a, dtype=F32)[-1])


def record_no_eps(sumsq, gscale, max_norm):
    """FAULTY: coef = min(1, max_norm / norm), without the 1e-6"""
    r = record(sumsq, gscale, max_norm)
    if not r['skip']:
        r['coef'] = min(1.0, float(max_norm) / r['norm']) if r['norm'] > 0 else 1.0
    return r


def as_f32(r):
    """a float64 record as the device would store it (fp32 norm and coef)"""
    return dict(norm=float(F32(r['norm'])), coef=float(F32(r['coef'])), skip=r['skip'])
