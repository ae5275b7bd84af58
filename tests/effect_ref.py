"""The EFFECT REDUCTION of include/drvae_hip.h in float64, with a bound per output element, and an fp32 emulation of the launch
with switchable faults (tests/test_effect_cpu.py holds the emulation to the bounds and shows that each fault leaves them;
tests/test_gpu_effect.py holds the kernel and the model-level interface to the same bounds).

THE BOUND PER ELEMENT, B_e >= |e_device - e_ref|, by counting roundings (u = 2^-24, the unit roundoff of fp32):

  mode 1 (e = b - a): ONE rounding, and the reference performs it: the float64 difference of two fp32 numbers is exact when
  their magnitudes lie within 2^28 of each other (or one is zero), so e_ref = fp32(b - a) IS the device's value and B_e = 0.
  Otherwise B_e = u |e|.
  mode 0 (e = log2f(b + c) - log2f(a + c)), e_ref = log2(b + c) - log2(a + c) in float64 from the fp32 operands:
    * the add of c (absent at c == 0): fl(a + c) = (a + c)(1 + d), |d| <= u, moves the logarithm by |log2(1 + d)| <= ADD = u (1 + u)
      / ln 2, per side;
    * log2f: within one ulp of its result, as the device library documents it.  An ulp of L is at most 2 u |L|; a result near
      zero (an argument near 1) is allowed the ulp of 1: LOG(L) = 2 u max(|L|, 1), per side;
    * the subtraction rounds the difference of the two COMPUTED logarithms: u (|e| + D) with D the sum of the four terms above.
  B_e = D + u (|e| + D), D = 2 ADD [c != 0] + LOG(log2(a + c)) + LOG(log2(b + c)).
An element is valid when e is finite; the inputs of the tests keep validity itself out of rounding's reach (no subnormal heads,
no sum that overflows).

THE BOUNDS PER STATISTIC over the set T of valid elements a (row block, group, gene) owns, N = |T| (ACC = 2 N 2^-53: the device
and this reference each add N float64 terms in an order of their own, first-order bound N 2^-53 sum |term| each):
    n          exact
    sum e      sum B_e + ACC sum |e|
    sum e^2    sum B_e (2 |e| + B_e) + ACC sum e^2        (the device squares the fp32 e exactly, in double)
    sum a, b   ACC sum |a|, ACC sum |b|                   (fp32 values added in double)
    n_up       in [sure, sure + undecided]: sure = #{e - B_e > delta}, undecided = #{e + B_e > delta} - sure; n_down likewise with
               -e.  With B_e = 0 nothing is undecided and the comparison is strict, as the launch's is.
"""
import functools

import numpy as np

U = 2.0 ** -24
ADD = U * (1 + U) / np.log(2.0)
STATS = ('n', 'sum_e', 'sum_e2', 'n_up', 'n_down', 'sum_a', 'sum_b')
UNDECIDED_CAP = 0.01


def elements(a, b, mode, c):
    """-> (e, B_e, valid) float64 / bool arrays from the fp32 operands"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        if mode == 1:
            lo, hi = np.minimum(np.abs(a), np.abs(b)), np.maximum(np.abs(a), np.abs(b))
            exact = (lo == 0) | (hi < lo * 2.0 ** 28)
            d = b - a
            e = np.where(exact, d.astype(np.float32).astype(np.float64), d)
            B = np.where(exact, 0.0, U * np.abs(d))
        else:
            c = float(np.float32(c))
            la, lb = np.log2(a + c), np.log2(b + c)
            e = lb - la
            log_ = lambda L: 2 * U * np.maximum(np.abs(L), 1.0)
            D = (2 * ADD if c != 0 else 0.0) + log_(la) + log_(lb)
            B = D + U * (np.abs(e) + D)
    valid = np.isfinite(e)
    return np.where(valid, e, 0.0), np.where(valid, B, 0.0), valid


def blocks_of(M, row_blocks):
    R = -(-M // row_blocks) if M else 0
    return [(min(q * R, M), min((q + 1) * R, M)) for q in range(row_blocks)]


def reference(a, b, *, mode, c=0.0, delta, grp=None, G=1, row_blocks=1):
    """-> dict: value, bound (row_blocks, G, 7, X) float64 -- for the two counts ``value`` is the SURE count and ``bound`` the
    number of undecided elements; ``elements`` / ``undecided``: totals over everything counted"""
    e, B, valid = elements(a, b, mode, c)
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    M, X = e.shape
    g = np.zeros(M, np.int64) if grp is None else np.asarray(grp, np.int64)
    val, bnd = np.zeros((row_blocks, G, 7, X)), np.zeros((row_blocks, G, 7, X))
    sure_up, may_up = (e - B > delta) & valid, (e + B > delta) & valid
    sure_dn, may_dn = (-e - B > delta) & valid, (-e + B > delta) & valid
    n_el = n_und = 0
    for q, (r0, r1) in enumerate(blocks_of(M, row_blocks)):
        for k in range(G):
            rows = np.arange(r0, r1)[g[r0:r1] == k]
            if rows.size == 0:
                continue
            v = valid[rows]
            N = v.sum(0).astype(np.float64)
            acc = 2 * N * 2.0 ** -53
            ee, BB = e[rows], B[rows]
            aa, bb = np.where(v, a64[rows], 0.0), np.where(v, b64[rows], 0.0)
            val[q, k, 0] = N
            val[q, k, 1], bnd[q, k, 1] = ee.sum(0), BB.sum(0) + acc * np.abs(ee).sum(0)
            val[q, k, 2], bnd[q, k, 2] = (ee * ee).sum(0), (BB * (2 * np.abs(ee) + BB)).sum(0) + acc * (ee * ee).sum(0)
            val[q, k, 3], bnd[q, k, 3] = sure_up[rows].sum(0), (may_up[rows] & ~sure_up[rows]).sum(0)
            val[q, k, 4], bnd[q, k, 4] = sure_dn[rows].sum(0), (may_dn[rows] & ~sure_dn[rows]).sum(0)
            val[q, k, 5], bnd[q, k, 5] = aa.sum(0), acc * np.abs(aa).sum(0)
            val[q, k, 6], bnd[q, k, 6] = bb.sum(0), acc * np.abs(bb).sum(0)
            n_el += int(N.sum())
            n_und += int(bnd[q, k, 3].sum() + bnd[q, k, 4].sum())
    return dict(value=val, bound=bnd, elements=n_el, undecided=n_und)


def fold_blocks(ref):
    """the reference of a launch, its row blocks added up: (G, 7, X) value and bound (bounds and undecided counts add)"""
    return dict(value=ref['value'].sum(0), bound=ref['bound'].sum(0), elements=ref['elements'], undecided=ref['undecided'])


def excess(got, ref):
    """how far ``got`` lies outside the reference: -> (worst |got - value| / bound over the five sums and n -- inf where a bound
    of zero is missed --, the number of count elements outside [sure, sure + undecided])"""
    got = np.asarray(got, np.float64)
    val, bnd = ref['value'], ref['bound']
    assert got.shape == val.shape, (got.shape, val.shape)
    sums = [0, 1, 2, 5, 6]
    err = np.abs(got[..., sums, :] - val[..., sums, :])
    with np.errstate(all='ignore'):
        ratio = np.where(err == 0, 0.0, err / bnd[..., sums, :])       # (x / 0 = inf: a bound of zero that is missed)
    ratio = np.where(np.isnan(got[..., sums, :]), np.inf, ratio)
    cnt = got[..., [3, 4], :]
    lo = val[..., [3, 4], :]
    bad = (cnt < lo) | (cnt > lo + bnd[..., [3, 4], :]) | (cnt != np.rint(cnt))
    return float(ratio.max()) if ratio.size else 0.0, int(bad.sum())


def hold(got, ref, what):
    worst, bad = excess(got, ref)
    print('%s: worst sum error %.3g of its bound, %d counts outside their interval, %d of %d elements undecided' % (
        what, worst, bad, ref['undecided'], 2 * ref['elements']))
    assert worst <= 1.0 and bad == 0, what


# ------------------------------------------------------------------------------------------- the fp32 emulation
FAULTS = ('ge', 'c_one_side', 'ln', 'seam_group', 'short_block_dropped', 'invalid_counted', 'left_out_counted')


def emulate(a, b, *, mode, c=0.0, delta, grp=None, G=1, row_blocks=1, fault=None):
    """the launch in numpy: fp32 elements, float64 sums (in numpy's order, not the launch's) -> (row_blocks, G, 7, X)"""
    assert fault is None or fault in FAULTS
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    c32, d32 = np.float32(c), np.float32(delta)
    M, X = a.shape
    with np.errstate(all='ignore'):
        if mode == 1:
            e = b - a
        else:
            log = np.log if fault == 'ln' else np.log2
            e = log(b + c32) - log(a + (np.float32(0) if fault == 'c_one_side' else c32))
    assert e.dtype == np.float32
    valid = np.isfinite(e)
    g = np.zeros(M, np.int64) if grp is None else np.asarray(grp, np.int64).copy()
    if fault == 'left_out_counted':
        g = np.clip(g, 0, G - 1)
    blocks = blocks_of(M, row_blocks)
    if fault == 'seam_group':
        for r0, r1 in blocks[1:]:
            if r0 < r1:
                g[r0] = g[r0 - 1]
    out = np.zeros((row_blocks, G, 7, X))
    for q, (r0, r1) in enumerate(blocks):
        if fault == 'short_block_dropped' and r1 - r0 < blocks[0][1] - blocks[0][0]:
            continue
        for k in range(G):
            rows = np.arange(r0, r1)[g[r0:r1] == k]
            v = valid[rows]
            ee = np.where(v, e[rows], np.float32(0)).astype(np.float64)
            out[q, k, 0] = (np.ones_like(v) if fault == 'invalid_counted' else v).sum(0)
            out[q, k, 1] = ee.sum(0)
            out[q, k, 2] = (ee * ee).sum(0)
            with np.errstate(invalid='ignore'):
                out[q, k, 3] = (v & ((e[rows] >= d32) if fault == 'ge' else (e[rows] > d32))).sum(0)
                out[q, k, 4] = (v & ((e[rows] <= -d32) if fault == 'ge' else (e[rows] < -d32))).sum(0)
            out[q, k, 5] = np.where(v, a[rows], np.float32(0)).astype(np.float64).sum(0)
            out[q, k, 6] = np.where(v, b[rows], np.float32(0)).astype(np.float64).sum(0)
    return out


# ------------------------------------------------------------------------------------------- the grid
XS = (1, 3, 4, 255, 256, 1020, 1024, 1025, 1028, 2052)
MS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 67)
LAYOUTS = ('none', 'one_class', 'alternating', 'empty_class', 'negative', 'too_big')
VIEWS = ('contiguous', 'columns', 'odd_offset')


def groups_of(layout, M, rs):
    """-> (G, grp or None)"""
    r = np.arange(M)
    if layout == 'none':
        return 1, None
    if layout == 'one_class':
        return 3, np.full(M, 1, np.int32)
    if layout == 'alternating':
        return 2, (r % 2).astype(np.int32)
    if layout == 'empty_class':
        return 3, (2 * (r % 2)).astype(np.int32)
    if layout == 'negative':
        return 2, np.where(r % 3 == 1, np.where(r % 2 == 0, -1, -5), r % 2).astype(np.int32)
    if layout == 'too_big':
        return 2, np.where(r % 3 == 2, np.where(r % 2 == 0, 2, 9), r % 2).astype(np.int32)
    raise ValueError(layout)


def row_block_choices(M):
    """1, 2, 3 and one past M / 2 (blocks of two rows: the last is short or empty), each where M admits it"""
    return sorted({rb for rb in (1, 2, 3, M // 2 + 1) if rb <= max(M, 1)})


def heads(M, X, mode, rs, ties=False):
    """continuous random mean heads (fp32): positive with a log2 fold change of sd 0.7 (mode 0), standard normal (mode 1).
    ``ties``: mode 1 on a quarter grid, so that e hits +-delta exactly in many elements"""
    if ties:
        a = rs.randint(-8, 9, (M, X)) / 4.0
        return a.astype(np.float32), (a + rs.randint(-4, 5, (M, X)) / 4.0).astype(np.float32)
    if mode == 1:
        return rs.standard_normal((M, X)).astype(np.float32), rs.standard_normal((M, X)).astype(np.float32)
    a = np.exp(1.5 * rs.standard_normal((M, X)))
    return a.astype(np.float32), (a * 2.0 ** (0.7 * rs.standard_normal((M, X)))).astype(np.float32)


def _cases():
    out = []
    i = 0
    for xi, X in enumerate(XS):
        for t in range(4):          # four cases per gene count: every axis cycles at its own pace, so all values meet
            M = MS[(3 * xi + 5 * t + (t == 3) * 2) % len(MS)] if t else MS[(xi + 9) % len(MS)]
            rbs = row_block_choices(M)
            out.append(dict(i=i, X=X, M=M, row_blocks=rbs[(xi + t) % len(rbs)], layout=LAYOUTS[(xi + 2 * t) % len(LAYOUTS)],
                            view=VIEWS[(xi + t) % len(VIEWS)], mode=(xi + t) % 3 == 2, c=float((xi + t // 2) % 2),
                            delta=(0.25, 1.0)[(xi + t) % 2]))
            i += 1
    # the corners the cycling may miss: an empty last block (M 8 in 5 blocks of 2), M 67 past M / 2, the ties of mode 1
    out.append(dict(i=i, X=1028, M=8, row_blocks=5, layout='alternating', view='columns', mode=0, c=0.0, delta=0.25))
    out.append(dict(i=i + 1, X=255, M=67, row_blocks=34, layout='negative', view='odd_offset', mode=0, c=1.0, delta=1.0))
    out.append(dict(i=i + 2, X=1025, M=67, row_blocks=3, layout='too_big', view='contiguous', mode=1, c=0.0, delta=0.25, ties=True))
    out.append(dict(i=i + 3, X=256, M=9, row_blocks=2, layout='empty_class', view='contiguous', mode=1, c=0.0, delta=1.0, ties=True))
    for cs in out:
        cs['mode'] = int(cs['mode'])
        if cs['mode'] == 1:
            cs['c'] = 0.0
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def grid_case(i):
    """-> (case with its operands a, b, grp, G; its reference) -- computed once, shared by the tests, never modified"""
    cs = dict(CASES[i])
    rs = np.random.RandomState(1000 + i)
    cs['a'], cs['b'] = heads(cs['M'], cs['X'], cs['mode'], rs, ties=cs.get('ties', False))
    cs['G'], cs['grp'] = groups_of(cs['layout'], cs['M'], rs)
    for k in ('a', 'b', 'grp'):
        if cs[k] is not None:
            cs[k].setflags(write=False)
    ref = reference(cs['a'], cs['b'], mode=cs['mode'], c=cs['c'], delta=cs['delta'], grp=cs['grp'], G=cs['G'],
                    row_blocks=cs['row_blocks'])
    return cs, ref


def launch_kw(cs):
    return dict(mode=cs['mode'], c=cs['c'], delta=cs['delta'], grp=cs['grp'], G=cs['G'], row_blocks=cs['row_blocks'])


# ------------------------------------------------------------------------------------------- two folds of the same terms
def fold_bound(raw, terms, abs_a=None, abs_b=None):
    """(G, 7, X): how far two float64 summations of the same numbers (at most ``terms`` of them per output element) may lie
    apart, per statistic: each is within (terms - 1) 2^-53 sum |term| of the exact sum to first order, so the factor ``terms``
    2^-52 times sum |term| covers the pair.  sum |term| is the sum itself for e^2 and for the positive heads of a count decoder
    (``abs_a`` / ``abs_b``, (G, X): sum |a|, sum |b| where the heads have either sign); for e it is at most sqrt(n sum e^2)
    by Cauchy-Schwarz.  Counts: 0."""
    raw = np.asarray(raw, np.float64)
    b = np.zeros_like(raw)
    f = terms * 2.0 ** -52
    b[:, 1] = f * np.sqrt(raw[:, 0] * raw[:, 2])
    b[:, 2] = f * raw[:, 2]
    b[:, 5] = f * (np.abs(raw[:, 5]) if abs_a is None else abs_a)
    b[:, 6] = f * (np.abs(raw[:, 6]) if abs_b is None else abs_b)
    return b
