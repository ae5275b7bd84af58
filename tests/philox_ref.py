"""The train step's N(0,1) source as SPECIFIED, in numpy: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11) + Box-Muller, with the counter / key layout that ``include/drvae_hip.h`` states for
``dv_fill_normal`` and ``dv_fill_normal_rows``.  Written from the algorithm's definition and the header's words; it
shares nothing with ``drvae_amd/csrc/optim.hip``, so that the two can be compared (tests/test_gpu_philox.py) and so
that the CPU engine (tests/kernel_ref.py) draws the device's numbers.

Integer part: uint64 arithmetic on arrays (a 32 x 32 -> 64 bit product fits).  Uniform mapping: in float32, exactly
as specified, so the reference holds the very fp32 uniforms a conforming kernel holds.  Transform: float64.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (Weyl sequence: golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)
R_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -33)))      # |z| <= 6.7637...: the smallest uniform is 2^-33


def _u64(x):
    """integers (python ints of any sign up to 64 bits, arrays) -> uint64 array holding their low 32 bits"""
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & 0xFFFFFFFF, dtype=np.uint64)
    x = np.asarray(x)
    if x.dtype != np.uint64:
        x = x.astype(np.int64).astype(np.uint64)
    return x & MASK


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """four uint32 output words (as uint32 arrays, broadcast over the inputs) of Philox4x32 with ten rounds"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    m0, m1, w0, w1 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1)
    for _ in range(ROUNDS):
        p0, p1 = m0 * c0, m1 * c2                      # hi / lo halves of the two products
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & MASK, (p0 >> _32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def u01(x):
    """uint32 word -> uniform in (0, 1], in float32 exactly as specified: (float32(x) + 0.5f) * 2^-32.
    Never 0 (u01(0) = 2^-33); exactly 1.0f for x >= 2^32 - 128 (float32(x) rounds to 2^32 there)."""
    x = np.asarray(x, dtype=np.uint32)
    return (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def normals(words):
    """Box-Muller in float64 on the fp32 uniforms of four words: (z, r, a), each shaped words[0].shape + (4,):
    z = (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1), r0 = sqrt(-2 ln u(w0)), a0 = 2 pi u(w1), r1 / a1 from w2 / w3;
    r and a are repeated per element (the error bound of a comparison is stated in them)."""
    u = [u01(w).astype(np.float64) for w in words]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], -1)
    return z, np.stack([r0, r0, r1, r1], -1), np.stack([a0, a0, a1, a1], -1)


def _split(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & 0xFFFFFFFF, v >> 32


def row_draws(grow, width, draw, seed, event):
    """(z, r, a), each (len(grow), width) float64: the row-keyed draw ``draw`` (scalar or one id per row) of the global
    rows ``grow`` at draw event ``event``: element (row, col) = lane col % 4 of
    Philox(counter = (col // 4, global row, draw id, event_lo), key = (seed_lo, seed_hi ^ event_hi))."""
    grow = np.asarray(grow).reshape(-1, 1)
    draw = np.broadcast_to(np.asarray(draw).reshape(-1, 1), grow.shape)
    s_lo, s_hi = _split(seed)
    e_lo, e_hi = _split(event)
    blk = np.arange((int(width) + 3) // 4, dtype=np.uint64).reshape(1, -1)
    out = normals(philox4x32_10(blk, grow, draw, e_lo, s_lo, s_hi ^ e_hi))
    return tuple(v.reshape(grow.shape[0], -1)[:, :int(width)] for v in out)


def rows_table(desc, seed, event):
    """What dv_fill_normal_rows must write for the descriptor table ``desc`` (n x {offset, width, draw id, global row}):
    (offsets, z, r, a), flat over every described element in table order -- arena[offsets[i]] = z[i]."""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    order = np.arange(len(desc))
    widths = desc[:, 1]
    pos = np.empty(len(desc) + 1, np.int64)
    pos[0] = 0
    np.cumsum(widths, out=pos[1:])
    n = int(pos[-1])
    offsets, z, r, a = np.empty(n, np.int64), np.empty(n), np.empty(n), np.empty(n)
    for w in np.unique(widths):                        # rows of one width at a time: a rectangular block of counters
        sel = order[widths == w]
        if w <= 0:
            continue
        zz, rr, aa = row_draws(desc[sel, 3], w, desc[sel, 2], seed, event)
        idx = (pos[sel][:, None] + np.arange(w)[None, :]).reshape(-1)
        offsets[idx] = (desc[sel, 0][:, None] + np.arange(w)[None, :]).reshape(-1)
        z[idx], r[idx], a[idx] = zz.reshape(-1), rr.reshape(-1), aa.reshape(-1)
    return offsets, z, r, a


def flat(n, seed, ctr=0):
    """What dv_fill_normal must write: (z, r, a), each (n,): element i = lane i % 4 of Philox(counter = (lo, hi, 0, 0) of
    the 64-bit ``ctr + i // 4``, key = (seed_lo, seed_hi))."""
    s_lo, s_hi = _split(seed)
    c = np.uint64(int(ctr) & 0xFFFFFFFFFFFFFFFF) + np.arange((int(n) + 3) // 4, dtype=np.uint64)    # wraps mod 2^64
    out = normals(philox4x32_10(c & MASK, c >> _32, 0, 0, s_lo, s_hi))
    return tuple(v.reshape(-1)[:int(n)] for v in out)


def step_noise(spec, n_rows, seed, event, row0=0, true_slot=None):
    """The draws of ONE train step (draw event ``event``) for the global rows row0 .. row0 + n_rows - 1, in the layout of
    ``oracle.models_ref.make_noise`` (float32 of the float64 value), from the draw ids of ``drvae_amd/plan.py``:
    0 / 1 the input noise of x1 / x2; 2 + l, 2 + L + l, 2 + 2L + l the z1 / z2 / z2Fz1 draws of sample l;
    2 + 3L + l Y + slot the z3 draw of class slot ``slot``; 2 + 3L + L Y + l the regression head's y sample.
    ``true_slot`` (universal plans, which give every row all Y class slots): per row, the class of a labeled row, -1
    for an unlabeled one -- a labeled row's one z3 draw, which the oracle reads at slot 0, is the draw of its TRUE
    class slot there (see ``FusedStep.set_noise``)."""
    L, Y, X, Z1, Z3 = spec.L, spec.dim_y, spec.dim_x, spec.dim_z1, spec.dim_z3
    g = int(row0) + np.arange(n_rows)
    d = lambda width, draw: row_draws(g, width, draw, seed, event)[0].astype(np.float32)
    out = {'nx1': d(X, 0), 'nx2': d(X, 1),
           'ez1': np.stack([d(Z1, 2 + l) for l in range(L)]),
           'ez2': np.stack([d(Z1, 2 + L + l) for l in range(L)]),
           'ez2F': np.stack([d(Z1, 2 + 2 * L + l) for l in range(L)]),
           'ez3': np.stack([np.stack([d(Z3, 2 + 3 * L + l * Y + j) for j in range(Y)]) for l in range(L)]),
           'ey': np.stack([d(Y, 2 + 3 * L + L * Y + l) for l in range(L)])}
    if true_slot is not None:
        ts = np.asarray(true_slot).reshape(-1)
        lab = np.nonzero(ts >= 0)[0]
        e3 = out['ez3']
        e3[:, 0, lab] = e3[:, ts[lab], lab]
    return out
