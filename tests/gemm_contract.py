"""Shared pieces of the fp32 GEMM family's contract tests (tests/test_gpu_gemm_contract.py on the device,
tests/test_gemm_contract_cpu.py for the checks themselves): the kernel variants ("routes"), the operand classes and shapes,
operands as views into poisoned buffers, the float64 reference with its element-wise bound, the sequential fp32 fma chain
that is the norm-wise yardstick, and the faulty emulations the CPU file proves the checks against.  No device, no library:
everything here is plain torch on host tensors (``Poisoned`` places them on whatever device it is given).

The element-wise bound (derived, not chosen).  An output element is alpha * sum_k a_k b_k through an epilogue.  However the
kernels split the chain over waves and K tiles, every product enters through one fma -- K roundings, each of a partial sum no
larger than S = sum_k |a_k| |b_k| -- and the partials of a K split (at most 8 waves, at most 16 additions with the two
halves of a wave's accumulator) are joined by additions of the same magnitude:

    |acc - c64| <= 1.01 (K + 16) U S,      U = 2^-24

(1.01: the second-order terms).  The epilogue adds its own roundings, written out in ``expected``."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import ref64
from tests.ref64 import U
from tests.test_x3_cpu import full_significands, scaled_permutation  # noqa: F401  (re-exported)

NAN = float('nan')
LAYOUTS = ((True, True), (True, False), (False, False))       # (a_kcontig, b_kcontig): x W^T, dy W, dy^T x
GUARD = 64                  # poisoned rows in front of and behind every operand (elements, for a vector)
SENTINEL = -7.25            # what the buffers around an OUTPUT hold
SHIFT = ref64.f32(1e-3)
C_NLL = 16                  # as tests/test_gpu_numerics.py

# ------------------------------------------------------------------------------------------------ routes
# (tiling, {option: value}, k-contiguous layouts only).  Which kernel each one names, from the dispatcher's conditions
# (gemm_launch in drvae_amd/csrc/gemm.hip) -- "ring": operands of class A (pipe_ok), otherwise "staged":
#   0            the heuristics: at these shapes (K <= 256, < 512 tiles) the 32x32 K-split tiling, as route 2
#   1            64x64x32 register-staged                      3   128x128x32 register-staged
#   17           32x32x32 seven-per-CU, register-staged        40  128x256x16 LDS-DMA ring (staged: falls back to 3)
#   46           64x64x32 LDS-DMA ring (staged: 64x64x32)      2   32x32x64, eight waves (dy^T x: four) -- ring / staged
#   2, opt[7]=1  32x32x64 four-wave K split, ring / staged
#   2, opt[8]=1  the dense 32x32x32 kernels at any size: gemm_kpipe_kernel<32,32,32,4> / gemm_kernel<32,32,32,1,1,4>
#   2, opt[3]=-1 never the ring: the register-staged form of the same tiling; with opt[8]=1 the staged dense kernel
ROUTES = ((0, {}, False), (1, {}, False), (3, {}, False), (17, {}, False), (40, {}, False), (46, {}, False),
          (2, {}, False), (2, {7: 1}, True), (2, {8: 1}, False), (2, {3: -1}, False), (2, {3: -1, 8: 1}, False))


def route_id(r):
    return 't%d' % r[0] + ''.join('-o%d=%d' % kv for kv in sorted(r[1].items()))


def route_layouts(r):
    return [l for l in LAYOUTS if l[0] or not r[2]]


class routed:
    """run the GEMM family on route ``r`` (a forced tiling plus dispatcher options); everything is restored on exit"""

    def __init__(self, K, r):
        self.K, self.tiling, self.opts = K, r[0], dict(r[1])

    def __enter__(self):
        assert self.K.gemm_force_tiling(self.tiling) == 0, 'product tiling %d missing from the library' % self.tiling
        for k, v in self.opts.items():
            assert self.K.gemm_set_option(k, v) == 0
        return self

    def __exit__(self, *a):
        self.K.gemm_force_tiling(0)
        for k in self.opts:
            self.K.gemm_set_option(k, -1 if k == 0 else 0)


# ------------------------------------------------------------------------------------------------ operand classes, shapes
# class A: 16-B aligned base, ld % 4 == 0, K % 4 == 0 (the LDS-DMA kernels run); B: ld % 4 == 0, K % 4 == 2 (vector loads,
# the ragged-K-tail widths vecA_t / vecB_t); C: odd ld (scalar loads); D: dense rows, ld == columns ("followed by more of
# the same buffer": an over-read chunk holds the start of the next row)
# (class, M, N, K, overread)
CASES = (('A', 150, 300, 200, True), ('A', 152, 300, 200, False), ('B', 150, 299, 202, False), ('C', 149, 299, 201, False),
         ('A', 70, 90, 4, True), ('A', 70, 90, 20, True), ('A', 70, 90, 36, True))
BASE = CASES[0]


def case_id(c):
    return '%s-%dx%dx%d%s' % (c[0], c[1], c[2], c[3], '-over' if c[4] else '')


def ld_of(cols, cls):
    if cls == 'C':
        return cols + (1 if cols % 2 == 0 else 2)
    if cls == 'D':
        return cols
    return (cols + 3) // 4 * 4 + 4


def bits(t):
    return t.view(torch.int32)


class Poisoned:
    """host tensor ``t`` (a matrix or a vector) as a view cut out of the MIDDLE of a wider buffer on ``dev``: ``GUARD`` rows
    in front and behind and the row pads hold ``fill`` (NaN for an operand: whatever is read outside it poisons what it
    feeds; a sentinel for an output: whatever is written outside it shows).  A stray access lands inside the allocation."""

    def __init__(self, t, dev, cls='A', fill=NAN):
        if t.dim() == 1:
            n = t.numel()
            self.buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=dev)
            self.view = self.buf[GUARD:GUARD + n]
        else:
            r, c = t.shape
            self.buf = torch.full((GUARD + r + GUARD, ld_of(c, cls)), fill, dtype=torch.float32, device=dev)
            self.view = self.buf[GUARD:GUARD + r, :c]
        self.view.copy_(t.to(dev))
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        if t.dim() == 1:
            self.inside[GUARD:GUARD + t.numel()] = True
        else:
            self.inside[GUARD:GUARD + t.shape[0], :t.shape[1]] = True
        self.before = bits(self.buf).clone()

    def unchanged(self):
        return torch.equal(bits(self.buf), self.before)

    def outside_untouched(self):
        return bool((bits(self.buf) == self.before)[~self.inside].all())


class Frame:
    """the operands and outputs of one call: ``inp`` / ``out`` place them, ``verify`` checks the memory contract"""

    def __init__(self, dev, cls='A'):
        self.dev, self.cls, self.ins, self.outs = dev, cls, [], []

    def inp(self, t, cls=None):
        if t is None:
            return None
        self.ins.append(Poisoned(t.float(), self.dev, cls or self.cls))
        return self.ins[-1].view

    def out(self, init, cls=None):
        """``init``: a shape (the view is pre-filled with NaN: the call may not read it) or its values (it accumulates)"""
        if not torch.is_tensor(init):
            init = torch.full(tuple(init), NAN)
        self.outs.append(Poisoned(init.float(), self.dev, cls or self.cls, fill=SENTINEL))
        return self.outs[-1].view

    def verify(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        for i, p in enumerate(self.ins):
            assert p.unchanged(), 'operand %d was written' % i
        for i, p in enumerate(self.outs):
            assert p.outside_untouched(), 'output %d: bytes outside the view were written' % i


def stored(op, kc):
    """the (rows, k) operand as it lies in memory: k-contiguous or not"""
    return op if kc else op.t()


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def random_operands(M, N, Kd, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 10007 * M + 101 * N + Kd)
    return torch.randn(M, Kd, generator=g), torch.randn(Kd, N, generator=g)


def scaled_selection(rows, cols, seed, along):
    """a (rows, cols) matrix of power-of-two scales with ONE non-zero per column (``along`` = 0) or per row (1), placed
    through a random permutation that wraps round: the generalisation of ``scaled_permutation`` to a rectangle -- every
    element of A @ P (of P @ B) is one exact product plus zeros"""
    rs = np.random.RandomState(seed)
    P = np.zeros((rows, cols), np.float32)
    if along == 0:
        P[rs.permutation(max(rows, cols))[:cols] % rows, np.arange(cols)] = np.exp2(rs.randint(-6, 7, size=cols))
    else:
        P[np.arange(rows), rs.permutation(max(rows, cols))[:rows] % cols] = np.exp2(rs.randint(-6, 7, size=rows))
    return torch.from_numpy(P)


@functools.lru_cache(maxsize=None)
def identity_operands(M, N, Kd):
    """(A, P) and (P', B): full 24-bit significands (exponents 2^-31 .. 2^14 after scaling: well inside the normal range)
    against scaled selections; and C0 of small integers for the accumulate form"""
    A, P = full_significands((M, Kd), 5 + Kd), scaled_selection(Kd, N, 6 + Kd, 0)
    P2, B = scaled_selection(M, Kd, 7 + Kd, 1), full_significands((Kd, N), 8 + Kd)
    C0 = torch.from_numpy(np.random.RandomState(9).randint(-8, 9, size=(M, N)).astype(np.float32))
    return (A, P), (P2, B), C0


def exact_product(A, B, alpha=1.0, beta=0.0, C0=None):
    """float64 product of an identity pair cast to fp32.  alpha is a power of two (exact); with beta = 1 the integer C0 is
    added to the exact product in ONE correctly rounded fp32 addition -- the float64 sum is exact, its cast that rounding"""
    p = A.double() @ B.double()
    assert torch.equal(p.float().double(), p)
    p = alpha * p
    return (p + beta * C0.double()).float() if beta else p.float()


def integer_operands(M, N, Kd, seed=3):
    rs = np.random.RandomState(seed + M + N)
    return (torch.from_numpy(rs.randint(-4, 5, size=(M, Kd)).astype(np.float32)),
            torch.from_numpy(rs.randint(-4, 5, size=(Kd, N)).astype(np.float32)))


def poison_points(M, N, Kd):
    """non-finite values at the first and last row of Aop, the first and last column of Bop (what the edge tiles clamp to)
    and one interior element; three of them at k = 0: in dense storage that is the element BEHIND the previous row's end.
    Returns ([(which, row, col, value)], expected mask of non-finite outputs)"""
    pts = [('A', 0, Kd - 1, NAN), ('A', M - 1, 0, math.inf), ('A', M // 2, 0, -math.inf),
           ('B', Kd - 1, 0, -math.inf), ('B', 0, N - 1, NAN)]
    want = torch.zeros(M, N, dtype=torch.bool)
    for w, r, c, _ in pts:
        if w == 'A':
            want[r, :] = True
        else:
            want[:, c] = True
    return pts, want


def poisoned_operands(M, N, Kd):
    A, B = (t.clone() for t in random_operands(M, N, Kd, seed=4))
    pts, want = poison_points(M, N, Kd)
    for w, r, c, v in pts:
        (A if w == 'A' else B)[r, c] = v
    return A, B, want


# ------------------------------------------------------------------------------------------------ the yardstick
def chain_matmul(A, B):
    """a plain sequential fp32 fma chain: k ascending, acc = fp32(acc + a_k * b_k) -- the float64 product (exact) and sum,
    rounded to fp32 at every step"""
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    A64, B64 = A.double(), B.double()
    for k in range(A.shape[1]):
        acc = (acc.double() + A64[:, k:k + 1] * B64[k:k + 1, :]).float()
    return acc


# ------------------------------------------------------------------------------------------------ epilogues
EPILOGUES = ('plain', 'plain-ab', 'bwd', 'bwd-ab', 'fwd')


@functools.lru_cache(maxsize=None)
def epilogue_case(name, M, N, seed=0):
    """host operands of an epilogue: dict(alpha, beta, C0, and per kind yref / scale, bias, resid)"""
    g = torch.Generator().manual_seed(77 + seed + 3 * M + N + 5 * EPILOGUES.index(name))
    ab = name.endswith('-ab')
    e = dict(kind=name.split('-')[0], alpha=-0.37 if ab else 1.0, beta=1.0 if ab else 0.0, h=N // 2)
    e['C0'] = torch.randn(M, N, generator=g) if ab else None
    if e['kind'] == 'bwd':
        ys = torch.randn(M, N, generator=g)
        ys[:, e['h']:] = ys[:, e['h']:].abs() + 0.5               # (a softplus output lies above its shift)
        e['yref'] = ys
    if e['kind'] == 'fwd':
        e['scale'] = torch.randn(N, generator=g).abs() + 0.5
        e['bias'] = torch.randn(N, generator=g)
        e['resid'] = torch.randn(M, e['h'], generator=g)
    return e


def epilogue_kwargs(K, e, place):
    """the launcher keywords of epilogue ``e``; ``place`` puts a host operand on the device (``Frame.inp``)"""
    kw = dict(alpha=e['alpha'], beta=e['beta'])
    if e['kind'] == 'bwd':
        kw.update(epi=K.EPI_BWD, yref=place(e['yref']), act0='elu', act1='softplus', shift0=0.0, shift1=SHIFT, split=e['h'])
    if e['kind'] == 'fwd':
        kw.update(epi=K.EPI_FWD, scale=place(e['scale']), bias=place(e['bias']), split=e['h'], act0='identity',
                  act1='softplus', shift0=0.0, shift1=SHIFT, resid=place(e['resid']), resid_cols=e['h'])
    return kw


def acc_bound(A, B):
    """(c64, element-wise bound of the fp32 accumulator): 1.01 (K + 16) U sum_k |a_k| |b_k|"""
    A64, B64 = A.double(), B.double()
    return A64 @ B64, 1.01 * (A.shape[1] + 16) * U * (A64.abs() @ B64.abs())


def expected(A, B, e, acc=None):
    """float64 reference and element-wise bound of epilogue ``e`` on A @ B; with ``acc`` (an fp32 accumulator, e.g.
    ``chain_matmul``) also that accumulator carried through the same epilogue in plain fp32 -- the yardstick's output.

    PLAIN / BWD (as the x3 tests): alpha * acc and * act' round once each, act' itself comes from y - shift (a few ulp of
    1 + |y|), + beta * C rounds the two magnitudes added.
    FWD: pre = scale * alpha * acc + bias rounds three times (2 |scale alpha c| + |pre|); the activation is 1-Lipschitz in
    the sense of its derivative at the far end of the interval (identity, softplus: monotone derivatives) and costs the
    rule of tests/ref64.py with C = 8; the shift and the residual round once each."""
    c64, dacc = acc_bound(A, B)
    a32, beta, h = ref64.f32(e['alpha']), e['beta'], e['h']
    N = B.shape[1]
    yard = None
    if e['kind'] in ('plain', 'bwd'):
        scale, ymag = torch.ones_like(c64), torch.zeros_like(c64)
        if e['kind'] == 'bwd':
            ys = e['yref']
            scale = torch.cat([ref64.dact_from_y('elu', ys[:, :h]), ref64.dact_from_y('softplus', ref64.f64(ys[:, h:]) - SHIFT)], 1)
            ymag = 1 + ref64.f64(ys).abs()
        prod = c64 * a32
        old = beta * e['C0'].double() if beta else torch.zeros_like(c64)
        want = prod * scale + old
        bound = dacc * abs(a32) * scale.abs() + U * (2 * (prod * scale).abs() + 8 * prod.abs() * ymag + 2 * old.abs() + 2 * want.abs())
        if acc is not None:
            yard = acc * torch.tensor(a32, dtype=torch.float32)
            if e['kind'] == 'bwd':
                yard = yard * scale.float()
            if beta:
                yard = yard + torch.tensor(beta, dtype=torch.float32) * e['C0']
        return want, bound, yard
    s, b = e['scale'].double(), e['bias'].double()
    sp, sh1 = e.get('act1', 'softplus') == 'softplus', e.get('shift1', SHIFT)      # (the second head: softplus or identity)
    lin = c64 * a32 * s
    pre = lin + b
    dpre = dacc * abs(a32) * s.abs() + U * (2 * lin.abs() + pre.abs())
    y = torch.cat([pre[:, :h], (F.softplus(pre[:, h:]) if sp else pre[:, h:]) + sh1], 1)
    slope = torch.cat([torch.ones_like(pre[:, :h]), torch.sigmoid(pre[:, h:] + dpre[:, h:]) if sp else torch.ones_like(pre[:, h:])], 1)
    extra = torch.cat([torch.zeros_like(pre[:, :h]), ref64.act_exp_extra('softplus' if sp else 'identity', pre[:, h:])], 1)
    want = y.clone()
    want[:, :h] += e['resid'].double()
    bound = 1.01 * slope * dpre + ref64.bound(8, y.abs(), extra) + U * (y.abs() + want.abs())
    if acc is not None:
        p32 = (acc * torch.tensor(a32, dtype=torch.float32)) * e['scale'] + e['bias']
        t1 = F.softplus(p32[:, h:]) if sp else p32[:, h:]
        yard = torch.cat([p32[:, :h] + e['resid'], t1 + torch.tensor(sh1, dtype=torch.float32)], 1)
    return want, bound, yard


def worst_excess(got, want, bound):
    """max |got - want| / bound; a non-finite output counts as inf"""
    return float(ref64.excess(got, want, bound).max())


def norm_ratio(got, yard, want):
    """Frobenius error of ``got`` against float64 over that of the yardstick"""
    e, ey = float(torch.linalg.norm(got.double() - want)), float(torch.linalg.norm(yard.double() - want))
    return e / max(ey, 1e-300)


def colsum_bound(dy):
    """db[m] = sum_k dy[k, m] on the matrix core's ones column: the same chain with b_k = 1"""
    d = dy.double()
    return d.sum(0), 1.01 * (dy.shape[0] + 16) * U * d.abs().sum(0)


def rows_bound(C, comps, extra, X, scale=0.5):
    """as tests/test_gpu_numerics.py: bound of scale * (row sum of X terms)"""
    return scale * (ref64.bound(C, comps, extra).sum(1) + ref64.row_sum_bound(ref64.f64(comps), X))


# ------------------------------------------------------------------------------------------------ tile maps
MAPS = (0, 1, 3, 16, 32)
# tiling -> (tile rows, tile columns) and two grids ragged in both directions: tile counts no multiple of 8 or of a band
# height, tiles_n >= tiles_m and tiles_n < tiles_m, at least 16 workgroups (below that map 1 is the linear map)
MAP_TILES = {2: (32, 32), 17: (32, 32), 1: (64, 64), 3: (128, 128), 40: (128, 256)}
MAP_GRIDS = {2: ((4, 14), (14, 4)), 17: ((4, 14), (14, 4)), 1: ((4, 14), (14, 4)), 3: ((5, 7), (7, 5)), 40: ((5, 7), (7, 5))}


def map_shape(tiling, grid):
    """(M, N) with ``grid`` = (tiles_m, tiles_n) tiles and a ragged rest of a few rows / one column"""
    bm, bn = MAP_TILES[tiling]
    return (grid[0] - 1) * bm + 5, (grid[1] - 1) * bn + 1


def tile_of_block(bid, nwg, tiles_m, tiles_n, tmap):
    """the workgroup -> tile maps as include/drvae_hip.h describes them (dv_gemm_tune.opt[0]): 0 linear; 1 XCD chunk-major
    (workgroups b, b + 8, ... share an XCD, which gets a contiguous range of the tile list ordered in chunks along the longer
    tile dimension; fewer than 16 workgroups: linear); >= 2 bands of that many tile rows swept column by column"""
    t = bid
    if tmap == 1 and nwg >= 16:
        x, j, base, rem = bid & 7, bid >> 3, nwg >> 3, nwg & 7
        t = x * base + min(x, rem) + j
        if tiles_n >= tiles_m:
            cw = (tiles_n + 7) >> 3
            c, r = divmod(t, cw * tiles_m)
            w = min(tiles_n - c * cw, cw)
            return r // w, c * cw + r % w
        ch = (tiles_m + 7) >> 3
        c, r = divmod(t, ch * tiles_n)
        hgt = min(tiles_m - c * ch, ch)
        return c * ch + r % hgt, r // hgt
    if tmap >= 2:
        grp, r = divmod(t, tmap * tiles_n)
        hgt = min(tiles_m - grp * tmap, tmap)
        return grp * tmap + r % hgt, r // hgt
    return t // tiles_n, t % tiles_n


def tile_of_block_skipping(bid, nwg, tiles_m, tiles_n, tmap):
    """FAULTY: the last workgroup lands on the first one's tile -- one tile is computed twice, one never"""
    return tile_of_block(0 if bid == nwg - 1 else bid, nwg, tiles_m, tiles_n, tmap)


def product_through_map(A, B, tiling, tmap, tile_of=tile_of_block):
    """emulated launch: C starts as NaN, workgroup ``bid`` computes the tile its map names (integer operands: exact)"""
    bm, bn = MAP_TILES[tiling]
    M, N = A.shape[0], B.shape[1]
    tiles_m, tiles_n = -(-M // bm), -(-N // bn)
    Cm = torch.full((M, N), NAN)
    for bid in range(tiles_m * tiles_n):
        tm, tn = tile_of(bid, tiles_m * tiles_n, tiles_m, tiles_n, tmap)
        Cm[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn] = A[tm * bm:(tm + 1) * bm] @ B[:, tn * bn:(tn + 1) * bn]
    return Cm


# ------------------------------------------------------------------------------------------------ faulty emulations
def truncated(t, bits_kept=10):
    """operands as a reduced-precision matrix instruction would see them: the significand cut to ``bits_kept`` bits"""
    drop = 23 - bits_kept
    return (t.contiguous().view(torch.int32) >> drop << drop).view(torch.float32)


def ksplit_matmul(A, B, parts=8, doubled=None):
    """the chain split into ``parts`` K ranges (one per wave), joined by additions; ``doubled``: that partial counted twice"""
    Kd = A.shape[1]
    edges = [Kd * i // parts for i in range(parts + 1)]
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for i in range(parts):
        p = chain_matmul(A[:, edges[i]:edges[i + 1]], B[edges[i]:edges[i + 1]])
        acc = acc + p * (2.0 if i == doubled else 1.0)
    return acc


def staged_matmul(bufA, geom, B, bk=16, lines='zero', mask='none'):
    """an emulated kernel reading its A operand (k lines as memory rows: the dy^T x layout, ``geom`` = (first row, K, M) of
    the view inside ``bufA``) from the poisoned buffer, K tile by K tile of ``bk`` lines, B's lines past K being zeros.
    ``lines``: what a k line past K reads -- 'zero' (a block of zeros, as the kernels do) or 'pad' (FAULTY: whatever lies
    behind the operand's last row: the guard rows).  ``mask``: how a line past K is switched off on top of that -- 'none' (B's
    zeros have to do it), 'select' or 'multiply' (FAULTY: value * 0)."""
    r0, Kd, M = geom
    kt = -(-Kd // bk) * bk
    if lines == 'pad':
        At = bufA[r0:r0 + kt, :M].clone()
    else:
        At = torch.cat([bufA[r0:r0 + Kd, :M], torch.zeros(kt - Kd, M)], 0)
    Bt = torch.cat([B, torch.zeros(kt - Kd, B.shape[1])], 0)
    live = (torch.arange(kt) < Kd)[:, None]
    if mask != 'none':
        At = torch.where(live, At, torch.zeros_like(At)) if mask == 'select' else At * live.float()
    return chain_matmul(At.t(), Bt)


def overread_matmul(flatA, M, Kd, ld, B, mask='select'):
    """an emulated kernel that loads the k-contiguous rows of A (row m at ``flatA[m * ld]``) in whole chunks of 4, the chunk
    that straddles K included (over-read: the row pad, or with dense rows the start of the NEXT row), and switches the
    elements past K off by 'select' or by 'multiply' (FAULTY: value * 0 keeps a NaN or an inf alive)"""
    k4 = (Kd + 3) // 4 * 4
    rows = torch.stack([flatA[m * ld:m * ld + k4] for m in range(M)])
    live = (torch.arange(k4) < Kd)[None, :]
    rows = torch.where(live, rows, torch.zeros_like(rows)) if mask == 'select' else rows * live.float()
    Bt = torch.cat([B, torch.zeros(k4 - Kd, B.shape[1])], 0)
    return (rows.double() @ Bt.double()).float()
