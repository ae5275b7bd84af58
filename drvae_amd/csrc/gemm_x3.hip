// Split-bf16 products for gfx950: dv_gemm_x3 / dv_gemm_x3_ok ("bf16x3") and dv_gemm_split / dv_gemm_split_ok (the ladder
// "bf16x3" | "bf16x2" | "bf16x1" by the number of bf16 parts per operand) of include/drvae_hip.h.  OPT-IN: nothing in the
// library routes here on its own; the fp32-MFMA family of gemm.hip is untouched.
//
// Arithmetic contract (three parts: dv_gemm_x3 = dv_gemm_split(parts = 3))
//  - every fp32 operand element a is split into three bf16 terms (round to nearest even):
//        hi = bf16_rn(a),  mid = bf16_rn(a - hi),  lo = bf16_rn(a - hi - mid)
//    (both differences are exact in fp32; for a normal-range a with a 24-bit significand hi + mid + lo == a exactly);
//  - the product of a and b is the sum of the six cross products of weight <= 2:
//        hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid        (the dropped ones are <= 2^-22 |a| |b| together);
//  - every bf16 x bf16 product is exact in fp32 and accumulation is fp32 (v_mfma_f32_32x32x16_bf16);
//  - no atomics and a fixed order of summation -> results are bitwise reproducible.  Every output element has TWO
//    accumulators: the hi*hi terms go to one, the five correction terms (per 16-deep k step lo*hi, hi*lo, mid*mid, mid*hi,
//    hi*mid) to the other, k steps in ascending order, and the two are added once in front of the epilogue.  The matrix
//    pipe rounds the accumulator once per instruction at the accumulator's magnitude: kept apart, only one instruction in
//    six rounds at the magnitude of the result, the other five at 2^-8 of it (one accumulator for all six measured 2.3 x
//    the norm-wise error of the fp32 MFMA product at K = 980, two 0.88 x: profiles/r07_experiments.md);
//  - a non-finite operand element makes every output element it feeds non-finite (an inf may come out as NaN: its mid
//    term is inf - inf).  Elements whose magnitude rounds to the bf16 infinity (>= 2^128 - 2^119) count as non-finite.
//
// Arithmetic contract of the cheaper rungs (dv_gemm_split, parts = P < 3): strictly less of the same work
//  - the parts of an operand element are the FIRST P of hi, mid, lo above (the same roundings to nearest even);
//  - P = 2 ("bf16x2"): the three terms hi*hi, hi*mid, mid*hi.  mid*mid is dropped on purpose: it is <= 2^-16 |a| |b|, the
//    size of the residuals a - hi - mid (<= 2^-16 |a|) that are dropped already; |c - exact| <= (3 2^-16 + 2^-30) sum |a||b|
//    before accumulation.  Two accumulators as above: hi*hi in one, per 16-deep k step mid*hi then hi*mid in the other,
//    added once in front of the epilogue;
//  - P = 1 ("bf16x1"): the one term hi*hi in ONE accumulator -- a plain bf16 product of the rounded operands with fp32
//    accumulation, |c - exact| <= (2^-7 + 2^-16) sum |a||b| before accumulation: a DIFFERENT dtype, not an fp32 product;
//  - everything else is the three-part contract word for word: exact bf16 x bf16 products, fp32 accumulation in a fixed
//    order without atomics (bitwise reproducible), layouts, epilogues, alpha / beta, a_colsum by a launch in front, the
//    K-tail and over-read rules, the refusals of x3_check, and non-finite operand elements (P = 1: inf * 0 = NaN or inf).
//
// Structure: 128 x 128 output tile, K tile 32, four waves as 2 x 2 of 64 x 64 (four 32 x 32 accumulators each).  The SPLIT
// HAPPENS IN THE STAGING PATH, once per tile element: waves 0-1 load the A tile, waves 2-3 the B tile as fp32 16-B chunks
// into registers (issued before the MFMAs of the previous tile, consumed after them), split them and store three bf16 planes
// [128 rows][32 k] per operand in LDS (48 KiB; two workgroups per CU: 218-240 VGPRs).  A row of a plane is four 16-B chunks of 8 k; chunk
// c of row r sits at slot c ^ ((r >> 2) & 3), which keeps the fragment reads (32 rows x one chunk) free of bank conflicts.
// K tail: chunks at or past K are stored as zeros and never loaded (K % 4 == 0: a chunk is inside or outside as a whole);
// rows past M / N likewise.  With K % 4 == 0 nothing is ever read past the end of a row, whatever desc->flags allows.
// K % 4 != 0 runs only where every k-contiguous operand may be over-read (desc->flags bit 0 for A, bit 1 for B: up to 3
// floats past the end of a row stay inside the allocation): the 16-B chunk that straddles K is loaded whole and its
// elements past K are replaced by zeros before the split -- still a zero-filled K tail in LDS, and no over-read beyond what
// `flags` allows (operands that are not k-contiguous have rows along M / N: no chunk of theirs straddles K).
// The rungs with P < 3 parts are the same kernel template: only the planes a rung uses are split, staged and read.  Their K
// tile is KT sub-tiles of 32 (x3_kt: each sub-tile fetched, masked and staged exactly as the one tile above, its P planes
// behind those of the sub-tile in front): fewer MFMAs per 32 k need more k between two barriers to hide a global load
// (profiles/r10_experiments.md has the depths that lost).
#include "gemm_common.inc"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int X3_BM = 128, X3_BN = 128, X3_BK = 32;
constexpr int X3_PLANE = 128 * X3_BK * 2;        // bytes of one bf16 plane of one operand tile
// K tile of a rung and layout in sub-tiles of X3_BK, by compiling and measuring (profiles/r10_experiments.md): one part takes
// 64 deep wherever an operand is strided along k (dW, dX), two parts where both are k-contiguous (forward; 64 deep spills
// in the mixed layout and buys nothing on dW)
template <int P, bool AKC, bool BKC>
constexpr int x3_kt() {
    return P == 1 ? ((AKC && BKC) ? 1 : 2) : P == 2 ? ((AKC && BKC) ? 2 : 1) : 1;
}

__device__ __forceinline__ uint32_t x3_pack(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32: round to nearest even
}
__device__ __forceinline__ float x3_lo_f(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float x3_hi_f(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }

__device__ __forceinline__ int x3_slot(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// two consecutive k of one row -> one 32-bit word per plane, the first P planes only
template <int P>
__device__ __forceinline__ void x3_split2(float a0, float a1, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = x3_pack(a0, a1);
    if constexpr (P > 1) {
        const float r0 = a0 - x3_lo_f(h), r1 = a1 - x3_hi_f(h);
        m = x3_pack(r0, r1);
        if constexpr (P > 2) l = x3_pack(r0 - x3_lo_f(m), r1 - x3_hi_f(m));
    }
}

// eight consecutive k of one row -> one 16-B chunk per plane
template <int P>
__device__ __forceinline__ void x3_store_chunk(char* opnd, int row, int chunk, float x0, float x1, float x2, float x3,
                                               float x4, float x5, float x6, float x7) {
    uint4 h, m, l;
    x3_split2<P>(x0, x1, h.x, m.x, l.x);
    x3_split2<P>(x2, x3, h.y, m.y, l.y);
    x3_split2<P>(x4, x5, h.z, m.z, l.z);
    x3_split2<P>(x6, x7, h.w, m.w, l.w);
    const int off = x3_slot(row, chunk);
    *reinterpret_cast<uint4*>(opnd + off) = h;
    if constexpr (P > 1) *reinterpret_cast<uint4*>(opnd + X3_PLANE + off) = m;
    if constexpr (P > 2) *reinterpret_cast<uint4*>(opnd + 2 * X3_PLANE + off) = l;
}

// One operand tile (128 rows x 32 k) by 128 threads (t = 0..127), eight 16-B chunks each.
//   k-contiguous (X[r * ld + k]):  rows (t >> 2) + 32 i, i = 0..3, the 8 k of chunk t & 3 (v[2 i], v[2 i + 1])
//   otherwise    (X[k * ld + r]):  rows 4 (t & 31) .. + 3, the 8 k of chunk t >> 5 (v[j] = k row j)
template <bool KC>
__device__ __forceinline__ void x3_fetch(const float* __restrict__ X, int64_t ld, int R, int K, int row0, int k0, int t,
                                         f32x4 (&v)[8]) {
    // Every full chunk is ONE unconditional 16-B load from an address clamped into the operand (row R - 1 / k chunk 0 / k row
    // K - 1 stand in for what lies outside); x3_mask replaces the stand-ins by zeros when the tile is staged, so that nothing
    // between the loads and the MFMAs they fly under waits for them.  (A load under a lane condition is compiled into
    // branches around element-wise loads.)
    if constexpr (KC) {
        const int k = k0 + (t & 3) * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + (t >> 2) + 32 * i;
            const float* p = X + (int64_t)(r < R ? r : R - 1) * ld;
            v[2 * i] = *reinterpret_cast<const f32x4*>(p + (k < K ? k : 0));
            v[2 * i + 1] = *reinterpret_cast<const f32x4*>(p + (k + 4 < K ? k + 4 : 0));
        }
    } else {
        const int r = row0 + 4 * (t & 31), kb = k0 + (t >> 5) * 8;
        if (r + 4 <= R) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kb + j;
                v[j] = *reinterpret_cast<const f32x4*>(X + (int64_t)(k < K ? k : K - 1) * ld + r);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kb + j;
                // the ragged last chunk of a row: element by element from addresses clamped into the row, never past its
                // end; what lies past R or K counts as zero.  (Whole-register assignments only: a member of v[j] written
                // under a condition keeps the array in scratch memory.)
                const float* p = X + (int64_t)(k < K ? k : K - 1) * ld;
                const bool in = k < K;
                const float x = (in && r < R) ? p[r < R ? r : R - 1] : 0.f;
                const float y = (in && r + 1 < R) ? p[r + 1 < R ? r + 1 : R - 1] : 0.f;
                const float z = (in && r + 2 < R) ? p[r + 2 < R ? r + 2 : R - 1] : 0.f;
                v[j] = f32x4{x, y, z, 0.f};
            }
        }
    }
}

// zeros for everything x3_fetch loaded from a stand-in address: rows past R, k past K
template <bool KC>
__device__ __forceinline__ void x3_mask(int R, int K, int row0, int k0, int t, f32x4 (&v)[8]) {
    if (row0 + 128 <= R && k0 + X3_BK <= K) return;        // (wave-uniform) an interior tile: nothing was a stand-in
    if constexpr (KC) {
        const int k = k0 + (t & 3) * 8;
        // K % 4 != 0 (only where desc->flags lets this operand's row ends be over-read, see x3_check): the chunk that
        // straddles K was loaded whole; what lies past K counts as zero, whatever it held
        const int kc = K & ~3, n = K & 3;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = row0 + (t >> 2) + 32 * (i >> 1), kk = k + 4 * (i & 1);
            const bool ok = r < R && kk < K, tail = n != 0 && kk == kc;      // (selects, not branches)
            v[i].x = ok ? v[i].x : 0.f;
            v[i].y = (ok && !(tail && n < 2)) ? v[i].y : 0.f;
            v[i].z = (ok && !(tail && n < 3)) ? v[i].z : 0.f;
            v[i].w = (ok && !tail) ? v[i].w : 0.f;
        }
    } else {
        const int kb = k0 + (t >> 5) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // (component by component: a conditional between the two float4 OBJECTS is a select of their addresses, which
            // keeps the whole array in scratch memory -- measured 27.0 ms against 8.5 ms on the wide weight-gradient product,
            // profiles/r07_experiments.md)
            const bool ok = kb + j < K;
            v[j].x = ok ? v[j].x : 0.f;
            v[j].y = ok ? v[j].y : 0.f;
            v[j].z = ok ? v[j].z : 0.f;
            v[j].w = ok ? v[j].w : 0.f;
        }
    }
}

template <int P, bool KC>
__device__ __forceinline__ void x3_stage(char* opnd, int t, const f32x4 (&v)[8]) {
    if constexpr (KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            x3_store_chunk<P>(opnd, (t >> 2) + 32 * i, t & 3, v[2 * i].x, v[2 * i].y, v[2 * i].z, v[2 * i].w,
                              v[2 * i + 1].x, v[2 * i + 1].y, v[2 * i + 1].z, v[2 * i + 1].w);
    } else {
        const int r = 4 * (t & 31), c = t >> 5;
        x3_store_chunk<P>(opnd, r, c, v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x);
        x3_store_chunk<P>(opnd, r + 1, c, v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y);
        x3_store_chunk<P>(opnd, r + 2, c, v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z);
        x3_store_chunk<P>(opnd, r + 3, c, v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w);
    }
}

__device__ __forceinline__ bf16x8 x3_frag(const char* plane, int row, int chunk) {
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(plane + x3_slot(row, chunk)));
}

// The wave's 64 x 64 block from its four accumulators (element r of one: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column
// lane & 31): C = [act'(yref - shift) *] alpha acc [+ beta C], the arithmetic of epi_store_col for the two epilogues this
// family carries, one accumulator at a time (the shared routine, inlined four times with all its epilogues, does not fit
// the register budget of two workgroups per CU)
template <bool BWD>
__device__ __forceinline__ void x3_epilogue(const dv_gemm_desc& g, const f32x16 (&acc)[2][2], int row0, int col0) {
    const bool use_old = g.beta != 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + 32 * j;
        if (col >= g.N) continue;
        const bool first = col < g.split;
        const int act = first ? g.act0 : g.act1;
        const float shift = first ? g.shift0 : g.shift1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // the accumulator's 16 reads of yref / C as one batch (clamped rows) in front of its stores, so that no load
            // waits behind a store
            float y[16], old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + 32 * i + (r & 3) + 8 * (r >> 2), rc = row < g.M ? row : g.M - 1;
                y[r] = BWD ? g.yref[(int64_t)rc * g.ldy + col] : 0.f;
                old[r] = use_old ? g.C[(int64_t)rc * g.ldc + col] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + 32 * i + (r & 3) + 8 * (r >> 2);
                float v = acc[i][j][r] * g.alpha;
                if constexpr (BWD) v *= dv_dact_from_y(act, y[r] - shift);
                if (use_old) v += g.beta * old[r];
                if (row < g.M) g.C[(int64_t)row * g.ldc + col] = v;
            }
        }
    }
}

// P parts per operand (3: "bf16x3", the six terms of the header | 2: "bf16x2", three | 1: "bf16x1", one), K tile of KT
// sub-tiles of X3_BK.  P = 3, KT = 1 is the three-part kernel as it has always been: same staging, same order of the MFMAs.
template <int P, int KT, bool AKC, bool BKC>
__global__ __launch_bounds__(256, 2) void gemm_x3_kernel(const dv_gemm_desc g) {
    constexpr int SUB = P * X3_PLANE;               // one sub-tile of one operand: its P planes (hi | mid | lo)
    constexpr int OPND = KT * SUB, BK = KT * X3_BK;
    __shared__ __attribute__((aligned(16))) char lds[2 * OPND];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (wave-uniform values stay in scalar registers)
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int tiles_m = (g.M + X3_BM - 1) / X3_BM, tiles_n = (g.N + X3_BN - 1) / X3_BN;
    int tm, tn;
    tile_of_block(blockIdx.x, gridDim.x, tiles_m, tiles_n, 16, tm, tn);
    const int m0 = tm * X3_BM, n0 = tn * X3_BN;
    // waves 0-1 stage A, waves 2-3 stage B (wave-uniform)
    const bool stage_a = wave < 2;
    const int t = tid & 127;
    char* const ldsA = lds;
    char* const ldsB = lds + OPND;

    f32x16 acc[2][2], cor[2][2];            // hi*hi | the correction terms (see the header; P = 1 has none)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = cor[i][j][r] = 0.f;

    // (native 4-vectors, not HIP's float4 struct: with one part the struct array stays in scratch memory,
    // profiles/r10_experiments.md)
    f32x4 v[KT][8];
    const int ktiles = (g.K + BK - 1) / BK;
    // (one code path where both operands have the same layout: the staging waves differ in their arguments only)
    const float* const X = stage_a ? g.A : g.B;
    const int64_t ldx = stage_a ? g.lda : g.ldb;
    const int R = stage_a ? g.M : g.N, row0 = stage_a ? m0 : n0;
    char* const ldsX = stage_a ? ldsA : ldsB;
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int ku = k0 + u * X3_BK;      // (a sub-tile at or past K loads from clamped addresses and is staged as zeros)
            if constexpr (AKC == BKC) {
                x3_fetch<AKC>(X, ldx, R, g.K, row0, ku, t, v[u]);
            } else {
                if (stage_a)
                    x3_fetch<AKC>(X, ldx, R, g.K, row0, ku, t, v[u]);
                else
                    x3_fetch<BKC>(X, ldx, R, g.K, row0, ku, t, v[u]);
            }
        }
    };
    auto stage = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int ku = k0 + u * X3_BK;
            if constexpr (AKC == BKC) {
                x3_mask<AKC>(R, g.K, row0, ku, t, v[u]);
                x3_stage<P, AKC>(ldsX + u * SUB, t, v[u]);
            } else {
                if (stage_a) {
                    x3_mask<AKC>(R, g.K, row0, ku, t, v[u]);
                    x3_stage<P, AKC>(ldsX + u * SUB, t, v[u]);
                } else {
                    x3_mask<BKC>(R, g.K, row0, ku, t, v[u]);
                    x3_stage<P, BKC>(ldsX + u * SUB, t, v[u]);
                }
            }
        }
    };
    fetch(0);

    for (int kt = 0; kt < ktiles; ++kt) {
        __syncthreads();            // the previous tile's fragments have been read
        stage(kt * BK);
        __syncthreads();
        if (kt + 1 < ktiles) fetch((kt + 1) * BK);      // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int s = 0; s < 2 * KT; ++s) {
            const int c = 2 * (s & 1) + lh;
            const char* const subA = ldsA + (s >> 1) * SUB;
            const char* const subB = ldsB + (s >> 1) * SUB;
            bf16x8 a[2][P];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < P; ++p) a[i][p] = x3_frag(subA + p * X3_PLANE, wm * 64 + i * 32 + li, c);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bf16x8 b[P];
#pragma unroll
                for (int p = 0; p < P; ++p) b[p] = x3_frag(subB + p * X3_PLANE, wn * 64 + j * 32 + li, c);
                // the terms, smallest first; consecutive MFMAs never chain on the same accumulator
#define X3_TERM(ACC, PA, PB)                                                                               \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) ACC[i][j] =                                               \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][PA], b[PB], ACC[i][j], 0, 0, 0)
                if constexpr (P == 3) {
                    X3_TERM(cor, 2, 0);
                    X3_TERM(cor, 0, 2);
                    X3_TERM(acc, 0, 0);
                    X3_TERM(cor, 1, 1);
                    X3_TERM(cor, 1, 0);
                    X3_TERM(cor, 0, 1);
                } else if constexpr (P == 2) {
                    X3_TERM(cor, 1, 0);
                    X3_TERM(acc, 0, 0);
                    X3_TERM(cor, 0, 1);
                } else {
                    X3_TERM(acc, 0, 0);
                }
#undef X3_TERM
            }
        }
    }

    if constexpr (P > 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] += cor[i][j];
    }
    if (g.epilogue == DV_EPI_BWD)
        x3_epilogue<true>(g, acc, m0 + wm * 64 + 4 * lh, n0 + wn * 64 + li);
    else
        x3_epilogue<false>(g, acc, m0 + wm * 64 + 4 * lh, n0 + wn * 64 + li);
}

inline bool x3_aligned(const float* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; }

// 1: dv_gemm_x3 runs the descriptor; 0: unsupported; -1: invalid arguments
int x3_check(const dv_gemm_desc* d) {
    if (d == nullptr) return -1;
    const dv_gemm_desc& g = *d;
    if (g.M < 0 || g.N < 0 || g.K < 1) return -1;
    if (g.A2 != nullptr || g.a_kscale != nullptr || g.pub_flag != nullptr) return 0;
    if (g.epilogue != DV_EPI_PLAIN && g.epilogue != DV_EPI_BWD) return 0;
    if (!g.a_kcontig && g.b_kcontig) return 0;
    if (g.a_colsum != nullptr && (g.a_kcontig || g.b_kcontig)) return 0;
    // K % 4 != 0: only with the caller's word that the k-contiguous operands' row ends may be over-read (see the header)
    if ((g.K & 3) && ((g.a_kcontig && !(g.flags & 1)) || (g.b_kcontig && !(g.flags & 2)))) return 0;
    if (g.M == 0 || g.N == 0) return 1;
    if (g.A == nullptr || g.B == nullptr || g.C == nullptr) return -1;
    if (g.epilogue == DV_EPI_BWD && g.yref == nullptr) return -1;
    if (!x3_aligned(g.A, g.lda) || !x3_aligned(g.B, g.ldb)) return 0;
    // (the tile grid is a 1-D launch)
    if ((int64_t)((g.M + X3_BM - 1) / X3_BM) * ((g.N + X3_BN - 1) / X3_BN) > 0x7fffffffLL) return 0;
    return 1;
}

// KT = 0: the K tile the rung takes in this layout (x3_kt); else that many sub-tiles (lab)
template <int P, int KT>
void x3_launch(const dv_gemm_desc& g, int tiles, hipStream_t st) {
    if (g.a_kcontig && g.b_kcontig)
        hipLaunchKernelGGL((gemm_x3_kernel<P, KT ? KT : x3_kt<P, true, true>(), true, true>), dim3(tiles), dim3(256), 0, st, g);
    else if (g.a_kcontig)
        hipLaunchKernelGGL((gemm_x3_kernel<P, KT ? KT : x3_kt<P, true, false>(), true, false>), dim3(tiles), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL((gemm_x3_kernel<P, KT ? KT : x3_kt<P, false, false>(), false, false>), dim3(tiles), dim3(256), 0, st, g);
}

// parts: 1..3 (checked by the callers); kt: 0 = the rung's own K tile (x3_kt), else a lab depth of the tuning build
int x3_run(const dv_gemm_desc* d, int parts, int kt, dv_stream_t stream) {
    const int ok = x3_check(d);
    if (ok < 0) return DV_ERR_ARG;
    if (ok == 0) return DV_ERR_UNSUPPORTED;
    if (d->M == 0 || d->N == 0) return DV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dv_gemm_desc g = *d;
    g.tune = nullptr;
    if (g.a_colsum != nullptr) {
        // the bias gradient of a dy^T x product: the column sums of dy by a launch in front (as the 128 x 256 fp32 tiling)
        const int rc = dv_colsum(g.A, g.lda, g.K, g.M, g.a_colsum, g.colsum_beta, st);
        if (rc != DV_OK) return rc;
        g.a_colsum = nullptr;
    }
    const int tiles = ((g.M + X3_BM - 1) / X3_BM) * ((g.N + X3_BN - 1) / X3_BN);
    switch (parts * 16 + kt) {
        case 3 * 16: x3_launch<3, 0>(g, tiles, st); break;
        case 2 * 16: x3_launch<2, 0>(g, tiles, st); break;
        case 1 * 16: x3_launch<1, 0>(g, tiles, st); break;
#ifdef DV_LAB
        case 2 * 16 + 1: x3_launch<2, 1>(g, tiles, st); break;
        case 2 * 16 + 2: x3_launch<2, 2>(g, tiles, st); break;
        case 1 * 16 + 1: x3_launch<1, 1>(g, tiles, st); break;
        case 1 * 16 + 2: x3_launch<1, 2>(g, tiles, st); break;
        case 1 * 16 + 4: x3_launch<1, 4>(g, tiles, st); break;
#endif
        default: return DV_ERR_UNSUPPORTED;
    }
    DV_RETURN_LAUNCH();
}

}  // namespace

extern "C" int dv_gemm_x3_ok(const dv_gemm_desc* d) { return x3_check(d) == 1 ? 1 : 0; }

extern "C" int dv_gemm_x3(const dv_gemm_desc* d, dv_stream_t stream) { return x3_run(d, 3, 0, stream); }

extern "C" int dv_gemm_split_ok(const dv_gemm_desc* d, int32_t parts) {
    return parts >= 1 && parts <= 3 && x3_check(d) == 1 ? 1 : 0;
}

// (tuning build only: parts + 16 * kt runs the rung on a K tile of kt sub-tiles of 32, tools/split_bench.py --lab)
extern "C" int dv_gemm_split(const dv_gemm_desc* d, int32_t parts, dv_stream_t stream) {
    int kt = 0;
#ifdef DV_LAB
    kt = parts >> 4;
    parts &= 15;
#endif
    if (parts < 1 || parts > 3) return DV_ERR_ARG;
    return x3_run(d, parts, kt, stream);
}
