// The nuisance variable s as device data (use_s / use_MMD extension, src/DrVAE.py:394-398,537-540; src/DGMMixin.py:42-66):
//   dv_nuisance_feed   -- one-hot(s) columns of the stacked encoder / decoder rows and the class of every batch row, gathered
//                         through the epoch's index table (or from a batch-local class vector)
//   dv_mmd_grouped_fwd -- the feature-mean differences of ALL terms (data group, sample, latent, class) of a step
//   dv_mmd_grouped_bwd -- the step's penalty value and its gradient w.r.t. the stacked sample rows
//   dv_mmd_masked_fwd / _bwd -- the same two on a batch-independent plan: the data groups of the batch are read as data too
// Which rows belong to which class is read from `cls` inside the launches: one captured step serves every composition.
// Every output element has exactly one writer (no atomics, no zero fill): results are bitwise reproducible.
#include "dv_common.h"

namespace {

constexpr float kTwoPi = 6.283185307179586f;

// ------------------------------------------------------------------------------------------------ nuisance feed
struct FeedArgs {
    const int32_t* s;
    const int32_t* table;
    int n_batches;
    const int32_t* ctr;
    const int32_t* base;
    int B;
    const int32_t* pair_rows;
    int Np, L, S;
    float* sohe;
    int64_t lde;
    float* sohd;
    int64_t ldd;
    int32_t* cls;
};

__global__ __launch_bounds__(256) void nuisance_feed_kernel(const FeedArgs a) {
    const int Me = a.B + a.Np, LB = a.L * a.B, LN = a.L * a.Np;
    const int Md = LB + 2 * LN;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= Me + Md) return;
    // batch row of this stacked row: encoder rows [x1 rows | x2 rows of the pairs], decoder rows [z1 | z2 | z2Fz1] x L
    int i;
    float* out;
    if (r < Me) {
        i = r < a.B ? r : a.pair_rows[r - a.B];
        out = a.sohe + (int64_t)r * a.lde;
    } else {
        const int q = r - Me;
        if (q < LB) i = q % a.B;
        else i = a.pair_rows[((q - LB) % LN) % a.Np];
        out = a.sohd + (int64_t)q * a.ldd;
    }
    i = min(max(i, 0), a.B - 1);
    int c;
    if (a.table != nullptr) {
        int b = a.ctr[0] - a.base[0];
        b = b < 0 ? 0 : (b >= a.n_batches ? a.n_batches - 1 : b);
        c = a.s[a.table[(int64_t)b * a.B + i]];
    } else {
        c = a.s[i];
    }
    for (int k = 0; k < a.S; ++k) out[k] = (k == c) ? 1.f : 0.f;
    if (r < a.B) a.cls[r] = c;
}

// ------------------------------------------------------------------------------------------------ grouped / masked MMD
constexpr int FT = 16;   // forward: columns (features | latent dimensions) per workgroup
constexpr int FG = 16;   //          row groups of a workgroup (FT x FG = 256 threads)
constexpr int FR = 4;    //          rows per thread and pass: one W element feeds FR products
constexpr int BT = 8;    // backward: rows per workgroup
constexpr int BW = 8;    //           W elements per lane held in registers (rows of up to 64 BW features)
static_assert(BT == 8, "the backward's wave reduction maps lane bits 5..3 to 8 rows");

// What both families of launches work on.  A term group is a list of rows of z with the batch row of each (its class is
// cls[batch row]).  GROUPED (dv_mmd_grouped_*): the lists are constant tables (grp_ptr / rows / src).  MASKED
// (dv_mmd_masked_*): term group tg = q G + g is the part of row list q (one Monte-Carlo sample's z1 or z2 rows of a
// batch-independent plan) whose batch rows are in data group g of THIS batch -- the forward reads the batch's flags, packs
// the members (ascending batch row) into `members` and the backward reads them back.  Everything behind the lists -- the
// sums, their order, the reductions -- is the same code.
struct MmdArgs {
    const float* z;
    int64_t ldz;
    int n_z, Z, R, S, B, n_groups;
    const int32_t* cls;
    const float* W;
    const float* b;
    float a, c, w, fac;
    float* theta;
    float* diff;
    int32_t* cnt;
    float* m2;
    float* value;
    float* dz;
    int64_t ldd;
    // grouped
    const int32_t* grp_ptr;
    const int32_t* rows;
    const int32_t* src;
    int n_entries;
    // masked
    const int32_t* hx;
    const int32_t* hy;
    int n_flags;
    const int32_t* table;
    int n_batches;
    const int32_t* ctr;
    const int32_t* base;
    int Np, L, model, G;
    int32_t* members;
};

__device__ __forceinline__ int classes_looped(int S) { return S == 2 ? 1 : S; }    // two classes: the first pair only

// number of the group's rows in every class -> s_cnt[0 .. S) (all threads of the workgroup call this)
__device__ __forceinline__ void count_classes(const MmdArgs& d, int e0, int n, int* s_cnt, int (*s_w)[DV_MMD_MAX_CLASSES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine[DV_MMD_MAX_CLASSES];
#pragma unroll
    for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) mine[k] = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        int c = -1;
        if (j < n) c = d.cls[min(max(d.src[e0 + j], 0), d.B - 1)];
#pragma unroll
        for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) mine[k] += __popcll(__ballot(c == k));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) s_w[wave][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < DV_MMD_MAX_CLASSES)
        s_cnt[threadIdx.x] = s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
    __syncthreads();
}

// ---- masked lists
// first row of z of row list q (z1 lists of the L samples, then their z2 lists) and its number of rows
__device__ __forceinline__ int list_base(const MmdArgs& d, int q) { return q < d.L ? q * d.B : d.L * d.B + (q - d.L) * d.Np; }
__device__ __forceinline__ int list_rows(const MmdArgs& d, int q) { return q < d.L ? d.B : d.Np; }

// the batch's row of the flag arrays for every batch row: through the epoch table like dv_batch_masks, or batch-local
__device__ __forceinline__ const int32_t* batch_of_table(const MmdArgs& d) {
    if (d.table == nullptr) return nullptr;
    int b = d.ctr[0] - d.base[0];
    b = b < 0 ? 0 : (b >= d.n_batches ? d.n_batches - 1 : b);
    return d.table + (int64_t)b * d.B;
}

// data group of batch row i in the reference's order, and whether the row is a pair
__device__ __forceinline__ int data_group(const MmdArgs& d, const int32_t* tb, int i, bool* pair) {
    const int r = min(max(tb != nullptr ? tb[i] : i, 0), d.n_flags - 1);
    const bool hx = d.hx != nullptr && d.hx[r] != 0, hy = d.hy != nullptr && d.hy[r] != 0;
    *pair = hx;
    if (d.model == DV_MMD_GROUPS_DRVAE) return hx ? (hy ? 2 : 3) : (hy ? 0 : 1);
    if (d.model == DV_MMD_GROUPS_PVAE) return hx ? 1 : 0;
    return hy ? 0 : 1;
}

// the members of (row list q, data group g) packed into s_mem in ascending batch row, their number per class -> s_cnt;
// returns the number of members (all threads of the workgroup call this)
__device__ __forceinline__ int gather_members(const MmdArgs& d, int q, int g, int* s_mem, int* s_cnt,
                                              int (*s_w)[DV_MMD_MAX_CLASSES], int* s_wn) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = list_rows(d, q);
    const bool z2 = q >= d.L;
    const int32_t* tb = batch_of_table(d);
    int mine[DV_MMD_MAX_CLASSES];
#pragma unroll
    for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) mine[k] = 0;
    int total = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        bool m = false;
        int c = -1;
        if (j < n) {
            bool pair;
            m = data_group(d, tb, j, &pair) == g && (!z2 || pair);      // a z2 row exists for the batch's pairs only
            if (m) c = d.cls[j];
        }
        const unsigned long long ball = __ballot(m);
#pragma unroll
        for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) mine[k] += __popcll(__ballot(c == k));
        if (lane == 0) s_wn[wave] = __popcll(ball);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wave; ++w) off += s_wn[w];
        if (m) s_mem[off + __popcll(ball & ((1ull << lane) - 1ull))] = j;
        total += (s_wn[0] + s_wn[1]) + (s_wn[2] + s_wn[3]);
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DV_MMD_MAX_CLASSES; ++k) s_w[wave][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < DV_MMD_MAX_CLASSES)
        s_cnt[threadIdx.x] = s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
    __syncthreads();
    return total;
}

// grid (column tiles, term groups).  KIND 1: random Fourier features, 0: identity.  MASKED: dynamic LDS of B ints
template <int KIND, bool MASKED>
__global__ __launch_bounds__(256) void mmd_fwd_kernel(const MmdArgs d) {
    extern __shared__ int s_mem[];
    __shared__ int s_cnt[DV_MMD_MAX_CLASSES];
    __shared__ int s_w[4][DV_MMD_MAX_CLASSES];
    __shared__ int s_wn[4];
    __shared__ float s_red[2][FG][FT];
    const int tg = blockIdx.y;
    const int D = KIND ? d.R : d.Z, Kc = classes_looped(d.S);
    const int cl = threadIdx.x % FT, rg = threadIdx.x / FT;
    const int col = blockIdx.x * FT + cl;
    const bool vec = KIND && ((d.ldz | (int64_t)d.Z) & 3) == 0 && (reinterpret_cast<uintptr_t>(d.z) & 15) == 0;
    int e0, n, zbase = 0;
    if constexpr (MASKED) {
        const int q = tg / d.G;
        e0 = tg * d.B;
        zbase = list_base(d, q);
        n = gather_members(d, q, tg - q * d.G, s_mem, s_cnt, s_w, s_wn);
        if (blockIdx.x == 0) {
            for (int j = threadIdx.x; j < n; j += 256) d.members[e0 + j] = s_mem[j];
            if (threadIdx.x < d.S) d.cnt[tg * (d.S + 1) + threadIdx.x] = s_cnt[threadIdx.x];
            if (threadIdx.x == 0) d.cnt[tg * (d.S + 1) + d.S] = n;
        }
    } else {
        e0 = d.grp_ptr[tg];
        n = d.grp_ptr[tg + 1] - e0;
        count_classes(d, e0, n, s_cnt, s_w);
        if (blockIdx.x == 0 && threadIdx.x < d.S) d.cnt[tg * d.S + threadIdx.x] = s_cnt[threadIdx.x];
    }
    for (int k = 0; k < Kc; ++k) {
        const int t = tg * Kc + k;
        const int n0 = s_cnt[k], n1 = n - n0;
        float s0 = 0.f, s1 = 0.f;
        if (col < D && n0 > 0 && n1 > 0) {
            const float* Wt = KIND ? d.W + ((int64_t)t * d.Z) * d.R + col : nullptr;
            const float phase = KIND ? kTwoPi * d.b[(int64_t)t * d.R + col] : 0.f;
            for (int j0 = rg * FR; j0 < n; j0 += FG * FR) {
                const float* zr[FR];
                bool in0[FR];
                int64_t th0[FR];      // this row's row of theta
#pragma unroll
                for (int i = 0; i < FR; ++i) {
                    const int e = e0 + min(j0 + i, n - 1);
                    int row, bi;
                    if constexpr (MASKED) {
                        bi = s_mem[e - e0];
                        row = min(zbase + bi, d.n_z - 1);
                        th0[i] = (int64_t)k * d.n_z + row;
                    } else {
                        bi = min(max(d.src[e], 0), d.B - 1);
                        row = min(max(d.rows[e], 0), d.n_z - 1);
                        th0[i] = (int64_t)k * d.n_entries + e0 + j0 + i;
                    }
                    zr[i] = d.z + (int64_t)row * d.ldz;
                    in0[i] = d.cls[bi] == k;
                }
                float v[FR];
                if (KIND) {
                    float acc[FR];
#pragma unroll
                    for (int i = 0; i < FR; ++i) acc[i] = 0.f;
                    if (vec) {       // rows of z 16-B aligned: four latent dimensions per load (same order of sums)
                        for (int zz = 0; zz < d.Z; zz += 4) {
                            const float w0 = Wt[(int64_t)zz * d.R], w1 = Wt[(int64_t)(zz + 1) * d.R];
                            const float w2 = Wt[(int64_t)(zz + 2) * d.R], w3 = Wt[(int64_t)(zz + 3) * d.R];
#pragma unroll
                            for (int i = 0; i < FR; ++i) {
                                const float4 zv = *reinterpret_cast<const float4*>(zr[i] + zz);
                                acc[i] = fmaf(zv.w, w3, fmaf(zv.z, w2, fmaf(zv.y, w1, fmaf(zv.x, w0, acc[i]))));
                            }
                        }
                    } else {
                        for (int zz = 0; zz < d.Z; ++zz) {
                            const float w = Wt[(int64_t)zz * d.R];
#pragma unroll
                            for (int i = 0; i < FR; ++i) acc[i] = fmaf(zr[i][zz], w, acc[i]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < FR; ++i) {
                        const float th = fmaf(d.a, acc[i], phase);
                        if (j0 + i < n) d.theta[th0[i] * d.R + col] = th;
                        v[i] = cosf(th);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < FR; ++i) v[i] = zr[i][col];
                }
#pragma unroll
                for (int i = 0; i < FR; ++i) {
                    if (j0 + i < n) {
                        if (in0[i]) s0 += v[i];
                        else s1 += v[i];
                    }
                }
            }
        }
        s_red[0][rg][cl] = s0;
        s_red[1][rg][cl] = s1;
        __syncthreads();
        if (rg == 0 && col < D) {
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int g = 0; g < FG; ++g) {
                a0 += s_red[0][g][cl];
                a1 += s_red[1][g][cl];
            }
            // an empty side: the term is defined as 0 (value and gradient)
            const float diff = (n0 > 0 && n1 > 0) ? (KIND ? d.c : 1.f) * (a0 / (float)n0 - a1 / (float)n1) : 0.f;
            d.diff[(int64_t)t * D + col] = diff;
        }
        __syncthreads();
    }
}

// sum of squares of n floats, the same number in every thread of every workgroup that asks (fixed order)
__device__ __forceinline__ float block_sumsq(const float* x, int n, float* s_part) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s = fmaf(x[i], x[i], s);
    s = dv_wave_sum_all(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    return (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// grid (row tiles, term groups); dynamic LDS: BT x (R + Z) floats (KIND 1) | BT x Z floats (KIND 0)
template <int KIND, bool MASKED>
__global__ __launch_bounds__(256) void mmd_bwd_kernel(const MmdArgs d) {
    extern __shared__ float s_dyn[];
    __shared__ float s_part[4];
    __shared__ float s_u[BT];
    __shared__ int s_row[BT];
    __shared__ int s_src[BT];
    const int tg = blockIdx.y;
    const int D = KIND ? d.R : d.Z, Kc = classes_looped(d.S), Z = d.Z;
    const int cs = MASKED ? d.S + 1 : d.S;       // ints of cnt per term group
    const int j0 = blockIdx.x * BT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int e0, n;
    if constexpr (MASKED) {
        e0 = tg * d.B;
        n = min(max(d.cnt[tg * cs + d.S], 0), d.B);
        const int q = tg / d.G;
        if (q >= d.L && tg - q * d.G == 0) {
            // the z2 rows of the slots that hold no pair in this batch belong to no term: their gradient is written as
            // zeros here, by the workgroups of a data group of single rows (which has no z2 members)
            const int32_t* tb = batch_of_table(d);
            for (int i = threadIdx.x; i < BT * Z; i += 256) {
                const int jl = i / Z, zz = i - jl * Z;
                bool pair = true;
                if (j0 + jl < d.Np) data_group(d, tb, j0 + jl, &pair);
                if (!pair) d.dz[(int64_t)min(list_base(d, q) + j0 + jl, d.n_z - 1) * d.ldd + zz] = 0.f;
            }
        }
        if (n == 0 && blockIdx.x == 0) {         // no members: the terms' m2 (of a difference written as zeros) all the same
            for (int k = 0; k < Kc; ++k) {
                const float m2 = block_sumsq(d.diff + (int64_t)(tg * Kc + k) * D, D, s_part);
                if (threadIdx.x == 0) d.m2[tg * Kc + k] = m2;
            }
        }
    } else {
        e0 = d.grp_ptr[tg];
        n = d.grp_ptr[tg + 1] - e0;
    }
    float* s_out = s_dyn;                    // [BT][Z]: the tile's gradient rows, summed over the classes
    float* s_G = s_dyn + BT * Z;             // [BT][R]: d m2 / d theta (up to the term's factor)
    if (j0 < n) {
        for (int i = threadIdx.x; i < BT * Z; i += 256) s_out[i] = 0.f;
        if (threadIdx.x < BT) {
            const int e = e0 + min(j0 + (int)threadIdx.x, n - 1);
            if constexpr (MASKED) {
                s_src[threadIdx.x] = min(max(d.members[e], 0), list_rows(d, tg / d.G) - 1);
                s_row[threadIdx.x] = min(list_base(d, tg / d.G) + s_src[threadIdx.x], d.n_z - 1);
            } else {
                s_src[threadIdx.x] = min(max(d.src[e], 0), d.B - 1);
                s_row[threadIdx.x] = min(max(d.rows[e], 0), d.n_z - 1);
            }
        }
        for (int k = 0; k < Kc; ++k) {
            const int t = tg * Kc + k;
            const int n0 = d.cnt[tg * cs + k], n1 = n - n0;
            const float m2 = block_sumsq(d.diff + (int64_t)t * D, D, s_part);
            // d(fac * -w sqrt(m2)) / d m2 * 2 (the 2 of d m2 / d diff = 2 diff); m2 == 0: the term's gradient is defined as 0
            const float coef = (m2 > 0.f && n0 > 0 && n1 > 0) ? -d.fac * d.w / sqrtf(m2) : 0.f;
            if (threadIdx.x < BT) {
                const int j = j0 + threadIdx.x;
                float u = 0.f;
                if (j < n && n0 > 0 && n1 > 0) u = d.cls[s_src[threadIdx.x]] == k ? 1.f / (float)n0 : -1.f / (float)n1;
                s_u[threadIdx.x] = u * coef * (KIND ? d.c * d.a : 1.f);
            }
            if (KIND) {
                for (int i = threadIdx.x; i < BT * d.R; i += 256) {
                    const int jl = i / d.R, r = i - jl * d.R;
                    float g = 0.f;
                    if (j0 + jl < n && coef != 0.f) {
                        const int64_t th0 = MASKED ? (int64_t)k * d.n_z + s_row[jl] : (int64_t)k * d.n_entries + e0 + j0 + jl;
                        g = -d.diff[(int64_t)t * D + r] * sinf(d.theta[th0 * d.R + r]);
                    }
                    s_G[i] = g;
                }
                __syncthreads();
                const float* Wt = d.W + ((int64_t)t * Z) * d.R;
                // a lane's share of one row of W (up to 64 BW features) sits in registers, and the NEXT latent dimension's is
                // requested before this one's products start: the loads of a row go out together instead of one per trip
                const bool regs = d.R <= 64 * BW;
                float wc[BW], wn[BW];
                if (regs) {
#pragma unroll
                    for (int q = 0; q < BW; ++q) wc[q] = (wave < Z && lane + 64 * q < d.R) ? Wt[(int64_t)wave * d.R + lane + 64 * q] : 0.f;
                }
                for (int zz = wave; zz < Z; zz += 4) {
                    float acc[BT];
#pragma unroll
                    for (int jl = 0; jl < BT; ++jl) acc[jl] = 0.f;
                    if (regs) {
#pragma unroll
                        for (int q = 0; q < BW; ++q)
                            wn[q] = (zz + 4 < Z && lane + 64 * q < d.R) ? Wt[(int64_t)(zz + 4) * d.R + lane + 64 * q] : 0.f;
#pragma unroll
                        for (int q = 0; q < BW; ++q) {
                            const int r = lane + 64 * q;
                            if (r < d.R) {
#pragma unroll
                                for (int jl = 0; jl < BT; ++jl) acc[jl] = fmaf(s_G[jl * d.R + r], wc[q], acc[jl]);
                            }
                        }
#pragma unroll
                        for (int q = 0; q < BW; ++q) wc[q] = wn[q];
                    } else {
                        for (int r = lane; r < d.R; r += 64) {
                            const float w = Wt[(int64_t)zz * d.R + r];
#pragma unroll
                            for (int jl = 0; jl < BT; ++jl) acc[jl] = fmaf(s_G[jl * d.R + r], w, acc[jl]);
                        }
                    }
                    // the 8 row sums over the wave's 64 lanes in 10 exchanges instead of 48: every halving step keeps half of
                    // the rows in each half of the lanes (lane bits 5, 4, 3 end up as the row), then 8 lanes per row remain
                    float v4[4], v2[2];
                    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        v4[i] = (h5 ? acc[i + 4] : acc[i]) + __shfl_xor(h5 ? acc[i] : acc[i + 4], 32, 64);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        v2[i] = (h4 ? v4[i + 2] : v4[i]) + __shfl_xor(h4 ? v4[i] : v4[i + 2], 16, 64);
                    float v1 = (h3 ? v2[1] : v2[0]) + __shfl_xor(h3 ? v2[0] : v2[1], 8, 64);
                    v1 += __shfl_xor(v1, 4, 64);
                    v1 += __shfl_xor(v1, 2, 64);
                    v1 += __shfl_xor(v1, 1, 64);
                    const int jl = lane >> 3;
                    if ((lane & 7) == 0) s_out[jl * Z + zz] += s_u[jl] * v1;
                }
                __syncthreads();
            } else {
                __syncthreads();
                for (int i = threadIdx.x; i < BT * Z; i += 256) {
                    const int jl = i / Z, zz = i - jl * Z;
                    s_out[i] += s_u[jl] * d.diff[(int64_t)t * D + zz];
                }
                __syncthreads();
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) d.m2[t] = m2;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < BT * Z; i += 256) {
            const int jl = i / Z, zz = i - jl * Z;
            if (j0 + jl < n) d.dz[(int64_t)s_row[jl] * d.ldd + zz] = s_out[i];
        }
    }
    // the step's value: one workgroup walks all terms
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        float val = 0.f;
        for (int t = 0; t < d.n_groups * Kc; ++t) val -= d.w * sqrtf(block_sumsq(d.diff + (int64_t)t * D, D, s_part));
        if (threadIdx.x == 0) d.value[0] = val;
    }
}

int check_desc(const dv_mmd_grouped_desc* d) {
    DV_REQUIRE(d != nullptr);
    DV_REQUIRE(d->kind == 0 || d->kind == 1);
    DV_REQUIRE(d->n_groups >= 1 && d->n_entries >= 1 && d->max_rows >= 1 && d->max_rows <= d->n_entries);
    DV_REQUIRE(d->Z >= 1 && d->n_z >= 1 && d->B >= 1 && d->S >= 2 && d->S <= DV_MMD_MAX_CLASSES);
    DV_REQUIRE(d->z && d->grp_ptr && d->rows && d->src && d->cls && d->diff && d->cnt);
    DV_REQUIRE(d->ldz >= d->Z);
    if (d->kind == 1) DV_REQUIRE(d->R >= 1 && d->W && d->b && d->theta);
    return DV_OK;
}

MmdArgs grouped_args(const dv_mmd_grouped_desc* d) {
    MmdArgs a{};
    a.z = d->z, a.ldz = d->ldz, a.n_z = d->n_z, a.Z = d->Z, a.R = d->R, a.S = d->S, a.B = d->B, a.n_groups = d->n_groups;
    a.cls = d->cls, a.W = d->W, a.b = d->b, a.a = d->a, a.c = d->c, a.w = d->w, a.fac = d->fac;
    a.theta = d->theta, a.diff = d->diff, a.cnt = d->cnt, a.m2 = d->m2, a.value = d->value, a.dz = d->dz, a.ldd = d->ldd;
    a.grp_ptr = d->grp_ptr, a.rows = d->rows, a.src = d->src, a.n_entries = d->n_entries;
    return a;
}

int masked_groups(int model) { return model == DV_MMD_GROUPS_DRVAE ? 4 : 2; }
int masked_lists(const dv_mmd_masked_desc* d) { return d->L * (d->Np > 0 ? 2 : 1); }

int check_desc(const dv_mmd_masked_desc* d) {
    DV_REQUIRE(d != nullptr);
    DV_REQUIRE(d->kind == 0 || d->kind == 1);
    DV_REQUIRE(d->model == DV_MMD_GROUPS_DRVAE || d->model == DV_MMD_GROUPS_PVAE || d->model == DV_MMD_GROUPS_VFAE);
    DV_REQUIRE(d->Z >= 1 && d->B >= 1 && d->L >= 1 && d->Np >= 0 && d->Np <= d->B && d->S >= 2 && d->S <= DV_MMD_MAX_CLASSES);
    DV_REQUIRE((int64_t)d->L * ((int64_t)d->B + d->Np) < (1ll << 31) / (masked_groups(d->model) * d->S));
    DV_REQUIRE(d->z && d->cls && d->diff && d->cnt && d->members && d->n_flags >= 1);
    DV_REQUIRE(d->Np == 0 || d->hx);         // z2 lists are lists of pairs
    DV_REQUIRE(d->table == nullptr || (d->ctr && d->base && d->n_batches >= 1));
    DV_REQUIRE(d->ldz >= d->Z);
    if (d->kind == 1) DV_REQUIRE(d->R >= 1 && d->W && d->b && d->theta);
    return DV_OK;
}

MmdArgs masked_args(const dv_mmd_masked_desc* d) {
    MmdArgs a{};
    a.z = d->z, a.ldz = d->ldz, a.n_z = d->L * (d->B + d->Np), a.Z = d->Z, a.R = d->R, a.S = d->S, a.B = d->B;
    a.G = masked_groups(d->model), a.n_groups = masked_lists(d) * a.G;
    a.cls = d->cls, a.W = d->W, a.b = d->b, a.a = d->a, a.c = d->c, a.w = d->w, a.fac = d->fac;
    a.theta = d->theta, a.diff = d->diff, a.cnt = d->cnt, a.m2 = d->m2, a.value = d->value, a.dz = d->dz, a.ldd = d->ldd;
    a.hx = d->hx, a.hy = d->hy, a.n_flags = d->n_flags, a.table = d->table, a.n_batches = d->n_batches, a.ctr = d->ctr;
    a.base = d->base, a.Np = d->Np, a.L = d->L, a.model = d->model, a.members = d->members;
    return a;
}

}  // namespace

extern "C" int dv_nuisance_feed(const int32_t* s, const int32_t* table, int32_t n_batches, const int32_t* ctr,
                                const int32_t* base, int32_t B, const int32_t* pair_rows, int32_t Np, int32_t L, int32_t S,
                                float* sohe, int64_t lde, float* sohd, int64_t ldd, int32_t* cls, dv_stream_t stream) {
    DV_REQUIRE(s && sohe && sohd && cls && B >= 1 && Np >= 0 && L >= 1 && S >= 1 && lde >= S && ldd >= S);
    DV_REQUIRE(Np == 0 || pair_rows);
    DV_REQUIRE(table == nullptr || (ctr && base && n_batches >= 1));
    const FeedArgs a{s, table, n_batches, ctr, base, B, pair_rows, Np, L, S, sohe, lde, sohd, ldd, cls};
    const int rows = (B + Np) + L * B + 2 * L * Np;
    hipLaunchKernelGGL(nuisance_feed_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_grouped_fwd(const dv_mmd_grouped_desc* d, dv_stream_t stream) {
    if (int e = check_desc(d)) return e;
    const int D = d->kind ? d->R : d->Z;
    const dim3 grid((D + FT - 1) / FT, d->n_groups);
    const MmdArgs a = grouped_args(d);
    if (d->kind)
        hipLaunchKernelGGL((mmd_fwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((mmd_fwd_kernel<0, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_grouped_bwd(const dv_mmd_grouped_desc* d, dv_stream_t stream) {
    if (int e = check_desc(d)) return e;
    DV_REQUIRE(d->m2 && d->value && d->dz && d->ldd >= d->Z);
    const size_t lds = sizeof(float) * BT * ((size_t)d->Z + (d->kind ? (size_t)d->R : 0));
    if (lds > 60 * 1024) return DV_ERR_UNSUPPORTED;
    const dim3 grid((d->max_rows + BT - 1) / BT, d->n_groups);
    const MmdArgs a = grouped_args(d);
    if (d->kind)
        hipLaunchKernelGGL((mmd_bwd_kernel<1, false>), grid, dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((mmd_bwd_kernel<0, false>), grid, dim3(256), lds, (hipStream_t)stream, a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_masked_fwd(const dv_mmd_masked_desc* d, dv_stream_t stream) {
    if (int e = check_desc(d)) return e;
    const size_t lds = sizeof(int) * (size_t)d->B;           // a list's members
    if (lds > 60 * 1024) return DV_ERR_UNSUPPORTED;
    const int D = d->kind ? d->R : d->Z;
    const MmdArgs a = masked_args(d);
    const dim3 grid((D + FT - 1) / FT, a.n_groups);
    if (d->kind)
        hipLaunchKernelGGL((mmd_fwd_kernel<1, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((mmd_fwd_kernel<0, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_masked_bwd(const dv_mmd_masked_desc* d, dv_stream_t stream) {
    if (int e = check_desc(d)) return e;
    DV_REQUIRE(d->m2 && d->value && d->dz && d->ldd >= d->Z);
    const size_t lds = sizeof(float) * BT * ((size_t)d->Z + (d->kind ? (size_t)d->R : 0));
    if (lds > 60 * 1024) return DV_ERR_UNSUPPORTED;
    const MmdArgs a = masked_args(d);
    const dim3 grid((d->B + BT - 1) / BT, a.n_groups);
    if (d->kind)
        hipLaunchKernelGGL((mmd_bwd_kernel<1, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((mmd_bwd_kernel<0, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    DV_RETURN_LAUNCH();
}
