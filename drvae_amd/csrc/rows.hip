// Row-wise kernels of the Dr.VAE ELBO hot path (gfx950): reparameterisation, diagonal-
// Gaussian KL with free bits, Gaussian log-likelihood over genes, the categorical head,
// the y-marginalisation, row gathers / segment sums, WeightNorm scale + backward.
// All are HBM/L2-bound streaming kernels: coalesced row reads (16-B per lane where the
// layout allows), one 64-lane wavefront per row for the reductions (__shfl), no atomics
// (results are bitwise reproducible).
#include "dv_common.h"

#include <type_traits>

namespace {

constexpr float kLog2Pi = 1.8378770664093453f;   // float(np.log(2*np.pi)), src/blocks.py:196,234

inline int grid_for(int64_t work, int per_block, int cap = 4096) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// ------------------------------------------------------------------ colsum / act_bwd
// 64 columns x 4 row-lanes per block; rows strided by 4*gridDim.y
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int64_t ldx, int M, int N,
                                                     float* __restrict__ out, float beta) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
    float s = 0.f;
    if (col < N) {
        // eight independent loads per trip (the loop is a chain of memory round trips otherwise: 0.88 ms for the
        // 4096 x 40000 gradient of the wide configuration's decoder heads, i.e. 0.7 TB/s); fixed summation order
        const float* p = X + (int64_t)rl * ldx + col;
        const int64_t st = 4 * ldx;
        int m = rl;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
        for (; m + 28 < M; m += 32, p += 8 * st) {
            const float v0 = p[0], v1 = p[st], v2 = p[2 * st], v3 = p[3 * st];
            const float v4 = p[4 * st], v5 = p[5 * st], v6 = p[6 * st], v7 = p[7 * st];
            a0 += v0; a1 += v1; a2 += v2; a3 += v3;
            a4 += v4; a5 += v5; a6 += v6; a7 += v7;
        }
        s = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
        for (; m < M; m += 4, p += st) s += p[0];
    }
    part[rl][c] = s;
    __syncthreads();
    if (rl == 0 && col < N) {
        s = part[0][c] + part[1][c] + part[2][c] + part[3][c];
        out[col] = (beta != 0.f ? beta * out[col] : 0.f) + s;
    }
}

__global__ void act_bwd_kernel(float* __restrict__ dY, int64_t ldd, const float* __restrict__ Y, int64_t ldy, int M,
                               int N, int split, int act0, int act1, float shift0, float shift1) {
    const int64_t total = (int64_t)M * N;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(e / N), n = (int)(e % N);
        const bool first = n < split;
        const float y = Y[(int64_t)m * ldy + n] - (first ? shift0 : shift1);
        dY[(int64_t)m * ldd + n] *= dv_dact_from_y(first ? act0 : act1, y);
    }
}

// --------------------------------------------------------------------- WeightNorm
__global__ __launch_bounds__(256) void wn_scale_kernel(const float* __restrict__ W, int64_t ldw,
                                                       const float* __restrict__ g, int N, int K,
                                                       float* __restrict__ scale, float* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* w = W + (int64_t)row * ldw;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += w[k] * w[k];
    s = dv_wave_sum_all(s);
    if (lane == 0) {
        const float nrm = sqrtf(s);
        if (norm) norm[row] = nrm;
        scale[row] = g[row] / nrm;
    }
}

__global__ __launch_bounds__(256) void wn_bwd_kernel(const float* __restrict__ dWraw, int64_t ldr,
                                                     const float* __restrict__ W, int64_t ldw,
                                                     const float* __restrict__ g, const float* __restrict__ norm,
                                                     int N, int K, float* __restrict__ dW, int64_t ldd,
                                                     float* __restrict__ dg, float beta) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* w = W + (int64_t)row * ldw;
    const float* r = dWraw + (int64_t)row * ldr;
    float dot = 0.f;
    for (int k = lane; k < K; k += 64) dot += w[k] * r[k];
    dot = dv_wave_sum_all(dot);
    const float nrm = norm[row], gg = g[row];
    const float sc = gg / nrm, cw = dot * gg / (nrm * nrm * nrm);
    float* o = dW + (int64_t)row * ldd;
    for (int k = lane; k < K; k += 64) {
        const float v = sc * r[k] - cw * w[k];
        o[k] = (beta != 0.f ? beta * o[k] : 0.f) + v;
    }
    if (lane == 0) dg[row] = (beta != 0.f ? beta * dg[row] : 0.f) + dot / nrm;
}

// ---------------------------------------------------------------------- reparam
__global__ void reparam_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ sd, int64_t ldq,
                                   const int32_t* __restrict__ src_idx, int n, int reps, int Z,
                                   const float* __restrict__ eps, int64_t lde, int mode, float* __restrict__ out,
                                   int64_t ldo, const float* __restrict__ sub, int64_t lds,
                                   float* __restrict__ out2, int64_t ldo2, float* __restrict__ out3, int64_t ldo3,
                                   const int32_t* __restrict__ out3_idx) {
    const int64_t total = (int64_t)n * reps * Z;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / Z), d = (int)(e % Z);
        const int j = r % n;
        const int64_t qi = src_idx ? src_idx[j] : j;
        const float s = sd[qi * ldq + d];
        const float std_ = mode == DV_GAUSS_LOGVAR ? expf(0.5f * s) : s;
        const float z = eps[(int64_t)r * lde + d] * std_ + mu[qi * ldq + d];
        out[(int64_t)r * ldo + d] = z;
        if (out2) out2[(int64_t)r * ldo2 + d] = z - sub[(int64_t)r * lds + d];
        if (out3) {
            const int t = out3_idx[r];
            if (t >= 0) out3[(int64_t)t * ldo3 + d] = z;
        }
    }
}

__global__ void reparam_bwd_kernel(const float* __restrict__ dz, int64_t ldz, const float* __restrict__ eps,
                                   int64_t lde, const float* __restrict__ sd, int64_t ldq,
                                   const int32_t* __restrict__ src_idx, int n, int reps, int Z, int mode,
                                   float* __restrict__ dmu, float* __restrict__ dsd, int64_t lddq, float beta) {
    const int64_t total = (int64_t)n * Z;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / Z), d = (int)(e % Z);
        const int64_t qi = src_idx ? src_idx[j] : j;
        float a = 0.f, b = 0.f;
        for (int l = 0; l < reps; ++l) {
            const int64_t r = (int64_t)l * n + j;
            const float g = dz[r * ldz + d];
            a += g;
            b += g * eps[r * lde + d];
        }
        if (mode == DV_GAUSS_LOGVAR) b *= 0.5f * expf(0.5f * sd[qi * ldq + d]);
        float* pm = dmu + qi * lddq + d;
        float* ps = dsd + qi * lddq + d;
        *pm = (beta != 0.f ? beta * *pm : 0.f) + a;
        *ps = (beta != 0.f ? beta * *ps : 0.f) + b;
    }
}

// CSR form: q row i collects the samples listed in seg_rows[seg_ptr[i]..seg_ptr[i+1]) (any number of
// draws per row, e.g. L z1-samples + L z2-samples of a paired row) plus, optionally, row-aligned
// (dmu | dsd) contributions listed in a second CSR (the KL(q(z1|x)||p(z1|z3,y)) gradients of its
// fprop rows).  One launch replaces reparam_bwd x2 + a segment sum; deterministic.
// ---- joins folded into consumers (dv_wait / dv_bump arguments): a launch may first park every workgroup
// on another chain's flag (thread 0 polls, bounded), and may end by advancing device counters
#define DV_MAX_PARKED_GRID 512
typedef dv_wait ParkArgs;
typedef dv_bump CounterBump;

__device__ __forceinline__ void bump_counters(const CounterBump& bump) {
    for (int t = 0; t < 2; ++t) {
        if (bump.c[t] != nullptr) counter_add_words(bump.c[t], bump.n[t], bump.inc[t]);
    }
}

// ---- formulas shared by the launches below: ONE definition each, whichever kernel a piece of row arithmetic was folded into
// d max(raw, kl_min) / d raw under coefficient c: c above the free-bits floor, 0 below, c/2 on a tie (torch.max)
__device__ __forceinline__ float free_bits_gate(float c, float rv, float kl_min) {
    return c * (rv > kl_min ? 1.f : (rv == kl_min ? 0.5f : 0.f));
}

// d/d(mu_q, logvar_q, mu_p, logvar_p) of one element's kl_term (times -1/2) in log-variance form
struct KlGrad {
    float gmq, gsq, gmp, gsp;
};
__device__ __forceinline__ KlGrad kl_grad_logvar(float mq, float sq, float mp, float sp) {
    const float dm = mq - mp, ivp = expf(-sp), vq = expf(sq);
    KlGrad g;
    g.gmq = dm * ivp;
    g.gsq = -0.5f * (1.f - vq * ivp);
    g.gmp = -g.gmq;
    g.gsp = -0.5f * (-1.f + (dm * dm + vq) * ivp);
    return g;
}

__global__ void reparam_bwd_seg_kernel(const float* __restrict__ dz, int64_t ldz, const float* __restrict__ eps,
                                       int64_t lde, const float* __restrict__ sd, int64_t ldq,
                                       const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ seg_rows,
                                       int nq, int Z, int mode, const float* __restrict__ extra, int64_t ldx,
                                       const int32_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_rows,
                                       float* __restrict__ dmu, float* __restrict__ dsd, int64_t lddq, float beta,
                                       CounterBump bump, const float* __restrict__ dz2, int64_t ldz2, int n2,
                                       ParkArgs park, dv_prior_kl pk) {
    park_block(park);
    // (the counters are not read by this kernel: whoever starts first may advance them)
    if (blockIdx.x == 0 && threadIdx.x == 0) bump_counters(bump);
    const int64_t total = (int64_t)nq * Z;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / Z), d = (int)(e % Z);
        float a = 0.f, b = 0.f;
        for (int t = seg_ptr[i]; t < seg_ptr[i + 1]; ++t) {
            const int64_t r = seg_rows[t];
            float g = dz[r * ldz + d];
            if (r < n2) g += dz2[r * ldz2 + d];
            a += g;
            b += g * eps[r * lde + d];
        }
        if (mode == DV_GAUSS_LOGVAR) b *= 0.5f * expf(0.5f * sd[(int64_t)i * ldq + d]);
        if (extra) {
            for (int t = ex_ptr[i]; t < ex_ptr[i + 1]; ++t) {
                const int64_t r = ex_rows[t];
                a += extra[r * ldx + d];
                b += extra[r * ldx + Z + d];
            }
        }
        float* pm = dmu + (int64_t)i * lddq + d;
        float* ps = dsd + (int64_t)i * lddq + d;
        float vm = (beta != 0.f ? beta * *pm : 0.f) + a;
        float vs = (beta != 0.f ? beta * *ps : 0.f) + b;
        if (pk.coef != nullptr) {       // + d/d(mu, logvar) of coef * max(KL(q_i || N(0,I)), kl_min): what dv_kl_rows_bwd(beta = 1) added
            const float c = free_bits_gate(pk.coef[i], pk.raw[i], pk.kl_min);
            const float mq = pk.mu[(int64_t)i * pk.ld + d], vq = expf(sd[(int64_t)i * ldq + d]);
            vm += c * (mq * 1.f);
            vs += c * (-0.5f * (1.f - vq * 1.f));
        }
        *pm = vm;
        *ps = vs;
    }
}

// Backward of everything that hangs on the z2Fz1 samples (src/DrVAE.py:431-433,459-487) in one
// pass: one wave per batch row i, lanes over the dims d, looping the L samples:
//   dz2F = DZ2F[(l,i)] (+ gradient of the decoded copy for pairs)
//   DP2[(l,i)] = (dmu2 | dlv2) of p(z2|z1): reparam backward (+ KL(q(z2|x2)||p(z2|z1)) wrt p for pairs)
//   DZ1[(l,i)] += dmu2 (residual path mu2 = z1 + ...) (+ DZ1B[(l,i)] + seg_beta * its fprop rows of seg_src: the side chain's share)
//   DQ2[jp]    = sum_l KL gradient wrt q(z2|x2)           (pairs only)
// kl_out / raw_out set: the pairs' KL rows (what a kl_rows_fwd_kernel launch in front wrote) are formed here, from the
// operands the gradients read anyway -- same lane mapping, same tree: same bits -- and gate the gradients
struct Z2FArgs {
    const float* dz2f; int64_t ld_dz2f;       // (L*B, Z)
    const float* dzdec_pert; int64_t ld_pert;  // (L*Np, Z) gradient of the decoded z2Fz1 copies, or NULL
    const int32_t* pair_slot;                  // (B) jp or -1
    const float* eps; int64_t lde;             // (L*B, Z)
    const float* p2; int64_t ldp2;             // (L*B, 2Z)  mu2 | lv2
    const float* q2; int64_t ldq2;             // (Np, 2Z)   mu | lv of q(z2|x2)
    const float* coef; const float* raw; float kl_min;   // (L*Np) KL coefficients / raw KL (free bits)
    const float* dz1b; int64_t ld_dz1b;        // (L*B, Z) or NULL
    float* dp2; int64_t ld_dp2;                // (L*B, 2Z) out
    float* dz1; int64_t ld_dz1;                // (L*B, Z) in/out (+=)
    float* dq2; int64_t ld_dq2;                // (Np, 2Z) out, or NULL
    int L, B, Np, Z;
    const float* prior_coef; const float* prior_raw;   // (Np) or NULL: the prior-KL gradient of q2 rides along (dv_prior_kl)
    float* kl_out; float* raw_out;             // (L*Np) out, or NULL: the KL rows are this launch's own
    const float* seg_src; int64_t ld_seg; const int32_t* seg_ptr; float seg_beta;   // fprop rows' d/dz1, or NULL
    float z1_dz2f;                             // d/dz1 also gets z1_dz2f * dz2f (classifier input [z1, z2Fz1 - z1]: -1)
};

__device__ __forceinline__ float kl_term(int mode, float mq, float sq, float mp, float sp) {
    const float dm = mq - mp;
    if (mode == DV_GAUSS_LOGVAR) return 1.f - sp + sq - (dm * dm + expf(sq)) / expf(sp);
    const float vq = sq * sq, vp = sp * sp;
    return 1.f - logf(vp) + logf(vq) - (dm * dm + vq) / vp;
}

// what one (sample row r, dim d) of the block reads besides q2
struct Z2FElem {
    float mp, lp, gc, g, eps, z1, add;
};

// ... of it what the launch's own chain has written before the launch starts
__device__ __forceinline__ void z2f_load_own(const Z2FArgs& a, int64_t r, int64_t kr, int d, Z2FElem& e) {
    e.mp = a.p2[r * a.ldp2 + d];
    e.lp = a.p2[r * a.ldp2 + a.Z + d];
    e.g = (kr >= 0 && a.dzdec_pert) ? a.dzdec_pert[kr * a.ld_pert + d] : 0.f;
    e.eps = a.eps[r * a.lde + d];
    e.z1 = a.dz1[r * a.ld_dz1 + d];
}

// ... and what the chain behind the park has: d/dz2F and its share of d/dz1 from its parts,
// add = (dz1b + seg_beta * sum of seg_src rows [t0, t1)) + z1_dz2f * dz2f
__device__ __forceinline__ void z2f_load_side(const Z2FArgs& a, int64_t r, int d, int t0, int t1, Z2FElem& e) {
    e.gc = a.dz2f ? a.dz2f[r * a.ld_dz2f + d] : 0.f;
    e.g = e.gc + e.g;
    e.add = a.dz1b ? a.dz1b[r * a.ld_dz1b + d] : 0.f;
    if (a.seg_src != nullptr) {      // (dv_rows_segment_sum's sum, in its order)
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += a.seg_src[(int64_t)t * a.ld_seg + d];
        e.add += a.seg_beta * s;
    }
    if (a.z1_dz2f != 0.f) e.add += a.z1_dz2f * e.gc;
}

// gradients of one (sample row, dim): stores dp2 / dz1, adds the sample's share of d/dq2 to (gq_mu, gq_lv)
__device__ __forceinline__ void z2f_elem(const Z2FArgs& a, int64_t r, int d, bool pair, float c, float mq, float lq,
                                         const Z2FElem& e, float& gq_mu, float& gq_lv) {
    float dmu = e.g, dlv = e.g * e.eps * 0.5f * expf(0.5f * e.lp);
    if (pair) {
        // (the means' terms keep their own association, (c dm) ivp: kl_grad_logvar's c (dm ivp) rounds differently)
        const float dm = mq - e.mp, ivp = expf(-e.lp);
        const KlGrad k = kl_grad_logvar(mq, lq, e.mp, e.lp);
        gq_mu += c * dm * ivp;
        gq_lv += c * k.gsq;
        dmu += -c * dm * ivp;
        dlv += c * k.gsp;
    }
    a.dp2[r * a.ld_dp2 + d] = dmu;
    a.dp2[r * a.ld_dp2 + a.Z + d] = dlv;
    a.dz1[r * a.ld_dz1 + d] = e.z1 + (dmu + e.add);
}

// a row's state across its samples (Z <= 128: two dims per lane), and two samples' operands in registers
struct Z2FRow {
    int jp;
    bool pair, own_kl, prior;
    float cpr, mq[2], lq[2], gm[2], gl[2];
};
struct Z2FPair {
    Z2FElem e[2][2];
    int t0[2], t1[2];
    float cf[2], rv[2];
};

__device__ __forceinline__ void z2f_row_begin(const Z2FArgs& a, int i, int lane, Z2FRow& w) {
    w.jp = a.pair_slot ? a.pair_slot[i] : -1;
    w.pair = w.jp >= 0;
    w.own_kl = w.pair && a.raw_out != nullptr;
    w.prior = w.pair && a.dq2 && a.prior_coef != nullptr;
    w.cpr = 0.f;
    if (w.prior)      // the prior term of q(z2|x2) row jp (what dv_kl_rows_bwd(beta = 1) added)
        w.cpr = free_bits_gate(a.prior_coef[w.jp], a.prior_raw[w.jp], a.kl_min);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int d = lane + 64 * c;
        w.mq[c] = w.lq[c] = w.gm[c] = w.gl[c] = 0.f;
        if (w.pair && d < a.Z) {
            w.mq[c] = a.q2[(int64_t)w.jp * a.ldq2 + d];
            w.lq[c] = a.q2[(int64_t)w.jp * a.ldq2 + a.Z + d];
        }
    }
}

// samples l0, l0 + 1 of row i, first half: everything that does not come from the chain behind the park -- the operands, and
// with them the launch's own KL rows (kl_rows_fwd_kernel's lane mapping and tree: its bits), stored by lane 0
__device__ __forceinline__ void z2f_pair_own(const Z2FArgs& a, const Z2FRow& w, int i, int l0, int lane, Z2FPair& g) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        g.t0[u] = g.t1[u] = 0;
        g.cf[u] = g.rv[u] = 0.f;
        if (l0 + u >= a.L) break;
        const int64_t r = (int64_t)(l0 + u) * a.B + i, kr = w.pair ? (int64_t)(l0 + u) * a.Np + w.jp : -1;
        if (a.seg_src != nullptr) {
            g.t0[u] = a.seg_ptr[r];
            g.t1[u] = a.seg_ptr[r + 1];
        }
        if (w.pair) g.cf[u] = a.coef[kr];
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (lane + 64 * c < a.Z) z2f_load_own(a, r, kr, lane + 64 * c, g.e[u][c]);
    }
    if (!w.own_kl) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (l0 + u >= a.L) break;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (lane + 64 * c < a.Z) s += kl_term(DV_GAUSS_LOGVAR, w.mq[c], w.lq[c], g.e[u][c].mp, g.e[u][c].lp);
        g.rv[u] = -0.5f * dv_wave_sum_all(s);
        if (lane == 0) {
            const int64_t kr = (int64_t)(l0 + u) * a.Np + w.jp;
            a.raw_out[kr] = g.rv[u];
            a.kl_out[kr] = fmaxf(g.rv[u], a.kl_min);
        }
    }
}

// ... second half, behind the park: the other chain's operands, the gates, the gradients
__device__ __forceinline__ void z2f_pair_finish(const Z2FArgs& a, Z2FRow& w, int i, int l0, int lane, Z2FPair& g) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (l0 + u >= a.L) break;
        const int64_t r = (int64_t)(l0 + u) * a.B + i;
        if (w.pair && !w.own_kl) g.rv[u] = a.raw[(int64_t)(l0 + u) * a.Np + w.jp];
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (lane + 64 * c < a.Z) z2f_load_side(a, r, lane + 64 * c, g.t0[u], g.t1[u], g.e[u][c]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (l0 + u >= a.L) break;
        const int64_t r = (int64_t)(l0 + u) * a.B + i;
        const float cg = w.pair ? free_bits_gate(g.cf[u], g.rv[u], a.kl_min) : 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (lane + 64 * c < a.Z)
                z2f_elem(a, r, lane + 64 * c, w.pair, cg, w.mq[c], w.lq[c], g.e[u][c], w.gm[c], w.gl[c]);
    }
}

__device__ __forceinline__ void z2f_row_end(const Z2FArgs& a, Z2FRow& w, int lane) {
    if (!(w.pair && a.dq2)) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int d = lane + 64 * c;
        if (d >= a.Z) continue;
        if (w.prior) {
            w.gm[c] += w.cpr * (w.mq[c] * 1.f);
            w.gl[c] += w.cpr * (-0.5f * (1.f - expf(w.lq[c]) * 1.f));
        }
        a.dq2[(int64_t)w.jp * a.ld_dq2 + d] = w.gm[c];
        a.dq2[(int64_t)w.jp * a.ld_dq2 + a.Z + d] = w.gl[c];
    }
}

// Z <= 128.  The launch sits behind the join, on the step's critical path, and what it reads was written by other CUs: every
// dependent trip to memory behind the park counts.  So the first two samples' own-chain operands are read, and the KL rows
// formed, IN FRONT of the park -- in the shadow of the wait -- and one trip behind it fetches the other chain's operands
__global__ __launch_bounds__(256) void z2f_post_bwd_kernel(Z2FArgs a, ParkArgs park) {
    const int lane = threadIdx.x & 63;
    int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool has = i < a.B;
    Z2FRow w;
    Z2FPair g;
    if (has) {
        z2f_row_begin(a, i, lane, w);
        z2f_pair_own(a, w, i, 0, lane, g);
    }
    park_block(park);         // (every thread of the workgroup, with or without a row)
    if (!has) return;
    z2f_pair_finish(a, w, i, 0, lane, g);
    for (int l0 = 2; l0 < a.L; l0 += 2) {
        z2f_pair_own(a, w, i, l0, lane, g);
        z2f_pair_finish(a, w, i, l0, lane, g);
    }
    z2f_row_end(a, w, lane);
    for (i += gridDim.x * 4; i < a.B; i += gridDim.x * 4) {
        z2f_row_begin(a, i, lane, w);
        for (int l0 = 0; l0 < a.L; l0 += 2) {
            z2f_pair_own(a, w, i, l0, lane, g);
            z2f_pair_finish(a, w, i, l0, lane, g);
        }
        z2f_row_end(a, w, lane);
    }
}

// Z > 128: the dims are walked twice per sample (row sum, then gradients); d/dq2 accumulates in its own element
__global__ __launch_bounds__(256) void z2f_post_bwd_wide_kernel(Z2FArgs a, ParkArgs park) {
    park_block(park);
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < a.B; i += gridDim.x * 4) {
        const int jp = a.pair_slot ? a.pair_slot[i] : -1;
        const bool pair = jp >= 0;
        const bool own_kl = pair && a.raw_out != nullptr;
        const bool prior = pair && a.dq2 && a.prior_coef != nullptr;
        const float cpr = prior ? free_bits_gate(a.prior_coef[jp], a.prior_raw[jp], a.kl_min) : 0.f;
        for (int l = 0; l < a.L; ++l) {
            const int64_t r = (int64_t)l * a.B + i, kr = pair ? (int64_t)l * a.Np + jp : -1;
            const int t0 = a.seg_src ? a.seg_ptr[r] : 0, t1 = a.seg_src ? a.seg_ptr[r + 1] : 0;
            float rv = 0.f;
            if (own_kl) {
                float s = 0.f;
                for (int d = lane; d < a.Z; d += 64)
                    s += kl_term(DV_GAUSS_LOGVAR, a.q2[(int64_t)jp * a.ldq2 + d], a.q2[(int64_t)jp * a.ldq2 + a.Z + d],
                                 a.p2[r * a.ldp2 + d], a.p2[r * a.ldp2 + a.Z + d]);
                rv = -0.5f * dv_wave_sum_all(s);
                if (lane == 0) {
                    a.raw_out[kr] = rv;
                    a.kl_out[kr] = fmaxf(rv, a.kl_min);
                }
            } else if (pair) {
                rv = a.raw[kr];
            }
            const float cg = pair ? free_bits_gate(a.coef[kr], rv, a.kl_min) : 0.f;
            for (int d = lane; d < a.Z; d += 64) {
                float mq = 0.f, lq = 0.f, gm = 0.f, gl = 0.f;
                float* qm = nullptr;
                if (pair) {
                    mq = a.q2[(int64_t)jp * a.ldq2 + d];
                    lq = a.q2[(int64_t)jp * a.ldq2 + a.Z + d];
                    if (a.dq2) {      // (this lane's own element: the samples in front of l added to it)
                        qm = a.dq2 + (int64_t)jp * a.ld_dq2 + d;
                        if (l > 0) {
                            gm = qm[0];
                            gl = qm[a.Z];
                        }
                    }
                }
                Z2FElem e;
                z2f_load_own(a, r, kr, d, e);
                z2f_load_side(a, r, d, t0, t1, e);
                z2f_elem(a, r, d, pair, cg, mq, lq, e, gm, gl);
                if (qm != nullptr) {
                    if (prior && l == a.L - 1) {
                        gm += cpr * (mq * 1.f);
                        gl += cpr * (-0.5f * (1.f - expf(lq) * 1.f));
                    }
                    qm[0] = gm;
                    qm[a.Z] = gl;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------- KL rows
struct KlArgs {
    const float *mu_q, *sd_q;
    int64_t ldq;
    const int32_t* qidx;
    const float *mu_p, *sd_p;
    int64_t ldp;
    const int32_t* pidx;
    float prior_mu, prior_sd;
    int n, reps, Z, mode;
};

// one KL row: this lane's share of the sum of kl_term over the row's dims (operands gathered through qidx / pidx, or the
// prior); zout != NULL: the reparameterised sample of q is written in the same pass
__device__ __forceinline__ float kl_row_sum(const KlArgs& a, int r, int lane, const float* __restrict__ eps = nullptr,
                                            int64_t lde = 0, float* __restrict__ zout = nullptr, int64_t ldz = 0) {
    const int j = r % a.n;
    const int64_t qi = a.qidx ? a.qidx[j] : j;
    const int64_t pi = a.pidx ? a.pidx[r] : r;
    float s = 0.f;
    for (int d = lane; d < a.Z; d += 64) {
        const float mq = a.mu_q[qi * a.ldq + d], sq = a.sd_q[qi * a.ldq + d];
        const float mp = a.mu_p ? a.mu_p[pi * a.ldp + d] : a.prior_mu;
        const float sp = a.mu_p ? a.sd_p[pi * a.ldp + d] : a.prior_sd;
        s += kl_term(a.mode, mq, sq, mp, sp);
        if (zout)
            zout[(int64_t)r * ldz + d] =
                mq + eps[(int64_t)r * lde + d] * (a.mode == DV_GAUSS_LOGVAR ? expf(0.5f * sq) : sq);
    }
    return s;
}

// ... and its value from the wave's sum (lane 0): raw = -sum / 2, stored where asked for, under the free-bits floor
__device__ __forceinline__ float kl_row_finish(float sum, int free_bits, float kl_min, float* raw_out, int r) {
    const float raw = -0.5f * sum;
    if (raw_out) raw_out[r] = raw;
    return free_bits ? fmaxf(raw, kl_min) : raw;
}

__global__ __launch_bounds__(256) void kl_rows_fwd_kernel(KlArgs a, int free_bits, float kl_min,
                                                          float* __restrict__ raw_out, float* __restrict__ out,
                                                          const float* __restrict__ add,
                                                          const float* __restrict__ eps, int64_t lde,
                                                          float* __restrict__ zout, int64_t ldz, ParkArgs park,
                                                          const float* __restrict__ mu2, const float* __restrict__ sd2,
                                                          int64_t ld2, int Z2, float* __restrict__ raw2_out) {
    park_block(park);
    const int lane = threadIdx.x & 63;
    const int rows = a.n * a.reps;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
        float s2 = 0.f;
        if (mu2)   // second term of the same row: KL(N(mu2, sd2) || N(prior_mu, prior_sd)), row-aligned
            for (int d = lane; d < Z2; d += 64)
                s2 += kl_term(a.mode, mu2[(int64_t)r * ld2 + d], sd2[(int64_t)r * ld2 + d], a.prior_mu, a.prior_sd);
        const float s = dv_wave_sum_all(kl_row_sum(a, r, lane, eps, lde, zout, ldz));
        if (mu2) s2 = dv_wave_sum_all(s2);
        if (lane == 0) {
            float v = kl_row_finish(s, free_bits, kl_min, raw_out, r) + (add ? add[r] : 0.f);
            if (mu2) v += kl_row_finish(s2, free_bits, kl_min, raw2_out, r);
            out[r] = v;
        }
    }
}

// Two independent sets of KL rows in ONE launch (round 5; PVAE's main chain runs KL(q(z1|x) || N(0,I)) and the pairs'
// KL(q(z2|x2) || p(z2|z1)) back to back: two launches of ~40 workgroups each): workgroups [0, blocks_a) take set a, the rest
// set b; per row the arithmetic and summation order of kl_rows_fwd_kernel (no fused sample, no second term, no park).
struct KlFwd {
    KlArgs k;
    int free_bits;
    float kl_min;
    float* raw_out;
    float* out;
    const float* add;
};

__global__ __launch_bounds__(256) void kl_rows_fwd_pair_kernel(KlFwd sa, KlFwd sb, int blocks_a) {
    const bool first = (int)blockIdx.x < blocks_a;
    const KlFwd& s = first ? sa : sb;
    const KlArgs& a = s.k;
    const int blk = first ? blockIdx.x : blockIdx.x - blocks_a;
    const int lane = threadIdx.x & 63;
    const int rows = a.n * a.reps;
    const int r = blk * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float sum = dv_wave_sum_all(kl_row_sum(a, r, lane));
    if (lane == 0) s.out[r] = kl_row_finish(sum, s.free_bits, s.kl_min, s.raw_out, r) + (s.add ? s.add[r] : 0.f);
}

__global__ void kl_rows_bwd_kernel(KlArgs a, const float* __restrict__ coef, const float* __restrict__ raw,
                                   int free_bits, float kl_min, float* __restrict__ dq_mu,
                                   float* __restrict__ dq_sd, int64_t lddq, float* __restrict__ dp_mu,
                                   float* __restrict__ dp_sd, int64_t lddp, float beta,
                                   const float* __restrict__ dz, int64_t ldz, const float* __restrict__ eps,
                                   int64_t lde) {
    const int64_t total = (int64_t)a.n * a.reps * a.Z;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / a.Z), d = (int)(e % a.Z);
        const int j = r % a.n;
        const int64_t qi = a.qidx ? a.qidx[j] : j;
        const int64_t pi = a.pidx ? a.pidx[r] : r;
        float c = coef[r];
        if (free_bits) c = free_bits_gate(c, raw[r], kl_min);
        const float mq = a.mu_q[qi * a.ldq + d], sq = a.sd_q[qi * a.ldq + d];
        const float mp = a.mu_p ? a.mu_p[pi * a.ldp + d] : a.prior_mu;
        const float sp = a.mu_p ? a.sd_p[pi * a.ldp + d] : a.prior_sd;
        KlGrad k;
        if (a.mode == DV_GAUSS_LOGVAR) {
            k = kl_grad_logvar(mq, sq, mp, sp);
        } else {
            const float dm = mq - mp, vp = sp * sp;
            k.gmq = dm / vp;
            k.gsq = -1.f / sq + sq / vp;
            k.gmp = -k.gmq;
            k.gsp = 1.f / sp - (dm * dm + sq * sq) / (vp * sp);
        }
        float tq_mu = c * k.gmq, tq_sd = c * k.gsq;
        if (dz) {   // the sample drawn from q in the forward pass: z = mu + eps*std
            const float g = dz[(int64_t)r * ldz + d];
            tq_mu += g;
            tq_sd += g * eps[(int64_t)r * lde + d] * (a.mode == DV_GAUSS_LOGVAR ? 0.5f * expf(0.5f * sq) : 1.f);
        }
        const int64_t oq = (int64_t)r * lddq + d;
        dq_mu[oq] = (beta != 0.f ? beta * dq_mu[oq] : 0.f) + tq_mu;
        dq_sd[oq] = (beta != 0.f ? beta * dq_sd[oq] : 0.f) + tq_sd;
        if (dp_mu) {
            const int64_t op = (int64_t)r * lddp + d;
            dp_mu[op] = (beta != 0.f ? beta * dp_mu[op] : 0.f) + c * k.gmp;
            dp_sd[op] = (beta != 0.f ? beta * dp_sd[op] : 0.f) + c * k.gsp;
        }
    }
}

// -------------------------------------------------------- Gaussian NLL over genes
__device__ __forceinline__ float nll_term(int mode, float x, float m, float s) {
    const float d = x - m;
    if (mode == DV_GAUSS_SIGMA) {
        const float v = s * s;
        return kLog2Pi + logf(v) + d * d / v;
    }
    return kLog2Pi + s + d * d / expf(s);
}

// one term of a row's Gaussian log-likelihood from the heads' RAW product (x W^T without bias / activation): mu = m + bm,
// sd = softplus(s + bs) + shift on the hardware transcendentals (the forward half of nll_raw_sp_elem below)
__device__ __forceinline__ float nll_raw_term(float shift, float xv, float mraw, float sraw, float bm, float bs) {
    const float a = sraw + bs;
    const float e = __expf(-fabsf(a));
    const float sdv = fmaxf(a, 0.f) + dv_log1p_hw(e, __frcp_rn(1.f + e)) + shift;
    const float t = (xv - (mraw + bm)) * __frcp_rn(sdv);
    return kLog2Pi + 2.f * __logf(sdv) + t * t;
}

// RAW (evaluation passes behind a plain heads product, round 5): mu / sd are the raw products, finished on the way
template <int VEC, bool RAW>
__global__ __launch_bounds__(256) void nll_rows_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                           const int32_t* __restrict__ xidx,
                                                           const float* __restrict__ mu,
                                                           const float* __restrict__ sd, int64_t ldp, int M, int X,
                                                           int mode, float* __restrict__ out,
                                                           const float* __restrict__ bias_mu,
                                                           const float* __restrict__ bias_sd, float shift) {
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < M; r += gridDim.x * 4) {
        const float* xr = x + (int64_t)(xidx ? xidx[r] : r) * ldx;
        const float* mr = mu + (int64_t)r * ldp;
        const float* sr = sd + (int64_t)r * ldp;
        float s = 0.f;
        auto term = [&](float xv, float m, float sv, int g) -> float {
            if constexpr (RAW) return nll_raw_term(shift, xv, m, sv, bias_mu[g], bias_sd[g]);
            else return nll_term(mode, xv, m, sv);
        };
        if constexpr (VEC == 4) {
            const int X4 = X >> 2;
            for (int c = lane; c < X4; c += 64) {
                const float4 xv = reinterpret_cast<const float4*>(xr)[c];
                const float4 mv = reinterpret_cast<const float4*>(mr)[c];
                const float4 sv = reinterpret_cast<const float4*>(sr)[c];
                s += term(xv.x, mv.x, sv.x, 4 * c) + term(xv.y, mv.y, sv.y, 4 * c + 1) +
                     term(xv.z, mv.z, sv.z, 4 * c + 2) + term(xv.w, mv.w, sv.w, 4 * c + 3);
            }
            for (int g = (X4 << 2) + lane; g < X; g += 64) s += term(xr[g], mr[g], sr[g], g);
        } else if constexpr (VEC == 2) {
            // (978-gene rows: the sigma half starts 8 B off a 16-B boundary -- 8-B loads, two pairs per trip; dword loads
            // hold a row pass at 3.9 TB/s, round 5)
            const int X2 = X >> 1;
            auto pair = [&](int c) -> float {
                const float2 xv = reinterpret_cast<const float2*>(xr)[c];
                const float2 mv = reinterpret_cast<const float2*>(mr)[c];
                const float2 sv = reinterpret_cast<const float2*>(sr)[c];
                if constexpr (RAW) {
                    const float2 bm = reinterpret_cast<const float2*>(bias_mu)[c];
                    const float2 bs = reinterpret_cast<const float2*>(bias_sd)[c];
                    return nll_raw_term(shift, xv.x, mv.x, sv.x, bm.x, bs.x) + nll_raw_term(shift, xv.y, mv.y, sv.y, bm.y, bs.y);
                } else {
                    return nll_term(mode, xv.x, mv.x, sv.x) + nll_term(mode, xv.y, mv.y, sv.y);
                }
            };
            int c = lane;
            for (; c + 64 < X2; c += 128) s += pair(c) + pair(c + 64);
            for (; c < X2; c += 64) s += pair(c);
            if ((X & 1) && lane == 0) s += term(xr[X - 1], mr[X - 1], sr[X - 1], X - 1);
        } else {
            // (four independent elements per trip)
            int g = lane;
            for (; g + 192 < X; g += 256)
                s += (term(xr[g], mr[g], sr[g], g) + term(xr[g + 64], mr[g + 64], sr[g + 64], g + 64)) +
                     (term(xr[g + 128], mr[g + 128], sr[g + 128], g + 128) + term(xr[g + 192], mr[g + 192], sr[g + 192], g + 192));
            for (; g < X; g += 64) s += term(xr[g], mr[g], sr[g], g);
        }
        s = dv_wave_sum_all(s);
        if (lane == 0) out[r] = -0.5f * s;
    }
}

// forward AND backward of the reconstruction term in one row pass: the loss is linear in the
// per-row log-likelihoods with coefficients known before the forward pass, so d/d(mu, pre-act of
// sd) can be emitted while the row sum is being formed (3 reads + 2 writes per element instead
// of 6 + 2 over two launches)
// ds = d sd / d (pre-activation of sd), see sd_finish
__device__ __forceinline__ void nll_fb_elem(int mode, float ds, float c, float xv, float m, float s, float& acc, float& gm,
                                            float& gs) {
    const float d = xv - m;
    if (mode == DV_GAUSS_SIGMA) {
        const float v = s * s;
        acc += kLog2Pi + logf(v) + d * d / v;
        gm = d / v;
        gs = -1.f / s + d * d / (v * s);
    } else {
        const float iv = expf(-s);
        acc += kLog2Pi + s + d * d * iv;
        gm = d * iv;
        gs = -0.5f * (1.f - d * d * iv);
    }
    gs *= ds;
    gm *= c;
    gs *= c;
}

// (sd, d sd / d pre) of one element: finished heads (raw == false) hold sd, its activation's slope is taken from the
// output; raw heads hold pre - bias and are finished here, the softplus slope taken from the pre-activation itself
// (sigmoid(a): from the output it is sd - shift, which has lost all but a few bits of softplus(a) near the floor)
__device__ __forceinline__ float sd_finish(bool raw, int act, float shift, float v, float bias, float& ds) {
    if (!raw) {
        ds = act == DV_ACT_IDENTITY ? 1.f : dv_dact_from_y(act, v - shift);
        return v;
    }
    const float a = v + bias, s = dv_act(act, a) + shift;
    if (act == DV_ACT_SOFTPLUS) {
        const float e = __expf(-fabsf(a));
        ds = (a >= 0.f ? 1.f : e) * __frcp_rn(1.f + e);
    } else {
        ds = act == DV_ACT_IDENTITY ? 1.f : dv_dact_from_y(act, s - shift);
    }
    return s;
}

template <bool VEC2>
__global__ __launch_bounds__(256) void nll_rows_fwdbwd_kernel(const float* __restrict__ coef,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              const int32_t* __restrict__ xidx,
                                                              const float* __restrict__ mu,
                                                              const float* __restrict__ sd, int64_t ldp, int M, int X,
                                                              int mode, int sd_act, float sd_shift,
                                                              float* __restrict__ out, float* __restrict__ dmu,
                                                              float* __restrict__ dsd, int64_t ldd,
                                                              const float* __restrict__ bias_mu,
                                                              const float* __restrict__ bias_sd) {
    // one WORKGROUP per row, its four waves splitting the genes: a few hundred rows of ~1000 genes is
    // too little for wave-per-row to fill the chip (596 waves = 149 workgroups), and each wave's
    // dependent load->store chain is then 4x shorter
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x; r < M; r += gridDim.x) {
        const float* xr = x + (int64_t)(xidx ? xidx[r] : r) * ldx;
        const float* mr = mu + (int64_t)r * ldp;
        const float* sr = sd + (int64_t)r * ldp;
        float* gmr = dmu + (int64_t)r * ldd;
        float* gsr = dsd + (int64_t)r * ldd;
        const float c = coef[r];
        float acc = 0.f;
        // bias_mu != NULL: mu / sd hold the heads' RAW products (x W^T, no bias, no activation) -- the chip-filling
        // heads product then runs with the plain epilogue (8192 x 40000 x 2048: 9.97 ms instead of 10.87 with bias +
        // softplus in its 128x128 tiles' epilogue) and this HBM-bound pass applies them on its way
        const bool raw = bias_mu != nullptr;
        auto fin_m = [&](float v, int g) { return raw ? v + bias_mu[g] : v; };
        auto fin_s = [&](float v, int g, float& ds) { return sd_finish(raw, sd_act, sd_shift, v, raw ? bias_sd[g] : 0.f, ds); };
        if (VEC2) {
            const int X2 = X >> 1;
            for (int q = threadIdx.x; q < X2; q += 256) {
                const float2 xv = reinterpret_cast<const float2*>(xr)[q];
                float2 mv = reinterpret_cast<const float2*>(mr)[q];
                float2 sv = reinterpret_cast<const float2*>(sr)[q];
                float2 ds;
                mv.x = fin_m(mv.x, 2 * q);
                mv.y = fin_m(mv.y, 2 * q + 1);
                sv.x = fin_s(sv.x, 2 * q, ds.x);
                sv.y = fin_s(sv.y, 2 * q + 1, ds.y);
                float2 gm, gs;
                nll_fb_elem(mode, ds.x, c, xv.x, mv.x, sv.x, acc, gm.x, gs.x);
                nll_fb_elem(mode, ds.y, c, xv.y, mv.y, sv.y, acc, gm.y, gs.y);
                reinterpret_cast<float2*>(gmr)[q] = gm;
                reinterpret_cast<float2*>(gsr)[q] = gs;
            }
            if ((X & 1) && threadIdx.x == 0) {
                float gm, gs, ds;
                const float s = fin_s(sr[X - 1], X - 1, ds);
                nll_fb_elem(mode, ds, c, xr[X - 1], fin_m(mr[X - 1], X - 1), s, acc, gm, gs);
                gmr[X - 1] = gm;
                gsr[X - 1] = gs;
            }
        } else {
            for (int g = threadIdx.x; g < X; g += 256) {
                float gm, gs, ds;
                const float s = fin_s(sr[g], g, ds);
                nll_fb_elem(mode, ds, c, xr[g], fin_m(mr[g], g), s, acc, gm, gs);
                gmr[g] = gm;
                gsr[g] = gs;
            }
        }
        acc = dv_wave_sum_all(acc);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) out[r] = -0.5f * ((part[0] + part[1]) + (part[2] + part[3]));
        __syncthreads();
    }
}

// The raw-heads case of the pass above for the decoder the models build (sigma head = softplus + shift), written for
// the size it exists for (wide configuration: 8192 rows x 20000 genes, 2.9 GB of traffic): four genes per lane and the
// hardware transcendentals -- one exp, two logs, two reciprocals per gene instead of the library softplus / log / exp /
// divisions, which made the pass compute-bound (1.0 ms; this form 0.6 ms = the HBM time).
//   a = sd_raw + b_sd;  e = exp(-|a|);  softplus(a) = max(a, 0) + log1p(e);  sigmoid(a) = (a >= 0 ? 1 : e) / (1 + e)
__device__ __forceinline__ void nll_raw_sp_elem(float c, float shift, float xv, float mraw, float sraw, float bm, float bs,
                                                float& acc, float& gm, float& gs) {
    const float m = mraw + bm, a = sraw + bs;
    const float e = __expf(-fabsf(a));
    const float r1 = __frcp_rn(1.f + e);
    const float s = fmaxf(a, 0.f) + dv_log1p_hw(e, r1) + shift;
    const float sig = (a >= 0.f ? 1.f : e) * r1;
    const float is = __frcp_rn(s), d = xv - m, t = d * is;
    acc += kLog2Pi + 2.f * __logf(s) + t * t;
    gm = c * t * is;
    gs = c * (t * t - 1.f) * is * sig;
}

__global__ __launch_bounds__(256) void nll_rows_raw_sp_kernel(const float* __restrict__ coef, const float* __restrict__ x,
                                                              int64_t ldx, const int32_t* __restrict__ xidx,
                                                              const float* __restrict__ mu, const float* __restrict__ sd,
                                                              int64_t ldp, int M, int X, float shift,
                                                              float* __restrict__ out, float* __restrict__ dmu,
                                                              float* __restrict__ dsd, int64_t ldd,
                                                              const float* __restrict__ bias_mu,
                                                              const float* __restrict__ bias_sd) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X4 = X >> 2;
    for (int r = blockIdx.x; r < M; r += gridDim.x) {
        const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)(xidx ? xidx[r] : r) * ldx);
        const float4* mr = reinterpret_cast<const float4*>(mu + (int64_t)r * ldp);
        const float4* sr = reinterpret_cast<const float4*>(sd + (int64_t)r * ldp);
        float4* gmr = reinterpret_cast<float4*>(dmu + (int64_t)r * ldd);
        float4* gsr = reinterpret_cast<float4*>(dsd + (int64_t)r * ldd);
        const float c = coef[r];
        float acc = 0.f;
        // (the raw heads are read once and the gradients written once, 2.6 GB of the pass's 3.3: non-temporal, so that
        // they do not push the targets -- shared by a row's L samples -- and the biases out of the caches)
        typedef float nt_f4 __attribute__((ext_vector_type(4)));
        for (int q = threadIdx.x; q < X4; q += 256) {
            const float4 xv = xr[q];
            const nt_f4 mv = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(mr) + q);
            const nt_f4 sv = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(sr) + q);
            const float4 bm = reinterpret_cast<const float4*>(bias_mu)[q], bs = reinterpret_cast<const float4*>(bias_sd)[q];
            nt_f4 gm, gs;
            float a, b;
            nll_raw_sp_elem(c, shift, xv.x, mv[0], sv[0], bm.x, bs.x, acc, a, b); gm[0] = a; gs[0] = b;
            nll_raw_sp_elem(c, shift, xv.y, mv[1], sv[1], bm.y, bs.y, acc, a, b); gm[1] = a; gs[1] = b;
            nll_raw_sp_elem(c, shift, xv.z, mv[2], sv[2], bm.z, bs.z, acc, a, b); gm[2] = a; gs[2] = b;
            nll_raw_sp_elem(c, shift, xv.w, mv[3], sv[3], bm.w, bs.w, acc, a, b); gm[3] = a; gs[3] = b;
            __builtin_nontemporal_store(gm, reinterpret_cast<nt_f4*>(gmr) + q);
            __builtin_nontemporal_store(gs, reinterpret_cast<nt_f4*>(gsr) + q);
        }
        acc = dv_wave_sum_all(acc);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) out[r] = -0.5f * ((part[0] + part[1]) + (part[2] + part[3]));
        __syncthreads();
    }
}

// The same pass with the bias gradient of the heads folded in (round 5): db = column sums of (dmu | dsd) over the rows
// used to be a pass of its own over the 1.3 GB of gradients this kernel has just written (wide configuration: 0.23 ms
// per step).  Here a workgroup owns 256 four-gene groups x a block of kNllCsRows rows: every lane keeps the column sums
// of its four genes in registers while it walks the rows, and a row's log-likelihood comes out as one partial per
// column chunk (the loss assembly sums a row's partials: dv_loss_term.row_len).  Per-block column sums go to a small
// workspace (row_blocks x ldw), summed in a fixed order by dv_colsum over row_blocks rows: deterministic, no atomics.
constexpr int kNllCsRows = 64;
struct NllCsArgs {
    const float* coef; const float* x; int64_t ldx; const int32_t* xidx; const float* mu; const float* sd; int64_t ldp;
    int M, X; float shift; float* out_part; int chunks; float* dmu; float* dsd; int64_t ldd;
    const float* bias_mu; const float* bias_sd; float* ws; int64_t ldw; int64_t sd_off;
};

template <bool FWD_ONLY>
__global__ __launch_bounds__(256) void nll_rows_raw_cs_kernel(NllCsArgs a) {
    __shared__ float part[4][kNllCsRows];
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X4 = a.X >> 2;
    const int chunk = blockIdx.x, rb = blockIdx.y;
    const int q = chunk * 256 + threadIdx.x;
    const bool on = q < X4;
    const int qc = on ? q : X4 - 1;
    const int r0 = rb * kNllCsRows, r1 = r0 + kNllCsRows < a.M ? r0 + kNllCsRows : a.M;
    const float4 bm = reinterpret_cast<const float4*>(a.bias_mu)[qc], bs = reinterpret_cast<const float4*>(a.bias_sd)[qc];
    float4 cm = make_float4(0.f, 0.f, 0.f, 0.f), cs = make_float4(0.f, 0.f, 0.f, 0.f);
    // two rows per trip: six 16-B loads in flight per lane (the loop is a chain of memory round trips otherwise)
    for (int r = r0; r < r1; r += 2) {
        const bool two = r + 1 < r1;
        const int ra = r, rbb = two ? r + 1 : r;
        const float c0 = a.coef[ra], c1 = a.coef[rbb];
        const float4 x0 = reinterpret_cast<const float4*>(a.x + (int64_t)(a.xidx ? a.xidx[ra] : ra) * a.ldx)[qc];
        const float4 x1 = reinterpret_cast<const float4*>(a.x + (int64_t)(a.xidx ? a.xidx[rbb] : rbb) * a.ldx)[qc];
        const nt_f4 m0 = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(a.mu + (int64_t)ra * a.ldp) + qc);
        const nt_f4 s0 = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(a.sd + (int64_t)ra * a.ldp) + qc);
        const nt_f4 m1 = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(a.mu + (int64_t)rbb * a.ldp) + qc);
        const nt_f4 s1 = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(a.sd + (int64_t)rbb * a.ldp) + qc);
        float acc0 = 0.f, acc1 = 0.f;
        nt_f4 gm0, gs0, gm1, gs1;
        float u, v;
        nll_raw_sp_elem(c0, a.shift, x0.x, m0[0], s0[0], bm.x, bs.x, acc0, u, v); gm0[0] = u; gs0[0] = v;
        nll_raw_sp_elem(c0, a.shift, x0.y, m0[1], s0[1], bm.y, bs.y, acc0, u, v); gm0[1] = u; gs0[1] = v;
        nll_raw_sp_elem(c0, a.shift, x0.z, m0[2], s0[2], bm.z, bs.z, acc0, u, v); gm0[2] = u; gs0[2] = v;
        nll_raw_sp_elem(c0, a.shift, x0.w, m0[3], s0[3], bm.w, bs.w, acc0, u, v); gm0[3] = u; gs0[3] = v;
        nll_raw_sp_elem(c1, a.shift, x1.x, m1[0], s1[0], bm.x, bs.x, acc1, u, v); gm1[0] = u; gs1[0] = v;
        nll_raw_sp_elem(c1, a.shift, x1.y, m1[1], s1[1], bm.y, bs.y, acc1, u, v); gm1[1] = u; gs1[1] = v;
        nll_raw_sp_elem(c1, a.shift, x1.z, m1[2], s1[2], bm.z, bs.z, acc1, u, v); gm1[2] = u; gs1[2] = v;
        nll_raw_sp_elem(c1, a.shift, x1.w, m1[3], s1[3], bm.w, bs.w, acc1, u, v); gm1[3] = u; gs1[3] = v;
        if constexpr (FWD_ONLY) {         // (evaluation: the row terms only -- no gradients, no column sums)
            if (!on) acc0 = acc1 = 0.f;
        } else if (on) {
            __builtin_nontemporal_store(gm0, reinterpret_cast<nt_f4*>(a.dmu + (int64_t)ra * a.ldd) + q);
            __builtin_nontemporal_store(gs0, reinterpret_cast<nt_f4*>(a.dsd + (int64_t)ra * a.ldd) + q);
            // (fixed order: row r, then row r + 1 -- the same sums whatever the grid)
            cm.x += gm0[0]; cm.y += gm0[1]; cm.z += gm0[2]; cm.w += gm0[3];
            cs.x += gs0[0]; cs.y += gs0[1]; cs.z += gs0[2]; cs.w += gs0[3];
            if (two) {
                __builtin_nontemporal_store(gm1, reinterpret_cast<nt_f4*>(a.dmu + (int64_t)rbb * a.ldd) + q);
                __builtin_nontemporal_store(gs1, reinterpret_cast<nt_f4*>(a.dsd + (int64_t)rbb * a.ldd) + q);
                cm.x += gm1[0]; cm.y += gm1[1]; cm.z += gm1[2]; cm.w += gm1[3];
                cs.x += gs1[0]; cs.y += gs1[1]; cs.z += gs1[2]; cs.w += gs1[3];
            }
        } else {
            acc0 = acc1 = 0.f;
        }
        acc0 = dv_wave_sum_all(acc0);
        acc1 = dv_wave_sum_all(acc1);
        if (lane == 0) {
            part[wave][ra - r0] = acc0;
            if (two) part[wave][rbb - r0] = acc1;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < r1 - r0) {
        const int t = threadIdx.x;
        a.out_part[(int64_t)(r0 + t) * a.chunks + chunk] = -0.5f * ((part[0][t] + part[1][t]) + (part[2][t] + part[3][t]));
    }
    if constexpr (!FWD_ONLY) {
        if (on) {
            float* w = a.ws + (int64_t)rb * a.ldw;
            reinterpret_cast<float4*>(w)[q] = cm;
            reinterpret_cast<float4*>(w + a.sd_off)[q] = cs;
        }
    }
}

// Bernoulli / Poisson reconstruction rows (type_rec = 'binary' / 'poisson': the decoders src/DrVAE.py:124-129 names;
// the reference ships neither class -- labelled extension).  v = the head's POST-activation output
// (probability = sigmoid(a), or rate = softplus(a) + shift); out[r] = sum_g log p(x|v); with coef != NULL also
// dpre[r,g] = coef[r] * d log p / d a (the gradient w.r.t. the head's pre-activation a).
//   Bernoulli: pc = clamp(v, 1e-10, 1 - 1e-10) (the clamp of src/blocks.py:463 applied to this decoder's probabilities);
//              log p = x log pc + (1-x) log(1-pc);  d/da = x - v inside the clamp, 0 outside
//   Poisson  : log p = x log v - v - lgamma(x+1);   d/da = (x/v - 1) * sigmoid(a), sigmoid(a) = -expm1(-(v - shift))
//   library-scaled (LIB, DV_REC_POISSON_LIB): the rate is m = s v with the row's size factor s; d/da = (x/v - s) * sigmoid(a)
//              (x/m * s = x/v: the slope is the UNSCALED head's).  !LIB: s is not read, the term as it ever was
template <bool LIB>
__device__ __forceinline__ float rec_term(int kind, float shift, float s, float xv, float v, float& g) {
    if (kind == DV_REC_BERNOULLI) {
        const float lo = 1e-10f, hi = (float)(1.0 - 1e-10);
        const float pc = fminf(fmaxf(v, lo), hi);
        g = (v > lo && v < hi) ? xv - v : 0.f;
        return xv * logf(pc) + (1.f - xv) * logf(1.f - pc);
    }
    const float m = LIB ? s * v : v;
    g = (xv / v - (LIB ? s : 1.f)) * dv_softplus_slope_from_y(v - shift);
    return xv * logf(m) - m - lgammaf(xv + 1.f);
}

// The observed size factor of a target row (library-scaled kinds): s = max(sum_g x_g, 1) / X, by the whole workgroup in a
// fixed order -- per-thread partials in index order, the wave sum, then the four waves as (p0 + p1) + (p2 + p3), like the
// row sums below.  (Integer counts with a total below 2^24 sum exactly in fp32 in ANY order: s is then one correctly
// rounded quotient.)  VEC: 16-byte loads.  Every thread returns s; `part` is free again on return
template <bool VEC>
__device__ __forceinline__ float row_size_factor(const float* __restrict__ xr, int X, float* part) {
    float acc = 0.f;
    if constexpr (VEC) {
        for (int q = threadIdx.x; q < (X >> 2); q += 256) {
            const float4 xv = reinterpret_cast<const float4*>(xr)[q];
            acc += xv.x, acc += xv.y, acc += xv.z, acc += xv.w;
        }
    } else {
        for (int g = threadIdx.x; g < X; g += 256) acc += xr[g];
    }
    acc = dv_wave_sum_all(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    const float tot = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();
    return fmaxf(tot, 1.f) / (float)X;
}

// Negative-binomial reconstruction rows (type_rec = 'nb': labelled extension, no counterpart in the reference): mean m > 0,
// inverse dispersion t > 0 (Var = m + m^2 / t), count x >= 0.
//   log p = [lgamma(x+t) - lgamma(t)] - lgamma(x+1) + t log(t/(t+m)) + x log(m/(t+m))
//   d/dm  = x/m - (x+t)/(t+m) = (x - m) / (m (1 + m/t));   d/dt = [psi(x+t) - psi(t)] + log(t/(t+m)) + (m - x)/(t+m)
// Every cancelling pair is formed as a difference, never as two large values subtracted:
//   * the lgamma and digamma pairs: n = min(x, steps that lift t to >= 8) recurrence steps (log of the product of t + k,
//     sum of 1 / (t + k): at most 8, and ALL of x when x is that small), then for the d = x - n steps left, from b = t + n >= 8
//     to a = b + d, the difference of the asymptotic series with the leading logs combined:
//       lgamma(a) - lgamma(b) = d log a + ((b - 1/2) log1p(d/b) - d) + (s(a) - s(b)),  s(z) = 1/12z - 1/360z^3 + 1/1260z^5
//       psi(a) - psi(b)       = log1p(d/b) + d/(2ab) + d(a+b)/(12 a^2 b^2) + (q(a) - q(b)),  q(z) = 1/120z^4 - 1/252z^6
//     (the series' next terms at z = 8: 3e-10 and 2e-10 absolute).  x = 0: n = d = 0, both pairs are exactly 0.
//   * log(t/(t+m)) = -log1p(m/t) and log(m/(t+m)) = -log1p(t/m): exact in the Poisson limit (t log(t/(t+m)) -> -m) and
//     in its mirror (t << m).
// g_m / g_t: the gradients w.r.t. the heads' pre-activations (softplus slope from the stored outputs, as rec_term does).
// LIB (DV_REC_NEGBIN_LIB): the mean is m = s v with the row's size factor s and the mean head's output v; the slope of
// g_m comes from the UNSCALED head, d/da_m = d/dm * s * slope = (x - m) / (v (1 + m/t)) * slope(v - shift); theta and g_t as
// they are, at m.  !LIB: s is not read and m = v, the term as it ever was
template <bool LIB>
__device__ __forceinline__ float nb_term(float shift, float s, float x, float v, float t, float& g_m, float& g_t) {
    const float m = LIB ? s * v : v;
    const float n8 = t < 8.f ? ceilf(8.f - t) : 0.f;
    const float n = fminf(x, n8), d = x - n;
    float prod = 1.f, rsum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float tk = t + (float)k;
        if ((float)k < n) {
            prod *= tk;
            rsum += 1.f / tk;
        }
    }
    float lg = n > 0.f ? logf(prod) : 0.f, ps = rsum;
    if (d > 0.f) {
        const float b = t + n, a = b + d;
        const float ra = 1.f / a, rb = 1.f / b, ra2 = ra * ra, rb2 = rb * rb;
        const float l1 = log1pf(d * rb);
        const float sa = ra * (1.f / 12.f - ra2 * (1.f / 360.f - ra2 * (1.f / 1260.f)));
        const float sb = rb * (1.f / 12.f - rb2 * (1.f / 360.f - rb2 * (1.f / 1260.f)));
        lg += d * logf(a) + (fmaf(b - 0.5f, l1, -d) + (sa - sb));
        const float qa = ra2 * ra2 * (1.f / 120.f - ra2 * (1.f / 252.f));
        const float qb = rb2 * rb2 * (1.f / 120.f - rb2 * (1.f / 252.f));
        ps += l1 + d * ra * rb * (0.5f + (a + b) * ra * rb * (1.f / 12.f)) + (qa - qb);
    }
    const float lt = -log1pf(m / t), lm = -log1pf(t / m);
    const float tm = t + m;
    g_m = (x - m) / (v * (1.f + m / t)) * dv_softplus_slope_from_y(v - shift);
    g_t = (ps + lt + (m - x) / tm) * dv_softplus_slope_from_y(t - DV_NB_THETA_SHIFT);
    return (lg - lgammaf(x + 1.f)) + (t * lt + x * lm);
}

// Zero-inflated negative-binomial reconstruction rows (type_rec = 'zinb': labelled extension, no counterpart in the
// reference): a third head, the dropout logit a (identity activation), pi = sigmoid(a), over the NB term at (m, t):
//   x > 0:  log p = -softplus(a) + logNB(x)              d/da = -pi;   d/da_m, d/da_t: the NB term's
//   x = 0:  log p = log(pi + (1 - pi) e^{L0}),  L0 = logNB(0) = -t log1p(m/t) (nb_term returns exactly that: its pairs are 0)
//           with rho = sigmoid(L0 - a), the NB component's responsibility for the zero:
//           d/da = (1 - rho) (1 - pi) (1 - e^{L0});      d/da_m, d/da_t: rho times the NB term's
// The x = 0 term never adds a vanishing addend to 1: with q = 1 - pi = sigmoid(-a) and z = q (-expm1(L0)) in [0, 1),
//   z <= 1/2: log1p(-z);   else max(u, w) + log1p(exp(-|a - L0|)),  u = -softplus(-a), w = -softplus(a) + L0  (u - w = a - L0)
// and its logit gradient is a product of non-negative factors, never sigmoid(a - L0) - sigmoid(a).  Both sigmoid pairs come
// from ONE exp(-|.|): (1, e) / (1 + e), no 1 - sigmoid.  LIB / shift / s / v: nb_term's, untouched (theta and the logit are
// never scaled)
template <bool LIB>
__device__ __forceinline__ float zinb_term(float shift, float s, float x, float v, float t, float a, float& g_m, float& g_t,
                                           float& g_d) {
    const float L = nb_term<LIB>(shift, s, x, v, t, g_m, g_t);
    const float e = expf(-fabsf(a)), r = 1.f / (1.f + e), l = log1pf(e);
    const float pi = a >= 0.f ? r : e * r, q = a >= 0.f ? e * r : r;
    const float sp = fmaxf(a, 0.f) + l;            // softplus(a); softplus(-a) = sp - a exactly as max(-a, 0) + l
    if (x > 0.f) {
        g_d = -pi;
        return L - sp;
    }
    const float em = -expm1f(L), z = q * em;
    const float d = L - a, ed = expf(-fabsf(d)), rd = 1.f / (1.f + ed);
    const float rho = d >= 0.f ? rd : ed * rd, nrho = d >= 0.f ? ed * rd : rd;
    g_m *= rho, g_t *= rho;
    g_d = nrho * z;
    if (z <= 0.5f) return log1pf(-z);
    const float u = -(fmaxf(-a, 0.f) + l), w = L - sp;
    return fmaxf(u, w) + log1pf(ed);
}

// lane j of a 16-byte quad, read and written (j is uniform in the walks that use them: scalar selects).  quad_at as a chain of
// flat selects: written as one nested conditional inside a function, the compiler turns it into branches on j
__device__ __forceinline__ float quad_at(float4 v, int j) {
    float r = v.w;
    r = j == 2 ? v.z : r, r = j == 1 ? v.y : r, r = j == 0 ? v.x : r;
    return r;
}
__device__ __forceinline__ void quad_put(float4& v, int j, float a) {
    v.x = j == 0 ? a : v.x, v.y = j == 1 ? a : v.y, v.z = j == 2 ? a : v.z, v.w = j == 3 ? a : v.w;
}

// the term of a family by its number of heads: h = the heads' outputs at one gene, g = the gradients w.r.t. their
// pre-activations (rec_term / nb_term / zinb_term: the one definition of each formula).  zinb_term scales two of its gradients
// after the fact; handed the array's elements it compiles to packed pairs and one more vector register in the scalar walk
// (72 -> 73 with LIB: a wave less per SIMD), so it writes scalars that are copied out
template <int HEADS, bool LIB>
__device__ __forceinline__ float count_term(int kind, float shift, float s, float x, const float (&h)[HEADS],
                                            float (&g)[HEADS]) {
    static_assert(HEADS >= 1 && HEADS <= 3);
    if constexpr (HEADS == 1) return rec_term<LIB>(kind, shift, s, x, h[0], g[0]);
    else if constexpr (HEADS == 2) return nb_term<LIB>(shift, s, x, h[0], h[1], g[0], g[1]);
    else {
        float a, b, d;
        const float r = zinb_term<LIB>(shift, s, x, h[0], h[1], h[2], a, b, d);
        g[0] = a, g[1] = b, g[2] = d;
        return r;
    }
}

// The training-side count rows (dv_rec_nll_rows), one workgroup per row: out[r] = sum_g log p(x[xidx[r], g] | heads), with
// coef != NULL also dpre = coef[r] * the gradients w.r.t. the heads' pre-activations.  A row of v holds the HEADS
// post-activation heads back to back, X columns each, and a row of dpre their gradients in the same order:
//   HEADS = 1 (Bernoulli / Poisson, the runtime `kind`): v = [p] or [rate]              dpre = [d/da]
//   HEADS = 2 (negative binomial; `kind` is not read)  : v = [mu | theta]               dpre = [d/da_m | d/da_t]
//   HEADS = 3 (zero-inflated; `kind` is not read)      : v = [mu | theta | RAW logit]   dpre = [d/da_m | d/da_t | d/da_d]
// LIB: the row's size factor first (row_size_factor; the term loops' read of the row then comes from cache).  VEC (X % 4
// == 0, 16-byte aligned rows: the dispatcher checks; HEADS >= 2 only): four genes per thread on 16-byte loads and stores,
// else one gene per thread.  Per-thread partials in index order, the wave sum, the four waves as (p0 + p1) + (p2 + p3)
template <int HEADS, bool VEC, bool LIB>
__global__ __launch_bounds__(256) void count_nll_rows_kernel(int kind, float shift, const float* __restrict__ coef,
                                                             const float* __restrict__ x, int64_t ldx,
                                                             const int32_t* __restrict__ xidx,
                                                             const float* __restrict__ v, int64_t ldv, int M, int X,
                                                             float* __restrict__ out, float* __restrict__ dpre,
                                                             int64_t ldd) {
    static_assert(HEADS > 1 || !VEC, "the one-head kinds have no 16-byte walk");
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x; r < M; r += gridDim.x) {
        const float* xr = x + (int64_t)(xidx ? xidx[r] : r) * ldx;
        const float* vr = v + (int64_t)r * ldv;
        // the gradient row's address: hoisted for two and three heads (formed at the stores, the scalar library-scaled walk of
        // three heads takes 74 VGPRs, not 72: a wave less per SIMD); for one head formed at the store, which spares the
        // gradient-free pass its scalar arithmetic and branch per row
        float* dr = HEADS > 1 && coef ? dpre + (int64_t)r * ldd : nullptr;
        const float c = coef ? coef[r] : 0.f;
        float sz = 1.f;
        if constexpr (LIB) sz = row_size_factor<VEC>(xr, X, part);
        float acc = 0.f;
        if constexpr (VEC) {
            for (int q = threadIdx.x; q < (X >> 2); q += 256) {
                const float4 xv = reinterpret_cast<const float4*>(xr)[q];
                float4 hv[HEADS], gv[HEADS];
#pragma unroll
                for (int k = 0; k < HEADS; ++k) {
                    hv[k] = reinterpret_cast<const float4*>(vr + k * (int64_t)X)[q];
                    gv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                // ONE copy of the term's code, walked four times (j is uniform: scalar selects); four inlined copies
                // interleave their branches' saved masks and run out of scalar registers
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    float h[HEADS], g[HEADS];
#pragma unroll
                    for (int k = 0; k < HEADS; ++k) h[k] = quad_at(hv[k], j);
                    acc += count_term<HEADS, LIB>(kind, shift, sz, quad_at(xv, j), h, g);
                    if (coef) {      // (inside the branch: a pass without gradients does not pay for them)
#pragma unroll
                        for (int k = 0; k < HEADS; ++k) quad_put(gv[k], j, c * g[k]);
                    }
                }
                if (coef) {
#pragma unroll
                    for (int k = 0; k < HEADS; ++k) reinterpret_cast<float4*>(dr + k * (int64_t)X)[q] = gv[k];
                }
            }
        } else {
            for (int i = threadIdx.x; i < X; i += 256) {
                float h[HEADS], g[HEADS];
#pragma unroll
                for (int k = 0; k < HEADS; ++k) h[k] = vr[k * (int64_t)X + i];
                acc += count_term<HEADS, LIB>(kind, shift, sz, xr[i], h, g);
                if (coef) {
                    float* d = HEADS > 1 ? dr : dpre + (int64_t)r * ldd;
#pragma unroll
                    for (int k = 0; k < HEADS; ++k) d[k * (int64_t)X + i] = c * g[k];
                }
            }
        }
        acc = dv_wave_sum_all(acc);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) out[r] = (part[0] + part[1]) + (part[2] + part[3]);
        __syncthreads();
    }
}

// The count rows with a GENE-WISE inverse dispersion (dv_gauss_nll_rows_raw_cs with a count kind; dispersion='gene'): theta is
// one (X,) pre-activation vector shared by all rows, not a head.  A workgroup owns one chunk of up to 1024 genes and one block
// of R rows; a thread owns four genes of the chunk for all of those rows -- one quad on 16-byte loads and stores (VEC: X % 4
// == 0, aligned rows; the dispatcher checks), else the genes tid + 256 j.  It forms its four thetas once, walks the rows in
// ascending order with four theta-gradient accumulators in registers and stores them once, to ws[row block, gene]: no atomics,
// the caller sums the blocks (dv_colsum).  The per-element term is nb_term / zinb_term above, unchanged: ONE copy of its code,
// walked four times (j is uniform; see count_nll_rows_kernel).  The row partial out_part[r, chunk]: per-thread partials in
// index order, the wave sum, the four waves as (p0 + p1) + (p2 + p3).
// theta = softplus(raw) + DV_NB_THETA_SHIFT is formed in double and rounded once: four per thread per launch, and the
// value is then the correctly rounded one a float64 reference can name (the row terms' bounds are stated at the fp32 theta the
// formula receives).
// LIB: 0 = no size factor; 1 = formed here per row (row_size_factor: chunks == 1, the workgroup reads the whole row anyway;
// also stored to `size` when given); 2 = read from `size`, which a launch in front has filled (size_rows_kernel: with more
// than one chunk every chunk would walk the whole target row again).
struct GeneRowsArgs {
    const float* coef; const float* x; int64_t ldx; const int32_t* xidx; const float* mu; const float* logit; int64_t ldp;
    int M, X; float shift; float* out_part; int chunks; float* dmu; float* dlogit; int64_t ldd; const float* theta_raw;
    float* ws; int64_t ldw; float* size; int R;
};

__device__ __forceinline__ float gene_theta(float raw) {
    const double a = (double)raw;
    return (float)(fmax(a, 0.0) + log1p(exp(-fabs(a))) + (double)DV_NB_THETA_SHIFT);
}

template <bool VEC>
__global__ __launch_bounds__(256) void size_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                        const int32_t* __restrict__ xidx, int M, int X,
                                                        float* __restrict__ size) {
    __shared__ float part[4];
    for (int r = blockIdx.x; r < M; r += gridDim.x) {
        const float s = row_size_factor<VEC>(x + (int64_t)(xidx ? xidx[r] : r) * ldx, X, part);
        if (threadIdx.x == 0) size[r] = s;
    }
}

// ... PER NUISANCE CLASS (dispersion='gene-batch'; CLS): theta_raw holds a row of X values per class at stride ldth, and the
// class is the grid's third dimension -- a workgroup owns one chunk, one row block and ONE class k.  It forms its thetas from
// row k, walks its block's rows in ascending order and skips a row of another class (cls[cls_src ? cls_src[r] : r] != k: a
// workgroup-uniform branch in front of every load of the row and of row_size_factor's barriers), and stores its accumulators
// to ws[row block, k X + gene].  One workgroup takes a row, so every out_part / dmu / dlogit / size element has one writer; a
// class outside [0, gridDim.z) is taken by none.  Every summation order is the shared-theta pass's.
struct GeneClsArgs {
    const int32_t* cls; const int32_t* cls_src; int64_t ldth;
};

struct GeneNoCls {};

template <bool ZI, int LIB, bool VEC, bool CLS = false>
__global__ __launch_bounds__(256) void gene_rows_kernel(GeneRowsArgs a, std::conditional_t<CLS, GeneClsArgs, GeneNoCls> cl) {
    __shared__ float part[2][4];
    __shared__ float spart[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const int gbase = chunk * 1024 + (VEC ? 4 * tid : tid);       // gene of slot j: gbase + (VEC ? j : 256 j)
    constexpr int kStep = VEC ? 1 : 256;
    const int r0 = (int)blockIdx.y * a.R, r1 = r0 + a.R < a.M ? r0 + a.R : a.M;
    const bool grad = a.dmu != nullptr;
    const bool quad_on = VEC && gbase < a.X;                      // (X % 4 == 0: a quad is inside or outside as a whole)
    float4 th = make_float4(1.f, 1.f, 1.f, 1.f), tacc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* traw = a.theta_raw;
    if constexpr (CLS) traw += (int64_t)blockIdx.z * cl.ldth;     // the class's row of the table
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = gbase + j * kStep;
        if (g < a.X) quad_put(th, j, gene_theta(traw[g]));
    }
    int taken = 0;                                                // (CLS) rows of this class so far: the slot of `part`
    for (int r = r0; r < r1; ++r) {
        if constexpr (CLS) {
            if (cl.cls[cl.cls_src ? cl.cls_src[r] : r] != (int)blockIdx.z) continue;
        }
        const float* xr = a.x + (int64_t)(a.xidx ? a.xidx[r] : r) * a.ldx;
        const float* mr = a.mu + (int64_t)r * a.ldp;
        const float* lr = ZI ? a.logit + (int64_t)r * a.ldp : nullptr;
        float sz = 1.f;
        if constexpr (LIB == 1) {
            sz = row_size_factor<VEC>(xr, a.X, spart);
            if (a.size != nullptr && tid == 0) a.size[r] = sz;
        } else if constexpr (LIB == 2) {
            sz = a.size[r];
        }
        const float c = grad ? a.coef[r] : 0.f;
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), mv = xv, lv = xv, gmv = xv, gdv = xv;
        if (quad_on) {
            const int q = gbase >> 2;
            xv = reinterpret_cast<const float4*>(xr)[q];
            mv = reinterpret_cast<const float4*>(mr)[q];
            if constexpr (ZI) lv = reinterpret_cast<const float4*>(lr)[q];
        }
        float acc = 0.f;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int g = gbase + j * kStep;
            if (g < a.X) {
                const float xe = VEC ? quad_at(xv, j) : xr[g], ve = VEC ? quad_at(mv, j) : mr[g];
                float gm, gt, gd = 0.f;
                if constexpr (ZI)
                    acc += zinb_term<LIB != 0>(a.shift, sz, xe, ve, quad_at(th, j), VEC ? quad_at(lv, j) : lr[g], gm, gt, gd);
                else
                    acc += nb_term<LIB != 0>(a.shift, sz, xe, ve, quad_at(th, j), gm, gt);
                if (grad) {
                    quad_put(tacc, j, quad_at(tacc, j) + c * gt);
                    if constexpr (VEC) {
                        quad_put(gmv, j, c * gm);
                        if constexpr (ZI) quad_put(gdv, j, c * gd);
                    } else {
                        a.dmu[(int64_t)r * a.ldd + g] = c * gm;
                        if constexpr (ZI) a.dlogit[(int64_t)r * a.ldd + g] = c * gd;
                    }
                }
            }
        }
        if (quad_on && grad) {
            const int q = gbase >> 2;
            reinterpret_cast<float4*>(a.dmu + (int64_t)r * a.ldd)[q] = gmv;
            if constexpr (ZI) reinterpret_cast<float4*>(a.dlogit + (int64_t)r * a.ldd)[q] = gdv;
        }
        acc = dv_wave_sum_all(acc);
        // two slots, taken in turn: the next row's partials land in the other one, so one barrier per row is enough
        // (CLS: in turn over the rows TAKEN -- two taken rows around a skipped one would share a slot of r - r0)
        float* p = part[(CLS ? taken++ : r - r0) & 1];
        if (lane == 0) p[wave] = acc;
        __syncthreads();
        if (tid == 0) a.out_part[(int64_t)r * a.chunks + chunk] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    if (grad) {
        float* w = a.ws + (int64_t)blockIdx.y * a.ldw + (CLS ? (int64_t)blockIdx.z * a.X : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = gbase + j * kStep;
            if (g < a.X) w[g] = quad_at(tacc, j);
        }
    }
}


__global__ void nll_rows_bwd_kernel(const float* __restrict__ coef, const float* __restrict__ x, int64_t ldx,
                                    const int32_t* __restrict__ xidx, const float* __restrict__ mu,
                                    const float* __restrict__ sd, int64_t ldp, int M, int X, int mode, int sd_act,
                                    float sd_shift, float* __restrict__ dmu, float* __restrict__ dsd, int64_t ldd,
                                    float* __restrict__ dx, int64_t lddx, float beta) {
    const int64_t total = (int64_t)M * X;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / X), g = (int)(e % X);
        const float c = coef[r];
        const float xv = x[(int64_t)(xidx ? xidx[r] : r) * ldx + g];
        const float m = mu[(int64_t)r * ldp + g], s = sd[(int64_t)r * ldp + g];
        const float d = xv - m;
        float gm, gs;
        if (mode == DV_GAUSS_SIGMA) {
            const float v = s * s;
            gm = d / v;
            gs = -1.f / s + d * d / (v * s);
        } else {
            const float iv = expf(-s);
            gm = d * iv;
            gs = -0.5f * (1.f - d * d * iv);
        }
        if (sd_act != DV_ACT_IDENTITY) gs *= dv_dact_from_y(sd_act, s - sd_shift);
        const int64_t o = (int64_t)r * ldd + g;
        dmu[o] = (beta != 0.f ? beta * dmu[o] : 0.f) + c * gm;
        dsd[o] = (beta != 0.f ? beta * dsd[o] : 0.f) + c * gs;
        if (dx) {
            const int64_t ox = (int64_t)r * lddx + g;
            dx[ox] = (beta != 0.f ? beta * dx[ox] : 0.f) - c * gm;
        }
    }
}

// ------------------------------------------------------------------- categorical
constexpr float kPMin = 1e-10f;
constexpr float kPMax = 1.f - 1e-10f;   // == 1.0f in fp32, as in the reference's fp32 clamp

// clamp(softmax) of one row from its logits a[0..Y) and their maximum mx
__device__ __forceinline__ void softmax_clamp_row(const float* a, float mx, int Y, float* p) {
    float den = 0.f;
    for (int j = 0; j < Y; ++j) den += expf(a[j] - mx);
    for (int j = 0; j < Y; ++j) p[j] = fminf(fmaxf(expf(a[j] - mx) / den, kPMin), kPMax);
}

// ... and its backward: d logits from (d probs, probs); the clamp passes the gradient only where the unclamped value lies
// inside [1e-10, 1]
__device__ __forceinline__ float softmax_clamp_bwd_dot(const float* g, const float* p, int Y) {
    float dot = 0.f;
    for (int j = 0; j < Y; ++j) dot += (p[j] > kPMin ? g[j] : 0.f) * p[j];
    return dot;
}
__device__ __forceinline__ float softmax_clamp_bwd_elem(const float* g, const float* p, int j, float dot) {
    return p[j] * ((p[j] > kPMin ? g[j] : 0.f) - dot);
}
__device__ __forceinline__ void softmax_clamp_bwd_row(const float* g, const float* p, int Y, float* dl) {
    const float dot = softmax_clamp_bwd_dot(g, p, Y);
    for (int j = 0; j < Y; ++j) dl[j] = softmax_clamp_bwd_elem(g, p, j, dot);
}

__global__ void softmax_clamp_fwd_kernel(const float* __restrict__ logits, int64_t ldl, int M, int Y, int sigmoid1,
                                         float* __restrict__ probs, int64_t ldp) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const float* a = logits + (int64_t)r * ldl;
    float* p = probs + (int64_t)r * ldp;
    if (sigmoid1) {
        const float s = 1.f / (1.f + expf(-a[0]));
        p[0] = fminf(fmaxf(1.f - s, kPMin), kPMax);
        p[1] = fminf(fmaxf(s, kPMin), kPMax);
        return;
    }
    float mx = a[0];
    for (int j = 1; j < Y; ++j) mx = fmaxf(mx, a[j]);
    softmax_clamp_row(a, mx, Y, p);
}

__global__ void softmax_clamp_bwd_kernel(const float* __restrict__ dprobs, int64_t lddp,
                                         const float* __restrict__ probs, int64_t ldp, int M, int Y, int sigmoid1,
                                         float* __restrict__ dlogits, int64_t ldl, float beta) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const float* g = dprobs + (int64_t)r * lddp;
    const float* p = probs + (int64_t)r * ldp;
    float* o = dlogits + (int64_t)r * ldl;
    if (sigmoid1) {      // (the clamp's pass rule of softmax_clamp_bwd_row)
        const float s = p[1], g1 = p[1] > kPMin ? g[1] : 0.f, g0 = p[0] > kPMin ? g[0] : 0.f;
        const float v = (g1 - g0) * s * (1.f - s);
        o[0] = (beta != 0.f ? beta * o[0] : 0.f) + v;
        return;
    }
    const float dot = softmax_clamp_bwd_dot(g, p, Y);
    for (int j = 0; j < Y; ++j) o[j] = (beta != 0.f ? beta * o[j] : 0.f) + softmax_clamp_bwd_elem(g, p, j, dot);
}

__global__ void cat_terms_fwd_kernel(const float* __restrict__ probs, int64_t ldp, int M, int Y,
                                     const int32_t* __restrict__ labels, const float* __restrict__ prior,
                                     int64_t ldpr, float* __restrict__ logp, float* __restrict__ kl, int64_t ldk,
                                     float* __restrict__ ent, int32_t* __restrict__ best) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const float* p = probs + (int64_t)r * ldp;
    if (logp) logp[r] = logf(p[labels[r]]);
    float e = 0.f, bv = p[0];
    int bi = 0;
    for (int j = 0; j < Y; ++j) {
        const float lp = logf(p[j]);
        if (kl) kl[(int64_t)r * ldk + j] = -p[j] * (logf(prior[(int64_t)r * ldpr + j]) - lp);
        e += p[j] * lp;
        if (p[j] > bv) {
            bv = p[j];
            bi = j;
        }
    }
    if (ent) ent[r] = -e;
    if (best) best[r] = bi;
}

__global__ void cat_terms_bwd_kernel(const float* __restrict__ probs, int64_t ldp, int M, int Y,
                                     const int32_t* __restrict__ labels, const float* __restrict__ prior,
                                     int64_t ldpr, const float* __restrict__ c_logp, const float* __restrict__ g_kl,
                                     int64_t ldg, const float* __restrict__ c_ent, float* __restrict__ dprobs,
                                     int64_t lddp, float beta) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const float* p = probs + (int64_t)r * ldp;
    for (int j = 0; j < Y; ++j) {
        const float lp = logf(p[j]);
        float v = 0.f;
        if (c_logp && labels[r] == j) v += c_logp[r] / p[j];
        if (g_kl) v += g_kl[(int64_t)r * ldg + j] * (lp - logf(prior[(int64_t)r * ldpr + j]) + 1.f);
        if (c_ent) v -= c_ent[r] * (lp + 1.f);
        float* o = dprobs + (int64_t)r * lddp + j;
        *o = (beta != 0.f ? beta * *o : 0.f) + v;
    }
}

// ------------------------------------------------- small-N linear head (the classifier)
// q(y|.) = clamp(softmax([a1|a2] W^T + b)) with N = dim_y <= 8 outputs: an MFMA tile would be
// >90 % padding, so one wavefront per row does the N dot products, the softmax and the clamp.
constexpr int kMaxSmallN = 8;

// y-marginalisation of one row from its class probabilities q (src/DrVAE.py:503-534): the labeled / marginalised KLD
// assembly (FWD: yl, kld) and its backward (BWD: the fprop rows' coefficients cfp and the row of dqy).  The one definition
// behind dv_ymarg_fwd / _bwd / _fwdbwd and the rider of the classifier head (dv_smalln_linear_fwd with a dv_ymarg).
// A row with one fprop row is labeled; label <= -2 is a labeled row of a batch-independent ("universal") plan: all Y class
// slots are materialised, the true class -2 - label is the one that counts (see dv_batch_masks).
// (cfp_out != NULL: the coefficients written to y.cfp are also returned, slot by slot; dq_out != NULL: the row of y.dqy)
template <bool FWD, bool BWD>
__device__ __forceinline__ void ymarg_row(const dv_ymarg& y, int r, int Y, const float* q, float* cfp_out = nullptr,
                                          float* dq_out = nullptr) {
    const int f0 = y.fp_ptr[r], nf = y.fp_ptr[r + 1] - f0;
    const float ck = BWD ? y.c_kld[r] : 0.f;
    float* dq = BWD ? y.dqy + (int64_t)r * y.lddq : nullptr;
    const int lab0 = y.label[r];
    if (nf == 1 || lab0 <= -2) {
        const int lab = nf == 1 ? lab0 : -2 - lab0;
        if (FWD) {
            y.yl[r] = logf(q[lab]);
            y.kld[r] = y.klfp[nf == 1 ? f0 : f0 + lab];
        }
        if (!BWD) return;
        for (int j = 0; j < Y; ++j) {
            const float v = (j == lab) ? y.c_yl[r] / q[j] : 0.f;
            dq[j] = v;
            if (dq_out) dq_out[j] = v;
        }
        if (nf == 1) {
            y.cfp[f0] = ck;
            if (cfp_out) cfp_out[0] = ck;
        } else {
            for (int j = 0; j < Y; ++j) {
                y.cfp[f0 + j] = (j == lab) ? ck : 0.f;
                if (cfp_out) cfp_out[j] = (j == lab) ? ck : 0.f;
            }
        }
    } else {
        float a = 0.f, b = 0.f;
        for (int j = 0; j < Y; ++j) {
            const float lp = y.log_prior_v ? y.log_prior_v[j] : y.log_prior, lq = logf(q[j]), kf = y.klfp[f0 + j];
            if (FWD) {
                a += q[j] * kf;
                b += -q[j] * (lp - lq);
            }
            if (BWD) {
                y.cfp[f0 + j] = ck * q[j];
                if (cfp_out) cfp_out[j] = ck * q[j];
                const float v = ck * (kf + lq - lp + 1.f);
                dq[j] = v;
                if (dq_out) dq_out[j] = v;
            }
        }
        if (FWD) {
            y.yl[r] = 0.f;
            y.kld[r] = a + b;
        }
    }
}

// the classifier's data gradient of row r right behind its y-marginalisation (dv_smalln_linear_fwd with a dv_clf_dgrad
// argument): lane 0 holds the row's d logits (softmax_clamp_bwd_row of the dqy / probs it has just stored), the wave writes the
// destinations' columns with the arithmetic of smalln_bwd_data_kernel (no segment start)
__device__ __forceinline__ void smalln_dgrad_row(const dv_clf_dgrad& g, int r, int N, const float* dl0,
                                                 const float* __restrict__ W, int64_t ldw, int lane) {
    float dl[kMaxSmallN];
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) dl[j] = j < N ? __shfl(dl0[j], 0, 64) : 0.f;
    for (int t = 0; t < g.n; ++t) {
        float* o = g.dst[t] + (int64_t)r * g.ld[t];
        for (int c = lane; c < g.ncol[t]; c += 64) {
            float s = 0.f, s2 = 0.f;
            for (int j = 0; j < N; ++j) s += dl[j] * W[(int64_t)j * ldw + g.col0[t] + c];
            if (g.alpha2[t] != 0.f)
                for (int j = 0; j < N; ++j) s2 += dl[j] * W[(int64_t)j * ldw + g.col1[t] + c];
            const float base = g.beta[t] != 0.f ? g.beta[t] * o[c] : 0.f;
            o[c] = base + g.alpha[t] * s + g.alpha2[t] * s2;
        }
    }
}

// the pieces the two classifier-head kernels below share (their load schedules differ, their arithmetic does not)
// one fprop row t from this lane's shares (s1, s3) of its two KL sums: raw1 / raw3 / klfp stored by lane 0; returns raw1,
// the gate of the z1 term's backward
__device__ __forceinline__ float fprop_kl_row(const dv_fprop_kl& kf, int t, float s1, float s3, int lane) {
    s1 = dv_wave_sum_all(s1);
    s3 = dv_wave_sum_all(s3);
    const float raw1 = -0.5f * s1;
    if (lane == 0) {
        kf.raw1[t] = raw1;
        kf.raw3[t] = -0.5f * s3;
        kf.klfp[t] = fmaxf(raw1, kf.kl_min) + fmaxf(-0.5f * s3, kf.kl_min);
    }
    return raw1;
}

// lane 0 of row r behind the wave sums acc[0..N): bias, the logits' store, clamp(softmax) and its store, then the riders --
// the y-marginalisation (cfp: acc is reused for the fprop rows' coefficients) and the row's d logits dl for the data gradient.
// ALL: the launch is known to carry probs, a dv_ymarg and a dv_fprop_kl (smalln_fwd2_kernel's dispatch); else they are looked at
template <bool ALL>
__device__ __forceinline__ void smalln_row_tail(const float* bias, int r, int N, float* acc, float* logits, int64_t ldl,
                                                float* probs, int64_t ldp, const dv_ymarg& ym, bool cfp, bool dgrad,
                                                float* dl) {
    float mx = -3.4e38f;
    for (int j = 0; j < N; ++j) {
        acc[j] += bias ? bias[j] : 0.f;
        if (logits) logits[(int64_t)r * ldl + j] = acc[j];
        mx = fmaxf(mx, acc[j]);
    }
    if (!ALL && !probs) return;
    float q[kMaxSmallN];
    softmax_clamp_row(acc, mx, N, q);
    for (int j = 0; j < N; ++j) probs[(int64_t)r * ldp + j] = q[j];
    if (!ALL && ym.fp_ptr == nullptr) return;
    float dq[kMaxSmallN];
    ymarg_row<true, true>(ym, r, N, q, (ALL || cfp) ? acc : nullptr, dgrad ? dq : nullptr);
    if (dgrad) softmax_clamp_bwd_row(dq, q, N, dl);
}

// backward of fprop row t's z1 term, element d, under the gated coefficient c of the y-marginalisation: dv_kl_rows_bwd's values
__device__ __forceinline__ void fprop_kl_bwd_elem(const dv_fprop_kl& kf, int t, int d, float c, float mq, float sq, float mp,
                                                  float sp) {
    const KlGrad k = kl_grad_logvar(mq, sq, mp, sp);
    float* dq = kf.dq + (int64_t)t * kf.lddq;
    float* dp = kf.dp + (int64_t)t * kf.lddp;
    dq[d] = c * k.gmq;
    dq[kf.Z1 + d] = c * k.gsq;
    dp[d] = c * k.gmp;
    dp[kf.Z1 + d] = c * k.gsp;
}

__global__ __launch_bounds__(256) void smalln_fwd_kernel(const float* __restrict__ a1, int64_t lda1, int K1,
                                                         const float* __restrict__ a2, int64_t lda2, int K2,
                                                         const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ bias, int M, int N,
                                                         float* __restrict__ logits, int64_t ldl,
                                                         float* __restrict__ probs, int64_t ldp, dv_ymarg ym,
                                                         ParkArgs park, dv_fprop_kl kf, dv_clf_dgrad dg) {
    park_block(park);
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    // (fprop rows of this classifier row: their KL terms first -- the y-marginalisation below consumes them)
    float raw1[kMaxSmallN];
    int f0 = 0, nf = 0;
    if (kf.mu_q != nullptr) {
        f0 = ym.fp_ptr[r];
        nf = ym.fp_ptr[r + 1] - f0;
#pragma unroll
        for (int u = 0; u < kMaxSmallN; ++u) {
            if (u >= nf) break;
            const int t = f0 + u;
            const float* q = kf.mu_q + (int64_t)kf.qidx[t] * kf.ldq;
            const float* pp = kf.mu_p + (int64_t)t * kf.ldp;
            const float* q3 = kf.mu3 + (int64_t)t * kf.ld3;
            float s1 = 0.f, s3 = 0.f;
            for (int d = lane; d < kf.Z1; d += 64) s1 += kl_term(DV_GAUSS_LOGVAR, q[d], q[kf.Z1 + d], pp[d], pp[kf.Z1 + d]);
            for (int d = lane; d < kf.Z3; d += 64) s3 += kl_term(DV_GAUSS_LOGVAR, q3[d], q3[kf.Z3 + d], 0.f, 0.f);
            raw1[u] = fprop_kl_row(kf, t, s1, s3, lane);
        }
    }
    float acc[kMaxSmallN], dl[kMaxSmallN];
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) acc[j] = dl[j] = 0.f;
    for (int k = lane; k < K1 + K2; k += 64) {
        const float x = k < K1 ? a1[(int64_t)r * lda1 + k] : a2[(int64_t)r * lda2 + (k - K1)];
#pragma unroll
        for (int j = 0; j < kMaxSmallN; ++j)
            if (j < N) acc[j] += x * W[(int64_t)j * ldw + k];
    }
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) acc[j] = dv_wave_sum_all(acc[j]);
    if (lane == 0) smalln_row_tail<false>(bias, r, N, acc, logits, ldl, probs, ldp, ym, kf.mu_q != nullptr, dg.n != 0, dl);
    if (dg.n) smalln_dgrad_row(dg, r, N, dl, W, ldw, lane);
    if (kf.mu_q != nullptr) {
        // backward of the z1 term with the coefficients of the y-marginalisation (lane 0 holds them): dv_kl_rows_bwd
#pragma unroll
        for (int u = 0; u < kMaxSmallN; ++u) {
            if (u >= nf) break;
            const int t = f0 + u;
            const float c = free_bits_gate(__shfl(acc[u], 0, 64), raw1[u], kf.kl_min);
            const float* q = kf.mu_q + (int64_t)kf.qidx[t] * kf.ldq;
            const float* pp = kf.mu_p + (int64_t)t * kf.ldp;
            for (int d = lane; d < kf.Z1; d += 64) fprop_kl_bwd_elem(kf, t, d, c, q[d], q[kf.Z1 + d], pp[d], pp[kf.Z1 + d]);
        }
    }
}

// The same launch for the train step's common case -- two classes, [z1 | z2F - z1] of <= 256 columns, latent widths <= 128 --
// with every operand in flight before the first result is formed (round 5).  The generic kernel above walks
// [fp_ptr -> qidx -> KL rows -> reduce] per fprop row, then the classifier's operands, then re-reads the KL rows for the
// backward: seven dependent round trips on the side chain's critical path (10.9 us isolated); here three --
// [classifier operands, fp_ptr] -> [qidx] -> [all KL rows] -- and the backward works from registers.  Same summation orders
// (the results agree to the rounding of contracted multiply-adds).  cfg 2: 10.9 -> 8.1 us isolated, and -- the side chain in
// front of the join is the step's critical path -- 0.1906 -> 0.1863 ms per step.
__global__ __launch_bounds__(256) void smalln_fwd2_kernel(const float* __restrict__ a1, int64_t lda1, int K1,
                                                          const float* __restrict__ a2, int64_t lda2, int K2,
                                                          const float* __restrict__ W, int64_t ldw,
                                                          const float* __restrict__ bias, int M, int N,
                                                          float* __restrict__ logits, int64_t ldl,
                                                          float* __restrict__ probs, int64_t ldp, dv_ymarg ym,
                                                          ParkArgs park, dv_fprop_kl kf, dv_clf_dgrad dg) {
    park_block(park);
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int Kt = K1 + K2, Z1 = kf.Z1, Z3 = kf.Z3;
    // ---- round trip 1: the classifier's operands and the row's fprop range
    float xs[4], w0[4], w1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = lane + 64 * c;
        xs[c] = w0[c] = w1[c] = 0.f;
        if (k < Kt) {
            xs[c] = k < K1 ? a1[(int64_t)r * lda1 + k] : a2[(int64_t)r * lda2 + (k - K1)];
            w0[c] = W[k];
            if (N > 1) w1[c] = W[ldw + k];
        }
    }
    const int f0 = ym.fp_ptr[r];
    int nf = ym.fp_ptr[r + 1] - f0;
    nf = nf < 2 ? nf : 2;                       // (one fprop row for a labeled row, one per class otherwise; N <= 2)
    // ---- round trip 2: which q row each fprop row reads
    int qi[2] = {0, 0};
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (u < nf) qi[u] = kf.qidx[f0 + u];
    // ---- round trip 3: the KL rows
    float qm[2][2], ql[2][2], pm[2][2], pl[2][2], tm[2][2], tl[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = lane + 64 * c;
            qm[u][c] = ql[u][c] = pm[u][c] = pl[u][c] = tm[u][c] = tl[u][c] = 0.f;
            if (u < nf) {
                const int t = f0 + u;
                if (d < Z1) {
                    const float* q = kf.mu_q + (int64_t)qi[u] * kf.ldq;
                    const float* pp = kf.mu_p + (int64_t)t * kf.ldp;
                    qm[u][c] = q[d]; ql[u][c] = q[Z1 + d]; pm[u][c] = pp[d]; pl[u][c] = pp[Z1 + d];
                }
                if (d < Z3) {
                    const float* q3 = kf.mu3 + (int64_t)t * kf.ld3;
                    tm[u][c] = q3[d]; tl[u][c] = q3[Z3 + d];
                }
            }
        }
    // ---- the fprop rows' KL terms
    float raw1[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (u >= nf) break;
        float s1 = 0.f, s3 = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (lane + 64 * c < Z1) s1 += kl_term(DV_GAUSS_LOGVAR, qm[u][c], ql[u][c], pm[u][c], pl[u][c]);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (lane + 64 * c < Z3) s3 += kl_term(DV_GAUSS_LOGVAR, tm[u][c], tl[u][c], 0.f, 0.f);
        }
        raw1[u] = fprop_kl_row(kf, f0 + u, s1, s3, lane);
    }
    // ---- the classifier and the y-marginalisation
    float acc[kMaxSmallN], dl[kMaxSmallN];
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) acc[j] = dl[j] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (lane + 64 * c < Kt) {
            acc[0] += xs[c] * w0[c];
            if (N > 1) acc[1] += xs[c] * w1[c];
        }
    acc[0] = dv_wave_sum_all(acc[0]);
    acc[1] = dv_wave_sum_all(acc[1]);
    if (lane == 0) smalln_row_tail<true>(bias, r, N, acc, logits, ldl, probs, ldp, ym, true, dg.n != 0, dl);
    if (dg.n) smalln_dgrad_row(dg, r, N, dl, W, ldw, lane);
    // ---- backward of the z1 term with those coefficients (lane 0 holds them), from the registers
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (u >= nf) break;
        const int t = f0 + u;
        const float c = free_bits_gate(__shfl(acc[u], 0, 64), raw1[u], kf.kl_min);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
            if (lane + 64 * cc < Z1) fprop_kl_bwd_elem(kf, t, lane + 64 * cc, c, qm[u][cc], ql[u][cc], pm[u][cc], pl[u][cc]);
    }
}

struct SmallNDst {
    float* dst[3];
    int64_t ld[3];
    int col0[3], ncol[3];     // columns [col0, col0+ncol) of W feed this destination
    int col1[3];              // optional second column block (alpha2 != 0): `[z1, z2F - z1]` inputs
    float alpha[3], alpha2[3], beta[3];
    int n;
    // destination 0 may start from a segment sum instead of beta*dst: sum of rows [seg_ptr[r], seg_ptr[r+1]) of seg_src
    const float* seg_src;
    int64_t ld_seg;
    const int32_t* seg_ptr;
};

// dst_t[r, c] = beta*dst_t[r, c] + sum_j dlogit[r,j] * (alpha*W[j, col0_t + c] + alpha2*W[j, col1_t + c])
__global__ void smalln_bwd_data_kernel(const float* __restrict__ dprobs, int64_t lddp,
                                       const float* __restrict__ probs, int64_t ldp, int from_probs,
                                       const float* __restrict__ W, int64_t ldw, int M, int N, SmallNDst d) {
    int total_cols = 0;
    for (int t = 0; t < d.n; ++t) total_cols += d.ncol[t];
    const int64_t total = (int64_t)M * total_cols;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / total_cols);
        int c = (int)(e % total_cols), t = 0;
        while (c >= d.ncol[t]) {
            c -= d.ncol[t];
            ++t;
        }
        float dl[kMaxSmallN];
        if (from_probs) {
            softmax_clamp_bwd_row(dprobs + (int64_t)r * lddp, probs + (int64_t)r * ldp, N, dl);
        } else {
            for (int j = 0; j < N; ++j) dl[j] = dprobs[(int64_t)r * lddp + j];
        }
        float s = 0.f, s2 = 0.f;
        for (int j = 0; j < N; ++j) s += dl[j] * W[(int64_t)j * ldw + d.col0[t] + c];
        if (d.alpha2[t] != 0.f)
            for (int j = 0; j < N; ++j) s2 += dl[j] * W[(int64_t)j * ldw + d.col1[t] + c];
        float* o = d.dst[t] + (int64_t)r * d.ld[t] + c;
        float base;
        if (t == 0 && d.seg_src != nullptr) {      // (dv_rows_segment_sum's sum, in its order)
            base = 0.f;
            for (int u = d.seg_ptr[r]; u < d.seg_ptr[r + 1]; ++u) base += d.seg_src[(int64_t)u * d.ld_seg + c];
        } else {
            base = d.beta[t] != 0.f ? d.beta[t] * *o : 0.f;
        }
        *o = base + d.alpha[t] * s + d.alpha2[t] * s2;
    }
}

// dW[j, k] = beta*dW + sum_r dlogit[r,j] * [a1|a2][r,k];  db[j] = beta*db + sum_r dlogit[r,j]
// block = 16 columns x 64 row-groups (1024 threads): every thread walks only M/64 rows, so the
// chain of dependent global loads is short; fixed-order LDS tree over the row-groups (deterministic)
constexpr int kSnCols = 16, kSnRG = 64;
// gridDim.y > 1 (round 5): the rows are split over gridDim.y workgroups per column block -- 26 workgroups of a 256-CU chip
// walked all 4096 rows of the wide configuration's classifier (85-113 us for 6 MB of input) -- each writes its partial
// sums to ws[split][N][KT + 1]; smalln_wgrad_reduce_kernel adds the splits up in a fixed order (deterministic)
__global__ __launch_bounds__(1024) void smalln_bwd_weight_kernel(const float* __restrict__ dprobs, int64_t lddp,
                                                                 const float* __restrict__ probs, int64_t ldp,
                                                                 int from_probs, const float* __restrict__ a1,
                                                                 int64_t lda1, int K1, const float* __restrict__ a2,
                                                                 int64_t lda2, int K2, int M, int N,
                                                                 float* __restrict__ dW, int64_t ldd,
                                                                 float* __restrict__ db, float beta, dv_publish pub,
                                                                 float* __restrict__ ws, int rows_per_split) {
    // (one spare class slot: a row-group stride of 144 floats = 16 banks, so the two row groups of a 32-lane access sit on
    // disjoint banks -- with 128 they shared them: 0.49 LDS bank conflicts per access in the round-5 counters)
    __shared__ float part[kSnRG][kMaxSmallN + 1][kSnCols];
    publish_block0(pub);
    const int c = threadIdx.x % kSnCols, rg = threadIdx.x / kSnCols;
    const int k = blockIdx.x * kSnCols + c, KT = K1 + K2;   // k == KT is the bias column
    const int m0 = blockIdx.y * rows_per_split, m1 = min(M, m0 + rows_per_split);
    float acc[kMaxSmallN];
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) acc[j] = 0.f;
    if (k <= KT && m1 > m0) {
        // four rows per trip with their loads issued together (rows past the end read the last row and are masked out):
        // the kernel is a chain of dependent-load round trips, so fewer trips is what shortens it
        const float* xs = k < K1 ? a1 + k : a2 + (k - K1);
        const int64_t ldx = k < K1 ? lda1 : lda2;
        for (int r0 = m0 + rg; r0 < m1; r0 += 4 * kSnRG) {
            float x[4], dl[4][kMaxSmallN];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + u * kSnRG, rc = r < m1 ? r : m1 - 1;
                x[u] = r < m1 ? (k == KT ? 1.f : xs[(int64_t)rc * ldx]) : 0.f;
                if (from_probs) {
                    softmax_clamp_bwd_row(dprobs + (int64_t)rc * lddp, probs + (int64_t)rc * ldp, N, dl[u]);
                } else {
                    for (int j = 0; j < N; ++j) dl[u][j] = dprobs[(int64_t)rc * lddp + j];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < kMaxSmallN; ++j)
                    if (j < N) acc[j] += dl[u][j] * x[u];
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxSmallN; ++j) part[rg][j][c] = acc[j];
    __syncthreads();
    for (int h = kSnRG / 2; h >= 1; h >>= 1) {
        if (rg < h)
            for (int j = 0; j < N; ++j) part[rg][j][c] += part[rg + h][j][c];
        __syncthreads();
    }
    if (rg == 0 && k <= KT) {
        for (int j = 0; j < N; ++j) {
            if (ws) {
                ws[((int64_t)blockIdx.y * N + j) * (KT + 1) + k] = part[0][j][c];
                continue;
            }
            float* o = k == KT ? (db ? db + j : nullptr) : dW + (int64_t)j * ldd + k;
            if (o) *o = (beta != 0.f ? beta * *o : 0.f) + part[0][j][c];
        }
    }
}

__global__ __launch_bounds__(256) void smalln_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int N, int KT,
                                                                  float* __restrict__ dW, int64_t ldd, float* __restrict__ db,
                                                                  float beta) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * (KT + 1)) return;
    const int j = e / (KT + 1), k = e % (KT + 1);
    float s_ = 0.f;
    for (int t = 0; t < splits; ++t) s_ += ws[((int64_t)t * N + j) * (KT + 1) + k];
    float* o = k == KT ? (db ? db + j : nullptr) : dW + (int64_t)j * ldd + k;
    if (o) *o = (beta != 0.f ? beta * *o : 0.f) + s_;
}

// ------------------------------------------------------------- y-marginalisation
// one thread per row of ymarg_row: forward (dv_ymarg_fwd), backward (dv_ymarg_bwd), or both in one pass (dv_ymarg_fwdbwd: the
// train step, whose coefficients are known); y carries the operands and outputs of the directions asked for
template <bool FWD, bool BWD>
__global__ void ymarg_kernel(const float* __restrict__ qy, int64_t ldq, dv_ymarg y, int R, int Y) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    ymarg_row<FWD, BWD>(y, r, Y, qy + (int64_t)r * ldq);
}

// ------------------------------------------------ regression head (type_y = 'cont')
// q(y|.) = N(mu, var) with mu = sigmoid(.) and a FIXED variance (src/DrVAE.py:167-169).  Per classifier
// row r = (l, i):  labeled -> yl[r] = log N(y_i; mu, var), the fprop input takes the true y;
// unlabeled -> y is sampled (SGVB, src/DrVAE.py:527-529): yv = mu + sd*eps, yl[r] = 0.
// The y columns of the two fprop inputs [z1 | y] and [z3 | y] are written here.
__global__ void ycont_fwd_kernel(const float* __restrict__ mu, int64_t ldm, const float* __restrict__ ylab,
                                 const int32_t* __restrict__ has_y, const float* __restrict__ eps, int64_t lde,
                                 float logvar, int sqerr, int R, int B, int Y, float* __restrict__ yl,
                                 float* __restrict__ fpin_y, int64_t ld1, float* __restrict__ z3in_y, int64_t ld2) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int i = r % B;
    const bool lab = has_y[i] != 0;
    const float sd = expf(0.5f * logvar), iv = expf(-logvar);
    float acc = 0.f;
    for (int d = 0; d < Y; ++d) {
        const float m = mu[(int64_t)r * ldm + d];
        float yv;
        if (lab) {
            yv = ylab[(int64_t)i * Y + d];
            const float df = yv - m;
            acc += sqerr ? 2.f * df * df : kLog2Pi + logvar + df * df * iv;    // (x -0.5 below)
        } else {
            yv = m + sd * eps[(int64_t)r * lde + d];
        }
        fpin_y[(int64_t)r * ld1 + d] = yv;
        z3in_y[(int64_t)r * ld2 + d] = yv;
    }
    yl[r] = lab ? -0.5f * acc : 0.f;
}

// dlogit[r,d] = dmu * mu(1-mu):  labeled dmu = c_yl[r]*(y-mu)/var;  unlabeled dmu = d/d(y columns of
// the two fprop inputs) (the sample is mu + const*eps).  cfp[r] = c_kld[r] (one fprop row per row).
__global__ void ycont_bwd_kernel(const float* __restrict__ mu, int64_t ldm, const float* __restrict__ ylab,
                                 const int32_t* __restrict__ has_y, float logvar, int sqerr,
                                 const float* __restrict__ c_yl, const float* __restrict__ c_kld,
                                 const float* __restrict__ dfpin_y, int64_t ld1,
                                 const float* __restrict__ dz3in_y, int64_t ld2, int R, int B, int Y,
                                 float* __restrict__ dlogit, int64_t ldd, float* __restrict__ cfp, int write_cfp) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int i = r % B;
    const bool lab = has_y[i] != 0;
    const float iv = expf(-logvar);
    if (write_cfp) {
        cfp[r] = c_kld[r];
        return;
    }
    for (int d = 0; d < Y; ++d) {
        const float m = mu[(int64_t)r * ldm + d];
        const float dmu = lab ? c_yl[r] * (ylab[(int64_t)i * Y + d] - m) * (sqerr ? 2.f : iv)
                              : dfpin_y[(int64_t)r * ld1 + d] + dz3in_y[(int64_t)r * ld2 + d];
        dlogit[(int64_t)r * ldd + d] = dmu * m * (1.f - m);
    }
}

// --------------------------------------------------- random-Fourier-feature MMD (K10)
// rf(x)[r] = c * cos(theta[i,r]), theta = a * x W + 2 pi b (the MFMA GEMM writes theta with its scale/bias
// epilogue);  diff[r] = mean_i rf(x1_i)[r] - mean_j rf(x2_j)[r];  mmd2 = sum_r diff[r]^2  (src/blocks.py:40-55).
// One block per 64 features, its 4 waves splitting the rows of theta1 then theta2 (lanes = consecutive r).
__global__ __launch_bounds__(256) void mmd_cos_means_kernel(const float* __restrict__ th1, int64_t ld1, int n1,
                                                            const float* __restrict__ th2, int64_t ld2, int n2, int R,
                                                            float c, float* __restrict__ diff) {
    __shared__ float part[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 64 + lane, rc = r < R ? r : R - 1;
    for (int side = 0; side < 2; ++side) {
        const float* th = side ? th2 : th1;
        const int64_t ld = side ? ld2 : ld1;
        const int n = side ? n2 : n1;
        float acc = 0.f;
        for (int i = wave; i < n; i += 4) acc += cosf(th[(int64_t)i * ld + rc]);
        part[side][wave][lane] = acc;
    }
    __syncthreads();
    if (wave == 0 && r < R) {
        const float s1 = (part[0][0][lane] + part[0][1][lane]) + (part[0][2][lane] + part[0][3][lane]);
        const float s2 = (part[1][0][lane] + part[1][1][lane]) + (part[1][2][lane] + part[1][3][lane]);
        diff[r] = c * (s1 / (float)n1 - s2 / (float)n2);
    }
}

// out[0] = sum_r diff[r]^2  (single block, fixed-order tree: deterministic)
__global__ __launch_bounds__(256) void mmd_sumsq_kernel(const float* __restrict__ diff, int R, float* __restrict__ out) {
    __shared__ float part[4];
    float s = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) s += diff[r] * diff[r];
    s = dv_wave_sum_all(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (part[0] + part[1]) + (part[2] + part[3]);
}

// G[i,r] = coef * gout[0] * (-diff[r]) * sin(theta[i,r])   -- d mmd2 / d theta up to the caller's constant
__global__ void mmd_dtheta_kernel(const float* __restrict__ th, int64_t ld, int n, int R,
                                  const float* __restrict__ diff, const float* __restrict__ gout, float coef,
                                  float* __restrict__ G, int64_t ldg) {
    const int64_t total = (int64_t)n * R;
    const float s = coef * gout[0];
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / R), r = (int)(e % R);
        G[(int64_t)i * ldg + r] = -s * diff[r] * sinf(th[(int64_t)i * ld + r]);
    }
}

// ---------------------------------------------------------------- row movement
__global__ void rows_gather_kernel(const float* __restrict__ src, int64_t lds, const int32_t* __restrict__ idx,
                                   int n, int W, const float* __restrict__ noise, int64_t ldn, float sigma,
                                   const int32_t* __restrict__ onehot_cls, int Y, float* __restrict__ out,
                                   int64_t ldo, ParkArgs park) {
    park_block(park);
    const int WT = W + (onehot_cls ? Y : 0);
    const int64_t total = (int64_t)n * WT;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / WT), d = (int)(e % WT);
        float v;
        if (d < W) {
            v = src[(int64_t)(idx ? idx[r] : r) * lds + d];
            if (noise) v = fmaf(sigma, noise[(int64_t)r * ldn + d], v);
        } else {
            v = (d - W) == onehot_cls[r] ? 1.f : 0.f;
        }
        out[(int64_t)r * ldo + d] = v;
    }
}

// Per-batch masks of a batch-INDEPENDENT ("universal") step plan: the plan materialises every row as a pair with
// every class slot, and which rows really are pairs / labeled is data -- coefficient and weight vectors computed
// here, on the device, from the flags of the batch (src/DrVAE.py:565-624: group split + per-example normalisers
// N_total / max(1, N_pairs) / max(1, N_labeled), with N_pairs and N_labeled counted per batch).  One workgroup.
// Row i of the batch is dataset row table[b, i] (graph-resident epoch feed) or i itself (table == NULL).
struct MaskArgs {
    const int32_t* table;
    int n_batches;
    const int32_t* ctr;
    const int32_t* base;
    const int32_t* hx;
    const int32_t* hy;
    const int32_t* y;
    int B, L, Np;     // Np: rows [0, Np) of the batch have pair slots (the batch-independent plan: Np == B)
    float n_tot, kl_rate, pert_rate, yl_rate;
    const float* beta;
    float* c_nll;     // (3 L B): z1 rows | z2 rows | z2Fz1 rows
    float* c_klz2;    // (L B)
    float* c_yl;      // (L B)
    float* w_recl;    // (2 L B)  weights of RECL over the z1 | z2 rows
    float* w_pert;    // (L B)
    float* w_yl;      // (L B)
    int32_t* label;   // (L B): -2 - class for labeled rows, 0 otherwise (see ymarg_*_kernel)
    float* c_klp;     // (2 B), optional: KL-to-prior rows of q(z1|x1) | q(z2|x2) (PVAE, src/PVAE.py:330-345)
    const int32_t* one_slot;   // (B), optional: rows of the plan with ONE class slot (labeled for sure): label = class
    const int32_t* gcounts;    // (n_batches, 2), optional: GLOBAL (N_pairs, N_labeled) of every batch (data parallelism)
    // annealing schedules (the trailing fields of dv_batch_masks_desc; sched_step == NULL: none, the launch as it ever was)
    const int32_t* sched_step; // the number of finished training iterations, a device scalar
    int pert_itermax, pert_offset, kl_itermax, yl_itermax, yl_offset, lr_itermax;     // itermax <= 0: that schedule is off
    float mmd_rate;
    float* sched;     // (4) the step's record {beta_pert, beta_kl, beta_yr, lr_scale}
    float* c_kld;     // (L B), optional: beta_kl / (L n_tot)
    float* w_klz2;    // (L Np), optional: c_klz2 without beta_kl (the weights of the reported KLD)
    float* w_klp;     // (B + Np), optional: c_klp without beta_kl
    float* w_elbo;    // (3)
    float* w_cmpl;    // (8)
};

// linear annealing coefficient of src/DGMMixin.py:77-89 in double, from the integers: the host's python expression
// operation by operation (one division, one addition, one min), so fp32 of it is the host's value bit for bit
__device__ __forceinline__ double anneal_coef(int it, int itermax, int offset) {
    if (itermax <= 0) return 1.0;
    const int d = it - offset;
    if (d <= 0) return 0.01;
    const double c = 0.01 + (double)d / (double)itermax;
    return c < 1.0 ? c : 1.0;
}

__device__ __forceinline__ void batch_masks_body(const MaskArgs& a) {
    __shared__ int cnt[2];
    __shared__ float sch[4];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool anneal = a.sched_step != nullptr;
    if (anneal && threadIdx.x == blockDim.x - 1) {
        // the step's schedule record: evaluated once, by one thread, from the step counter as this (the step's first) launch
        // reads it; plain stores -- every reader is a later launch.  (The last thread: the first two carry the counts below)
        const int it = a.sched_step[0];
        const double lr_c = 1.0 - anneal_coef(it, a.lr_itermax, 0);
        sch[0] = (float)anneal_coef(it, a.pert_itermax, a.pert_offset);
        sch[1] = (float)anneal_coef(it, a.kl_itermax, 0);
        sch[2] = (float)anneal_coef(it, a.yl_itermax, a.yl_offset);
        sch[3] = a.lr_itermax > 0 ? (float)(lr_c > 0.01 ? lr_c : 0.01) : 1.f;
        for (int k = 0; k < 4; ++k) a.sched[k] = sch[k];
        a.w_elbo[0] = 1.f;
        a.w_elbo[1] = -sch[1];
        a.w_elbo[2] = a.hx ? sch[0] * a.pert_rate : 0.f;
        for (int k = 0; k < 8; ++k) a.w_cmpl[k] = 0.f;
        a.w_cmpl[3] = a.hy ? -(sch[2] * a.yl_rate) : 0.f;
        a.w_cmpl[4] = a.mmd_rate != 0.f ? -a.mmd_rate : 0.f;
        a.w_cmpl[5] = -1.f;
    }
    const int32_t* tb = nullptr;
    int b = 0;
    if (a.table) {
        b = a.ctr[0] - a.base[0];
        b = b < 0 ? 0 : (b >= a.n_batches ? a.n_batches - 1 : b);
        tb = a.table + (int64_t)b * a.B;
    }
    if (a.gcounts) {
        // data parallelism: this rank runs a slice of the global batch; the normalisers are the GLOBAL counts of the batch
        // (table data: every rank drew the same global table), not this slice's own
        if (threadIdx.x < 2) cnt[threadIdx.x] = a.gcounts[2 * b + threadIdx.x];
    } else {
        int np = 0, nl = 0;
        for (int i = threadIdx.x; i < a.B; i += blockDim.x) {
            const int src = tb ? tb[i] : i;
            np += (a.hx && a.hx[src] != 0) ? 1 : 0;
            nl += (a.hy && a.hy[src] != 0) ? 1 : 0;
        }
        // integer counts: order-independent, so atomics keep the step reproducible
        if (np) atomicAdd(&cnt[0], np);
        if (nl) atomicAdd(&cnt[1], nl);
    }
    __syncthreads();
    const float Lf = (float)a.L, beta = anneal ? sch[0] : (a.beta ? a.beta[0] : 1.f);
    const float b_kl = anneal ? sch[1] : 1.f, b_yr = anneal ? sch[2] : 1.f;
    const float n_pairs = cnt[0] > 0 ? (float)cnt[0] : 1.f, n_lab = cnt[1] > 0 ? (float)cnt[1] : 1.f;
    const float c_tot = 1.f / (Lf * a.n_tot);
    const int LB = a.L * a.B, LP = a.L * a.Np;
    // pair slots: slot q = (l, j) belongs to batch row j < Np (rows from Np on have no x2 / z2 rows in this plan:
    // the feed puts the batch's pairs first)
    if (a.c_nll && a.hx)
        for (int q = threadIdx.x; q < LP; q += blockDim.x) {
            const int j = q % a.Np, src = tb ? tb[j] : j;
            const bool px = a.hx[src] != 0;
            a.c_nll[LB + q] = px ? -c_tot : 0.f;
            a.w_recl[LB + q] = px ? c_tot : 0.f;
            a.c_nll[LB + LP + q] = px ? -beta * a.pert_rate / (Lf * n_pairs) : 0.f;
            a.w_pert[q] = px ? 1.f / (Lf * n_pairs) : 0.f;
            const float kz = px ? beta * a.kl_rate * c_tot : 0.f;
            a.c_klz2[q] = anneal ? kz * b_kl : kz;
            if (a.w_klz2) a.w_klz2[q] = kz;
        }
    for (int r = threadIdx.x; r < LB; r += blockDim.x) {
        const int i = r % a.B, src = tb ? tb[i] : i;
        const bool py = a.hy && a.hy[src] != 0;
        if (a.c_nll) {
            a.c_nll[r] = -c_tot;
            a.w_recl[r] = c_tot;
        }
        if (a.hy) {
            const float cy = py ? -a.yl_rate / (Lf * n_lab) : 0.f;
            a.c_yl[r] = anneal ? cy * b_yr : cy;
            a.w_yl[r] = 1.f / (Lf * n_lab);
            a.label[r] = (a.one_slot && a.one_slot[i]) ? a.y[src] : (py ? -2 - a.y[src] : 0);
        }
        if (a.c_kld) a.c_kld[r] = b_kl * c_tot;
    }
    if (a.c_klp)
        for (int i = threadIdx.x; i < a.B; i += blockDim.x) {
            const int src = tb ? tb[i] : i;
            const float k1 = 1.f / a.n_tot, k2 = (a.hx && a.hx[src] != 0) ? 1.f / a.n_tot : 0.f;
            a.c_klp[i] = anneal ? k1 * b_kl : k1;
            if (i < a.Np) a.c_klp[a.B + i] = anneal ? k2 * b_kl : k2;
            if (a.w_klp) {
                a.w_klp[i] = k1;
                if (i < a.Np) a.w_klp[a.B + i] = k2;
            }
        }
}

__global__ __launch_bounds__(1024) void batch_masks_kernel(MaskArgs a) { batch_masks_body(a); }

// Graph-resident input feed: batch `b = ctr - base` of an epoch's index table is gathered from
// the HBM-resident dataset straight into the step's input rows ([x1 rows ; x2 rows of the pairs],
// + training noise), and the label-dependent index buffers of the step are refreshed, in ONE
// launch whose arguments never change -- so the whole epoch is replays of one captured graph.
// SPLIT (dv_batch_feed_desc.xt given: raw-count inputs): the wave that owns row r also writes the RAW row to xt[r,:] -- the
// reconstruction target, without noise -- and the encoder's row becomes T(x) + sigma*noise, T = log1p with `transform` == 1.
// A compile-time variant: the default launch keeps its instruction stream (it heads the step's critical path)
// NORM (`transform` == 3, 'log1p_norm'; a compile-time variant of SPLIT): T(x) = log1p(x / s) with the row's observed size
// factor s = max(sum_g x_g, 1) / X.  The wave sums its SOURCE row first (never xin: the sum is taken before the noise) --
// lane partials in index order, then dv_wave_sum_all, one fixed order on every path -- and divides every element by s (a
// true division: one rounding).  A row of up to 1024 columns already sits in the lane's four 16-byte groups and is summed
// from registers; a wider row is walked twice, the second walk from cache.  Integer counts with a row total below 2^24
// sum exactly in fp32 in ANY order: s is then the ONE correctly rounded quotient that row_size_factor forms in the row
// kernels.  Non-integer input: not guaranteed bit-equal to the decoder's s (the two sums run in different orders)
__device__ __forceinline__ float feed_T(int transform, float x) { return transform ? log1pf(x) : x; }
__device__ __forceinline__ float feed_Tn(float x, float s) { return log1pf(x / s); }
__device__ __forceinline__ float feed_size(float acc, int X) { return fmaxf(dv_wave_sum_all(acc), 1.f) / (float)X; }

// the lane's partial of a row's sum: 16-byte groups q = lane, lane + 64, ... below X4, then scalars from g0 on
__device__ __forceinline__ float feed_row_partial(const float* __restrict__ src, int X4, int g0, int X, int lane) {
    float acc = 0.f;
    for (int q = lane; q < X4; q += 64) {
        const float4 xv = reinterpret_cast<const float4*>(src)[q];
        acc += xv.x, acc += xv.y, acc += xv.z, acc += xv.w;
    }
    for (int g = g0 + lane; g < X; g += 64) acc += src[g];
    return acc;
}

// The feed's label blocks, thread t: the label-dependent index buffers of the step.  ONE text for the dense and the sparse feed,
// expanded in both kernels over their (equally named) arguments -- the dense kernel compiles to the instruction stream it had
#define DV_FEED_LABEL_BLOCKS()                                                                                             \
    const int t = ((int)blockIdx.x - row_blocks) * 256 + threadIdx.x;                                                      \
    if (label_r && t < L * B) {                                                                                            \
        const int i = t % B;                                                                                               \
        label_r[t] = has_y[i] ? y[tb[i]] : 0;                                                                              \
    }                                                                                                                      \
    if (ylab && t < B * Yc) { /* regression targets (type_y='cont'): ylab[i,:] = yf[row of slot i,:] */                    \
        const int i = t / Yc, d = t % Yc;                                                                                  \
        ylab[t] = yf[(int64_t)tb[i] * Yc + d];                                                                             \
    }                                                                                                                      \
    if (fp_cls && t < Mf) {                                                                                                \
        const int cls = fp_lab[t] ? y[tb[fp_i[t]]] : fp_slot[t];                                                           \
        fp_cls[t] = cls;                                                                                                   \
        if (onehot)                                                                                                        \
            for (int c = 0; c < Y; ++c) onehot[(int64_t)t * ldh + c] = c == cls ? 1.f : 0.f;                               \
        if (onehot2) /* (a second copy of the block: the class columns of both fprop inputs) */                            \
            for (int c = 0; c < Y; ++c) onehot2[(int64_t)t * ldh2 + c] = c == cls ? 1.f : 0.f;                             \
    }

template <bool SPLIT, bool NORM>
__global__ __launch_bounds__(256) void batch_feed_kernel(
    const float* __restrict__ x1, int64_t ld1, const float* __restrict__ x2, int64_t ld2,
    const int32_t* __restrict__ y, const int32_t* __restrict__ table, int n_batches,
    const int32_t* __restrict__ ctr, const int32_t* __restrict__ base, int B, const int32_t* __restrict__ pair_rows,
    int Np, int X, const float* __restrict__ noise, int64_t ldn, float sigma, float* __restrict__ xin, int64_t ldo,
    const int32_t* __restrict__ has_y, int L, int32_t* __restrict__ label_r, const int32_t* __restrict__ fp_i,
    const int32_t* __restrict__ fp_lab, const int32_t* __restrict__ fp_slot, int Mf, int32_t* __restrict__ fp_cls,
    float* __restrict__ onehot, int64_t ldh, int Y, int row_blocks, int vec4, const float* __restrict__ yf,
    float* __restrict__ ylab, int Yc, float* __restrict__ onehot2, int64_t ldh2, int mask_block, MaskArgs masks,
    ParkArgs park, float* __restrict__ xt, int64_t ldt, int transform) {
    static_assert(SPLIT || !NORM, "the normalised feed is a variant of the split feed");
    park_block(park);
    if ((int)blockIdx.x == mask_block) {        // (batch-independent plan: the batch's masks ride on this launch)
        batch_masks_body(masks);
        return;
    }
    int b = ctr[0] - base[0];
    b = b < 0 ? 0 : (b >= n_batches ? n_batches - 1 : b);
    const int32_t* tb = table + (int64_t)b * B;
    if ((int)blockIdx.x < row_blocks) {
        const int lane = threadIdx.x & 63;
        const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (r >= B + Np) return;
        const float* src = r < B ? x1 + (int64_t)tb[r] * ld1 : x2 + (int64_t)tb[pair_rows[r - B]] * ld2;
        const float* nz = noise ? noise + (int64_t)r * ldn : nullptr;
        float* dst = xin + (int64_t)r * ldo;
        float* raw = nullptr;
        if constexpr (SPLIT) raw = xt + (int64_t)r * ldt;
        if (vec4) {
            // (a wave per row: four 16-B groups per lane in flight at a time -- a 978-gene row is ONE round trip of loads,
            // not four load -> store iterations; this launch is the head of the step's critical path)
            const int X4 = X >> 2;
            float sz = 1.f;
            if constexpr (NORM) {       // (a row wider than one outer iteration, or narrower than one group: summed by a walk)
                if (X4 > 256 || X4 == 0) sz = feed_size(feed_row_partial(src, X4, X & ~3, X, lane), X);
            }
            for (int q0 = 0; q0 < X4; q0 += 256) {
                float4 v[4], e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + lane + 64 * u, qc = q < X4 ? q : X4 - 1;
                    v[u] = reinterpret_cast<const float4*>(src)[qc];
                    e[u] = nz ? reinterpret_cast<const float4*>(nz)[qc] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if constexpr (NORM) {
                    if (X4 <= 256) {        // (the whole row is in registers: this is the only iteration)
                        float acc = 0.f;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (lane + 64 * u < X4) acc += v[u].x, acc += v[u].y, acc += v[u].z, acc += v[u].w;
                        for (int g = (X & ~3) + lane; g < X; g += 64) acc += src[g];
                        sz = feed_size(acc, X);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + lane + 64 * u;
                    if constexpr (SPLIT) {
                        if (q < X4) reinterpret_cast<float4*>(raw)[q] = v[u];
                        if constexpr (NORM)
                            v[u] = make_float4(feed_Tn(v[u].x, sz), feed_Tn(v[u].y, sz), feed_Tn(v[u].z, sz),
                                               feed_Tn(v[u].w, sz));
                        else
                            v[u] = make_float4(feed_T(transform, v[u].x), feed_T(transform, v[u].y), feed_T(transform, v[u].z),
                                               feed_T(transform, v[u].w));
                    }
                    if (q < X4)
                        reinterpret_cast<float4*>(dst)[q] = make_float4(fmaf(sigma, e[u].x, v[u].x), fmaf(sigma, e[u].y, v[u].y),
                                                                        fmaf(sigma, e[u].z, v[u].z), fmaf(sigma, e[u].w, v[u].w));
                }
            }
            if constexpr (SPLIT) {
                for (int g = (X & ~3) + lane; g < X; g += 64) {
                    const float xv = src[g], tv = NORM ? feed_Tn(xv, sz) : feed_T(transform, xv);
                    raw[g] = xv;
                    dst[g] = nz ? fmaf(sigma, nz[g], tv) : tv;
                }
            } else {
                for (int g = (X & ~3) + lane; g < X; g += 64) dst[g] = nz ? fmaf(sigma, nz[g], src[g]) : src[g];
            }
        } else if constexpr (SPLIT) {
            float sz = 1.f;
            if constexpr (NORM) sz = feed_size(feed_row_partial(src, 0, 0, X, lane), X);
            for (int g = lane; g < X; g += 64) {
                const float xv = src[g], tv = NORM ? feed_Tn(xv, sz) : feed_T(transform, xv);
                raw[g] = xv;
                dst[g] = nz ? fmaf(sigma, nz[g], tv) : tv;
            }
        } else {
            for (int g = lane; g < X; g += 64) dst[g] = nz ? fmaf(sigma, nz[g], src[g]) : src[g];
        }
        return;
    }
    DV_FEED_LABEL_BLOCKS()
}

// Sparse rows (dv_batch_feed_desc.csr1_* / csr2_*): the CSR triples of the two matrices; ptr == NULL: that matrix is dense
struct CsrArgs {
    const int64_t* ptr1;
    const int32_t* idx1;
    const float* val1;
    const int64_t* ptr2;
    const int32_t* idx2;
    const float* val2;
};

constexpr int kCsrChunk = 1024;      // columns a wave stages at a time: the dense kernel's outer iteration (4 x 64 16-byte groups)

// the wave's own LDS writes are ordered before its LDS reads that follow (one wave: no workgroup barrier)
__device__ __forceinline__ void csr_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Columns [c0, c0 + n) of a CSR row into the wave's chunk `st`: zeroes, then the entries [e, end) of the row whose column
// lies below c0 + n -- one contiguous range from the running offset e, the row being sorted.  Returns the offset behind them.
// An entry whose column is outside [c0, c0 + n) is never stored (n <= kCsrChunk, c0 + n <= X): whatever the caller's arrays
// hold, the stores stay inside the chunk.
__device__ __forceinline__ int64_t csr_stage_chunk(float* __restrict__ st, const int32_t* __restrict__ idx,
                                                   const float* __restrict__ val, int64_t e, int64_t end, int c0, int n,
                                                   int lane) {
#pragma unroll
    for (int u = 0; u < 4; ++u) reinterpret_cast<float4*>(st)[lane + 64 * u] = make_float4(0.f, 0.f, 0.f, 0.f);
    while (e < end) {       // (wave-uniform: e and end are)
        const int64_t k = e + lane;
        const bool live = k < end;
        const int64_t off = (live ? (int64_t)idx[k] : 0) - c0;
        const bool below = live && off < n;
        if (below && off >= 0) st[off] = val[k];
        const int took = __popcll(__ballot(below));
        e += took;
        if (took < 64) break;
    }
    return e;
}

// ... and the same columns of a dense row (the other matrix of a launch with one sparse matrix may be dense)
__device__ __forceinline__ void dense_stage_chunk(float* __restrict__ st, const float* __restrict__ src, int c0, int n, int lane) {
    for (int g = lane; g < n; g += 64) st[g] = src[c0 + g];
}

// the lane's partial of a CSR row's total over the columns inside [0, X): entries lane, lane + 64, ... in index order
__device__ __forceinline__ float csr_row_partial(const int32_t* __restrict__ idx, const float* __restrict__ val, int64_t e,
                                                 int64_t end, int X, int lane) {
    float acc = 0.f;
    for (int64_t k = e + lane; k < end; k += 64)
        if ((unsigned)idx[k] < (unsigned)X) acc += val[k];
    return acc;
}

// The feed with one or both matrices held as CSR rows.  Only the way the row's wave obtains the source values differs from
// batch_feed_kernel: chunk by chunk (kCsrChunk columns = the dense kernel's outer iteration) the wave stages the row in its
// own 4 KiB of LDS and reads from there the groups / scalars that kernel loads from HBM; the xt store, the transform, the fmaf
// with the noise and the store pattern are that kernel's, in its order -- the outputs are the bits it writes for the
// densified matrix.  NORM: a row of up to kCsrChunk columns is summed from the staged row in the dense kernel's order (equal bits
// for any values), a wider one from the CSR values (exact for integer counts with a total below 2^24)
template <bool SPLIT, bool NORM>
__global__ __launch_bounds__(256) void batch_feed_csr_kernel(
    const float* __restrict__ x1, int64_t ld1, const float* __restrict__ x2, int64_t ld2,
    const int32_t* __restrict__ y, const int32_t* __restrict__ table, int n_batches,
    const int32_t* __restrict__ ctr, const int32_t* __restrict__ base, int B, const int32_t* __restrict__ pair_rows,
    int Np, int X, const float* __restrict__ noise, int64_t ldn, float sigma, float* __restrict__ xin, int64_t ldo,
    const int32_t* __restrict__ has_y, int L, int32_t* __restrict__ label_r, const int32_t* __restrict__ fp_i,
    const int32_t* __restrict__ fp_lab, const int32_t* __restrict__ fp_slot, int Mf, int32_t* __restrict__ fp_cls,
    float* __restrict__ onehot, int64_t ldh, int Y, int row_blocks, int vec4, const float* __restrict__ yf,
    float* __restrict__ ylab, int Yc, float* __restrict__ onehot2, int64_t ldh2, int mask_block, MaskArgs masks,
    ParkArgs park, float* __restrict__ xt, int64_t ldt, int transform, CsrArgs csr) {
    static_assert(SPLIT || !NORM, "the normalised feed is a variant of the split feed");
    __shared__ __attribute__((aligned(16))) float stage[4][kCsrChunk];
    park_block(park);
    if ((int)blockIdx.x == mask_block) {
        batch_masks_body(masks);
        return;
    }
    int b = ctr[0] - base[0];
    b = b < 0 ? 0 : (b >= n_batches ? n_batches - 1 : b);
    const int32_t* tb = table + (int64_t)b * B;
    if ((int)blockIdx.x < row_blocks) {
        const int lane = threadIdx.x & 63;
        const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (r >= B + Np) return;        // (no workgroup barrier below: a wave may leave alone)
        float* st = stage[threadIdx.x >> 6];
        const bool first = r < B;
        const int64_t row = first ? tb[r] : tb[pair_rows[r - B]];
        // (wave-uniform: this row's matrix is sparse or dense)
        const int64_t* ptr = first ? csr.ptr1 : csr.ptr2;
        const int32_t* idx = first ? csr.idx1 : csr.idx2;
        const float* val = first ? csr.val1 : csr.val2;
        const float* src = ptr ? nullptr : (first ? x1 + row * ld1 : x2 + row * ld2);
        int64_t e = 0, end = 0;
        if (ptr) e = ptr[row], end = ptr[row + 1];
        const float* nz = noise ? noise + (int64_t)r * ldn : nullptr;
        float* dst = xin + (int64_t)r * ldo;
        float* raw = nullptr;
        if constexpr (SPLIT) raw = xt + (int64_t)r * ldt;
        const int X4 = vec4 ? X >> 2 : 0;       // (the scalar path: no groups, every column a scalar of its chunk)
        float sz = 1.f;
        if constexpr (NORM) {       // (a row wider than one chunk: summed in front, from the entries / by the dense kernel's walk)
            if (X > kCsrChunk)
                sz = feed_size(ptr ? csr_row_partial(idx, val, e, end, X, lane) : feed_row_partial(src, X4, X4 << 2, X, lane), X);
        }
        for (int c0 = 0; c0 < X; c0 += kCsrChunk) {
            const int n = X - c0 < kCsrChunk ? X - c0 : kCsrChunk;
            if (ptr)
                e = csr_stage_chunk(st, idx, val, e, end, c0, n, lane);
            else
                dense_stage_chunk(st, src, c0, n, lane);
            csr_wave_sync();
            const int q0 = c0 >> 2;
            if (q0 < X4) {      // this chunk's 16-byte groups: batch_feed_kernel's outer iteration, its loads from the staged chunk
                float4 v[4], e4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + lane + 64 * u, qc = q < X4 ? q : X4 - 1;
                    v[u] = reinterpret_cast<const float4*>(st)[qc - q0];
                    e4[u] = nz ? reinterpret_cast<const float4*>(nz)[qc] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if constexpr (NORM) {
                    if (X <= kCsrChunk) {        // (the whole row is staged: this is the only chunk)
                        float acc = 0.f;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (lane + 64 * u < X4) acc += v[u].x, acc += v[u].y, acc += v[u].z, acc += v[u].w;
                        for (int g = (X & ~3) + lane; g < X; g += 64) acc += st[g];
                        sz = feed_size(acc, X);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + lane + 64 * u;
                    if constexpr (SPLIT) {
                        if (q < X4) reinterpret_cast<float4*>(raw)[q] = v[u];
                        if constexpr (NORM)
                            v[u] = make_float4(feed_Tn(v[u].x, sz), feed_Tn(v[u].y, sz), feed_Tn(v[u].z, sz),
                                               feed_Tn(v[u].w, sz));
                        else
                            v[u] = make_float4(feed_T(transform, v[u].x), feed_T(transform, v[u].y), feed_T(transform, v[u].z),
                                               feed_T(transform, v[u].w));
                    }
                    if (q < X4)
                        reinterpret_cast<float4*>(dst)[q] = make_float4(fmaf(sigma, e4[u].x, v[u].x), fmaf(sigma, e4[u].y, v[u].y),
                                                                        fmaf(sigma, e4[u].z, v[u].z), fmaf(sigma, e4[u].w, v[u].w));
                }
            } else if constexpr (NORM) {
                // (no group in the row: X < 4 on the 16-byte path, or the scalar path -- the dense kernel's scalar walk)
                if (X <= kCsrChunk) {
                    float acc = 0.f;
                    for (int g = lane; g < X; g += 64) acc += st[g];
                    sz = feed_size(acc, X);
                }
            }
            // the chunk's scalars: the columns behind the last group (16-byte path), or every column (scalar path)
            const int g0 = (X4 << 2) > c0 ? (X4 << 2) : c0;
            for (int g = g0 + lane; g < c0 + n; g += 64) {
                const float xv = st[g - c0];
                if constexpr (SPLIT) {
                    const float tv = NORM ? feed_Tn(xv, sz) : feed_T(transform, xv);
                    raw[g] = xv;
                    dst[g] = nz ? fmaf(sigma, nz[g], tv) : tv;
                } else {
                    dst[g] = nz ? fmaf(sigma, nz[g], xv) : xv;
                }
            }
            csr_wave_sync();        // (the next chunk's zeroes come behind this chunk's reads)
        }
        return;
    }
    DV_FEED_LABEL_BLOCKS()
}
#undef DV_FEED_LABEL_BLOCKS

__global__ void rows_segment_sum_kernel(const float* __restrict__ src, int64_t lds,
                                        const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ seg_rows,
                                        const float* __restrict__ w, int n, int W,
                                        const int32_t* __restrict__ dst_idx, float* __restrict__ dst, int64_t ldd,
                                        float beta, ParkArgs park) {
    park_block(park);
    const int64_t total = (int64_t)n * W;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / W), d = (int)(e % W);
        float s = 0.f;
        if (seg_ptr) {
            for (int t = seg_ptr[i]; t < seg_ptr[i + 1]; ++t)
                s += (w ? w[t] : 1.f) * src[(int64_t)(seg_rows ? seg_rows[t] : t) * lds + d];
        } else {
            s = (w ? w[i] : 1.f) * src[(int64_t)(seg_rows ? seg_rows[i] : i) * lds + d];
        }
        float* o = dst + (int64_t)(dst_idx ? dst_idx[i] : i) * ldd + d;
        *o = (beta != 0.f ? beta * *o : 0.f) + s;
    }
}

__global__ __launch_bounds__(256) void weighted_sum_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const int32_t* __restrict__ idx, int n, float scale,
                                                           float* __restrict__ out, float beta) {
    __shared__ float part[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += (w ? w[i] : 1.f) * x[idx ? idx[i] : i];
    s = dv_wave_sum_all(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = (part[0] + part[1]) + (part[2] + part[3]);
        out[0] = (beta != 0.f ? beta * out[0] : 0.f) + scale * s;
    }
}

// ------------------------------------------------ reconstruction metrics (evaluation, N1)
// per row i: [ sum (x-r)^2, mean x, mean r, sum (x-mx)^2, sum (r-mr)^2, sum (x-mx)(r-mr) ]
// two passes over the (cache-hot) row so that the centred sums do not cancel in fp32; the
// per-row Pearson r and the RMSE of src/DGMMixin.py:128-156 follow from these six numbers.
__global__ __launch_bounds__(256) void recon_row_stats_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ r, int64_t ldr, int M, int X,
                                                              float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < M; i += gridDim.x * 4) {
        const float* xr = x + (int64_t)i * ldx;
        const float* rr = r + (int64_t)i * ldr;
        float sx = 0.f, sr = 0.f, sse = 0.f;
        for (int g = lane; g < X; g += 64) {
            const float a = xr[g], b = rr[g];
            sx += a;
            sr += b;
            sse += (a - b) * (a - b);
        }
        sx = dv_wave_sum_all(sx);
        sr = dv_wave_sum_all(sr);
        sse = dv_wave_sum_all(sse);
        const float mx = sx / X, mr = sr / X;
        float cxx = 0.f, crr = 0.f, cxr = 0.f;
        for (int g = lane; g < X; g += 64) {
            const float a = xr[g] - mx, b = rr[g] - mr;
            cxx += a * a;
            crr += b * b;
            cxr += a * b;
        }
        cxx = dv_wave_sum_all(cxx);
        crr = dv_wave_sum_all(crr);
        cxr = dv_wave_sum_all(cxr);
        if (lane == 0) {
            float* o = out + (int64_t)i * 6;
            o[0] = sse; o[1] = mx; o[2] = mr; o[3] = cxx; o[4] = crr; o[5] = cxr;
        }
    }
}

// per column g: sum_i x[i,g] and sum_i x[i,g]^2 (double accumulation) and sum_i (x-r)^2:
// the ingredients of the variance-weighted R^2 (sklearn r2_score, src/DGMMixin.py:137)
constexpr int kCmRG = 16;       // row groups (waves) of a column-moment workgroup
__global__ __launch_bounds__(64 * kCmRG) void col_moments_kernel(const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ r, int64_t ldr, int M, int X,
                                                                 double* __restrict__ out, int rows_per_block,
                                                                 const int32_t* __restrict__ sel,
                                                                 const float* __restrict__ r_bias) {
    // workgroup = (64 columns, one row block): 16 row groups of 64 lanes walk the block's rows, coalesced along the
    // columns; partial sums of the block go to out[blockIdx.y] (the caller adds the blocks up in a fixed order).  Sixteen
    // waves per block, not four: the same waves in flight over a quarter of the blocks -- dv_recon_finalize, ONE
    // workgroup, walks every block's partials (8192 rows: 64 -> 16 blocks, 28 -> 10 us)
    __shared__ double part[kCmRG][3][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int g = blockIdx.x * 64 + c;
    const int i0 = blockIdx.y * rows_per_block, i1 = min(M, i0 + rows_per_block);
    double s1 = 0., s2 = 0., se = 0.;
    if (g < X) {
        const float rb = r_bias ? r_bias[g] : 0.f;      // (r = a raw heads product: its bias is added here)
        for (int ii = i0 + rg; ii < i1; ii += kCmRG) {
            const int i = sel ? sel[ii] : ii;       // (sel: the M rows that count, e.g. the rows with a second profile)
            const double a = x[(int64_t)i * ldx + g], b = r_bias ? r[(int64_t)i * ldr + g] + rb : r[(int64_t)i * ldr + g];
            s1 += a;
            s2 += a * a;
            se += (a - b) * (a - b);
        }
    }
    part[rg][0][c] = s1;
    part[rg][1][c] = s2;
    part[rg][2][c] = se;
    __syncthreads();
    if (rg < 3 && g < X) {          // (wave k adds statistic k up, row groups in order)
        double t = 0.;
#pragma unroll
        for (int q = 0; q < kCmRG; ++q) t += part[q][rg][c];
        out[((int64_t)blockIdx.y * 3 + rg) * X + g] = t;
    }
}

// ---- the perturbation effect's column statistics (dv_draw_desc.fx; include/drvae_hip.h, "THE EFFECT REDUCTION", is the
// specification).  Two finished mean heads a (from z1) and b (from z2) -> per (row block, group, gene) the seven float64
// sufficient statistics of e = log2f(b + c) - log2f(a + c) (mode 0) or b - a (mode 1) over the VALID (finite e) elements.
// A workgroup owns 64 genes x one row block x ONE group (the grid's third dimension, as gene_rows_kernel's class): col_moments'
// 64-column shape, because the partials cost 56 bytes per (block, group, gene) against 8 bytes per (row, gene) read -- 1024-gene
// chunks would need ~256 row blocks to fill the chip at 978 genes and write more than they read.  Inside the workgroup a
// thread holds a QUAD of genes (16 lanes span the 64 genes: a 16-byte load each where the rows allow, four dwords otherwise)
// and one of 16 row slots; a row of another group is skipped in front of its loads.  Both paths add the same numbers in the
// same order: slots ((s0 + s1) + (s2 + s3)) by two xor shuffles, then the four waves ((w0 + w1) + (w2 + w3)) through LDS.
struct EffectArgs {
    const float* a; int64_t lda; const float* b; int64_t ldb; const int32_t* grp; int M, X, R, mode; float delta, c; double* out;
};

template <bool VEC>
__global__ __launch_bounds__(256) void effect_cols_kernel(EffectArgs p) {
    __shared__ double part[4][7][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q4 = 4 * (tid & 15), slot = tid >> 4;
    const int g0 = (int)blockIdx.x * 64 + q4;
    const int k = (int)blockIdx.z;
    const int64_t r0 = (int64_t)blockIdx.y * p.R, r1 = r0 + p.R < p.M ? r0 + p.R : p.M;
    const float nan = __int_as_float(0x7fc00000);
    double se[4], s2[4], sa[4], sb[4];
    int n[4], up[4], dn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        se[j] = s2[j] = sa[j] = sb[j] = 0.;
        n[j] = up[j] = dn[j] = 0;
    }
    if (g0 < p.X) {
        for (int64_t r = r0 + slot; r < r1; r += 16) {
            if ((p.grp ? p.grp[r] : 0) != k) continue;
            const float* ar = p.a + r * p.lda;
            const float* br = p.b + r * p.ldb;
            float av[4], bv[4];
            if constexpr (VEC) {          // (X % 4 == 0: a quad is inside or outside as a whole)
                const float4 x = *reinterpret_cast<const float4*>(ar + g0), y = *reinterpret_cast<const float4*>(br + g0);
                av[0] = x.x; av[1] = x.y; av[2] = x.z; av[3] = x.w;
                bv[0] = y.x; bv[1] = y.y; bv[2] = y.z; bv[3] = y.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {      // (a gene past X: NaN, an invalid element)
                    av[j] = g0 + j < p.X ? ar[g0 + j] : nan;
                    bv[j] = g0 + j < p.X ? br[g0 + j] : nan;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = p.mode == 0 ? log2f(bv[j] + p.c) - log2f(av[j] + p.c) : bv[j] - av[j];
                if (fabsf(e) <= 3.402823466e38f) {      // finite (a NaN compares false)
                    const double ed = (double)e;
                    n[j] += 1;
                    se[j] += ed;
                    s2[j] += ed * ed;
                    up[j] += e > p.delta;
                    dn[j] += e < -p.delta;
                    sa[j] += (double)av[j];
                    sb[j] += (double)bv[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double v[7] = {(double)n[j], se[j], s2[j], (double)up[j], (double)dn[j], sa[j], sb[j]};
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            v[t] += __shfl_xor(v[t], 16, 64);
            v[t] += __shfl_xor(v[t], 32, 64);
            if (lane < 16) part[wave][t][q4 + j] = v[t];
        }
    }
    __syncthreads();
    double* o = p.out + ((int64_t)blockIdx.y * gridDim.z + k) * 7 * p.X;
    for (int i = tid; i < 7 * 64; i += 256) {
        const int t = i >> 6, c = i & 63, g = (int)blockIdx.x * 64 + c;
        if (g < p.X) o[(int64_t)t * p.X + g] = (part[0][t][c] + part[1][t][c]) + (part[2][t][c] + part[3][t][c]);
    }
}

// dv_recon_row_stats + the log-likelihood rows in ONE pass over (x, mu, sd) for rows of up to 1024 columns (whole-set
// evaluation: 978 genes): a wave holds its row in registers (16 columns per lane), the centred second pass costs no
// memory traffic.  Same outputs (and, on the dword path, summation orders) as recon_row_stats_kernel / nll_rows_fwd_kernel.
// RAW: mu / sd are the heads' raw products, finished on the way (mu + bias_mu, softplus(sd + bias_sd) + shift) -- the
// decoder's heads of the inference pass run as a plain product.
constexpr int kRcG = 16;
struct RcArgs {
    const float* x; int64_t ldx; const float* mu; const float* sd; int64_t ldp;
    const float* bias_mu; const float* bias_sd; float shift;
    int M, X;
    float* rows; float* ll;
};

// V2: 8-B loads -- a lane holds the column PAIRS lane + 64 k (even X, 8-B aligned rows); element e of the lane's registers is
// column 2 (lane + 64 (e / 2)) + e % 2
template <bool RAW, bool V2>
__global__ __launch_bounds__(256) void recon_rows_kernel(RcArgs a) {
    const int lane = threadIdx.x & 63;
    const int X = a.X;
    auto col = [lane](int e) { return V2 ? 2 * (lane + 64 * (e >> 1)) + (e & 1) : lane + 64 * e; };
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < a.M; i += gridDim.x * 4) {
        const float* xr = a.x + (int64_t)i * a.ldx;
        const float* mr = a.mu + (int64_t)i * a.ldp;
        const float* sr = a.sd + (int64_t)i * a.ldp;
        float av[kRcG], bv[kRcG], tv[kRcG];
        auto elem = [&](int k, float xv, float m, float sv, float bm, float bs) {
            av[k] = xv;
            if constexpr (RAW) {
                bv[k] = m + bm;
                tv[k] = nll_raw_term(a.shift, xv, m, sv, bm, bs);
            } else {
                bv[k] = m;
                tv[k] = nll_term(DV_GAUSS_SIGMA, xv, m, sv);
            }
        };
#pragma unroll
        for (int k = 0; k < kRcG; ++k) av[k] = bv[k] = tv[k] = 0.f;
        if constexpr (V2) {
#pragma unroll
            for (int k = 0; k < kRcG / 2; ++k) {
                const int c = lane + 64 * k;
                if (2 * c < X) {        // (X even: the pair is whole)
                    const float2 xv = reinterpret_cast<const float2*>(xr)[c];
                    const float2 mv = reinterpret_cast<const float2*>(mr)[c];
                    const float2 sv = reinterpret_cast<const float2*>(sr)[c];
                    float2 bm = make_float2(0.f, 0.f), bs = make_float2(0.f, 0.f);
                    if constexpr (RAW) {
                        bm = reinterpret_cast<const float2*>(a.bias_mu)[c];
                        bs = reinterpret_cast<const float2*>(a.bias_sd)[c];
                    }
                    elem(2 * k, xv.x, mv.x, sv.x, bm.x, bs.x);
                    elem(2 * k + 1, xv.y, mv.y, sv.y, bm.y, bs.y);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRcG; ++k) {
                const int g = lane + 64 * k;
                if (g < X) elem(k, xr[g], mr[g], sr[g], RAW ? a.bias_mu[g] : 0.f, RAW ? a.bias_sd[g] : 0.f);
            }
        }
        float sx = 0.f, sb = 0.f, sse = 0.f, sl = 0.f;
#pragma unroll
        for (int k = 0; k < kRcG; ++k)
            if (col(k) < X) {
                sx += av[k];
                sb += bv[k];
                sse += (av[k] - bv[k]) * (av[k] - bv[k]);
            }
        // (the log-likelihood terms in the order of nll_rows_fwd_kernel's scalar path: four per trip while four fit)
#pragma unroll
        for (int k = 0; k < kRcG; k += 4) {
            if (col(k + 3) < X && col(k) < X) {
                sl += (tv[k] + tv[k + 1]) + (tv[k + 2] + tv[k + 3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (col(k + q) < X) sl += tv[k + q];
            }
        }
        sx = dv_wave_sum_all(sx);
        sb = dv_wave_sum_all(sb);
        sse = dv_wave_sum_all(sse);
        sl = dv_wave_sum_all(sl);
        const float mx = sx / X, mb = sb / X;
        float cxx = 0.f, cbb = 0.f, cxb = 0.f;
#pragma unroll
        for (int k = 0; k < kRcG; ++k)
            if (col(k) < X) {
                const float p = av[k] - mx, q = bv[k] - mb;
                cxx += p * p;
                cbb += q * q;
                cxb += p * q;
            }
        cxx = dv_wave_sum_all(cxx);
        cbb = dv_wave_sum_all(cbb);
        cxb = dv_wave_sum_all(cxb);
        if (lane == 0) {
            float* o = a.rows + (int64_t)i * 6;
            o[0] = sse; o[1] = mx; o[2] = mb; o[3] = cxx; o[4] = cbb; o[5] = cxb;
            if (a.ll) a.ll[i] = -0.5f * sl;
        }
    }
}

// The COUNT kinds of dv_recon_rows (type_rec = 'binary' / 'poisson' / 'nb' / 'zinb'): the six row statistics between the target row
// x and the finished mean r, the kind's log-likelihood row at that mean (rec_term / nb_term / zinb_term above: the one definition
// of each formula, their gradient outputs dead code here) and, optionally, the stored mean -- one workgroup per row like
// count_nll_rows_kernel, any X.  v / t: the POST-activation heads (mean | theta).  DV_REC_ZINB: a row of t holds
// [theta | RAW dropout logit] back to back, X columns each (ldt >= 2X); r is the negative-binomial mean, never (1 - pi) r, so
// the statistics and the stored mean are DV_REC_NEGBIN's and only the term reads the logit.  LIB: r = s v with the
// size factor s of the row xs[i,:] (row_size_factor; xs = the target itself, or ANOTHER matrix: the prediction of x2 is made
// at x1's depth); !LIB: r = v, xs is not read.  Walk 1 forms sum x, sum r, sum (x-r)^2 and the term sum (and stores r), walk
// 2 -- over the cache-hot row -- the centred sums at the means of walk 1, as recon_row_stats_kernel does (counts reach the
// thousands: raw moments would cancel).  The r of the statistics is ONE rounded product (__fmul_rn: never contracted into its
// consumers), so both walks and the stored mean see the same number.  The term forms its own m = s * v inside rec_term /
// nb_term, a plain product the compiler may contract into a neighbour (x log m - s v as one fma): inside the count of
// roundings the row kernels are held to, not necessarily the bits of r.  ro may alias v: every element is read and written by the same
// lane, and walk 2 reads r back from ro when there is one (v holds r then).  Per-thread partials in index order, the wave
// sum, the four waves as (p0 + p1) + (p2 + p3): no atomics, equal bits on every launch.
// VEC (X % 4 == 0, 16-byte aligned rows: the dispatcher checks): 16-byte loads and stores; the term walked one gene at a
// time (#pragma unroll 1: see count_nll_rows_kernel -- four inlined copies of nb_term run out of scalar registers)
struct RcCountArgs {
    const float* x; int64_t ldx; const float* v; int64_t ldv; const float* t; int64_t ldt;
    const float* xs; int64_t ldxs; float* ro; int64_t ldo;
    int M, X;
    float* rows; float* ll;
};

template <int KIND, bool LIB>
__device__ __forceinline__ float rc_count_term(float s, float x, float v, float t, float a, float& r) {
    r = LIB ? __fmul_rn(s, v) : v;
    if constexpr (KIND == DV_REC_ZINB) {
        float gm, gt, gd;
        return zinb_term<LIB>(0.f, s, x, v, t, a, gm, gt, gd);
    } else if constexpr (KIND == DV_REC_NEGBIN) {
        float gm, gt;
        return nb_term<LIB>(0.f, s, x, v, t, gm, gt);
    } else {
        float g;
        return rec_term<LIB>(KIND, 0.f, s, x, v, g);
    }
}

template <int KIND, bool LIB, bool VEC>
__global__ __launch_bounds__(256) void recon_rows_count_kernel(RcCountArgs a) {
    __shared__ float part[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X = a.X;
    constexpr bool ZI = KIND == DV_REC_ZINB, NB = KIND == DV_REC_NEGBIN || ZI;      // (NB: a theta head is read)
    {       // (grid = M workgroups, no row loop: the scalar registers of a loop's bookkeeping are the ones nb_term runs out of)
        const int i = blockIdx.x;
        const float* xr = a.x + (int64_t)i * a.ldx;
        const float* vr = a.v + (int64_t)i * a.ldv;
        const float* tr = NB ? a.t + (int64_t)i * a.ldt : nullptr;
        const float* ar = ZI ? tr + X : nullptr;      // (the logit block behind theta's: 16-byte aligned with it, X % 4 == 0)
        float* ro = a.ro ? a.ro + (int64_t)i * a.ldo : nullptr;
        float sz = 1.f;
        if constexpr (LIB) sz = row_size_factor<VEC>(a.xs + (int64_t)i * a.ldxs, X, &part[0][0]);
        float sx = 0.f, sr = 0.f, sse = 0.f, sl = 0.f;
        if constexpr (VEC) {
            for (int q = threadIdx.x; q < (X >> 2); q += 256) {
                const float4 xv = reinterpret_cast<const float4*>(xr)[q];
                const float4 mv = reinterpret_cast<const float4*>(vr)[q];
                float4 tv = make_float4(1.f, 1.f, 1.f, 1.f), rv = make_float4(0.f, 0.f, 0.f, 0.f);
                float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (NB) tv = reinterpret_cast<const float4*>(tr)[q];
                if constexpr (ZI) av = reinterpret_cast<const float4*>(ar)[q];
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const float xj = quad_at(xv, j), mj = quad_at(mv, j), tj = quad_at(tv, j);
                    float r;
                    sl += rc_count_term<KIND, LIB>(sz, xj, mj, tj, ZI ? quad_at(av, j) : 0.f, r);
                    sx += xj;
                    sr += r;
                    sse += (xj - r) * (xj - r);
                    quad_put(rv, j, r);
                }
                if (ro) reinterpret_cast<float4*>(ro)[q] = rv;
            }
        } else {
            for (int g = threadIdx.x; g < X; g += 256) {
                const float xg = xr[g];
                float r;
                sl += rc_count_term<KIND, LIB>(sz, xg, vr[g], NB ? tr[g] : 1.f, ZI ? ar[g] : 0.f, r);
                sx += xg;
                sr += r;
                sse += (xg - r) * (xg - r);
                if (ro) ro[g] = r;
            }
        }
        sx = dv_wave_sum_all(sx);
        sr = dv_wave_sum_all(sr);
        sse = dv_wave_sum_all(sse);
        sl = dv_wave_sum_all(sl);
        if (lane == 0) part[0][wave] = sx, part[1][wave] = sr, part[2][wave] = sse, part[3][wave] = sl;
        __syncthreads();
        const float mx = ((part[0][0] + part[0][1]) + (part[0][2] + part[0][3])) / X;
        const float mr = ((part[1][0] + part[1][1]) + (part[1][2] + part[1][3])) / X;
        const float tse = (part[2][0] + part[2][1]) + (part[2][2] + part[2][3]);
        const float tl = (part[3][0] + part[3][1]) + (part[3][2] + part[3][3]);
        __syncthreads();
        // walk 2: the centred sums.  r as walk 1 formed it: read back where it was stored (v may hold it by now), else the
        // same one product again
        float cxx = 0.f, crr = 0.f, cxr = 0.f;
        const float* rr = ro ? ro : vr;
        const bool scale = LIB && !ro;
        if constexpr (VEC) {
            for (int q = threadIdx.x; q < (X >> 2); q += 256) {
                const float4 xv = reinterpret_cast<const float4*>(xr)[q];
                float4 rv = reinterpret_cast<const float4*>(rr)[q];
                if (scale) rv.x = __fmul_rn(sz, rv.x), rv.y = __fmul_rn(sz, rv.y), rv.z = __fmul_rn(sz, rv.z), rv.w = __fmul_rn(sz, rv.w);
                const float p0 = xv.x - mx, p1 = xv.y - mx, p2 = xv.z - mx, p3 = xv.w - mx;
                const float q0 = rv.x - mr, q1 = rv.y - mr, q2 = rv.z - mr, q3 = rv.w - mr;
                if constexpr (ZI) {
                    // rows are kind 3's BIT FOR BIT, and which of these sums become fused multiply-adds is the compiler's
                    // choice per instantiation (it pairs two of the three into packed fmas: for every kind-3 instantiation
                    // crr and cxr, p * p a rounded product; left alone it paired cxx and crr here): kind 3's roundings, spelled out
                    cxx = __fadd_rn(cxx, __fmul_rn(p0, p0)), cxx = __fadd_rn(cxx, __fmul_rn(p1, p1));
                    cxx = __fadd_rn(cxx, __fmul_rn(p2, p2)), cxx = __fadd_rn(cxx, __fmul_rn(p3, p3));
                    crr = __fmaf_rn(q0, q0, crr), crr = __fmaf_rn(q1, q1, crr), crr = __fmaf_rn(q2, q2, crr), crr = __fmaf_rn(q3, q3, crr);
                    cxr = __fmaf_rn(p0, q0, cxr), cxr = __fmaf_rn(p1, q1, cxr), cxr = __fmaf_rn(p2, q2, cxr), cxr = __fmaf_rn(p3, q3, cxr);
                } else {
                    cxx += p0 * p0, cxx += p1 * p1, cxx += p2 * p2, cxx += p3 * p3;
                    crr += q0 * q0, crr += q1 * q1, crr += q2 * q2, crr += q3 * q3;
                    cxr += p0 * q0, cxr += p1 * q1, cxr += p2 * q2, cxr += p3 * q3;
                }
            }
        } else {
            for (int g = threadIdx.x; g < X; g += 256) {
                const float r = scale ? __fmul_rn(sz, rr[g]) : rr[g];
                const float p = xr[g] - mx, q = r - mr;
                cxx += p * p;
                crr += q * q;
                cxr += p * q;
            }
        }
        cxx = dv_wave_sum_all(cxx);
        crr = dv_wave_sum_all(crr);
        cxr = dv_wave_sum_all(cxr);
        if (lane == 0) part[0][wave] = cxx, part[1][wave] = crr, part[2][wave] = cxr;
        __syncthreads();
        if (threadIdx.x == 0) {
            float* o = a.rows + (int64_t)i * 6;
            o[0] = tse; o[1] = mx; o[2] = mr;
            o[3] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
            o[4] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
            o[5] = (part[2][0] + part[2][1]) + (part[2][2] + part[2][3]);
            if (a.ll) a.ll[i] = tl;
        }
    }
}

// ------------------------------------------------------------------ kernel-mixture MMD (src/blocks.py:29-38,59-76; round 5)
// mmd_objective(kernel = 'rbf' | 'poly'): mean_ij k(a_i, b_j) with k = 1/nb sum_b f(., gamma_b) over three Gram products
// (x1 x1^T, x2 x2^T, x1 x2^T: dv_gemm).  The element-wise mixture, its mean and its derivative were library element-wise
// chains (pow / exp per bandwidth, five times over); here one row pass each way.
//   poly: f = (gamma G_ij + 1)^2                     (degree 2, bias 1: what mmd_objective calls, src/blocks.py:34-35,70-74)
//   rbf : f = exp(-gamma (|a_i|^2 + |b_j|^2 - 2 G_ij))   (the Gram form of src/blocks.py:29-32's intent)
// |a_i|^2 = the diagonal of a a^T: sa[i * sa_stride], no pass of its own.
struct MixArgs {
    const float* G; int64_t ldg; int M, N, kind, nb; float gam[8];
    const float* sa; int64_t sa_stride; const float* sb; int64_t sb_stride;
};

__device__ __forceinline__ float mix_val(const MixArgs& a, float g, float d2, float& dv) {
    float v = 0.f;
    dv = 0.f;
    for (int b = 0; b < a.nb; ++b) {
        const float gm = a.gam[b];
        if (a.kind == 0) {
            const float t = fmaf(gm, g, 1.f);
            v += t * t;
            dv += 2.f * gm * t;             // d/dG
        } else {
            const float e = __expf(-gm * d2);
            v += e;
            dv -= gm * e;                   // d/d(d2)
        }
    }
    const float inv = 1.f / (float)a.nb;
    dv *= inv;
    return v * inv;
}

// part[i] = sum_j k_ij (fwd) | W[i, j] = c * dk_ij, rs[i] = sum_j W[i, j] (bwd; c = coef * gout[0]); one workgroup per row
template <bool BWD>
__global__ __launch_bounds__(256) void mmd_mix_kernel(MixArgs a, float* __restrict__ part, const float* __restrict__ gout,
                                                      float coef, float* __restrict__ W, int64_t ldw, float* __restrict__ rs) {
    __shared__ float red[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* g = a.G + (int64_t)i * a.ldg;
    const float sai = a.kind ? a.sa[(int64_t)i * a.sa_stride] : 0.f;
    const float c = BWD ? coef * gout[0] : 0.f;
    float acc = 0.f;
    for (int j = threadIdx.x; j < a.N; j += 256) {
        const float gij = g[j];
        const float d2 = a.kind ? fmaxf(sai + a.sb[(int64_t)j * a.sb_stride] - 2.f * gij, 0.f) : 0.f;
        float dv;
        const float v = mix_val(a, gij, d2, dv);
        if (BWD) {
            const float w = c * dv;
            W[(int64_t)i * ldw + j] = w;
            acc += w;
        } else {
            acc += v;
        }
    }
    acc = dv_wave_sum_all(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) (BWD ? rs : part)[i] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = m11 - 2 m12 + m22 (the MMD^2), out[1..3] = the three means; fixed summation order, one thread
__global__ void mmd_mix_combine_kernel(const float* p11, int n11, float c11, const float* p12, int n12, float c12,
                                       const float* p22, int n22, float c22, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s11 = 0., s12 = 0., s22 = 0.;
    for (int i = 0; i < n11; ++i) s11 += p11[i];
    for (int i = 0; i < n12; ++i) s12 += p12[i];
    for (int i = 0; i < n22; ++i) s22 += p22[i];
    const double m11 = s11 / c11, m12 = s12 / c12, m22 = s22 / c22;
    out[0] = (float)(m11 - 2. * m12 + m22);
    out[1] = (float)m11;
    out[2] = (float)m12;
    out[3] = (float)m22;
}

// identity kernel (src/blocks.py:37-38): out[0] = || mean(x1, 0) - mean(x2, 0) ||^2, diff[d] = the difference of the means
__global__ __launch_bounds__(256) void mmd_identity_fwd_kernel(const float* __restrict__ x1, int64_t ld1, int n1,
                                                               const float* __restrict__ x2, int64_t ld2, int n2, int Z,
                                                               float* __restrict__ diff, float* __restrict__ out) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc = 0.f;
    for (int d = threadIdx.x; d < Z; d += 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < n1; ++i) s1 += x1[(int64_t)i * ld1 + d];
        for (int i = 0; i < n2; ++i) s2 += x2[(int64_t)i * ld2 + d];
        const float df = s1 / (float)n1 - s2 / (float)n2;
        diff[d] = df;
        acc += df * df;
    }
    acc = dv_wave_sum_all(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dx[i, d] = coef * gout[0] * diff[d]     (d ||diff||^2 / d x1[i, d] = 2 diff[d] / n1: coef = +-2 / n)
__global__ void mmd_identity_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ gout, float coef, int n,
                                        int Z, float* __restrict__ dx, int64_t ldd) {
    const int64_t total = (int64_t)n * Z;
    const float c = coef * gout[0];
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        dx[(e / Z) * ldd + (e % Z)] = c * diff[e % Z];
}

// ------------------------------------------------------------------ evaluation tail (round 5)
// What follows the big kernels of a whole-set evaluation (src/DGMMixin.py:128-190) used to be ~75 small library launches
// per evaluation (two sorts, scans, gathers, float64 element-wise chains); as three launches:
//   recon_finalize : the float64 combination of dv_recon_row_stats / dv_col_moments / the log-likelihood rows
//   pair_counts    : per labeled row i and class: how many rows (positives) score above / equal -- O(n^2) integer
//                    counting over the chip instead of a sort (n <= 32768: 8192 rows = 67 M pairs = a few us)
//   rank_finalize  : accuracy, ROC-AUC and average precision from those counts
// ROC-AUC = sum over negatives j of (#pos above j + 1/2 #pos tied with j) / (n_pos n_neg)  -- the trapezoids over the
// distinct thresholds, sklearn's roc_auc_score; integer arithmetic, exact.  AP = 1/n_pos sum over positives i of
// (#pos >= s_i) / (#all >= s_i) -- sklearn's average_precision_score (one threshold per distinct score).

// out[0..3] = rmse, variance-weighted R^2, mean per-row Pearson r, mean log-likelihood (float64); rows: (M_all, 6) of
// dv_recon_row_stats; sel (n rows, optional): the rows that count; cols: (row_blocks, 3, X) partials of dv_col_moments
// over the same rows; ll (per row, optional).  One workgroup, fixed summation order.
__global__ __launch_bounds__(1024) void recon_finalize_kernel(const float* __restrict__ rows, const int32_t* __restrict__ sel,
                                                              int n, int X, const double* __restrict__ cols, int row_blocks,
                                                              const float* __restrict__ ll, double* __restrict__ out) {
    __shared__ double red[5][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sse = 0., pr = 0., sl = 0., num = 0., den = 0.;
    for (int e = threadIdx.x; e < n; e += 1024) {
        const int i = sel ? sel[e] : e;
        const float* o = rows + (int64_t)i * 6;
        sse += (double)o[0];
        pr += (double)o[5] / sqrt((double)o[3] * (double)o[4]);
        if (ll) sl += (double)ll[i];
    }
    for (int g = threadIdx.x; g < X; g += 1024) {
        double c0 = 0., c1 = 0., c2 = 0.;
        for (int b = 0; b < row_blocks; ++b) {
            const double* c = cols + (int64_t)b * 3 * X;
            c0 += c[g];
            c1 += c[X + g];
            c2 += c[2 * (int64_t)X + g];
        }
        num += c2;
        den += c1 - c0 * c0 / (double)n;
    }
    double v[5] = {sse, pr, sl, num, den};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double t = v[k];
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) red[k][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[5];
        for (int k = 0; k < 5; ++k) {
            t[k] = 0.;
            for (int w = 0; w < 16; ++w) t[k] += red[k][w];
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        out[0] = n ? sqrt(t[0] / ((double)n * X)) : nan;
        out[1] = 1.0 - t[3] / t[4];
        out[2] = n ? t[1] / n : nan;
        out[3] = (ll && n) ? t[2] / n : nan;
    }
}

// out[0..2] = rmse, R^2, Pearson r (float64) of a continuous target over the n selected rows x Y columns, both arrays
// flattened (src/DGMMixin.py:181-188).  TWO passes -- the means, then the centred sums: the one-pass moment formula
// cancels for targets clustered in (0,1).  One workgroup; every thread walks its elements in a fixed order, the waves
// and then the 16 wave sums are added in a fixed order: two calls give the same bits.
__global__ __launch_bounds__(1024) void reg_metrics_kernel(const float* __restrict__ pred, int64_t ldp,
                                                           const float* __restrict__ y, int64_t ldy,
                                                           const int32_t* __restrict__ sel, int n, int Y,
                                                           double* __restrict__ out) {
    __shared__ double red[4][16];
    __shared__ double mean[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)n * Y;
    double sy = 0., sp = 0.;
    for (int64_t e = threadIdx.x; e < total; e += 1024) {
        const int r = (int)(e / Y), c = (int)(e - (int64_t)r * Y);
        const int64_t i = sel ? sel[r] : r;
        sy += (double)y[i * ldy + c];
        sp += (double)pred[i * ldp + c];
    }
    for (int off = 32; off >= 1; off >>= 1) {
        sy += __shfl_xor(sy, off);
        sp += __shfl_xor(sp, off);
    }
    if (lane == 0) {
        red[0][wave] = sy;
        red[1][wave] = sp;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.;
        for (int w = 0; w < 16; ++w) t += red[threadIdx.x][w];
        mean[threadIdx.x] = t / (double)total;
    }
    __syncthreads();
    const double my = mean[0], mp = mean[1];
    double v[4] = {0., 0., 0., 0.};      // sum (y-p)^2, sum yc^2, sum pc^2, sum yc pc
    for (int64_t e = threadIdx.x; e < total; e += 1024) {
        const int r = (int)(e / Y), c = (int)(e - (int64_t)r * Y);
        const int64_t i = sel ? sel[r] : r;
        const double yv = (double)y[i * ldy + c], pv = (double)pred[i * ldp + c];
        const double d = yv - pv, yc = yv - my, pc = pv - mp;
        v[0] += d * d;
        v[1] += yc * yc;
        v[2] += pc * pc;
        v[3] += yc * pc;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double t = v[k];
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) red[k][wave] = t;     // (the means were read out of ``mean`` behind the barrier above)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4];
        for (int k = 0; k < 4; ++k) {
            t[k] = 0.;
            for (int w = 0; w < 16; ++w) t[k] += red[k][w];
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const double den = sqrt(t[1] * t[2]);
        out[0] = total ? sqrt(t[0] / (double)total) : nan;
        out[1] = t[1] > 0. ? 1.0 - t[0] / t[1] : nan;
        out[2] = den > 0. ? t[3] / den : nan;
    }
}

// counts[c][e][0..3] += { rows scoring above e, rows tied with e (e itself included), positives above, positives tied }
// over the j-range of this workgroup; e, j index the selected rows; class c scores proba[row, c0 + c]
constexpr int kPairJ = 512;
__global__ __launch_bounds__(256) void pair_counts_kernel(const float* __restrict__ proba, int64_t ldp,
                                                          const int32_t* __restrict__ y, const int32_t* __restrict__ sel,
                                                          int n, int c0, int binary, int32_t* __restrict__ counts) {
    __shared__ float sj[kPairJ];
    __shared__ int pj[kPairJ];
    const int cls = c0 + blockIdx.z;
    const int j0 = blockIdx.y * kPairJ, j1 = min(n, j0 + kPairJ);
    for (int t = threadIdx.x; t < j1 - j0; t += 256) {
        const int row = sel ? sel[j0 + t] : j0 + t;
        sj[t] = proba[(int64_t)row * ldp + cls];
        pj[t] = binary ? (y[row] > 0) : (y[row] == cls);
    }
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float si = proba[(int64_t)(sel ? sel[e] : e) * ldp + cls];
    int ga = 0, ea = 0, gp = 0, ep = 0;
    for (int t = 0; t < j1 - j0; ++t) {
        const float v = sj[t];
        const int p = pj[t];
        const int g = v > si, q = v == si;
        ga += g; ea += q; gp += g & p; ep += q & p;
    }
    int32_t* o = counts + ((int64_t)blockIdx.z * n + e) * 4;
    // (integer atomics: order-independent, the result is reproducible)
    atomicAdd(o + 0, ga); atomicAdd(o + 1, ea); atomicAdd(o + 2, gp); atomicAdd(o + 3, ep);
}

// per class c (one workgroup each): out[c*2 + 0] = ROC-AUC, out[c*2 + 1] = average precision (nan / 0 for the degenerate
// cases like metrics.roc_auc / average_precision); class 0's workgroup also writes acc -> out[2*n_cls] (nan without pred).  Zeroes the
// counts it has read: the buffer is ready for the next evaluation.
__global__ __launch_bounds__(1024) void rank_finalize_kernel(int32_t* __restrict__ counts, const int32_t* __restrict__ y,
                                                             const int32_t* __restrict__ pred, const int32_t* __restrict__ sel,
                                                             int n, int c0, int binary, int n_cls, double* __restrict__ out) {
    __shared__ double red[16];
    __shared__ long long redi[3][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x, cls = c0 + c;
    long long s2 = 0, npos = 0, hit = 0;
    double ap = 0.;
    for (int e = threadIdx.x; e < n; e += 1024) {
        const int row = sel ? sel[e] : e;
        int32_t* o = counts + ((int64_t)c * n + e) * 4;
        const int ga = o[0], ea = o[1], gp = o[2], ep = o[3];
        o[0] = o[1] = o[2] = o[3] = 0;
        const int p = binary ? (y[row] > 0) : (y[row] == cls);
        if (p) {
            npos += 1;
            ap += (double)(gp + ep) / (double)(ga + ea);
        } else {
            s2 += 2LL * gp + ep;
        }
        if (pred) hit += pred[row] == y[row];
    }
    long long vi[3] = {s2, npos, hit};
    for (int off = 32; off >= 1; off >>= 1) ap += __shfl_xor(ap, off);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off >= 1; off >>= 1) vi[k] += __shfl_xor(vi[k], off);
    if (lane == 0) {
        red[wave] = ap;
        for (int k = 0; k < 3; ++k) redi[k][wave] = vi[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.;
        long long t[3] = {0, 0, 0};
        for (int w = 0; w < 16; ++w) {
            a += red[w];
            for (int k = 0; k < 3; ++k) t[k] += redi[k][w];
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const long long np = t[1], nn = (long long)n - np;
        out[2 * c + 0] = (n == 0 || np == 0 || nn == 0) ? nan : ((double)t[0] * 0.5) / ((double)np * (double)nn);
        out[2 * c + 1] = (n == 0 || np == 0) ? 0.0 : a / (double)np;
        // (no prediction given is not "0 % correct": nan, like no rows)
        if (c == 0) out[2 * n_cls] = (n && pred) ? (double)((float)t[2] / (float)n) : nan;
    }
}

// ---------------------------------------------------------------------- BatchNorm1d / Dropout (blocks.MLP options)
// nn.BatchNorm1d(affine=True) over the rows of x (M, N) (src/blocks.py:137-149): one workgroup per 64 columns,
// 4 row groups; training: batch mean and biased variance (two passes: mean, then sum of squared deviations), the
// running statistics move by `momentum` (running_var takes the UNBIASED variance, like torch); eval: the running
// statistics.  mean / rstd of the batch are kept for the backward pass.
__global__ __launch_bounds__(256) void bn_fwd_kernel(const float* __restrict__ x, int64_t ldx, int M, int N,
                                                     const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     float* __restrict__ y, int64_t ldy, float* __restrict__ rmean,
                                                     float* __restrict__ rvar, float momentum, int training) {
    __shared__ float part[4][64];
    __shared__ float stat[2][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int g = blockIdx.x * 64 + c;
    const bool ok = g < N;
    if (training) {
        float s = 0.f;
        if (ok)
            for (int i = rg; i < M; i += 4) s += x[(int64_t)i * ldx + g];
        part[rg][c] = s;
        __syncthreads();
        if (rg == 0) stat[0][c] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (float)M;
        __syncthreads();
        const float mu = stat[0][c];
        float q = 0.f;
        if (ok)
            for (int i = rg; i < M; i += 4) {
                const float d = x[(int64_t)i * ldx + g] - mu;
                q += d * d;
            }
        __syncthreads();
        part[rg][c] = q;
        __syncthreads();
        if (rg == 0) {
            const float var = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (float)M;
            stat[1][c] = 1.f / sqrtf(var + eps);
            if (ok) {
                mean_out[g] = mu;
                rstd_out[g] = stat[1][c];
                if (rmean) rmean[g] = (1.f - momentum) * rmean[g] + momentum * mu;
                if (rvar) rvar[g] = (1.f - momentum) * rvar[g] + momentum * (M > 1 ? var * (float)M / (float)(M - 1) : var);
            }
        }
        __syncthreads();
    } else {
        if (rg == 0) {
            stat[0][c] = ok ? rmean[g] : 0.f;
            stat[1][c] = ok ? 1.f / sqrtf(rvar[g] + eps) : 0.f;
            if (ok) {
                mean_out[g] = stat[0][c];
                rstd_out[g] = stat[1][c];
            }
        }
        __syncthreads();
    }
    if (ok) {
        const float mu = stat[0][c], rs = stat[1][c], ww = w ? w[g] : 1.f, bb = b ? b[g] : 0.f;
        for (int i = rg; i < M; i += 4) y[(int64_t)i * ldy + g] = (x[(int64_t)i * ldx + g] - mu) * rs * ww + bb;
    }
}

// backward: dw = sum dy*xhat, db = sum dy; training: dx = w*rstd*(dy - db/M - xhat*dw/M); eval: dx = dy*w*rstd
__global__ __launch_bounds__(256) void bn_bwd_kernel(const float* __restrict__ dy, int64_t ldd, const float* __restrict__ x,
                                                     int64_t ldx, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ w, int M,
                                                     int N, float* __restrict__ dx, int64_t lddx, float* __restrict__ dw,
                                                     float* __restrict__ db, int training) {
    __shared__ float p1[4][64], p2[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int g = blockIdx.x * 64 + c;
    const bool ok = g < N;
    const float mu = ok ? mean[g] : 0.f, rs = ok ? rstd[g] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    if (ok)
        for (int i = rg; i < M; i += 4) {
            const float d = dy[(int64_t)i * ldd + g];
            s1 += d;
            s2 += d * ((x[(int64_t)i * ldx + g] - mu) * rs);
        }
    p1[rg][c] = s1;
    p2[rg][c] = s2;
    __syncthreads();
    const float sd = (p1[0][c] + p1[1][c]) + (p1[2][c] + p1[3][c]);
    const float sx = (p2[0][c] + p2[1][c]) + (p2[2][c] + p2[3][c]);
    if (!ok) return;
    if (rg == 0) {
        if (dw) dw[g] = sx;
        if (db) db[g] = sd;
    }
    if (dx == nullptr) return;
    const float ww = w ? w[g] : 1.f, im = 1.f / (float)M;
    for (int i = rg; i < M; i += 4) {
        const float d = dy[(int64_t)i * ldd + g];
        const float xh = (x[(int64_t)i * ldx + g] - mu) * rs;
        dx[(int64_t)i * lddx + g] = training ? ww * rs * (d - sd * im - xh * sx * im) : d * ww * rs;
    }
}

// y = x * mask * scale (nn.Dropout forward with its keep mask, and its backward: the same map on dy)
__global__ void mask_scale_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ mask, int64_t ldm,
                                  float scale, int M, int N, float* __restrict__ y, int64_t ldy) {
    const int64_t total = (int64_t)M * N;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / N, j = e - i * N;
        y[i * ldy + j] = x[i * ldx + j] * mask[i * ldm + j] * scale;
    }
}

struct LossTerms {
    dv_loss_term t[DV_MAX_LOSS_TERMS];
    int n;
};

// all loss scalars of a step in ONE single-workgroup launch: loss[out] += scale * sum_i w[i]*x[i]
// per term, then ELBO = <w_elbo, loss[0:3]>, CMPL = <w_cmpl, loss[0:8]>  (src/DrVAE.py:611-624)
constexpr int kLossThreads = 1024;
__global__ __launch_bounds__(kLossThreads) void loss_assemble_kernel(LossTerms lt, const float* __restrict__ w_elbo,
                                                            const float* __restrict__ w_cmpl,
                                                            float* __restrict__ loss, int32_t* flag,
                                                            const int32_t* ctr, int add, int32_t* err, int max_spins,
                                                            CounterBump bump, const int32_t* __restrict__ halt,
                                                            int n_halt, float* __restrict__ accum) {
    __shared__ float part[DV_MAX_LOSS_TERMS][kLossThreads / 64];
    __shared__ float acc[8];
    if (flag != nullptr) {      // park until the other launch chain has published its results
        if (threadIdx.x == 0) {
            const int want = ctr[0] + add;
            const long long t0 = wall_clock64();
            int n = 0;
            while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - want < 0) {
                __builtin_amdgcn_s_sleep(4);
                if (++n > max_spins) {
                    atomicExch(err, 1);
                    break;
                }
            }
            atomicAdd(err + 1, (int32_t)(wall_clock64() - t0));
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every wave acquires (see park_block)
    }
    // every term's per-thread partial sum first -- all loads of all terms are independent and in flight together
    // (this is ONE workgroup: its time is the number of dependent load round trips) -- then one reduction stage;
    // fixed order throughout
    // (the weights and the running sums thread 0 combines at the end travel together with the terms' loads)
    float we[3] = {0.f, 0.f, 0.f}, wc[8], ac[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wc[i] = ac[i] = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) we[i] = w_elbo[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) wc[i] = w_cmpl[i];
        if (accum != nullptr) {
#pragma unroll
            for (int i = 0; i < 8; ++i) ac[i] = accum[i];
        }
    }
    float ps[DV_MAX_LOSS_TERMS];
#pragma unroll
    for (int k = 0; k < DV_MAX_LOSS_TERMS; ++k) {
        ps[k] = 0.f;
        if (k >= lt.n) continue;
        const dv_loss_term t = lt.t[k];
        if (t.w == nullptr && t.n >= 4 * kLossThreads && (reinterpret_cast<uintptr_t>(t.x) & 15) == 0) {
            // long unweighted terms (per-tile partial sums of dv_gemm_heads): 16-B loads, four per trip
            const float4* x4 = reinterpret_cast<const float4*>(t.x);
            const int n4 = t.n >> 2;
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
            int i = threadIdx.x;
            for (; i + 3 * kLossThreads < n4; i += 4 * kLossThreads) {
                const float4 v0 = x4[i], v1 = x4[i + kLossThreads], v2 = x4[i + 2 * kLossThreads],
                             v3 = x4[i + 3 * kLossThreads];
                a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
                a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
                a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
                a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
            }
            for (; i < n4; i += kLossThreads) {
                const float4 v0 = x4[i];
                a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
            }
            float q = ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w)) +
                      (((a2.x + a2.y) + (a2.z + a2.w)) + ((a3.x + a3.y) + (a3.z + a3.w)));
            for (int j = (n4 << 2) + threadIdx.x; j < t.n; j += kLossThreads) q += t.x[j];
            ps[k] = q;
        } else {
            float q = 0.f;
            const int rl = t.row_len > 1 ? t.row_len : 1;     // x is (rows, row_len): one weight per ROW
            if (rl == 1) {
                for (int i = threadIdx.x; i < t.n; i += kLossThreads) q += (t.w ? t.w[i] : 1.f) * t.x[i];
            } else if (t.w != nullptr) {
                // one thread per ROW: its weight once, its row_len partials as independent loads (the element loop
                // below pays an integer division and a dependent weight load per element: 38 trips per thread for the
                // 620 x 62 per-tile partials of a bucketed sampler plan)
                const int rows = t.n / rl;
                for (int r = threadIdx.x; r < rows; r += kLossThreads) {
                    const float* xr = t.x + (int64_t)r * rl;
                    // (sixteen loads per trip: this is one workgroup, its time is the number of dependent round trips --
                    // the 62 per-tile partials of a row in four trips instead of sixteen)
                    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                    int j = 0;
                    for (; j + 15 < rl; j += 16) {
                        float v[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) v[u] = xr[j + u];
                        s0 += (v[0] + v[4]) + (v[8] + v[12]);
                        s1 += (v[1] + v[5]) + (v[9] + v[13]);
                        s2 += (v[2] + v[6]) + (v[10] + v[14]);
                        s3 += (v[3] + v[7]) + (v[11] + v[15]);
                    }
                    for (; j + 3 < rl; j += 4) {
                        s0 += xr[j];
                        s1 += xr[j + 1];
                        s2 += xr[j + 2];
                        s3 += xr[j + 3];
                    }
                    for (; j < rl; ++j) s0 += xr[j];
                    q += t.w[r] * ((s0 + s1) + (s2 + s3));
                }
            } else {
                for (int i = threadIdx.x; i < t.n; i += kLossThreads) q += t.x[i];
            }
            ps[k] = q;
        }
    }
#pragma unroll
    for (int k = 0; k < DV_MAX_LOSS_TERMS; ++k) {
        if (k >= lt.n) continue;
        const float q = dv_wave_sum_all(ps[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int k = 0; k < lt.n; ++k) {
            float q = 0.f;
            for (int w = 0; w < kLossThreads / 64; ++w) q += part[k][w];
            acc[lt.t[k].out] += lt.t[k].scale * q;
        }
    }
    if (threadIdx.x == 0) {
        if (!(flag != nullptr && lt.n == 0)) {     // (parked variant without terms: only the wait and the counters)
            acc[5] = we[0] * acc[0] + we[1] * acc[1] + we[2] * acc[2];
            float c = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) c += wc[i] * acc[i];
            acc[6] = c;
            // a device-side wait of this step's chains has timed out at some point (sticky error words):
            // whatever was computed since is built on stale data -- poison the scalars the host reads
            bool bad = false;
            for (int i = 0; i < n_halt; ++i)
                bad = bad || __hip_atomic_load(halt + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            for (int i = 0; i < 8; ++i) loss[i] = bad ? __builtin_nanf("") : acc[i];
            // running sums of a training epoch (only the launch that assembled the scalars adds them: the parked
            // variant without terms of the dual-graph step must not add a second time)
            if (accum != nullptr) {
#pragma unroll
                for (int i = 0; i < 8; ++i) accum[i] = ac[i] + (bad ? __builtin_nanf("") : acc[i]);
            }
        }
        // end of the step's use of the device counters on this chain: advance them here (saves the
        // separate counter launch in front of the optimiser)
        bump_counters(bump);
    }
}

__global__ void axpby_kernel(const float* __restrict__ x, float a, float* __restrict__ y, float b, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = a * x[i] + (b != 0.f ? b * y[i] : 0.f);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define ST(s) static_cast<hipStream_t>(s)

static bool park_ok(const dv_wait* p) { return p == nullptr || p->flag == nullptr || (p->ctr && p->err && p->max_spins > 0); }
static bool bump_ok(const dv_bump* b) {
    return b == nullptr || ((!b->c[0] || b->n[0] == 1 || b->n[0] == 2) && (!b->c[1] || b->n[1] == 1 || b->n[1] == 2));
}

// an entry point's optional dv_wait, for its launch of `grid` workgroups (0: it launches nothing): *park = the wait, or none.
// DV_ERR_ARG: a malformed wait, or one without a launch to ride on.  DV_ERR_UNSUPPORTED: every workgroup of a parked launch
// polls -- such grids stay far below what the chip holds resident (256 CUs x 8 workgroups), or the chain that is to publish
// may find no slot to run in
static int take_park(const dv_wait* in, int64_t grid, ParkArgs* park) {
    DV_REQUIRE(park_ok(in));
    *park = in ? *in : ParkArgs{};
    if (park->flag == nullptr) return DV_OK;
    DV_REQUIRE(grid > 0);
    return grid > DV_MAX_PARKED_GRID ? DV_ERR_UNSUPPORTED : DV_OK;
}

extern "C" int dv_colsum(const float* X, int64_t ldx, int32_t M, int32_t N, float* out, float beta,
                         dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 0);
    if (N == 0) return DV_OK;
    DV_REQUIRE(X && out);
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, ST(stream), X, ldx, M, N, out, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_act_bwd(float* dY, int64_t ldd, const float* Y, int64_t ldy, int32_t M, int32_t N, int32_t split,
                          int32_t act0, int32_t act1, float shift0, float shift1, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return DV_OK;
    DV_REQUIRE(dY && Y);
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for((int64_t)M * N, 256)), dim3(256), 0, ST(stream), dY, ldd, Y,
                       ldy, M, N, split, act0, act1, shift0, shift1);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_wn_scale(const float* W, int64_t ldw, const float* g, int32_t N, int32_t K, float* scale,
                           float* norm, dv_stream_t stream) {
    DV_REQUIRE(N >= 0 && K >= 0);
    if (N == 0) return DV_OK;
    DV_REQUIRE(W && g && scale);
    hipLaunchKernelGGL(wn_scale_kernel, dim3((N + 3) / 4), dim3(256), 0, ST(stream), W, ldw, g, N, K, scale, norm);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_wn_bwd(const float* dWraw, int64_t ldr, const float* W, int64_t ldw, const float* g,
                         const float* norm, int32_t N, int32_t K, float* dW, int64_t ldd, float* dg, float beta,
                         dv_stream_t stream) {
    DV_REQUIRE(N >= 0 && K >= 0);
    if (N == 0) return DV_OK;
    DV_REQUIRE(dWraw && W && g && norm && dW && dg);
    hipLaunchKernelGGL(wn_bwd_kernel, dim3((N + 3) / 4), dim3(256), 0, ST(stream), dWraw, ldr, W, ldw, g, norm, N,
                       K, dW, ldd, dg, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_reparam_fwd(const float* mu, const float* sd, int64_t ldq, const int32_t* src_idx, int32_t n,
                              int32_t reps, int32_t Z, const float* eps, int64_t lde, int32_t mode, float* out,
                              int64_t ldo, const float* sub, int64_t lds, float* out2, int64_t ldo2, float* out3,
                              int64_t ldo3, const int32_t* out3_idx, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && reps >= 0 && Z >= 0);
    if (n == 0 || reps == 0 || Z == 0) return DV_OK;
    DV_REQUIRE(mu && sd && eps && out);
    DV_REQUIRE(out2 == nullptr || sub != nullptr);
    DV_REQUIRE(out3 == nullptr || out3_idx != nullptr);
    hipLaunchKernelGGL(reparam_fwd_kernel, dim3(grid_for((int64_t)n * reps * Z, 256)), dim3(256), 0, ST(stream), mu,
                       sd, ldq, src_idx, n, reps, Z, eps, lde, mode, out, ldo, sub, lds, out2, ldo2, out3, ldo3,
                       out3_idx);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_reparam_bwd(const float* dz, int64_t ldz, const float* eps, int64_t lde, const float* sd,
                              int64_t ldq, const int32_t* src_idx, int32_t n, int32_t reps, int32_t Z, int32_t mode,
                              float* dmu, float* dsd, int64_t lddq, float beta, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && reps >= 0 && Z >= 0);
    if (n == 0 || Z == 0) return DV_OK;
    DV_REQUIRE(dz && eps && sd && dmu && dsd);
    hipLaunchKernelGGL(reparam_bwd_kernel, dim3(grid_for((int64_t)n * Z, 256)), dim3(256), 0, ST(stream), dz, ldz,
                       eps, lde, sd, ldq, src_idx, n, reps, Z, mode, dmu, dsd, lddq, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_reparam_bwd_seg(const float* dz, int64_t ldz, const float* eps, int64_t lde, const float* sd,
                                  int64_t ldq, const int32_t* seg_ptr, const int32_t* seg_rows, int32_t nq,
                                  int32_t Z, int32_t mode, const float* extra, int64_t ldx, const int32_t* ex_ptr,
                                  const int32_t* ex_rows, float* dmu, float* dsd, int64_t lddq, float beta,
                                  const dv_bump* bump_in, const dv_seg_add* add, const dv_wait* park_in,
                                  const dv_prior_kl* prior, dv_stream_t stream) {
    DV_REQUIRE(bump_ok(bump_in));
    DV_REQUIRE(prior == nullptr || prior->coef == nullptr || (prior->raw && prior->mu && mode == DV_GAUSS_LOGVAR));
    const dv_prior_kl pk = prior ? *prior : dv_prior_kl{};
    const CounterBump bump = bump_in ? *bump_in : CounterBump{};
    DV_REQUIRE(nq >= 0 && Z >= 0);
    DV_REQUIRE(!(bump.c[0] || bump.c[1]) || (nq > 0 && Z > 0));      // a bump (like a wait) needs a launch to ride on
    DV_REQUIRE(add == nullptr || add->n == 0 || (add->dz && add->n > 0));
    ParkArgs park;
    if (int rc = take_park(park_in, nq > 0 && Z > 0 ? grid_for((int64_t)nq * Z, 256) : 0, &park)) return rc;
    if (nq == 0 || Z == 0) return DV_OK;
    DV_REQUIRE(dz && eps && sd && seg_ptr && seg_rows && dmu && dsd);
    DV_REQUIRE(extra == nullptr || (ex_ptr && ex_rows));
    hipLaunchKernelGGL(reparam_bwd_seg_kernel, dim3(grid_for((int64_t)nq * Z, 256)), dim3(256), 0, ST(stream), dz,
                       ldz, eps, lde, sd, ldq, seg_ptr, seg_rows, nq, Z, mode, extra, ldx, ex_ptr, ex_rows, dmu, dsd,
                       lddq, beta, bump, add ? add->dz : nullptr, add ? add->ld : 0, add ? add->n : 0, park, pk);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_z2f_post_bwd(const dv_z2f_desc* dsc, const dv_wait* park_in, dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr);
    const dv_z2f_desc& d = *dsc;
    DV_REQUIRE(d.L >= 0 && d.B >= 0 && d.Np >= 0 && d.Z >= 0);
    ParkArgs park;
    if (int rc = take_park(park_in, d.L > 0 && d.B > 0 && d.Z > 0 ? grid_for(d.B, 4) : 0, &park)) return rc;
    if (d.L == 0 || d.B == 0 || d.Z == 0) return DV_OK;
    DV_REQUIRE(d.eps && d.p2 && d.dp2 && d.dz1);   // dz2f == NULL: nothing flows into the z2Fz1 samples from a classifier
    DV_REQUIRE((d.kl_out == nullptr) == (d.raw_out == nullptr));
    DV_REQUIRE(d.Np == 0 || (d.pair_slot && d.q2 && d.coef && (d.raw || d.raw_out)));
    DV_REQUIRE((d.prior_coef == nullptr) == (d.prior_raw == nullptr));
    DV_REQUIRE((d.seg_src == nullptr) == (d.seg_ptr == nullptr));
    Z2FArgs a{d.dz2f, d.ld_dz2f, d.dzdec_pert, d.ld_pert, d.Np ? d.pair_slot : nullptr, d.eps, d.lde, d.p2, d.ldp2,
              d.q2, d.ldq2, d.coef, d.raw, d.kl_min, d.dz1b, d.ld_dz1b, d.dp2, d.ld_dp2, d.dz1, d.ld_dz1, d.dq2,
              d.ld_dq2, d.L, d.B, d.Np, d.Z, d.Np ? d.prior_coef : nullptr, d.Np ? d.prior_raw : nullptr,
              d.Np ? d.kl_out : nullptr, d.Np ? d.raw_out : nullptr, d.seg_src, d.ld_seg, d.seg_ptr, d.seg_beta,
              d.dz2f ? d.z1_dz2f : 0.f};
    if (d.Z <= 128)
        hipLaunchKernelGGL(z2f_post_bwd_kernel, dim3(grid_for(d.B, 4)), dim3(256), 0, ST(stream), a, park);
    else
        hipLaunchKernelGGL(z2f_post_bwd_wide_kernel, dim3(grid_for(d.B, 4)), dim3(256), 0, ST(stream), a, park);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_kl_rows_fwd(const dv_kl_rows_desc* dsc, const dv_wait* park_in, dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr);
    const dv_kl_rows_desc& d = *dsc;
    DV_REQUIRE(d.n >= 0 && d.reps >= 0 && d.Z >= 0);
    DV_REQUIRE((d.mu2 == nullptr) == (d.sd2 == nullptr) && (d.mu2 == nullptr || d.Z2 >= 0));
    ParkArgs park;
    if (int rc = take_park(park_in, d.n > 0 && d.reps > 0 ? grid_for((int64_t)d.n * d.reps, 4) : 0, &park)) return rc;
    if (d.n == 0 || d.reps == 0) return DV_OK;
    DV_REQUIRE(d.mu_q && d.sd_q && d.out);
    DV_REQUIRE((d.mu_p == nullptr) == (d.sd_p == nullptr));
    DV_REQUIRE(d.zout == nullptr || d.eps != nullptr);
    KlArgs a{d.mu_q, d.sd_q, d.ldq, d.qidx, d.mu_p, d.sd_p, d.ldp, d.pidx, d.prior_mu, d.prior_sd, d.n, d.reps, d.Z, d.mode};
    hipLaunchKernelGGL(kl_rows_fwd_kernel, dim3(grid_for((int64_t)d.n * d.reps, 4)), dim3(256), 0, ST(stream), a,
                       d.free_bits, d.kl_min, d.raw_out, d.out, d.add, d.eps, d.lde, d.zout, d.ldz, park, d.mu2, d.sd2,
                       d.ld2, d.Z2, d.raw2_out);
    DV_RETURN_LAUNCH();
}

static int kl_fwd_of(const dv_kl_rows_desc& d, KlFwd& f) {
    DV_REQUIRE(d.n >= 0 && d.reps >= 0 && d.Z >= 0 && d.mu_q && d.sd_q && d.out);
    DV_REQUIRE((d.mu_p == nullptr) == (d.sd_p == nullptr));
    DV_REQUIRE(d.zout == nullptr && d.eps == nullptr && d.mu2 == nullptr && d.sd2 == nullptr);   // (plain rows only)
    f = KlFwd{KlArgs{d.mu_q, d.sd_q, d.ldq, d.qidx, d.mu_p, d.sd_p, d.ldp, d.pidx, d.prior_mu, d.prior_sd, d.n, d.reps, d.Z,
                     d.mode},
              d.free_bits, d.kl_min, d.raw_out, d.out, d.add};
    return DV_OK;
}

extern "C" int dv_kl_rows_fwd_pair(const dv_kl_rows_desc* d1, const dv_kl_rows_desc* d2, dv_stream_t stream) {
    DV_REQUIRE(d1 != nullptr && d2 != nullptr);
    KlFwd a, b;
    int rc = kl_fwd_of(*d1, a);
    if (rc != DV_OK) return rc;
    rc = kl_fwd_of(*d2, b);
    if (rc != DV_OK) return rc;
    const int64_t ba = ((int64_t)d1->n * d1->reps + 3) / 4, bb = ((int64_t)d2->n * d2->reps + 3) / 4;
    if (ba + bb == 0) return DV_OK;
    if (ba + bb > 0x7fffffff) return DV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kl_rows_fwd_pair_kernel, dim3((unsigned)(ba + bb)), dim3(256), 0, ST(stream), a, b, (int)ba);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_kl_rows_bwd(const dv_kl_rows_desc* dsc, const dv_kl_rows_grad* grad, dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr && grad != nullptr);
    const dv_kl_rows_desc& d = *dsc;
    const dv_kl_rows_grad& g = *grad;
    DV_REQUIRE(d.n >= 0 && d.reps >= 0 && d.Z >= 0);
    if (d.n == 0 || d.reps == 0 || d.Z == 0) return DV_OK;
    DV_REQUIRE(g.coef && d.mu_q && d.sd_q && g.dq_mu && g.dq_sd);
    DV_REQUIRE(!d.free_bits || d.raw_out != nullptr);
    DV_REQUIRE((d.mu_p == nullptr) == (d.sd_p == nullptr));
    DV_REQUIRE((g.dp_mu == nullptr) == (g.dp_sd == nullptr));
    DV_REQUIRE(g.dp_mu == nullptr || d.mu_p != nullptr);
    DV_REQUIRE(g.dz == nullptr || d.eps != nullptr);
    KlArgs a{d.mu_q, d.sd_q, d.ldq, d.qidx, d.mu_p, d.sd_p, d.ldp, d.pidx, d.prior_mu, d.prior_sd, d.n, d.reps, d.Z, d.mode};
    hipLaunchKernelGGL(kl_rows_bwd_kernel, dim3(grid_for((int64_t)d.n * d.reps * d.Z, 256)), dim3(256), 0, ST(stream), a,
                       g.coef, (const float*)d.raw_out, d.free_bits, d.kl_min, g.dq_mu, g.dq_sd, g.lddq, g.dp_mu, g.dp_sd,
                       g.lddp, g.beta, g.dz, g.ldz, d.eps, d.lde);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_gauss_nll_rows_fwd(const float* x, int64_t ldx, const int32_t* xidx, const float* mu,
                                     const float* sd, int64_t ldp, int32_t M, int32_t X, int32_t mode, float* out,
                                     const float* bias_mu, const float* bias_sd, float sd_shift, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 0);
    if (M == 0) return DV_OK;
    DV_REQUIRE(x && mu && sd && out && ((bias_mu == nullptr) == (bias_sd == nullptr)));
    DV_REQUIRE(bias_mu == nullptr || mode == DV_GAUSS_SIGMA);      // (raw heads: the sigma head = softplus + shift)
    const bool v4 = aligned16(x) && aligned16(mu) && aligned16(sd) && (ldx % 4 == 0) && (ldp % 4 == 0);
    auto a8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    const bool v2 = a8(x) && a8(mu) && a8(sd) && (ldx % 2 == 0) && (ldp % 2 == 0) && (!bias_mu || (a8(bias_mu) && a8(bias_sd)));
    const dim3 grid(grid_for(M, 4, 8192)), block(256);
#define DV_NLL_FWD(VEC, RAW)                                                                                             \
    hipLaunchKernelGGL((nll_rows_fwd_kernel<VEC, RAW>), grid, block, 0, ST(stream), x, ldx, xidx, mu, sd, ldp, M, X, mode, \
                       out, bias_mu, bias_sd, sd_shift)
    if (bias_mu) {
        if (v4) DV_NLL_FWD(4, true);
        else if (v2) DV_NLL_FWD(2, true);
        else DV_NLL_FWD(1, true);
    } else {
        if (v4) DV_NLL_FWD(4, false);
        else if (v2) DV_NLL_FWD(2, false);
        else DV_NLL_FWD(1, false);
    }
#undef DV_NLL_FWD
    DV_RETURN_LAUNCH();
}

extern "C" int dv_gauss_nll_rows_fwdbwd(const float* coef, const float* x, int64_t ldx, const int32_t* xidx,
                                        const float* mu, const float* sd, int64_t ldp, int32_t M, int32_t X,
                                        int32_t mode, int32_t sd_act, float sd_shift, float* out, float* dmu,
                                        float* dsd, int64_t ldd, const float* bias_mu, const float* bias_sd,
                                        dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 0);
    if (M == 0) return DV_OK;
    DV_REQUIRE(coef && x && mu && sd && out && dmu && dsd && ((bias_mu == nullptr) == (bias_sd == nullptr)));
    auto a8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    const bool v2 = a8(x) && a8(mu) && a8(sd) && a8(dmu) && a8(dsd) && (ldx % 2 == 0) && (ldp % 2 == 0) && (ldd % 2 == 0);
    const dim3 grid(M < 16384 ? M : 16384), block(256);
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (bias_mu && mode == DV_GAUSS_SIGMA && sd_act == DV_ACT_SOFTPLUS && X % 4 == 0 && ldx % 4 == 0 && ldp % 4 == 0 &&
        ldd % 4 == 0 && a16(x) && a16(mu) && a16(sd) && a16(dmu) && a16(dsd) && a16(bias_mu) && a16(bias_sd)) {
        hipLaunchKernelGGL(nll_rows_raw_sp_kernel, grid, block, 0, ST(stream), coef, x, ldx, xidx, mu, sd, ldp, M, X,
                           sd_shift, out, dmu, dsd, ldd, bias_mu, bias_sd);
        DV_RETURN_LAUNCH();
    }
    if (v2)
        hipLaunchKernelGGL(nll_rows_fwdbwd_kernel<true>, grid, block, 0, ST(stream), coef, x, ldx, xidx, mu, sd, ldp, M,
                           X, mode, sd_act, sd_shift, out, dmu, dsd, ldd, bias_mu, bias_sd);
    else
        hipLaunchKernelGGL(nll_rows_fwdbwd_kernel<false>, grid, block, 0, ST(stream), coef, x, ldx, xidx, mu, sd, ldp,
                           M, X, mode, sd_act, sd_shift, out, dmu, dsd, ldd, bias_mu, bias_sd);
    DV_RETURN_LAUNCH();
}

template <bool ZI, int LIB>
static void launch_gene_rows(bool vec, const GeneRowsArgs& a, int row_blocks, int n_cls, const GeneClsArgs& cl,
                             dv_stream_t stream) {
    const dim3 grid(a.chunks, row_blocks, n_cls > 0 ? n_cls : 1), block(256);
    if (n_cls > 0) {          // a dispersion per (class, gene): the class is the grid's third dimension
        if (vec)
            hipLaunchKernelGGL((gene_rows_kernel<ZI, LIB, true, true>), grid, block, 0, ST(stream), a, cl);
        else
            hipLaunchKernelGGL((gene_rows_kernel<ZI, LIB, false, true>), grid, block, 0, ST(stream), a, cl);
    } else if (vec)
        hipLaunchKernelGGL((gene_rows_kernel<ZI, LIB, true>), grid, block, 0, ST(stream), a, GeneNoCls{});
    else
        hipLaunchKernelGGL((gene_rows_kernel<ZI, LIB, false>), grid, block, 0, ST(stream), a, GeneNoCls{});
}

// the count kinds of dv_gauss_nll_rows_raw_cs (gene-wise theta): every refusal in front of the first launch, at M == 0 too
static int gene_rows(const dv_nll_raw_cs_desc& d, dv_stream_t stream) {
    const bool zi = d.kind == DV_REC_ZINB || d.kind == DV_REC_ZINB_LIB;
    const bool lib = d.kind == DV_REC_NEGBIN_LIB || d.kind == DV_REC_ZINB_LIB;
    DV_REQUIRE(zi || lib || d.kind == DV_REC_NEGBIN);
    DV_REQUIRE(d.M >= 0 && d.X >= 1);
    DV_REQUIRE(d.theta_raw && d.x && d.mu && d.out_part);
    DV_REQUIRE(zi ? d.sd != nullptr : d.sd == nullptr);
    DV_REQUIRE(d.bias_mu == nullptr && d.bias_sd == nullptr && d.sd_off == 0);
    DV_REQUIRE(d.chunks == (d.X + 1023) / 1024);
    DV_REQUIRE(d.row_blocks >= 1 && d.row_blocks <= (d.M > 1 ? d.M : 1) && d.row_blocks <= 65535);
    DV_REQUIRE(d.ldx >= d.X && d.ldp >= d.X);
    DV_REQUIRE(d.n_cls >= 0 && d.n_cls <= 65535);
    if (d.n_cls >= 1) DV_REQUIRE(d.cls != nullptr && d.ldth >= d.X);
    const bool grad = d.dmu != nullptr;
    if (grad) {
        DV_REQUIRE(d.ws && d.coef && d.ldw >= d.X && d.ldd >= d.X);
        DV_REQUIRE(d.ldw >= (int64_t)d.n_cls * d.X);
        DV_REQUIRE(zi ? d.dsd != nullptr : d.dsd == nullptr);
    } else {
        DV_REQUIRE(d.ws == nullptr && d.dsd == nullptr);
    }
    DV_REQUIRE(!(lib && d.chunks > 1 && d.size == nullptr));
    if (d.M == 0) return DV_OK;
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec_x = d.X % 4 == 0 && a16(d.x) && d.ldx % 4 == 0;
    const bool vec = vec_x && a16(d.mu) && d.ldp % 4 == 0 && (!zi || a16(d.sd)) &&
                     (!grad || (a16(d.dmu) && d.ldd % 4 == 0 && (!zi || a16(d.dsd))));
    const int rows = (d.M + d.row_blocks - 1) / d.row_blocks;
    const GeneRowsArgs a{d.coef, d.x, d.ldx, d.xidx, d.mu, d.sd, d.ldp, d.M, d.X, d.shift, d.out_part, d.chunks, d.dmu, d.dsd,
                         d.ldd, d.theta_raw, d.ws, d.ldw, d.size, rows};
    const int libmode = !lib ? 0 : d.chunks == 1 ? 1 : 2;
    if (libmode == 2) {       // the size factor of every row first: two launches behind one call, as dv_grad_norm_clip is
        const dim3 grid(grid_for(d.M, 1, 4096)), block(256);
        if (vec_x)
            hipLaunchKernelGGL(size_rows_kernel<true>, grid, block, 0, ST(stream), d.x, d.ldx, d.xidx, d.M, d.X, d.size);
        else
            hipLaunchKernelGGL(size_rows_kernel<false>, grid, block, 0, ST(stream), d.x, d.ldx, d.xidx, d.M, d.X, d.size);
    }
    static constexpr decltype(&launch_gene_rows<false, 0>) launch[2][3] = {
        {launch_gene_rows<false, 0>, launch_gene_rows<false, 1>, launch_gene_rows<false, 2>},
        {launch_gene_rows<true, 0>, launch_gene_rows<true, 1>, launch_gene_rows<true, 2>}};
    launch[zi][libmode](vec, a, d.row_blocks, d.n_cls, GeneClsArgs{d.cls, d.cls_src, d.ldth}, stream);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_gauss_nll_rows_raw_cs(const dv_nll_raw_cs_desc* dsc, dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr);
    const dv_nll_raw_cs_desc& d = *dsc;
    if (d.kind != 0) return gene_rows(d, stream);
    DV_REQUIRE(d.n_cls == 0);                      // (classes: the count kinds only)
    DV_REQUIRE(d.M >= 0 && d.X >= 4 && d.X % 4 == 0);
    if (d.M == 0) return DV_OK;
    const bool fwd_only = d.dmu == nullptr;        // (evaluation: row terms only)
    DV_REQUIRE(d.x && d.mu && d.sd && d.out_part && d.bias_mu && d.bias_sd);
    DV_REQUIRE(fwd_only ? (d.dsd == nullptr && d.ws == nullptr) : (d.coef && d.dsd && d.ws));
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    DV_REQUIRE(a16(d.x) && a16(d.mu) && a16(d.sd) && a16(d.bias_mu) && a16(d.bias_sd));
    DV_REQUIRE(d.ldx % 4 == 0 && d.ldp % 4 == 0);
    if (!fwd_only) {
        DV_REQUIRE(a16(d.dmu) && a16(d.dsd) && a16(d.ws) && d.ldd % 4 == 0 && d.ldw % 4 == 0 && d.sd_off % 4 == 0);
        DV_REQUIRE(d.sd_off >= d.X && d.sd_off + d.X <= d.ldw);
    }
    const int chunks = dv_nll_raw_cs_chunks(d.X), row_blocks = dv_nll_raw_cs_row_blocks(d.M);
    DV_REQUIRE(d.chunks == chunks && d.row_blocks == row_blocks && row_blocks <= 65535);
    NllCsArgs a{d.coef, d.x, d.ldx, d.xidx, d.mu, d.sd, d.ldp, d.M, d.X, d.shift, d.out_part, chunks, d.dmu, d.dsd, d.ldd,
                d.bias_mu, d.bias_sd, d.ws, d.ldw, d.sd_off};
    if (fwd_only)
        hipLaunchKernelGGL(nll_rows_raw_cs_kernel<true>, dim3(chunks, row_blocks), dim3(256), 0, ST(stream), a);
    else
        hipLaunchKernelGGL(nll_rows_raw_cs_kernel<false>, dim3(chunks, row_blocks), dim3(256), 0, ST(stream), a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_nll_raw_cs_chunks(int32_t X) { return X < 4 ? 0 : ((X >> 2) + 255) / 256; }
extern "C" int dv_nll_raw_cs_row_blocks(int32_t M) { return M <= 0 ? 0 : (M + kNllCsRows - 1) / kNllCsRows; }

template <int HEADS, bool LIB>
static void launch_count_nll_rows(bool vec, int kind, float shift, const float* coef, const float* x, int64_t ldx,
                                  const int32_t* xidx, const float* v, int64_t ldv, int M, int X, float* out, float* dpre,
                                  int64_t ldd, dv_stream_t stream) {
    const dim3 grid(grid_for(M, 1, 4096)), block(256);
    if constexpr (HEADS > 1) {
        if (vec) {
            hipLaunchKernelGGL((count_nll_rows_kernel<HEADS, true, LIB>), grid, block, 0, ST(stream), kind, shift, coef, x,
                               ldx, xidx, v, ldv, M, X, out, dpre, ldd);
            return;
        }
    }
    hipLaunchKernelGGL((count_nll_rows_kernel<HEADS, false, LIB>), grid, block, 0, ST(stream), kind, shift, coef, x, ldx,
                       xidx, v, ldv, M, X, out, dpre, ldd);
}

extern "C" int dv_rec_nll_rows(int32_t kind, float shift, const float* coef, const float* x, int64_t ldx,
                               const int32_t* xidx, const float* v, int64_t ldv, int32_t M, int32_t X, float* out,
                               float* dpre, int64_t ldd, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 1 && kind >= DV_REC_BERNOULLI && kind <= DV_REC_ZINB_LIB);
    if (M == 0) return DV_OK;
    DV_REQUIRE(x && v && out && (coef == nullptr || dpre != nullptr));
    // the library-scaled kinds: the unscaled kind's kernel, compiled with the size-factor sweep in front of its term loop
    const bool lib = kind == DV_REC_POISSON_LIB || kind == DV_REC_NEGBIN_LIB || kind == DV_REC_ZINB_LIB;
    const int heads = kind == DV_REC_NEGBIN || kind == DV_REC_NEGBIN_LIB ? 2
                      : kind == DV_REC_ZINB || kind == DV_REC_ZINB_LIB ? 3 : 1;
    bool vec = false;
    if (heads > 1) {      // v and dpre: `heads` blocks of X columns each
        const int64_t w = heads * (int64_t)X;
        DV_REQUIRE(ldv >= w && (coef == nullptr || ldd >= w));
        auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        vec = X % 4 == 0 && a16(x) && a16(v) && ldx % 4 == 0 && ldv % 4 == 0 &&
              (coef == nullptr || (a16(dpre) && ldd % 4 == 0));
    }
    const int k = kind == DV_REC_POISSON_LIB ? DV_REC_POISSON : kind;      // (read by the one-head kernels only)
    static constexpr decltype(&launch_count_nll_rows<1, false>) launch[3][2] = {
        {launch_count_nll_rows<1, false>, launch_count_nll_rows<1, true>},
        {launch_count_nll_rows<2, false>, launch_count_nll_rows<2, true>},
        {launch_count_nll_rows<3, false>, launch_count_nll_rows<3, true>}};
    launch[heads - 1][lib](vec, k, shift, coef, x, ldx, xidx, v, ldv, M, X, out, dpre, ldd, stream);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_gauss_nll_rows_bwd(const float* coef, const float* x, int64_t ldx, const int32_t* xidx,
                                     const float* mu, const float* sd, int64_t ldp, int32_t M, int32_t X,
                                     int32_t mode, int32_t sd_act, float sd_shift, float* dmu, float* dsd,
                                     int64_t ldd, float* dx, int64_t lddx, float beta, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 0);
    if (M == 0 || X == 0) return DV_OK;
    DV_REQUIRE(coef && x && mu && sd && dmu && dsd);
    hipLaunchKernelGGL(nll_rows_bwd_kernel, dim3(grid_for((int64_t)M * X, 256, 8192)), dim3(256), 0, ST(stream),
                       coef, x, ldx, xidx, mu, sd, ldp, M, X, mode, sd_act, sd_shift, dmu, dsd, ldd, dx, lddx, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_softmax_clamp_fwd(const float* logits, int64_t ldl, int32_t M, int32_t Y, int32_t sigmoid1,
                                    float* probs, int64_t ldp, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && Y >= 1);
    if (M == 0) return DV_OK;
    DV_REQUIRE(logits && probs);
    DV_REQUIRE(!sigmoid1 || Y == 2);
    hipLaunchKernelGGL(softmax_clamp_fwd_kernel, dim3((M + 255) / 256), dim3(256), 0, ST(stream), logits, ldl, M, Y,
                       sigmoid1, probs, ldp);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_softmax_clamp_bwd(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp, int32_t M,
                                    int32_t Y, int32_t sigmoid1, float* dlogits, int64_t ldl, float beta,
                                    dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && Y >= 1);
    if (M == 0) return DV_OK;
    DV_REQUIRE(dprobs && probs && dlogits);
    DV_REQUIRE(!sigmoid1 || Y == 2);
    hipLaunchKernelGGL(softmax_clamp_bwd_kernel, dim3((M + 255) / 256), dim3(256), 0, ST(stream), dprobs, lddp,
                       probs, ldp, M, Y, sigmoid1, dlogits, ldl, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_cat_terms_fwd(const float* probs, int64_t ldp, int32_t M, int32_t Y, const int32_t* labels,
                                const float* prior, int64_t ldpr, float* logp, float* kl, int64_t ldk, float* ent,
                                int32_t* best, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && Y >= 1);
    if (M == 0) return DV_OK;
    DV_REQUIRE(probs);
    DV_REQUIRE(logp == nullptr || labels != nullptr);
    DV_REQUIRE(kl == nullptr || prior != nullptr);
    hipLaunchKernelGGL(cat_terms_fwd_kernel, dim3((M + 255) / 256), dim3(256), 0, ST(stream), probs, ldp, M, Y,
                       labels, prior, ldpr, logp, kl, ldk, ent, best);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_cat_terms_bwd(const float* probs, int64_t ldp, int32_t M, int32_t Y, const int32_t* labels,
                                const float* prior, int64_t ldpr, const float* c_logp, const float* g_kl,
                                int64_t ldg, const float* c_ent, float* dprobs, int64_t lddp, float beta,
                                dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && Y >= 1);
    if (M == 0) return DV_OK;
    DV_REQUIRE(probs && dprobs);
    DV_REQUIRE(c_logp == nullptr || labels != nullptr);
    DV_REQUIRE(g_kl == nullptr || prior != nullptr);
    hipLaunchKernelGGL(cat_terms_bwd_kernel, dim3((M + 255) / 256), dim3(256), 0, ST(stream), probs, ldp, M, Y,
                       labels, prior, ldpr, c_logp, g_kl, ldg, c_ent, dprobs, lddp, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_smalln_linear_fwd(const float* a1, int64_t lda1, int32_t K1, const float* a2, int64_t lda2,
                                    int32_t K2, const float* W, int64_t ldw, const float* bias, int32_t M, int32_t N,
                                    float* logits, int64_t ldl, float* probs, int64_t ldp, const dv_ymarg* ymarg,
                                    const dv_wait* park_in, const dv_fprop_kl* kf_in, const dv_clf_dgrad* dg_in,
                                    dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 1 && N <= kMaxSmallN && K1 >= 0 && K2 >= 0);
    ParkArgs park;
    if (int rc = take_park(park_in, (M + 3) / 4, &park)) return rc;
    if (M == 0) return DV_OK;
    DV_REQUIRE(a1 && W && (a2 || K2 == 0) && (logits || probs));
    dv_ymarg ym{};
    if (ymarg != nullptr && ymarg->fp_ptr != nullptr) {
        ym = *ymarg;
        DV_REQUIRE(probs && ym.label && ym.klfp && ym.c_kld && ym.c_yl && ym.yl && ym.kld && ym.cfp && ym.dqy);
    }
    dv_fprop_kl kf{};
    if (kf_in != nullptr && kf_in->mu_q != nullptr) {
        kf = *kf_in;
        DV_REQUIRE(ym.fp_ptr != nullptr && kf.klfp == ym.klfp && kf.qidx && kf.mu_p && kf.mu3 && kf.raw1 && kf.raw3 &&
                   kf.dq && kf.dp && kf.Z1 >= 0 && kf.Z3 >= 0);
    }
    dv_clf_dgrad dg{};
    if (dg_in != nullptr && dg_in->n != 0) {
        dg = *dg_in;
        DV_REQUIRE(ym.fp_ptr != nullptr && dg.n >= 1 && dg.n <= 2);
        for (int t = 0; t < dg.n; ++t) {
            DV_REQUIRE(dg.dst[t] != nullptr && dg.ncol[t] >= 0 && dg.col0[t] >= 0 && dg.col0[t] + dg.ncol[t] <= K1 + K2);
            DV_REQUIRE(dg.alpha2[t] == 0.f || (dg.col1[t] >= 0 && dg.col1[t] + dg.ncol[t] <= K1 + K2));
        }
    }
    if (kf.mu_q != nullptr && probs != nullptr && N <= 2 && K1 + K2 <= 256 && kf.Z1 <= 128 && kf.Z3 <= 128) {
        // (the train step's launch at its common shape: every operand in flight first, see smalln_fwd2_kernel)
        hipLaunchKernelGGL(smalln_fwd2_kernel, dim3((M + 3) / 4), dim3(256), 0, ST(stream), a1, lda1, K1, a2, lda2, K2, W,
                           ldw, bias, M, N, logits, ldl, probs, ldp, ym, park, kf, dg);
        DV_RETURN_LAUNCH();
    }
    hipLaunchKernelGGL(smalln_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, ST(stream), a1, lda1, K1, a2, lda2, K2, W,
                       ldw, bias, M, N, logits, ldl, probs, ldp, ym, park, kf, dg);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_smalln_linear_bwd_data(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp,
                                         const float* W, int64_t ldw, int32_t M, int32_t N, int32_t n_dst,
                                         float* const* dst, const int64_t* ld, const int32_t* col0,
                                         const int32_t* ncol, const float* alpha, const float* beta,
                                         const int32_t* col1, const float* alpha2, const float* seg_src,
                                         int64_t ld_seg, const int32_t* seg_ptr, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 1 && N <= kMaxSmallN && n_dst >= 1 && n_dst <= 3);
    DV_REQUIRE((seg_src == nullptr) == (seg_ptr == nullptr));
    if (M == 0) return DV_OK;
    DV_REQUIRE(dprobs && W && dst && ld && col0 && ncol && alpha && beta);
    SmallNDst d;
    d.n = n_dst;
    d.seg_src = seg_src;
    d.ld_seg = ld_seg;
    d.seg_ptr = seg_ptr;
    int cols = 0;
    for (int t = 0; t < n_dst; ++t) {
        DV_REQUIRE(dst[t] != nullptr && ncol[t] >= 0);
        d.dst[t] = dst[t];
        d.ld[t] = ld[t];
        d.col0[t] = col0[t];
        d.ncol[t] = ncol[t];
        d.alpha[t] = alpha[t];
        d.beta[t] = beta[t];
        d.col1[t] = col1 ? col1[t] : 0;
        d.alpha2[t] = alpha2 ? alpha2[t] : 0.f;
        cols += ncol[t];
    }
    if (cols == 0) return DV_OK;
    hipLaunchKernelGGL(smalln_bwd_data_kernel, dim3(grid_for((int64_t)M * cols, 256)), dim3(256), 0, ST(stream),
                       dprobs, lddp, probs, ldp, probs != nullptr, W, ldw, M, N, d);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_smalln_linear_bwd_weight(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp,
                                           const float* a1, int64_t lda1, int32_t K1, const float* a2,
                                           int64_t lda2, int32_t K2, int32_t M, int32_t N, float* dW, int64_t ldd,
                                           float* db, float beta, const dv_publish* pub_in, float* ws, int32_t ws_splits,
                                           dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 1 && N <= kMaxSmallN && K1 >= 0 && K2 >= 0);
    DV_REQUIRE(dprobs && a1 && dW && (a2 || K2 == 0) && ws_splits >= 0 && (ws || ws_splits <= 1));
    dv_publish pub;
    if (int rc = take_publish(pub_in, &pub)) return rc;
    const int col_blocks = (K1 + K2 + 1 + kSnCols - 1) / kSnCols;
    // rows split over workgroups only where a column block's workgroup would walk many rows (>= 1024) on a mostly idle
    // chip; the caller's workspace holds ws_splits x N x (K1 + K2 + 1) floats
    int splits = (ws && ws_splits > 1) ? (M + 255) / 256 : 1;
    if (splits > ws_splits) splits = ws_splits > 0 ? ws_splits : 1;
    if (M < 1024 || splits < 2) splits = 1;
    const int rps = splits > 1 ? (M + splits - 1) / splits : (M > 0 ? M : 1);
    hipLaunchKernelGGL(smalln_bwd_weight_kernel, dim3(col_blocks, splits), dim3(1024), 0,
                       ST(stream), dprobs,
                       lddp, probs, ldp, probs != nullptr, a1, lda1, K1, a2, lda2, K2, M, N, dW, ldd, db, beta, pub,
                       splits > 1 ? ws : (float*)nullptr, rps);
    if (splits > 1)
        hipLaunchKernelGGL(smalln_wgrad_reduce_kernel, dim3((N * (K1 + K2 + 1) + 255) / 256), dim3(256), 0, ST(stream), ws,
                           splits, N, K1 + K2, dW, ldd, db, beta);
    DV_RETURN_LAUNCH();
}

template <bool FWD, bool BWD>
static int ymarg_launch(const float* qy, int64_t ldq, const dv_ymarg& y, int32_t R, int32_t Y, dv_stream_t stream) {
    DV_REQUIRE(R >= 0 && Y >= 1);
    if (R == 0) return DV_OK;
    DV_REQUIRE(qy && y.label && y.fp_ptr && y.klfp);
    DV_REQUIRE(!FWD || (y.yl && y.kld));
    DV_REQUIRE(!BWD || (y.c_kld && y.c_yl && y.cfp && y.dqy));
    hipLaunchKernelGGL((ymarg_kernel<FWD, BWD>), dim3((R + 255) / 256), dim3(256), 0, ST(stream), qy, ldq, y, R, Y);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_ymarg_fwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr,
                            const float* klfp, float log_prior, const float* log_prior_v, int32_t R, int32_t Y,
                            float* yl, float* kld, dv_stream_t stream) {
    return ymarg_launch<true, false>(qy, ldq, dv_ymarg{label, fp_ptr, klfp, log_prior, log_prior_v, nullptr, nullptr, yl, kld,
                                                       nullptr, nullptr, 0}, R, Y, stream);
}

extern "C" int dv_ymarg_fwdbwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr,
                               const float* klfp, float log_prior, const float* log_prior_v, const float* c_kld,
                               const float* c_yl, int32_t R, int32_t Y, float* yl, float* kld, float* cfp,
                               float* dqy, int64_t lddq, dv_stream_t stream) {
    return ymarg_launch<true, true>(qy, ldq, dv_ymarg{label, fp_ptr, klfp, log_prior, log_prior_v, c_kld, c_yl, yl, kld, cfp,
                                                      dqy, lddq}, R, Y, stream);
}

extern "C" int dv_ymarg_bwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr,
                            const float* klfp, float log_prior, const float* log_prior_v, const float* c_kld,
                            const float* c_yl, int32_t R, int32_t Y, float* cfp, float* dqy, int64_t lddq,
                            dv_stream_t stream) {
    return ymarg_launch<false, true>(qy, ldq, dv_ymarg{label, fp_ptr, klfp, log_prior, log_prior_v, c_kld, c_yl, nullptr,
                                                       nullptr, cfp, dqy, lddq}, R, Y, stream);
}

extern "C" int dv_ycont_fwd(const float* mu, int64_t ldm, const float* ylab, const int32_t* has_y, const float* eps,
                            int64_t lde, float logvar, int32_t sqerr, int32_t R, int32_t B, int32_t Y, float* yl,
                            float* fpin_y, int64_t ld1, float* z3in_y, int64_t ld2, dv_stream_t stream) {
    DV_REQUIRE(R >= 0 && B >= 1 && Y >= 1);
    if (R == 0) return DV_OK;
    DV_REQUIRE(mu && ylab && has_y && eps && yl && fpin_y && z3in_y);
    hipLaunchKernelGGL(ycont_fwd_kernel, dim3((R + 255) / 256), dim3(256), 0, ST(stream), mu, ldm, ylab, has_y, eps, lde,
                       logvar, sqerr, R, B, Y, yl, fpin_y, ld1, z3in_y, ld2);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_ycont_bwd(const float* mu, int64_t ldm, const float* ylab, const int32_t* has_y, float logvar,
                            int32_t sqerr, const float* c_yl, const float* c_kld, const float* dfpin_y, int64_t ld1,
                            const float* dz3in_y, int64_t ld2, int32_t R, int32_t B, int32_t Y, float* dlogit,
                            int64_t ldd, float* cfp, dv_stream_t stream) {
    DV_REQUIRE(R >= 0 && B >= 1 && Y >= 1);
    if (R == 0) return DV_OK;
    DV_REQUIRE(has_y && ((cfp && c_kld) || (mu && ylab && c_yl && dfpin_y && dz3in_y && dlogit)));
    hipLaunchKernelGGL(ycont_bwd_kernel, dim3((R + 255) / 256), dim3(256), 0, ST(stream), mu, ldm, ylab, has_y, logvar,
                       sqerr, c_yl, c_kld, dfpin_y, ld1, dz3in_y, ld2, R, B, Y, dlogit, ldd, cfp, dlogit == nullptr ? 1 : 0);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_rff_fwd(const float* th1, int64_t ld1, int32_t n1, const float* th2, int64_t ld2, int32_t n2,
                              int32_t R, float c, float* diff, float* mmd2, dv_stream_t stream) {
    DV_REQUIRE(n1 >= 1 && n2 >= 1 && R >= 1);
    DV_REQUIRE(th1 && th2 && diff && mmd2);
    hipLaunchKernelGGL(mmd_cos_means_kernel, dim3((R + 63) / 64), dim3(256), 0, ST(stream), th1, ld1, n1, th2, ld2, n2, R,
                       c, diff);
    hipLaunchKernelGGL(mmd_sumsq_kernel, dim3(1), dim3(256), 0, ST(stream), diff, R, mmd2);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_rff_bwd(const float* th, int64_t ld, int32_t n, int32_t R, const float* diff, const float* gout,
                              float coef, float* G, int64_t ldg, dv_stream_t stream) {
    DV_REQUIRE(n >= 1 && R >= 1);
    DV_REQUIRE(th && diff && gout && G);
    hipLaunchKernelGGL(mmd_dtheta_kernel, dim3(grid_for((int64_t)n * R, 256)), dim3(256), 0, ST(stream), th, ld, n, R,
                       diff, gout, coef, G, ldg);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_rows_gather(const float* src, int64_t lds, const int32_t* idx, int32_t n, int32_t W,
                              const float* noise, int64_t ldn, float sigma, const int32_t* onehot_cls, int32_t Y,
                              float* out, int64_t ldo, const dv_wait* park_in, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && W >= 0 && Y >= 0);
    const int64_t total = (int64_t)n * (W + (onehot_cls ? Y : 0));
    ParkArgs park;
    if (int rc = take_park(park_in, total > 0 ? grid_for(total, 256, 128) : 0, &park)) return rc;      // (128: see below)
    if (n == 0) return DV_OK;
    DV_REQUIRE(out && (src || W == 0));
    if (total == 0) return DV_OK;
    // (a parked launch polls from every workgroup: its grid stays small -- 128 workgroups, the element loop strides --
    // so that the polling does not crowd the chain it waits for)
    hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_for(total, 256, park.flag != nullptr ? 128 : 4096)),
                       dim3(256), 0, ST(stream), src, lds, idx, n, W, noise, ldn, sigma, onehot_cls, Y, out, ldo, park);
    DV_RETURN_LAUNCH();
}

static bool masks_ok(const dv_batch_masks_desc& m, int B) {
    // (the schedule's outputs come with its step counter: without one none of them may be set -- a zeroed tail is "no schedule")
    const bool sched_ok = m.sched_step ? (m.sched && m.w_elbo && m.w_cmpl && (m.w_klz2 == nullptr || m.c_klz2) &&
                                          (m.w_klp == nullptr || m.c_klp))
                                       : !(m.sched || m.c_kld || m.w_klz2 || m.w_klp || m.w_elbo || m.w_cmpl);
    return m.Np >= 0 && m.Np <= B && m.n_tot > 0.f && m.c_nll && m.w_recl && (m.hx == nullptr || (m.c_klz2 && m.w_pert)) &&
           (m.hy == nullptr || (m.y && m.c_yl && m.w_yl && m.label)) && sched_ok;
}

static MaskArgs mask_args(const dv_batch_masks_desc& m, const int32_t* table, int n_batches, const int32_t* ctr,
                          const int32_t* base, int B, int L) {
    return MaskArgs{table, n_batches, ctr, base, m.hx, m.hy, m.y, B, L, m.Np, m.n_tot, m.kl_rate, m.pert_rate, m.yl_rate,
                    m.beta, m.c_nll, m.c_klz2, m.c_yl, m.w_recl, m.w_pert, m.w_yl, m.label, m.c_klp, m.one_slot, m.gcounts,
                    m.sched_step, m.pert_itermax, m.pert_offset, m.kl_itermax, m.yl_itermax, m.yl_offset, m.lr_itermax,
                    m.mmd_rate, m.sched, m.c_kld, m.w_klz2, m.w_klp, m.w_elbo, m.w_cmpl};
}

// (ONE list of the feed kernels' common arguments: the variants differ in the descriptor's tail)
#define DV_FEED_ARGS                                                                                                       \
    d.x1, d.ld1, d.x2, d.ld2, d.y, d.table, d.n_batches, d.ctr, d.base, B, d.pair_rows, Np, d.X, d.noise, d.ldn, d.sigma,  \
        d.xin, d.ldo, d.has_y, L, d.label_r, d.fp_i, d.fp_lab, d.fp_slot, Mf, d.fp_cls, d.onehot, d.ldh, d.Y, row_blocks,  \
        v4 ? 1 : 0, d.yf, d.ylab, d.Yc, d.onehot2, d.ldh2, mask_block, ma, park
// the sparse feed's launches: defined at the END of this file -- the templates a host function launches are emitted in the order
// of their first use, so the sparse instantiations come last in the code object and every kernel that was there keeps its place
static void launch_batch_feed_csr(const dv_batch_feed_desc& d, dim3 grid, dim3 block, int row_blocks, bool v4, int mask_block,
                                  const MaskArgs& ma, const ParkArgs& park, dv_stream_t stream);

extern "C" int dv_batch_feed(const dv_batch_feed_desc* dsc, const dv_batch_masks_desc* masks, const dv_wait* park_in,
                             dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr && park_ok(park_in));      // (a malformed wait is refused even where B == 0 launches nothing)
    const dv_batch_feed_desc& d = *dsc;
    const int B = d.B, Np = d.Np, L = d.L, Mf = d.Mf;
    DV_REQUIRE(B >= 0 && Np >= 0 && d.X >= 0 && d.n_batches >= 1 && L >= 1 && Mf >= 0 && d.Y >= 0 && d.Yc >= 0);
    DV_REQUIRE(!d.ylab || (d.yf && d.Yc >= 1));
    // sparse rows: a CSR triple is whole or absent, and a matrix is dense or sparse, never both
    const bool s1 = d.csr1_ptr != nullptr, s2 = d.csr2_ptr != nullptr;
    DV_REQUIRE(s1 == (d.csr1_idx != nullptr) && s1 == (d.csr1_val != nullptr) && !(s1 && d.x1));
    DV_REQUIRE(s2 == (d.csr2_idx != nullptr) && s2 == (d.csr2_val != nullptr) && !(s2 && d.x2));
    if (B == 0) return DV_OK;
    DV_REQUIRE((d.x1 || s1) && d.table && d.ctr && d.base && d.xin && (Np == 0 || ((d.x2 || s2) && d.pair_rows)));
    DV_REQUIRE(!d.label_r || (d.y && d.has_y));
    DV_REQUIRE(!d.fp_cls || Mf == 0 || (d.y && d.fp_i && d.fp_lab && d.fp_slot));
    // split form (raw-count inputs): targets to xt, encoder rows T(x) + sigma*noise to xin
    // (`transform`: 0 none, 1 log1p, 3 log1p_norm -- the row's own size factor divides it first; 2 is no code)
    DV_REQUIRE((d.transform == 0 || d.transform == 1 || d.transform == 3) && (d.transform == 0 || d.xt != nullptr));
    DV_REQUIRE(d.xt == nullptr || (aligned16(d.xt) && d.ldt >= d.X));
    const int row_blocks = (B + Np + 3) / 4;
    int nlab = (d.label_r ? L * B : 0) > (d.fp_cls ? Mf : 0) ? (d.label_r ? L * B : 0) : (d.fp_cls ? Mf : 0);
    if (d.ylab && B * d.Yc > nlab) nlab = B * d.Yc;
    const int lab_blocks = (nlab + 255) / 256;
    // (a sparse matrix has no dense rows to align: its rows are read from the wave's staged chunk)
    const bool v4 = (s1 || (aligned16(d.x1) && d.ld1 % 4 == 0)) && (Np == 0 || s2 || (aligned16(d.x2) && d.ld2 % 4 == 0)) &&
                    aligned16(d.xin) && (!d.noise || aligned16(d.noise)) && d.ldo % 4 == 0 && (!d.noise || d.ldn % 4 == 0) &&
                    (!d.xt || d.ldt % 4 == 0);
    MaskArgs ma{};
    if (masks) {
        DV_REQUIRE(masks_ok(*masks, B));
        ma = mask_args(*masks, d.table, d.n_batches, d.ctr, d.base, B, L);
    }
    const int feed_blocks = row_blocks + lab_blocks;
    ParkArgs park;
    if (int rc = take_park(park_in, feed_blocks + 1, &park)) return rc;
    const dim3 grid(feed_blocks + (masks ? 1 : 0)), block(256);
    const int mask_block = masks ? feed_blocks : -1;
    if (s1 || (s2 && Np > 0))        // a matrix that is read is sparse: the sibling kernel, chosen by the descriptor alone
        launch_batch_feed_csr(d, grid, block, row_blocks, v4, mask_block, ma, park, stream);
    else if (d.xt && d.transform == 3)
        hipLaunchKernelGGL((batch_feed_kernel<true, true>), grid, block, 0, ST(stream), DV_FEED_ARGS, d.xt, d.ldt, d.transform);
    else if (d.xt)
        hipLaunchKernelGGL((batch_feed_kernel<true, false>), grid, block, 0, ST(stream), DV_FEED_ARGS, d.xt, d.ldt, d.transform);
    else
        hipLaunchKernelGGL((batch_feed_kernel<false, false>), grid, block, 0, ST(stream), DV_FEED_ARGS, nullptr, 0, 0);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_batch_masks(const dv_batch_masks_desc* m, const int32_t* table, int32_t n_batches, const int32_t* ctr,
                              const int32_t* base, int32_t B, int32_t L, dv_stream_t stream) {
    DV_REQUIRE(m != nullptr && B >= 1 && L >= 1 && masks_ok(*m, B));
    DV_REQUIRE(table == nullptr || (ctr && base && n_batches >= 1));
    MaskArgs a = mask_args(*m, table, n_batches, ctr, base, B, L);
    hipLaunchKernelGGL(batch_masks_kernel, dim3(1), dim3(1024), 0, ST(stream), a);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_rows_segment_sum(const float* src, int64_t lds, const int32_t* seg_ptr, const int32_t* seg_rows,
                                   const float* w, int32_t n, int32_t W, const int32_t* dst_idx, float* dst,
                                   int64_t ldd, float beta, const dv_wait* park_in, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && W >= 0);
    ParkArgs park;
    if (int rc = take_park(park_in, n > 0 && W > 0 ? grid_for((int64_t)n * W, 256) : 0, &park)) return rc;
    if (n == 0 || W == 0) return DV_OK;
    DV_REQUIRE(src && dst);
    hipLaunchKernelGGL(rows_segment_sum_kernel, dim3(grid_for((int64_t)n * W, 256)), dim3(256), 0, ST(stream), src,
                       lds, seg_ptr, seg_rows, w, n, W, dst_idx, dst, ldd, beta, park);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_weighted_sum(const float* x, const float* w, const int32_t* idx, int32_t n, float scale,
                               float* out, float beta, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && out);
    DV_REQUIRE(n == 0 || x);
    hipLaunchKernelGGL(weighted_sum_kernel, dim3(1), dim3(256), 0, ST(stream), x, w, idx, n, scale, out, beta);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_recon_row_stats(const float* x, int64_t ldx, const float* r, int64_t ldr, int32_t M, int32_t X,
                                  float* out, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 1);
    if (M == 0) return DV_OK;
    DV_REQUIRE(x && r && out);
    hipLaunchKernelGGL(recon_row_stats_kernel, dim3(grid_for(M, 4, 8192)), dim3(256), 0, ST(stream), x, ldx, r, ldr,
                       M, X, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_col_moments(const float* x, int64_t ldx, const float* r, int64_t ldr, int32_t M, int32_t X,
                              double* out, int32_t row_blocks, const int32_t* sel, const float* r_bias,
                              dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 1 && row_blocks >= 1 && row_blocks <= 65535);
    DV_REQUIRE(x && r && out);
    const int rpb = (M + row_blocks - 1) / row_blocks;
    hipLaunchKernelGGL(col_moments_kernel, dim3((X + 63) / 64, row_blocks), dim3(64 * kCmRG), 0, ST(stream), x, ldx, r, ldr, M, X, out,
                       rpb > 0 ? rpb : 1, sel, r_bias);
    DV_RETURN_LAUNCH();
}

// the effect reduction (dv_draw_desc.fx, carried by dv_fill_normal in optim.hip): every refusal in front of the launch, at
// M == 0 too
int dv_effect_cols_launch(const dv_effect_desc& f, int32_t M, int32_t X, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && X >= 1 && X <= 0x7fffffc0);             // (the last gene chunk's indices stay inside int32)
    DV_REQUIRE(f.n_grp >= 1 && f.n_grp <= 65535);
    DV_REQUIRE(f.row_blocks >= 1 && f.row_blocks <= (M > 1 ? M : 1) && f.row_blocks <= 65535);
    DV_REQUIRE(f.lda >= X && f.ldb >= X);
    DV_REQUIRE(f.mode == 0 || f.mode == 1);
    DV_REQUIRE(f.delta >= 0.f);                                  // (a NaN fails every comparison)
    DV_REQUIRE(f.pseudo >= 0.f && f.pseudo <= 3.402823466e38f);
    DV_REQUIRE(f.mode == 0 || f.pseudo == 0.f);
    if (M == 0) return DV_OK;
    DV_REQUIRE(f.a && f.b && f.out);
    auto al = [](const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; };
    const bool vec = X % 4 == 0 && al(f.a, f.lda) && al(f.b, f.ldb);
    const EffectArgs a{f.a, f.lda, f.b, f.ldb, f.grp, M, X, (int)(((int64_t)M + f.row_blocks - 1) / f.row_blocks),
                       f.mode, f.delta, f.pseudo, f.out};
    const dim3 grid((unsigned)((X + 63) / 64), (unsigned)f.row_blocks, (unsigned)f.n_grp), block(256);
    if (vec) hipLaunchKernelGGL(effect_cols_kernel<true>, grid, block, 0, ST(stream), a);
    else hipLaunchKernelGGL(effect_cols_kernel<false>, grid, block, 0, ST(stream), a);
    DV_RETURN_LAUNCH();
}

template <int KIND, bool LIB>
static void launch_recon_rows_count(bool vec, const RcCountArgs& a, dv_stream_t stream) {
    const dim3 grid(a.M), block(256);
    if (vec) hipLaunchKernelGGL((recon_rows_count_kernel<KIND, LIB, true>), grid, block, 0, ST(stream), a);
    else hipLaunchKernelGGL((recon_rows_count_kernel<KIND, LIB, false>), grid, block, 0, ST(stream), a);
}

// the count kinds of dv_recon_rows (d.kind != DV_RECON_GAUSS): every refusal before any launch
static int recon_rows_count(const dv_recon_rows_desc& d, dv_stream_t stream) {
    DV_REQUIRE(d.kind == DV_RECON_BERNOULLI || d.kind == DV_RECON_POISSON || d.kind == DV_RECON_NEGBIN ||
               d.kind == DV_RECON_ZINB);
    const bool zi = d.kind == DV_RECON_ZINB, nb = d.kind == DV_RECON_NEGBIN || zi, lib = d.size_x != nullptr;
    DV_REQUIRE(d.bias_mu == nullptr && d.bias_sd == nullptr);      // (count heads leave their launch finished)
    DV_REQUIRE(!(lib && d.kind == DV_RECON_BERNOULLI));             // (probabilities have no depth)
    DV_REQUIRE(!nb || d.ldt >= (zi ? 2 : 1) * (int64_t)d.X);        // (theta has a row stride of its own; ZINB: [theta | logit])
    DV_REQUIRE(d.rec_out == nullptr || lib);                        // (without a size source the mean IS the head: no copy)
    if (d.M == 0) return DV_OK;
    DV_REQUIRE(d.x && d.mu && d.rows && (!nb || d.sd));
    DV_REQUIRE(d.ldx >= d.X && d.ldp >= d.X && (!lib || d.size_ld >= d.X) && (!d.rec_out || d.rec_ld >= d.X));
    auto a16 = [](const void* p, int64_t ld) { return p == nullptr || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0); };
    const bool vec = d.X % 4 == 0 && a16(d.x, d.ldx) && a16(d.mu, d.ldp) && (!nb || a16(d.sd, d.ldt)) &&
                     a16(d.size_x, d.size_ld) && a16(d.rec_out, d.rec_ld);
    RcCountArgs a{d.x, d.ldx, d.mu, d.ldp, nb ? d.sd : nullptr, d.ldt, d.size_x, d.size_ld, d.rec_out, d.rec_ld,
                  d.M, d.X, d.rows, d.ll};
    if (zi) {
        if (lib) launch_recon_rows_count<DV_REC_ZINB, true>(vec, a, stream);
        else launch_recon_rows_count<DV_REC_ZINB, false>(vec, a, stream);
    } else if (nb) {
        if (lib) launch_recon_rows_count<DV_REC_NEGBIN, true>(vec, a, stream);
        else launch_recon_rows_count<DV_REC_NEGBIN, false>(vec, a, stream);
    } else if (d.kind == DV_RECON_POISSON) {
        if (lib) launch_recon_rows_count<DV_REC_POISSON, true>(vec, a, stream);
        else launch_recon_rows_count<DV_REC_POISSON, false>(vec, a, stream);
    } else {
        launch_recon_rows_count<DV_REC_BERNOULLI, false>(vec, a, stream);
    }
    DV_RETURN_LAUNCH();
}

extern "C" int dv_recon_rows(const dv_recon_rows_desc* dsc, dv_stream_t stream) {
    DV_REQUIRE(dsc != nullptr);
    const dv_recon_rows_desc& d = *dsc;
    DV_REQUIRE(d.M >= 0 && d.X >= 1);
    if (d.kind != DV_RECON_GAUSS) return recon_rows_count(d, stream);
    DV_REQUIRE(d.size_x == nullptr && d.rec_out == nullptr);       // (the count kinds' operands)
    if (d.X > DV_RECON_ROWS_MAX_X) return DV_ERR_UNSUPPORTED;
    if (d.M == 0) return DV_OK;
    DV_REQUIRE(d.x && d.mu && d.sd && d.rows);
    DV_REQUIRE((d.bias_mu == nullptr) == (d.bias_sd == nullptr));
    RcArgs a{d.x, d.ldx, d.mu, d.sd, d.ldp, d.bias_mu, d.bias_sd, d.sd_shift, d.M, d.X, d.rows, d.ll};
    const dim3 grid(grid_for(d.M, 4, 8192)), block(256);
    auto a8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    const bool v2 = d.X % 2 == 0 && d.ldx % 2 == 0 && d.ldp % 2 == 0 && a8(d.x) && a8(d.mu) && a8(d.sd) &&
                    (!d.bias_mu || (a8(d.bias_mu) && a8(d.bias_sd)));
    if (d.bias_mu) {
        if (v2) hipLaunchKernelGGL((recon_rows_kernel<true, true>), grid, block, 0, ST(stream), a);
        else hipLaunchKernelGGL((recon_rows_kernel<true, false>), grid, block, 0, ST(stream), a);
    } else {
        if (v2) hipLaunchKernelGGL((recon_rows_kernel<false, true>), grid, block, 0, ST(stream), a);
        else hipLaunchKernelGGL((recon_rows_kernel<false, false>), grid, block, 0, ST(stream), a);
    }
    DV_RETURN_LAUNCH();
}

static int mix_args(MixArgs& a, const float* G, int64_t ldg, int32_t M, int32_t N, int32_t kind, const float* gammas,
                    int32_t nb, const float* sa, int64_t sa_stride, const float* sb, int64_t sb_stride) {
    DV_REQUIRE(G && M >= 1 && N >= 1 && (kind == 0 || kind == 1) && gammas && nb >= 1 && nb <= 8);
    DV_REQUIRE(kind == 0 || (sa && sb));
    a = MixArgs{G, ldg, M, N, kind, nb, {0}, sa, sa_stride, sb, sb_stride};
    for (int b = 0; b < nb; ++b) a.gam[b] = gammas[b];
    return DV_OK;
}

extern "C" int dv_mmd_mix_fwd(const float* G, int64_t ldg, int32_t M, int32_t N, int32_t kind, const float* gammas,
                              int32_t nb, const float* sa, int64_t sa_stride, const float* sb, int64_t sb_stride,
                              float* part, dv_stream_t stream) {
    MixArgs a;
    const int rc = mix_args(a, G, ldg, M, N, kind, gammas, nb, sa, sa_stride, sb, sb_stride);
    if (rc != DV_OK) return rc;
    DV_REQUIRE(part != nullptr);
    hipLaunchKernelGGL(mmd_mix_kernel<false>, dim3(M), dim3(256), 0, ST(stream), a, part, (const float*)nullptr, 0.f,
                       (float*)nullptr, (int64_t)0, (float*)nullptr);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_mix_bwd(const float* G, int64_t ldg, int32_t M, int32_t N, int32_t kind, const float* gammas,
                              int32_t nb, const float* sa, int64_t sa_stride, const float* sb, int64_t sb_stride,
                              const float* gout, float coef, float* W, int64_t ldw, float* rs, dv_stream_t stream) {
    MixArgs a;
    const int rc = mix_args(a, G, ldg, M, N, kind, gammas, nb, sa, sa_stride, sb, sb_stride);
    if (rc != DV_OK) return rc;
    DV_REQUIRE(gout && W && rs);
    hipLaunchKernelGGL(mmd_mix_kernel<true>, dim3(M), dim3(256), 0, ST(stream), a, (float*)nullptr, gout, coef, W, ldw, rs);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_mix_combine(const float* p11, int32_t n11, float c11, const float* p12, int32_t n12, float c12,
                                  const float* p22, int32_t n22, float c22, float* out, dv_stream_t stream) {
    DV_REQUIRE(p11 && p12 && p22 && out && n11 >= 1 && n12 >= 1 && n22 >= 1 && c11 > 0.f && c12 > 0.f && c22 > 0.f);
    hipLaunchKernelGGL(mmd_mix_combine_kernel, dim3(1), dim3(64), 0, ST(stream), p11, n11, c11, p12, n12, c12, p22, n22, c22, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_identity_fwd(const float* x1, int64_t ld1, int32_t n1, const float* x2, int64_t ld2, int32_t n2,
                                   int32_t Z, float* diff, float* out, dv_stream_t stream) {
    DV_REQUIRE(x1 && x2 && diff && out && n1 >= 1 && n2 >= 1 && Z >= 1);
    hipLaunchKernelGGL(mmd_identity_fwd_kernel, dim3(1), dim3(256), 0, ST(stream), x1, ld1, n1, x2, ld2, n2, Z, diff, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mmd_identity_bwd(const float* diff, const float* gout, float coef, int32_t n, int32_t Z, float* dx,
                                   int64_t ldd, dv_stream_t stream) {
    DV_REQUIRE(diff && gout && dx && n >= 1 && Z >= 1);
    hipLaunchKernelGGL(mmd_identity_bwd_kernel, dim3(grid_for((int64_t)n * Z, 256)), dim3(256), 0, ST(stream), diff, gout,
                       coef, n, Z, dx, ldd);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_recon_finalize(const float* rows, const int32_t* sel, int32_t n, int32_t X, const double* cols,
                                 int32_t row_blocks, const float* ll, double* out, dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && X >= 1 && row_blocks >= 1 && rows && cols && out);
    hipLaunchKernelGGL(recon_finalize_kernel, dim3(1), dim3(1024), 0, ST(stream), rows, sel, n, X, cols, row_blocks, ll, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_reg_metrics(const float* pred, int64_t ldp, const float* y, int64_t ldy, const int32_t* sel, int32_t n,
                              int32_t Y, double* out, dv_stream_t stream) {
    DV_REQUIRE(pred && y && out && n >= 0 && Y >= 1 && ldp >= Y && ldy >= Y);
    hipLaunchKernelGGL(reg_metrics_kernel, dim3(1), dim3(1024), 0, ST(stream), pred, ldp, y, ldy, sel, n, Y, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_rank_metrics(const float* proba, int64_t ldp, const int32_t* y, const int32_t* pred, const int32_t* sel,
                               int32_t n, int32_t c0, int32_t n_cls, int32_t binary, int32_t* counts, double* out,
                               dv_stream_t stream) {
    DV_REQUIRE(n >= 0 && c0 >= 0 && n_cls >= 1 && n_cls <= 64 && proba && y && counts && out);
    if (n > DV_RANK_MAX_ROWS) return DV_ERR_UNSUPPORTED;
    if (n > 0)
        hipLaunchKernelGGL(pair_counts_kernel, dim3((n + 255) / 256, (n + kPairJ - 1) / kPairJ, n_cls), dim3(256), 0,
                           ST(stream), proba, ldp, y, sel, n, c0, binary, counts);
    hipLaunchKernelGGL(rank_finalize_kernel, dim3(n_cls), dim3(1024), 0, ST(stream), counts, y, pred, sel, n, c0, binary,
                       n_cls, out);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_bn_fwd(const float* x, int64_t ldx, int32_t M, int32_t N, const float* w, const float* b, float eps,
                         float* mean_out, float* rstd_out, float* y, int64_t ldy, float* running_mean,
                         float* running_var, float momentum, int32_t training, dv_stream_t stream) {
    DV_REQUIRE(M >= 1 && N >= 1 && x && y && mean_out && rstd_out && eps >= 0.f);
    DV_REQUIRE(training || (running_mean && running_var));
    hipLaunchKernelGGL(bn_fwd_kernel, dim3((N + 63) / 64), dim3(256), 0, ST(stream), x, ldx, M, N, w, b, eps, mean_out,
                       rstd_out, y, ldy, running_mean, running_var, momentum, training);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_bn_bwd(const float* dy, int64_t ldd, const float* x, int64_t ldx, const float* mean, const float* rstd,
                         const float* w, int32_t M, int32_t N, float* dx, int64_t lddx, float* dw, float* db,
                         int32_t training, dv_stream_t stream) {
    DV_REQUIRE(M >= 1 && N >= 1 && dy && x && mean && rstd);
    hipLaunchKernelGGL(bn_bwd_kernel, dim3((N + 63) / 64), dim3(256), 0, ST(stream), dy, ldd, x, ldx, mean, rstd, w, M, N,
                       dx, lddx, dw, db, training);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_mask_scale(const float* x, int64_t ldx, const float* mask, int64_t ldm, float scale, int32_t M,
                             int32_t N, float* y, int64_t ldy, dv_stream_t stream) {
    DV_REQUIRE(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return DV_OK;
    DV_REQUIRE(x && mask && y);
    hipLaunchKernelGGL(mask_scale_kernel, dim3(grid_for((int64_t)M * N, 256)), dim3(256), 0, ST(stream), x, ldx, mask,
                       ldm, scale, M, N, y, ldy);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_loss_assemble(const dv_loss_term* terms, int32_t n_terms, const float* w_elbo,
                                const float* w_cmpl, float* loss, const int32_t* halt, int32_t n_halt,
                                float* accum, dv_stream_t stream) {
    DV_REQUIRE(n_terms >= 0 && n_terms <= DV_MAX_LOSS_TERMS && (terms || n_terms == 0));
    DV_REQUIRE(n_halt >= 0 && (halt || n_halt == 0));
    DV_REQUIRE(w_elbo && w_cmpl && loss);
    LossTerms lt;
    lt.n = n_terms;
    for (int i = 0; i < n_terms; ++i) {
        DV_REQUIRE(terms[i].out >= 0 && terms[i].out < 5 && terms[i].n >= 0 && (terms[i].x || terms[i].n == 0));
        lt.t[i] = terms[i];
    }
    hipLaunchKernelGGL(loss_assemble_kernel, dim3(1), dim3(kLossThreads), 0, ST(stream), lt, w_elbo, w_cmpl, loss,
                       (int32_t*)nullptr, (const int32_t*)nullptr, 0, (int32_t*)nullptr, 0, CounterBump{}, halt, n_halt,
                       accum);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_loss_assemble_after(const dv_wait* wait, const dv_loss_term* terms, int32_t n_terms,
                                      const float* w_elbo, const float* w_cmpl, float* loss, const dv_bump* bump_in,
                                      const int32_t* halt, int32_t n_halt, float* accum, dv_stream_t stream) {
    DV_REQUIRE(n_halt >= 0 && (halt || n_halt == 0));
    DV_REQUIRE(n_terms >= 0 && n_terms <= DV_MAX_LOSS_TERMS && (terms || n_terms == 0));
    ParkArgs w;       // flag == NULL: no wait
    if (int rc = take_park(wait, 1, &w)) return rc;
    DV_REQUIRE(w_elbo && w_cmpl && loss);
    const CounterBump bump = bump_in ? *bump_in : CounterBump{};
    for (int i = 0; i < 2; ++i) DV_REQUIRE(!bump.c[i] || bump.n[i] == 1 || bump.n[i] == 2);
    LossTerms lt;
    lt.n = n_terms;
    for (int i = 0; i < n_terms; ++i) {
        DV_REQUIRE(terms[i].out >= 0 && terms[i].out <= 4 && terms[i].n >= 0 && (terms[i].x || terms[i].n == 0));
        lt.t[i] = terms[i];
    }
    hipLaunchKernelGGL(loss_assemble_kernel, dim3(1), dim3(kLossThreads), 0, ST(stream), lt, w_elbo, w_cmpl, loss, w.flag,
                       w.ctr, w.add, w.err, w.max_spins, bump, halt, n_halt, accum);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_axpby(const float* x, float a, float* y, float b, int64_t n, dv_stream_t stream) {
    DV_REQUIRE(n >= 0);
    if (n == 0) return DV_OK;
    DV_REQUIRE(x && y);
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ST(stream), x, a, y, b, n);
    DV_RETURN_LAUNCH();
}


// (see the declaration in front of dv_batch_feed: last in the file on purpose)
static void launch_batch_feed_csr(const dv_batch_feed_desc& d, dim3 grid, dim3 block, int row_blocks, bool v4, int mask_block,
                                  const MaskArgs& ma, const ParkArgs& park, dv_stream_t stream) {
    const int B = d.B, Np = d.Np, L = d.L, Mf = d.Mf;
    const CsrArgs csr{d.csr1_ptr, d.csr1_idx, d.csr1_val, d.csr2_ptr, d.csr2_idx, d.csr2_val};
    if (d.xt && d.transform == 3)
        hipLaunchKernelGGL((batch_feed_csr_kernel<true, true>), grid, block, 0, ST(stream), DV_FEED_ARGS, d.xt, d.ldt, d.transform, csr);
    else if (d.xt)
        hipLaunchKernelGGL((batch_feed_csr_kernel<true, false>), grid, block, 0, ST(stream), DV_FEED_ARGS, d.xt, d.ldt, d.transform, csr);
    else
        hipLaunchKernelGGL((batch_feed_csr_kernel<false, false>), grid, block, 0, ST(stream), DV_FEED_ARGS, nullptr, 0, 0, csr);
}
#undef DV_FEED_ARGS
