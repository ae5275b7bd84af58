// Fused Adam (coupled L2) over a flat fp32 arena, device-side step/RNG counters and the
// on-device N(0,1) generator (Philox4x32-10 + Box-Muller) of the Dr.VAE train step.
// All HBM-streaming: 16-B per lane, grid-stride, 7 words of traffic per parameter.
#include "dv_common.h"
#include <cstring>
#include <type_traits>

namespace {

struct AdamC {
    float lr_over_bc1, inv_unused, bc2_sqrt, eps, wd, one_minus_b1, b2, one_minus_b2, gscale;
};

// bias corrections from the device-side step counter, in double like torch's python floats
// (``n_skipped``: steps the non-finite guard of a clipped sweep has skipped -- they leave no trace in the corrections)
// (``lr_scale``: the learning-rate annealing coefficient of the step, a device scalar -- dv_adam_hyper.lr_scale; the rate is
// rounded to fp32 once, as the host's python float is when it is handed to a sweep; NULL or 1.0f: lr's own bits)
__device__ __forceinline__ void adam_consts(float lr, float b1, float b2, const int32_t* step_dev, float* step_size,
                                            float* bc2_sqrt, const float* lr_scale, int n_skipped = 0,
                                            float* decay = nullptr, float wd = 0.f) {
    if (lr_scale != nullptr) lr = (float)((double)lr * (double)lr_scale[0]);
    // decoupled weight decay (dv_adam_hyper.decoupled): p is multiplied by fl32(1 - lr_eff wd) before the update, the product
    // in double and rounded once like the rate itself (torch's python float 1 - lr * weight_decay handed to mul_)
    if (decay != nullptr) *decay = (float)(1.0 - (double)lr * (double)wd);
    const double t = (double)(step_dev[0] - n_skipped);
    const double bc1 = 1.0 - pow((double)b1, t);
    const double bc2 = 1.0 - pow((double)b2, t);
    *step_size = (float)((double)lr / bc1);
    *bc2_sqrt = (float)sqrt(bc2);
}

// DEC: decoupled weight decay (torch/optim/adamw.py, the same _single_tensor_adam): p *= 1 - lr*wd first -- ``wd`` then carries
// that factor -- and the gradient takes no wd*p term; everything behind it is the coupled form's sequence
template <bool DEC = false>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float step_size, float bc2_sqrt,
                                         float eps, float wd, float w1, float b2, float w2, float gscale) {
    // torch/optim/adam.py::_single_tensor_adam (2.x): grad += wd*p; m.lerp_(g, 1-b1);
    // v = v*b2 + (1-b2)*g*g; denom = sqrt(v)/sqrt(bc2) + eps; p += -(lr/bc1) * (m/denom)
    // Every fused multiply-add is written out and nothing else may be contracted: left to the compiler, the float4 loops
    // fused all four (g, m, v, p) while the scalar loops -- whose g*gscale | wd*p and v*b2 | (w2*g)*g the vectoriser packs
    // into one two-wide multiply each -- fused none of those two, so one element came out an ulp apart depending on the
    // alignment of the view it was swept through (tests/test_gpu_optim.py, path equality).  This is the float4 loops' form.
#pragma clang fp contract(off)
    if (DEC) {
        p = p * wd;
        g = g * gscale;
    } else {
        g = g * gscale;
        if (wd != 0.f) g = __builtin_fmaf(wd, p, g);
    }
    m = __builtin_fmaf(w1, g - m, m);
    v = __builtin_fmaf(w2 * g, g, v * b2);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = __builtin_fmaf(-step_size, m / denom, p);
}

// the parameter average (dv_adam_hyper.avg): e += w (p_new - e), w = fl32(1 - avg_decay); the subtraction rounded, one fma --
// the same form in every loop of every sweep
__device__ __forceinline__ void avg_one(float& e, float p_new, float w) {
#pragma clang fp contract(off)
    e = __builtin_fmaf(w, p_new - e, e);
}

// sticky error words of the step's device-side waits: (err, ticks) pairs, see dv_wait in drvae_hip.h
__device__ __forceinline__ int any_halt(const int32_t* halt, int n_halt) {
    int bad = 0;
    for (int i = 0; i < n_halt; ++i)
        bad |= __hip_atomic_load(halt + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    return bad;
}

// optional gate of the optimiser sweep: the elements [lo, hi) of the arena (gradients another launch chain
// still writes) are touched only after that chain has published `flag` (see dv_flag_publish)
struct AdamGate {
    int32_t* flag;
    const int32_t* ctr;
    int add;
    int32_t* err;
    int max_spins;
    int64_t lo, hi;
};

// CLIP: the sweep of a step with gradient-norm clipping (dv_adam_l2_clipped / dv_adamax_l2_clipped): ``clip`` is the record the norm pass has
// written -- skip set: nothing is touched (not sticky, no halt word involved); else gscale * coef scales the gradient and the
// bias corrections count the steps taken.  CLIP = false is the sweep as it ever was (adam_kernel and adam_stream_kernel: the same
// instructions but for the kernel-argument offsets; adamax_kernel: the same arithmetic, the halt loop scheduled in front of pow()).
// DEC: decoupled weight decay (dv_adam_hyper.decoupled; see adam_one).  AVG: the parameter average rides on the sweep
// (dv_adam_hyper.avg: one more stream, loaded and stored like p; a sweep that returns early touches none of it).  Both false is
// the sweep as it was: the flags are compile-time, the element loops of the plain instantiations carry no trace of them.
template <bool CLIP, bool DEC, bool AVG>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd_in, float gscale_in,
                                                   const int32_t* __restrict__ step_dev, int vec4, AdamGate gate,
                                                   const int32_t* __restrict__ halt, int n_halt,
                                                   const dv_clip_record* __restrict__ clip,
                                                   const float* __restrict__ lr_scale, float* __restrict__ avg,
                                                   float avg_decay) {
    __shared__ float sc[DEC ? 3 : 2];
    __shared__ int halted;
    // only the workgroups whose elements overlap the gated range park (typically one): a parked
    // workgroup or two can never starve the chain that is to publish
    bool need = false;
    if (gate.flag != nullptr) {
        const int64_t per = vec4 ? 4 : 1, span = (int64_t)blockDim.x * per;
        const int64_t bstride = (int64_t)gridDim.x * span;
        need = gate.hi > (vec4 ? ((n >> 2) << 2) : n) && gate.lo < n;       // the scalar tail (all workgroups sweep it)
        for (int64_t e0 = blockIdx.x * span; e0 < n; e0 += bstride) need = need || (e0 < gate.hi && e0 + span > gate.lo);
    }
    if (threadIdx.x == 0) {
        // (the gate's counter and flag and the error words are loaded FIRST: their round trips run under the two
        // double-precision pow() of the bias corrections instead of behind them)
        int want = 0, seen = 0;
        if (need) {
            want = gate.ctr[0] + gate.add;
            seen = __hip_atomic_load(gate.flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        }
        int h = any_halt(halt, n_halt);
        if (CLIP) {
            // a skipped first step has t = 0: the corrections are not evaluated, the sweep returns before it would use them
            if (clip->skip) h = 1;
            else if constexpr (DEC) adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, clip->n_skipped, &sc[2], wd_in);
            else adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, clip->n_skipped);
        } else {
            if constexpr (DEC) adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, 0, &sc[2], wd_in);
            else adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale);
        }
        if (need && seen - want < 0) {
            const long long t0 = wall_clock64();
            int k = 0;
            while (__hip_atomic_load(gate.flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - want < 0) {
                __builtin_amdgcn_s_sleep(4);
                if (++k > gate.max_spins) {
                    atomicExch(gate.err, 1);
                    break;
                }
            }
            atomicAdd(gate.err + 1, (int32_t)(wall_clock64() - t0));
            // one decision per workgroup, taken by the thread that waited (a per-thread re-read of the error words
            // could split a workgroup between updated and untouched elements)
            h = h || any_halt(halt, n_halt);
        }
        halted = h;
    }
    if (need) {
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every wave acquires (see park_block)
    }
    __syncthreads();
    // a chain wait has timed out (now or in an earlier step): the gradients may be built on stale data --
    // leave parameters and moments as they are (the loss scalars come out NaN, the host raises).  In the one step in
    // which THIS launch's gate times out only the parked workgroups see it: the others have swept their elements
    // already -- that step is applied everywhere but on the parked workgroups' elements (every span they visit, their
    // share of the scalar tail: at least the gated slice), every later one nowhere (tests/test_gpu_optim.py)
    if (halted) return;
    const float step_size = sc[0], bc2_sqrt = sc[1];
    float wd = wd_in;                                                    // DEC: the factor fl32(1 - lr_eff wd) in wd's place
    if constexpr (DEC) wd = sc[2];
    const float gscale = CLIP ? gscale_in * clip->coef : gscale_in;      // fl32(gscale * coef): coef == 1.0f gives gscale's bits
    // (float)(1 - beta) computed in double first, as python does before the op sees it
    const float w1 = (float)(1.0 - (double)b1), w2 = (float)(1.0 - (double)b2);
    const float wa = AVG ? (float)(1.0 - (double)avg_decay) : 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (vec4) {
        const int64_t n4 = n >> 2;
        float4* p4 = reinterpret_cast<float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
        float4* e4 = reinterpret_cast<float4*>(avg);
        for (int64_t i = t0; i < n4; i += stride) {
            float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ee;
            if (AVG) ee = e4[i];
            adam_one<DEC>(pp.x, gg.x, mm.x, vv.x, step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            adam_one<DEC>(pp.y, gg.y, mm.y, vv.y, step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            adam_one<DEC>(pp.z, gg.z, mm.z, vv.z, step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            adam_one<DEC>(pp.w, gg.w, mm.w, vv.w, step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            p4[i] = pp;
            m4[i] = mm;
            v4[i] = vv;
            if (AVG) {
                avg_one(ee.x, pp.x, wa);
                avg_one(ee.y, pp.y, wa);
                avg_one(ee.z, pp.z, wa);
                avg_one(ee.w, pp.w, wa);
                e4[i] = ee;
            }
        }
        for (int64_t i = (n4 << 2) + t0; i < n; i += stride) {
            adam_one<DEC>(p[i], g[i], m[i], v[i], step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            if (AVG) avg_one(avg[i], p[i], wa);
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            adam_one<DEC>(p[i], g[i], m[i], v[i], step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
            if (AVG) avg_one(avg[i], p[i], wa);
        }
    }
}

// The same sweep for arenas far larger than the Infinity Cache (wide configuration: 125 M parameters = 3.5 GB per step):
// two 16-B groups per thread in flight, non-temporal loads and stores (nothing of the sweep is read again before the next
// step has streamed gigabytes through the caches), 16384 workgroups.  tools/adam_probe.hip alone: 0.629 -> 0.564 ms = 5.57 -> 6.20
// TB/s (the guide's float4-copy figure is 6.29); inside the step (behind the dW products) 0.68 -> 0.63 ms.  Ungated (the chip-filling steps have no side chain to gate on).
typedef float adam_f4 __attribute__((ext_vector_type(4)));
template <bool CLIP, bool DEC, bool AVG>
__global__ __launch_bounds__(256) void adam_stream_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                          float b1, float b2, float eps, float wd_in, float gscale_in,
                                                          const int32_t* __restrict__ step_dev,
                                                          const int32_t* __restrict__ halt, int n_halt,
                                                          const dv_clip_record* __restrict__ clip,
                                                          const float* __restrict__ lr_scale, float* __restrict__ avg,
                                                          float avg_decay) {
    __shared__ float sc[DEC ? 3 : 2];
    __shared__ int halted;
    if (threadIdx.x == 0) {
        if (CLIP) {       // (see adam_kernel)
            const int skip = clip->skip;
            if (!skip) {
                if constexpr (DEC) adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, clip->n_skipped, &sc[2], wd_in);
                else adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, clip->n_skipped);
            }
            halted = any_halt(halt, n_halt) | skip;
        } else {
            if constexpr (DEC) adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale, 0, &sc[2], wd_in);
            else adam_consts(lr, b1, b2, step_dev, &sc[0], &sc[1], lr_scale);
            halted = any_halt(halt, n_halt);
        }
    }
    __syncthreads();
    if (halted) return;
    const float step_size = sc[0], bc2_sqrt = sc[1];
    float wd = wd_in;                                                    // (see adam_kernel)
    if constexpr (DEC) wd = sc[2];
    const float gscale = CLIP ? gscale_in * clip->coef : gscale_in;
    const float w1 = (float)(1.0 - (double)b1), w2 = (float)(1.0 - (double)b2);
    const float wa = AVG ? (float)(1.0 - (double)avg_decay) : 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n4 = n >> 2;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    adam_f4* p4 = reinterpret_cast<adam_f4*>(p);
    const adam_f4* g4 = reinterpret_cast<const adam_f4*>(g);
    adam_f4* m4 = reinterpret_cast<adam_f4*>(m);
    adam_f4* v4 = reinterpret_cast<adam_f4*>(v);
    adam_f4* e4 = reinterpret_cast<adam_f4*>(avg);
    for (int64_t i = t0; i < n4; i += 2 * stride) {
        adam_f4 pp[2], gg[2], mm[2], vv[2], ee[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t j = i + u * stride < n4 ? i + u * stride : i;
            pp[u] = __builtin_nontemporal_load(p4 + j);
            gg[u] = __builtin_nontemporal_load(g4 + j);
            mm[u] = __builtin_nontemporal_load(m4 + j);
            vv[u] = __builtin_nontemporal_load(v4 + j);
            if (AVG) ee[u] = __builtin_nontemporal_load(e4 + j);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = pp[u][e], b = mm[u][e], c = vv[u][e];
                adam_one<DEC>(a, gg[u][e], b, c, step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
                pp[u][e] = a; mm[u][e] = b; vv[u][e] = c;
                if (AVG) {
                    float d = ee[u][e];
                    avg_one(d, a, wa);
                    ee[u][e] = d;
                }
            }
            const int64_t j = i + u * stride;
            if (j < n4) {
                __builtin_nontemporal_store(pp[u], p4 + j);
                __builtin_nontemporal_store(mm[u], m4 + j);
                __builtin_nontemporal_store(vv[u], v4 + j);
                if (AVG) __builtin_nontemporal_store(ee[u], e4 + j);
            }
        }
    }
    for (int64_t i = (n4 << 2) + t0; i < n; i += stride) {
        adam_one<DEC>(p[i], g[i], m[i], v[i], step_size, bc2_sqrt, eps, wd, w1, b2, w2, gscale);
        if (AVG) avg_one(avg[i], p[i], wa);
    }
}

// ------------------------------------------------------------------ gradient-norm clipping
// Sum of squares of a contiguous fp32 range, in double from the square on (the square of a widened fp32 is exact in double),
// for the global-norm clip of the optimiser sweep.  Deterministic: the elements a thread visits, the wave tree, the order of the
// wave sums and the grid are functions of n and of the pointer's offset within 16 bytes alone -- no atomics; one double
// partial per workgroup, summed in index order by clip_finalize_kernel.  16-B loads over the aligned body (four in flight per
// lane), the <= 3 + 3 elements in front of and behind it by the first lanes of workgroup 0.  NT: non-temporal loads, for
// ranges far beyond the Infinity Cache (the threshold of the streaming sweep).
static inline int sumsq_blocks(int64_t n) { return (int)DV_SUMSQ_PARTIALS(n); }

template <bool NT>
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double wsum[4];
    int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15)) & 15u) >> 2);
    if (head > n) head = n;
    const int64_t n4 = (n - head) >> 2, tail0 = head + (n4 << 2);
    const adam_f4* g4 = reinterpret_cast<const adam_f4*>(g + head);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double acc = 0.0;
    for (int64_t i = t0; i < n4; i += 4 * stride) {
        adam_f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = i + u * stride;
            if (j < n4) x[u] = NT ? __builtin_nontemporal_load(g4 + j) : g4[j];
            else x[u] = adam_f4{0.f, 0.f, 0.f, 0.f};          // (+0.0 * +0.0 added to a sum that is never -0.0: no trace)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)x[u][e];
                acc = __builtin_fma(d, d, acc);
            }
        }
    }
    if (t0 < head) {
        const double d = (double)g[t0];
        acc = __builtin_fma(d, d, acc);
    }
    if (tail0 + t0 < n) {
        const double d = (double)g[tail0 + t0];
        acc = __builtin_fma(d, d, acc);
    }
    // wave tree (64 lanes), then the four wave sums in wave order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// the partials in index order -> the clip record of the step: norm = |gscale| sqrt(sumsq), coef = min(1, max_norm / (norm +
// 1e-6)) in double, stored as fp32; a non-finite sum of squares (some gradient element is inf or NaN: finite fp32 inputs cannot
// overflow the double sum) -> skip = 1, coef = 0 and the running count of skipped steps goes up by one
// (max_norm is device data the host cannot check: a value that is not > 0 clips nothing)
__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ part, int n_part, float gscale,
                                                            dv_clip_state* __restrict__ st) {
    dv_clip_record* rec = &st->rec;
    const double max_norm = st->max_norm;
    __shared__ double sp[DV_SUMSQ_MAX_BLOCKS];
    for (int i = threadIdx.x; i < n_part; i += blockDim.x) sp[i] = part[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n_part; ++i) s += sp[i];
    const int skip = !(fabs(s) <= 1.7976931348623157e308);       // inf or NaN
    const double norm = fabs((double)gscale) * sqrt(s);
    double coef = max_norm > 0.0 ? max_norm / (norm + 1e-6) : 1.0;
    coef = coef < 1.0 ? coef : 1.0;
    rec->norm = (float)norm;
    rec->coef = skip ? 0.f : (float)coef;
    rec->skip = skip;
    rec->n_skipped = rec->n_skipped + skip;
}

__global__ void counter_add_kernel(int32_t* c, int n_words, int64_t inc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counter_add_words(c, n_words, inc);
}

__global__ void counters_add2_kernel(int32_t* c1, int n1, int64_t inc1, int32_t* c2, int n2, int64_t inc2, dv_publish pub) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    publish_block0(pub);      // (before the counters move: pub.ctr may be one of them)
    counter_add_words(c1, n1, inc1);
    counter_add_words(c2, n2, inc2);
}

// ------------------------------------------------------------------ Philox4x32-10
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                             uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)x + 0.5f) * 2.3283064365386963e-10f; }

// 10 rounds of Philox4x32 in place: the four output words of counter (c0..c3) under key (k0, k1)
__device__ __forceinline__ void philox_block(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                             uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// four N(0,1) values of one block: Box-Muller over its word pairs (0, 1) and (2, 3)
__device__ __forceinline__ void philox_normal4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1, float (&z)[4]) {
    philox_block(c0, c1, c2, c3, k0, k1);
    const float r0 = sqrtf(-2.f * logf(u01(c0))), r1 = sqrtf(-2.f * logf(u01(c2)));
    float s0, co0, s1, co1;
    sincosf(6.283185307179586f * u01(c1), &s0, &co0);
    sincosf(6.283185307179586f * u01(c3), &s1, &co1);
    z[0] = r0 * co0;
    z[1] = r0 * s0;
    z[2] = r1 * co1;
    z[3] = r1 * s1;
}

// Row-keyed draws (SURVEY.md 8(e) "RNG under DP"): element (row, col) of the noise arena is
// Philox(key = seed ^ step_hi, counter = (col/4, global row, draw id, step_lo))[col%4], so a value depends only
// on WHICH draw of WHICH global minibatch row of WHICH step it is -- not on how rows are grouped into
// buffers or sharded over ranks.  desc[r] = {offset into arena (floats), width, draw id, global row};
// one wave per row.  (dv_fill_normal_rows)
// KEEPS: the noise arena of a step with hidden-layer dropout (dv_fill_noise_rows): rows [0, n_normal) of the table are those
// N(0,1) rows (same calls, same values); rows [n_normal, n_rows) are KEEP rows -- element (row, col) is 1.0f where word
// col % 4 of the same Philox block (counter and key laid out as for the normals) is < keep_thr, else 0.0f: an integer
// compare, no float uniform.  The row kind is wave-uniform.
template <bool KEEPS>
__global__ __launch_bounds__(256) void fill_rows_kernel(float* __restrict__ arena, const int4* __restrict__ desc,
                                                        int n_rows, uint64_t seed, const int32_t* ctr_dev,
                                                        dv_wait park) {
    park_block(park);         // (the counter below is read behind the wait: its advance is part of what is waited for)
    int n_normal = n_rows;
    uint32_t keep_thr = 0;
    if (KEEPS) {
        // the trailer row behind the table: {number of keep rows at the table's END, keep_thr's bits, 0, 0} -- counted from
        // the end, so that a caller may hand over the table from any of its rows on
        const int4 tr = desc[n_rows];
        // (device data the host cannot check: a count outside [0, n_rows] is clamped, never an index outside the table)
        n_normal = n_rows - (tr.x < 0 ? 0 : tr.x > n_rows ? n_rows : tr.x);
        keep_thr = (uint32_t)tr.y;
    }
    uint32_t step_lo = 0, step_hi = 0;
    if (ctr_dev) {
        step_lo = (uint32_t)ctr_dev[0];
        step_hi = (uint32_t)ctr_dev[1];
    }
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ step_hi;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwave = gridDim.x * (blockDim.x >> 6);
    for (int r = wave; r < n_rows; r += nwave) {
        const int4 d = desc[r];
        float* out = arena + d.x;
        const int w = d.y, w4 = (w + 3) >> 2;
        const bool al = ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
        const bool keep_row = KEEPS && r >= n_normal;
        for (int c = lane; c < w4; c += 64) {
            float z[4];
            if (keep_row) {
                uint32_t c0 = (uint32_t)c, c1 = (uint32_t)d.w, c2 = (uint32_t)d.z, c3 = step_lo;
                philox_block(c0, c1, c2, c3, k0, k1);
                z[0] = c0 < keep_thr ? 1.f : 0.f;
                z[1] = c1 < keep_thr ? 1.f : 0.f;
                z[2] = c2 < keep_thr ? 1.f : 0.f;
                z[3] = c3 < keep_thr ? 1.f : 0.f;
            } else {
                philox_normal4((uint32_t)c, (uint32_t)d.w, (uint32_t)d.z, step_lo, k0, k1, z);
            }
            const int o = c << 2;
            if (al && o + 4 <= w) {
                *reinterpret_cast<float4*>(out + o) = make_float4(z[0], z[1], z[2], z[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (o + e < w) out[o + e] = z[e];
            }
        }
    }
}

__global__ __launch_bounds__(256) void fill_normal_kernel(float* __restrict__ out, int64_t n, uint64_t seed,
                                                          const int32_t* __restrict__ ctr_dev) {
    uint64_t base = 0;
    if (ctr_dev) base = ((uint64_t)(uint32_t)ctr_dev[1] << 32) | (uint32_t)ctr_dev[0];
    const int64_t n4 = (n + 3) >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t ctr = base + (uint64_t)i;
        float z[4];
        philox_normal4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), z);
        const int64_t o = i << 2;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (o + e < n) out[o + e] = z[e];
    }
}

// ------------------------------------------------------------------ count sampler (dv_draw_desc)
// The posterior-predictive draw of every data decoder, element by element as include/drvae_hip.h specifies it ("The
// sampler", above dv_fill_normal): every value is a function of (seed, event, sample k, global row R, gene g) and the
// element's operands.  Block b of an element is Philox(counter = (g, R, (k << 8) | b, event_lo), key = (seed_lo,
// seed_hi ^ event_hi)).  Every loop is bounded (8 Gamma attempts, 64 inversion steps, 16 PTRS attempts); the loop bodies
// touch registers only.
struct draw_key {
    uint32_t k0, k1, g, R, ks, e_lo;      // ks = k << 8
};

__device__ __forceinline__ void draw_block(const draw_key& q, uint32_t b, uint32_t& w0, uint32_t& w1, uint32_t& w2,
                                           uint32_t& w3) {
    w0 = q.g;
    w1 = q.R;
    w2 = q.ks | b;
    w3 = q.e_lo;
    philox_block(w0, w1, w2, w3, q.k0, q.k1);
}

#define DV_DRAW_GAMMA_TRIES 8
#define DV_DRAW_POIS_BLOCK0 8          // the Poisson draw's first block behind a Gamma draw
#define DV_DRAW_PTRS_TRIES 16
#define DV_DRAW_INV_STEPS 64
#define DV_DRAW_GATE_BLOCK 16
#define DV_DRAW_LAM_MAX 16777216.f     // 2^24

// Poisson(lam), lam >= 0 (not NaN), from the blocks b0, b0 + 1, ...
__device__ __forceinline__ float draw_poisson(const draw_key& q, uint32_t b0, float lam) {
    if (!(lam < DV_DRAW_LAM_MAX)) return fminf(lam, 3.4028234663852886e38f);
    uint32_t w0, w1, w2, w3;
    draw_block(q, b0, w0, w1, w2, w3);
    if (lam < 10.f) {
        // inversion by sequential search from ONE uniform
        const float u = u01(w0);
        float p = expf(-lam), cdf = p, k = 0.f;
        bool done = !(u > cdf);
#pragma unroll 1
        for (int i = 1; i <= DV_DRAW_INV_STEPS && !done; ++i) {
            k = (float)i;
            p *= lam / k;
            cdf += p;
            done = !(u > cdf);
        }
        return done ? k : rintf(lam);
    }
    // Hoermann's PTRS (transformed rejection with squeeze)
    const float slam = sqrtf(lam), loglam = logf(lam);
    const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
    const float lia = logf(1.1239f + 1.1328f / (b - 3.4f)), vr = 0.9277f - 3.6224f / (b - 2.f);
#pragma unroll 1
    for (int j = 0; j < DV_DRAW_PTRS_TRIES; ++j) {
        if (j != 0 && !(j & 1)) draw_block(q, b0 + (uint32_t)(j >> 1), w0, w1, w2, w3);
        const float U = u01((j & 1) ? w2 : w0) - 0.5f, V = u01((j & 1) ? w3 : w1);
        const float us = 0.5f - fabsf(U);
        const float k = floorf((2.f * a / us + b) * U + lam + 0.43f);
        if (us >= 0.07f && V <= vr) return k;
        if (k < 0.f || (us < 0.013f && V > us)) continue;
        if (logf(V) + lia - logf(a / (us * us) + b) <= -lam + k * loglam - lgammaf(k + 1.f)) return k;
    }
    return rintf(lam);
}

// the rate of a negative-binomial element: G ~ Gamma(shape theta, scale m / theta) by Marsaglia-Tsang from blocks 0 .. 7
// (m > 0 finite, theta > 0, neither NaN)
__device__ __forceinline__ float draw_gamma_rate(const draw_key& q, float m, float theta) {
    if (theta > 3.4028234663852886e38f) return m;         // theta = +inf: the Poisson limit
    const bool boost = theta < 1.f;
    const float d = (boost ? theta + 1.f : theta) - 0.3333333333333333f, c = 1.f / sqrtf(9.f * d);
    float lg = 0.f, ub = 1.f;
    bool ok = false;
#pragma unroll 1
    for (uint32_t j = 0; j < DV_DRAW_GAMMA_TRIES && !ok; ++j) {
        uint32_t w0, w1, w2, w3;
        draw_block(q, j, w0, w1, w2, w3);
        if (j == 0) ub = u01(w3);
        const float x = sqrtf(-2.f * logf(u01(w0))) * cosf(6.283185307179586f * u01(w1));
        const float t = c * x;
        if (t > -1.f) {
            const float l1 = log1pf(t);
            const float h = 0.5f * x * x + d * (3.f * l1 - t * (3.f + t * (3.f + t)));
            if (logf(u01(w2)) < h) {
                ok = true;
                lg = logf(d / theta) + 3.f * l1;      // ln(G / theta): the two logarithms' magnitudes never meet
            }
        }
    }
    if (!ok) return m;                                     // (past the cap: the Gamma's mean)
    // theta < 1: + ln u / theta.  A theta so small that the quotient d / theta or ln u / theta overflows (a denormal) has no finite
    // q: the rate is 0 there, as it is for every q below exp's range
    if (boost) lg += logf(ub) / theta;
    if (!(lg < 3.4028234663852886e38f) || lg != lg) return 0.f;
    return m * expf(lg);
}

__device__ __forceinline__ float draw_element(int kind, const draw_key& q, float mu, float p2, float lgt, float s) {
    uint32_t w0, w1, w2, w3;
    if (kind == DV_RECON_GAUSS) {
        draw_block(q, 0u, w0, w1, w2, w3);
        return mu + p2 * (sqrtf(-2.f * logf(u01(w0))) * cosf(6.283185307179586f * u01(w1)));
    }
    if (kind == DV_RECON_BERNOULLI) {
        if (mu != mu) return mu;
        draw_block(q, 0u, w0, w1, w2, w3);
        return u01(w0) <= mu ? 1.f : 0.f;
    }
    const float m = s * mu;
    if (m != m) return m;
    if (kind == DV_RECON_POISSON) return m > 0.f ? draw_poisson(q, 0u, m) : 0.f;
    if (p2 != p2 || !(p2 > 0.f)) return __int_as_float(0x7fc00000);
    if (kind == DV_RECON_ZINB) {
        if (lgt != lgt) return lgt;
        draw_block(q, DV_DRAW_GATE_BLOCK, w0, w1, w2, w3);
        if (u01(w0) <= 1.f / (1.f + expf(-lgt))) return 0.f;
    }
    if (!(m > 0.f)) return 0.f;
    if (m > 3.4028234663852886e38f) return 3.4028234663852886e38f;      // m = +inf
    return draw_poisson(q, DV_DRAW_POIS_BLOCK0, draw_gamma_rate(q, m, p2));
}

// one workgroup per (1024-gene chunk, row, sample); QUAD: a thread owns four consecutive genes (16-byte loads and stores),
// else the genes tid, tid + 256, ... of the chunk.  Rows and samples beyond the grid's limits are walked by stride.
template <bool QUAD>
__global__ __launch_bounds__(256) void draw_kernel(dv_draw_desc d, uint64_t seed, const int32_t* __restrict__ ctr_dev) {
    uint32_t e_lo = 0, e_hi = 0;
    if (ctr_dev) {
        e_lo = (uint32_t)ctr_dev[0];
        e_hi = (uint32_t)ctr_dev[1];
    }
    draw_key q;
    q.k0 = (uint32_t)seed;
    q.k1 = (uint32_t)(seed >> 32) ^ e_hi;
    q.e_lo = e_lo;
    const int kind = d.kind;
    const float* p2 = kind == DV_RECON_GAUSS ? d.sd : d.theta;
    const int64_t ld2 = kind == DV_RECON_GAUSS ? d.lds : d.ldt;
    const int g0 = blockIdx.x * 1024;
    for (int k = blockIdx.z; k < d.S; k += gridDim.z) {
        q.ks = (uint32_t)(d.k0 + k) << 8;
        for (int r = blockIdx.y; r < d.M; r += gridDim.y) {
            q.R = d.grow ? (uint32_t)d.grow[r] : (uint32_t)(d.row0 + r);
            const float s = d.size ? d.size[r] : 1.f;
            const float* mu = d.mu + (int64_t)r * d.ldm;
            const float* pp = p2 ? p2 + (int64_t)r * ld2 : nullptr;
            const float* lg = d.logit ? d.logit + (int64_t)r * d.ldl : nullptr;
            float* out = d.out + (int64_t)k * d.sso + (int64_t)r * d.ldo;
            if (QUAD) {
                const int g = g0 + (threadIdx.x << 2);
                if (g < d.X) {      // (X % 4 == 0: the quad is whole)
                    const float4 m4 = *reinterpret_cast<const float4*>(mu + g);
                    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 t4 = pp ? *reinterpret_cast<const float4*>(pp + g) : z4;
                    const float4 l4 = lg ? *reinterpret_cast<const float4*>(lg + g) : z4;
                    float4 o = z4;
#pragma unroll 1
                    for (int e = 0; e < 4; ++e) {      // (one copy of the draw's code; the quad's lanes by selects)
                        q.g = (uint32_t)(g + e);
                        const float v = draw_element(kind, q, e == 0 ? m4.x : e == 1 ? m4.y : e == 2 ? m4.z : m4.w,
                                                     e == 0 ? t4.x : e == 1 ? t4.y : e == 2 ? t4.z : t4.w,
                                                     e == 0 ? l4.x : e == 1 ? l4.y : e == 2 ? l4.z : l4.w, s);
                        o.x = e == 0 ? v : o.x;
                        o.y = e == 1 ? v : o.y;
                        o.z = e == 2 ? v : o.z;
                        o.w = e == 3 ? v : o.w;
                    }
                    *reinterpret_cast<float4*>(out + g) = o;
                }
            } else {
#pragma unroll 1
                for (int i = 0; i < 4; ++i) {
                    const int g = g0 + (int)threadIdx.x + (i << 8);
                    if (g < d.X) {
                        q.g = (uint32_t)g;
                        out[g] = draw_element(kind, q, mu[g], pp ? pp[g] : 0.f, lg ? lg[g] : 0.f, s);
                    }
                }
            }
        }
    }
}

}  // namespace

#define ST(s) static_cast<hipStream_t>(s)

extern "C" int dv_abi_version(void) { return DV_ABI_VERSION; }

// torch.optim.Adamax (2.x `_single_tensor_adamax`), the other branch of src/DGMMixin.py:37-38:
// grad += wd*p; m.lerp_(g, 1-b1); u = max(u*b2, |g|+eps); p += -(lr/(1-b1^t)) * (m/u)
// AVG: the parameter average rides on the sweep (see adam_kernel); there is no decoupled Adamax
template <bool CLIP, bool AVG>
__global__ __launch_bounds__(256) void adamax_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ u, int64_t n, float lr,
                                                     float b1, float b2, float eps, float wd, float gscale_in,
                                                     const int32_t* __restrict__ step_dev,
                                                     const int32_t* __restrict__ halt, int n_halt,
                                                     const dv_clip_record* __restrict__ clip,
                                                     const float* __restrict__ lr_scale, float* __restrict__ avg,
                                                     float avg_decay) {
    __shared__ float sc[2];
    __shared__ int halted;
    if (threadIdx.x == 0) {
        // (the second correction goes to a local nobody reads: a store to the shared array of a template instantiation is not
        // dropped as dead, and the pow() behind it would stay)
        float clr0 = 0.f, unused;
        if (CLIP) {       // (see adam_kernel)
            const int skip = clip->skip;
            if (!skip) adam_consts(lr, b1, b2, step_dev, &clr0, &unused, lr_scale, clip->n_skipped);
            halted = any_halt(halt, n_halt) | skip;
        } else {
            adam_consts(lr, b1, b2, step_dev, &clr0, &unused, lr_scale);
            halted = any_halt(halt, n_halt);
        }
        sc[0] = clr0;
    }
    __syncthreads();
    if (halted) return;
    const float clr = sc[0];
    const float gscale = CLIP ? gscale_in * clip->coef : gscale_in;
    const float w1 = (float)(1.0 - (double)b1);
    const float wa = AVG ? (float)(1.0 - (double)avg_decay) : 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        float gg = g[i] * gscale;
        const float pp = p[i];
        if (wd != 0.f) gg = gg + wd * pp;
        const float mm = m[i] + w1 * (gg - m[i]);
        const float uu = fmaxf(u[i] * b2, fabsf(gg) + eps);
        m[i] = mm;
        u[i] = uu;
        const float pn = pp + (-clr) * (mm / uu);
        p[i] = pn;
        if (AVG) {
            float e = avg[i];
            avg_one(e, pn, wa);
            avg[i] = e;
        }
    }
}

/* sha256 over the library's sources (csrc/ *.hip *.inc *.h + include/drvae_hip.h, see drvae_amd/build.py::source_hash),
 * baked in at build time: lets a test on the GPU box assert that the shipped binary was built from the tree next to it */
#ifndef DV_SOURCE_HASH
#define DV_SOURCE_HASH "unhashed"
#endif
static const char dv_src_tag[] = DV_SOURCE_HASH;      /* "dv-src-sha256:<hex>": the tag lets build.py find it in the file */
extern "C" const char* dv_source_hash(void) {
    const char* c = strchr(dv_src_tag, ':');
    return c ? c + 1 : dv_src_tag;
}

extern "C" const char* dv_error_string(int code) {
    switch (code) {
        case DV_OK: return "ok";
        case DV_ERR_ARG: return "invalid argument";
        case DV_ERR_LAUNCH: return "kernel launch failed";
        case DV_ERR_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown error";
    }
}

// compile-time flags from run-time switches: f(integral_constant<bool, a>, <b>) and f(<a>, <b>, <c>)
template <typename F>
static void with_flags(bool a, bool b, F f) {
    auto second = [&](auto A) {
        if (b) f(A, std::true_type{});
        else f(A, std::false_type{});
    };
    if (a) second(std::true_type{});
    else second(std::false_type{});
}

template <typename F>
static void with_flags(bool a, bool b, bool c, F f) {
    with_flags(a, b, [&](auto A, auto B) {
        if (c) f(A, B, std::true_type{});
        else f(A, B, std::false_type{});
    });
}

// the trailing fields of dv_adam_hyper a sweep may not be launched with (checked before any launch)
static bool avg_ok(const dv_adam_hyper* h) {
    if (h->avg == nullptr) return true;
    return h->avg_decay > 0.f && h->avg_decay < 1.f && (reinterpret_cast<uintptr_t>(h->avg) & 3) == 0;
}

static int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                       const int32_t* step_dev, const AdamGate& gate, const int32_t* halt, int32_t n_halt,
                       dv_stream_t stream, const dv_clip_record* clip) {
    DV_REQUIRE(h != nullptr && n >= 0 && n_halt >= 0 && (halt || n_halt == 0));
    DV_REQUIRE(avg_ok(h));
    if (n == 0) return DV_OK;
    DV_REQUIRE(p && g && m && v && step_dev);
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const int vec4 = al(p) && al(g) && al(m) && al(v) && al(h->avg);      // (a NULL average is aligned)
    int64_t blocks = ((vec4 ? (n >> 2) : n) + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (vec4 && gate.flag == nullptr && n >= (int64_t(16) << 20)) {       // far beyond the Infinity Cache: the streaming sweep
        const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks));
        with_flags(clip != nullptr, h->decoupled != 0, h->avg != nullptr, [&](auto C, auto D, auto A) {
            hipLaunchKernelGGL((adam_stream_kernel<decltype(C)::value, decltype(D)::value, decltype(A)::value>), grid, dim3(256), 0,
                               ST(stream), p, g, m, v, n, h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->gscale, step_dev,
                               halt, n_halt, clip, h->lr_scale, h->avg, h->avg_decay);
        });
        DV_RETURN_LAUNCH();
    }
    if (blocks > 2048) blocks = 2048;
    with_flags(clip != nullptr, h->decoupled != 0, h->avg != nullptr, [&](auto C, auto D, auto A) {
        hipLaunchKernelGGL((adam_kernel<decltype(C)::value, decltype(D)::value, decltype(A)::value>), dim3((unsigned)blocks),
                           dim3(256), 0, ST(stream), p, g, m, v, n, h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->gscale,
                           step_dev, vec4, gate, halt, n_halt, clip, h->lr_scale, h->avg, h->avg_decay);
    });
    DV_RETURN_LAUNCH();
}

extern "C" int dv_adam_l2_gated(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                                const int32_t* step_dev, const dv_wait* gate, int64_t lo, int64_t hi,
                                const int32_t* halt, int32_t n_halt, dv_stream_t stream) {
    DV_REQUIRE(h != nullptr && gate != nullptr);
    DV_REQUIRE(gate->flag && gate->ctr && gate->err && gate->max_spins > 0 && lo >= 0 && hi >= lo && hi <= n);
    return adam_launch(p, g, m, v, n, h, step_dev, AdamGate{gate->flag, gate->ctr, gate->add, gate->err, gate->max_spins, lo, hi},
                       halt, n_halt, stream, nullptr);
}

static int adamax_launch(float* p, const float* g, float* m, float* u, int64_t n, const dv_adam_hyper* h,
                         const int32_t* step_dev, const int32_t* halt, int32_t n_halt, dv_stream_t stream,
                         const dv_clip_record* clip) {
    DV_REQUIRE(h != nullptr && n >= 0 && n_halt >= 0 && (halt || n_halt == 0));
    DV_REQUIRE(h->decoupled == 0 && avg_ok(h));       // (torch has no decoupled Adamax: nothing to be equal to)
    if (n == 0) return DV_OK;
    DV_REQUIRE(p && g && m && u && step_dev);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    with_flags(clip != nullptr, h->avg != nullptr, [&](auto C, auto A) {
        hipLaunchKernelGGL((adamax_kernel<decltype(C)::value, decltype(A)::value>), dim3((unsigned)blocks), dim3(256), 0, ST(stream),
                           p, g, m, u, n, h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->gscale, step_dev, halt, n_halt,
                           clip, h->lr_scale, h->avg, h->avg_decay);
    });
    DV_RETURN_LAUNCH();
}

// gradient-norm clipping: the NORM PASS (sum of squares into the workspace behind the state, then the record) and the two
// sweeps reading that record; the state's first word is the step they count by
extern "C" int dv_grad_norm_clip(const float* g, int64_t n, float gscale, dv_clip_state* st, dv_stream_t stream) {
    DV_REQUIRE(st && (reinterpret_cast<uintptr_t>(st) & 7) == 0);
    DV_REQUIRE(n >= 0 && (g || n == 0) && (reinterpret_cast<uintptr_t>(g) & 3) == 0);
    double* part = reinterpret_cast<double*>(st + 1);
    const int blocks = sumsq_blocks(n);
    if (n >= (int64_t(16) << 20))
        hipLaunchKernelGGL(sumsq_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ST(stream), g, n, part);
    else
        hipLaunchKernelGGL(sumsq_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ST(stream), g, n, part);
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, ST(stream), part, blocks, gscale, st);
    DV_RETURN_LAUNCH();
}

static_assert(sizeof(dv_clip_state) == 32 && DV_SUMSQ_PARTIALS(1) == 1 && DV_SUMSQ_PARTIALS(int64_t(1) << 40) == DV_SUMSQ_MAX_BLOCKS,
              "dv_clip_state / DV_SUMSQ_PARTIALS of the header");

extern "C" int dv_adam_l2(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                          const int32_t* step_dev, const int32_t* halt, int32_t n_halt, dv_stream_t stream) {
    return adam_launch(p, g, m, v, n, h, step_dev, AdamGate{}, halt, n_halt, stream, nullptr);
}

extern "C" int dv_adam_l2_clipped(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                                  const dv_clip_state* st, const int32_t* halt, int32_t n_halt, dv_stream_t stream) {
    DV_REQUIRE(st && (reinterpret_cast<uintptr_t>(st) & 7) == 0);
    return adam_launch(p, g, m, v, n, h, &st->step, AdamGate{}, halt, n_halt, stream, &st->rec);
}

extern "C" int dv_adamax_l2(float* p, const float* g, float* m, float* u, int64_t n, const dv_adam_hyper* h,
                            const int32_t* step_dev, const int32_t* halt, int32_t n_halt, dv_stream_t stream) {
    return adamax_launch(p, g, m, u, n, h, step_dev, halt, n_halt, stream, nullptr);
}

extern "C" int dv_adamax_l2_clipped(float* p, const float* g, float* m, float* u, int64_t n, const dv_adam_hyper* h,
                                    const dv_clip_state* st, const int32_t* halt, int32_t n_halt, dv_stream_t stream) {
    DV_REQUIRE(st && (reinterpret_cast<uintptr_t>(st) & 7) == 0);
    return adamax_launch(p, g, m, u, n, h, &st->step, halt, n_halt, stream, &st->rec);
}

// Device-side ordering between two concurrently running launch chains (two root branches of one
// hipGraph): the producer chain publishes flag = ctr + add after the kernel whose results are
// needed, the consumer chain parks a one-thread kernel on the flag.  Data visibility is provided by
// the ordinary kernel boundaries on either side; only the flag itself is accessed atomically.
__global__ void flag_publish_kernel(int32_t* flag, const int32_t* ctr, int add) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, ctr[0] + add, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void flag_wait_kernel(int32_t* flag, const int32_t* ctr, int add, int32_t* err, int max_spins, dv_publish pub) {
    if (threadIdx.x != 0) return;
    // (pub: published on entry, like dv_flag_publish -- everything before this launch in its stream is complete)
    publish_block0(pub);
    const int want = ctr[0] + add;
    const long long t0 = wall_clock64();
    int n = 0;
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - want < 0) {
        __builtin_amdgcn_s_sleep(4);
        if (++n > max_spins) {       // never hang the device: report and let the chain run on
            atomicExch(err, 1);
            break;
        }
    }
    atomicAdd(err + 1, (int32_t)(wall_clock64() - t0));   // time parked, in constant-clock ticks (tuning statistic; no-return atomic)
}

extern "C" int dv_flag_publish(int32_t* flag, const int32_t* ctr, int32_t add, dv_stream_t stream) {
    DV_REQUIRE(flag && ctr);
    hipLaunchKernelGGL(flag_publish_kernel, dim3(1), dim3(64), 0, ST(stream), flag, ctr, add);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_flag_wait(int32_t* flag, const int32_t* ctr, int32_t add, int32_t* err, int32_t max_spins,
                            const dv_publish* pub_in, dv_stream_t stream) {
    DV_REQUIRE(flag && ctr && err && max_spins > 0);
    dv_publish pub;
    if (int rc = take_publish(pub_in, &pub)) return rc;
    hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, ST(stream), flag, ctr, add, err, max_spins, pub);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_counter_add(int32_t* counter_lo_hi, int32_t n_words, int64_t inc, dv_stream_t stream) {
    DV_REQUIRE(counter_lo_hi && (n_words == 1 || n_words == 2));
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, ST(stream), counter_lo_hi, n_words, inc);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_counters_add2(int32_t* c1, int32_t n1, int64_t inc1, int32_t* c2, int32_t n2, int64_t inc2,
                                const dv_publish* pub_in, dv_stream_t stream) {
    DV_REQUIRE(c1 && c2 && (n1 == 1 || n1 == 2) && (n2 == 1 || n2 == 2));
    dv_publish pub;
    if (int rc = take_publish(pub_in, &pub)) return rc;
    hipLaunchKernelGGL(counters_add2_kernel, dim3(1), dim3(64), 0, ST(stream), c1, n1, inc1, c2, n2, inc2, pub);
    DV_RETURN_LAUNCH();
}

// the two row-keyed fills (dv_fill_noise_rows: the table's trailer sits at row n_rows): the park's validation, the grid -- one
// wave per row, four rows per workgroup -- and the launch
template <bool KEEPS>
static int fill_rows_launch(float* arena, const int32_t* desc, int32_t n_rows, uint64_t seed, const int32_t* ctr_dev,
                            const dv_wait* park_in, dv_stream_t stream) {
    DV_REQUIRE(n_rows >= 0);
    dv_wait park = park_in ? *park_in : dv_wait{nullptr, nullptr, 0, 0, nullptr};
    DV_REQUIRE(park.flag == nullptr || (park.ctr && park.err && park.max_spins > 0));
    if (n_rows == 0) return park.flag ? DV_ERR_UNSUPPORTED : DV_OK;
    DV_REQUIRE(arena && desc && (reinterpret_cast<uintptr_t>(desc) & 15) == 0);
    int blocks = (n_rows + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    if (park.flag != nullptr && blocks > 512) blocks = 512;      // a parked grid stays well below the chip's resident capacity
    hipLaunchKernelGGL(fill_rows_kernel<KEEPS>, dim3((unsigned)blocks), dim3(256), 0, ST(stream), arena,
                       reinterpret_cast<const int4*>(desc), n_rows, seed, ctr_dev, park);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_fill_normal_rows(float* arena, const int32_t* desc, int32_t n_rows, uint64_t seed,
                                   const int32_t* ctr_dev, const dv_wait* park, dv_stream_t stream) {
    return fill_rows_launch<false>(arena, desc, n_rows, seed, ctr_dev, park, stream);
}

extern "C" int dv_fill_noise_rows(float* arena, const int32_t* table, int32_t n_rows, uint64_t seed,
                                  const int32_t* ctr_dev, const dv_wait* park, dv_stream_t stream) {
    return fill_rows_launch<true>(arena, table, n_rows, seed, ctr_dev, park, stream);
}

// the sampler launch of dv_fill_normal (draw != NULL): every refusal in front of the launch, at M == 0 / S == 0 too
static int draw_launch(const dv_draw_desc* dp, uint64_t seed, const int32_t* ctr_dev, dv_stream_t stream) {
    const dv_draw_desc d = *dp;
    const int64_t X = d.X;
    DV_REQUIRE(d.kind >= DV_RECON_GAUSS && d.kind <= DV_RECON_ZINB);
    DV_REQUIRE(d.M >= 0 && d.X >= 0 && d.S >= 0 && d.k0 >= 0 && (int64_t)d.k0 + d.S <= DV_DRAW_MAX_SAMPLES);
    DV_REQUIRE(d.row0 >= 0 && d.row0 + (int64_t)d.M <= DV_DRAW_MAX_ROW && (d.grow == nullptr || d.row0 == 0));
    const bool nb = d.kind == DV_RECON_NEGBIN || d.kind == DV_RECON_ZINB;
    DV_REQUIRE(d.mu != nullptr && d.ldm >= X);
    DV_REQUIRE(d.kind != DV_RECON_GAUSS || (d.sd != nullptr && d.lds >= X));
    DV_REQUIRE(!nb || (d.theta != nullptr && (d.ldt == 0 || d.ldt >= X)));
    DV_REQUIRE(d.kind != DV_RECON_ZINB || (d.logit != nullptr && d.ldl >= X));
    DV_REQUIRE(d.size == nullptr || d.kind >= DV_RECON_POISSON);
    DV_REQUIRE(d.ldo >= X && (d.S <= 1 || d.M == 0 || d.sso >= (int64_t)(d.M - 1) * d.ldo + X));
    if (d.M == 0 || d.X == 0 || d.S == 0) return DV_OK;
    DV_REQUIRE(d.out != nullptr);
    // the quad path: every row of every operand the kind reads starts on a 16-byte boundary
    auto al = [](const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; };
    bool quad = (d.X & 3) == 0 && al(d.mu, d.ldm) && al(d.out, d.ldo) && (d.sso & 3) == 0;
    if (d.kind == DV_RECON_GAUSS) quad = quad && al(d.sd, d.lds);
    if (nb) quad = quad && al(d.theta, d.ldt);
    if (d.kind == DV_RECON_ZINB) quad = quad && al(d.logit, d.ldl);
    dv_draw_desc k = d;       // (the kernel reads the operands of its kind only)
    if (d.kind != DV_RECON_GAUSS) k.sd = nullptr;
    if (!nb) k.theta = nullptr;
    if (d.kind != DV_RECON_ZINB) k.logit = nullptr;
    const dim3 grid((unsigned)((d.X + 1023) / 1024), (unsigned)(d.M < 65535 ? d.M : 65535), (unsigned)(d.S < 1024 ? d.S : 1024));
    if (quad) hipLaunchKernelGGL(draw_kernel<true>, grid, dim3(256), 0, ST(stream), k, seed, ctr_dev);
    else hipLaunchKernelGGL(draw_kernel<false>, grid, dim3(256), 0, ST(stream), k, seed, ctr_dev);
    DV_RETURN_LAUNCH();
}

extern "C" int dv_fill_normal(float* out, int64_t n, uint64_t seed, const int32_t* ctr_dev, dv_stream_t stream,
                              const dv_draw_desc* draw) {
    if (draw != nullptr && draw->fx != nullptr) {       // the effect reduction (rows.hip): the outer descriptor carries M and X only
        const dv_draw_desc& d = *draw;
        DV_REQUIRE(out == nullptr && n == 0 && seed == 0 && ctr_dev == nullptr);
        DV_REQUIRE(d.kind == 0 && d.S == 0 && !d.mu && d.ldm == 0 && !d.sd && d.lds == 0 && !d.theta && d.ldt == 0 && !d.logit &&
                   d.ldl == 0 && !d.size && !d.out && d.ldo == 0 && d.sso == 0 && d.row0 == 0 && !d.grow && d.k0 == 0);
        return dv_effect_cols_launch(*d.fx, d.M, d.X, stream);
    }
    if (draw != nullptr) return draw_launch(draw, seed, ctr_dev, stream);
    DV_REQUIRE(n >= 0);
    if (n == 0) return DV_OK;
    DV_REQUIRE(out);
    int64_t blocks = (((n + 3) >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), out, n, seed, ctr_dev);
    DV_RETURN_LAUNCH();
}
