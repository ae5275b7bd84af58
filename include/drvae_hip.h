/* drvae_hip.h -- C-ABI of libdrvae_hip.so: the Dr.VAE ELBO training hot path as
 * hand-written HIP kernels for gfx950 (MI355X / CDNA4).
 *
 * The reference (rampasek/DrVAE, pure Python on PyTorch CPU ATen, no native layer,
 * no FFI) reaches this arithmetic only through `import blocks as blk` /
 * `import layers as lyr` (src/DrVAE.py:21, src/blocks.py:12).  The Python modules
 * `drvae_amd.blocks` / `drvae_amd.layers` mirror that interface and call the entry
 * points below through ctypes (INTEGRATION.md shows the stub).  Each entry point
 * cites the reference expression it replaces.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, int sizes, leading dimensions in ELEMENTS,
 *    `dv_stream_t` = hipStream_t passed as void*.  No torch types.
 *  - all matrices fp32 row-major with unit inner stride; index arrays int32.
 *  - every call only ENQUEUES work on `stream`: no allocation, no host sync, no
 *    hidden state (nothing is armed, cached or remembered between calls: whatever a launch
 *    waits on or advances is an explicit argument of THAT call) -> re-entrant and
 *    hipGraph-capturable (SURVEY.md 8(b) threading).
 *  - returns DV_OK (0) or a negative DV_ERR_* code; never throws, never aborts.
 *  - `beta` arguments: out = beta*out + result (beta == 0 never reads out).
 */
#ifndef DRVAE_HIP_H
#define DRVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dv_stream_t;

#define DV_ABI_VERSION 13

enum { DV_OK = 0, DV_ERR_ARG = -1, DV_ERR_LAUNCH = -2, DV_ERR_UNSUPPORTED = -3 };

/* activation ids -- the `nonlinearities` table of src/blocks.py:21-24 (+ cos for the
 * random-Fourier MMD features of src/blocks.py:53-54; forward only) */
enum {
    DV_ACT_IDENTITY = 0, DV_ACT_ELU = 1, DV_ACT_SOFTPLUS = 2, DV_ACT_SIGMOID = 3, DV_ACT_TANH = 4,
    DV_ACT_RELU = 5, DV_ACT_LEAKY_RELU = 6, DV_ACT_SELU = 7, DV_ACT_SOFTSIGN = 8, DV_ACT_COS = 9
};

/* Gaussian parametrisation: GaussianLogVarMixin (src/blocks.py:166-202) or
 * GaussianSigmaMixin (src/blocks.py:204-240) */
enum { DV_GAUSS_LOGVAR = 0, DV_GAUSS_SIGMA = 1 };

enum { DV_EPI_PLAIN = 0, DV_EPI_FWD = 1, DV_EPI_BWD = 2, DV_EPI_KLQ = 3 };

int dv_abi_version(void);
const char* dv_error_string(int code);
/* hex sha256 over the sources this binary was built from (every file of drvae_amd/csrc/ that is compiled or included,
 * in name order, + this header; `drvae_amd.build.source_hash()` recomputes it from a tree) -- "unhashed" for a build that
 * did not go through drvae_amd/build.py.  The reference has no native layer, hence no counterpart. */
const char* dv_source_hash(void);

/* A device-side wait carried by a launch (see dv_flag_wait): the launch first parks until
 * flag[0] >= ctr[0] + add.  Bounded: after max_spins polls it records err[0] = 1 (sticky: nothing on
 * the device clears it) and goes on; err[1] accumulates the time parked (wall_clock64 ticks).  Every
 * consumer of err words -- dv_loss_assemble*, dv_adam_l2*, dv_adamax_l2 through their `halt`
 * argument -- then poisons the loss scalars with NaN and freezes the parameters, so a timed-out wait
 * can never train on stale data silently.  flag == NULL: no wait. */
typedef struct dv_wait {
    int32_t* flag;
    const int32_t* ctr;
    int32_t add;
    int32_t max_spins;
    int32_t* err;
} dv_wait;

/* "this launch has started, so everything in front of it in its stream is complete": a launch that carries a
 * dv_publish stores flag[0] = ctr[0] + add (release, agent scope) on entry, like dv_flag_publish but without a
 * launch of its own (dv_gemm_desc has the same three fields).  flag == NULL / NULL pointer: nothing published */
typedef struct dv_publish {
    int32_t* flag;
    const int32_t* ctr;
    int32_t add;
} dv_publish;

/* The KL rows of the fprop rows riding on the classifier-head launch, in front of and behind its y-marginalisation
 * (dv_smalln_linear_fwd with a dv_ymarg AND a dv_fprop_kl argument; train step): for every fprop row t of classifier
 * row r (fp_ptr of the dv_ymarg): raw1[t] = KL(q(z1|x)[qidx[t]] || p(z1|z3,y)[t]), raw3[t] = KL(q(z3|z1,y)[t] || N(0,I)),
 * klfp[t] = max(raw1, kl_min) + max(raw3, kl_min) (dv_kl_rows_fwd with its second term; LOGVAR parametrisation), then the
 * classifier head and the y-marginalisation, then the backward of the z1 term with the coefficient the y-marginalisation
 * has just produced: row-aligned d/d(q) -> dq, d/d(p) -> dp (dv_kl_rows_bwd, free bits, beta = 0).  mu_q == NULL: none */
typedef struct dv_fprop_kl {
    const float* mu_q;         /* (mu | logvar) rows of q(z1|x), ld = ldq; logvar at column offset Z1 of the same row */
    int64_t ldq;
    const int32_t* qidx;
    const float* mu_p;         /* (mu | logvar) of p(z1|z3,y), row t */
    int64_t ldp;
    const float* mu3;          /* (mu | logvar) of q(z3|z1,y), row t; Z3 columns each */
    int64_t ld3;
    int32_t Z1;
    int32_t Z3;
    float kl_min;
    float* klfp;               /* out, per fprop row (the dv_ymarg's klfp must be this buffer) */
    float* raw1;
    float* raw3;
    float* dq;                 /* out (Mf, 2*Z1): d/d(mu_q | logvar_q), row-aligned */
    int64_t lddq;
    float* dp;                 /* out (Mf, 2*Z1): d/d(mu_p | logvar_p) */
    int64_t lddp;
} dv_fprop_kl;

/* up to two device counters (1 or 2 int32 words each: int32 / uint64 little-endian) advanced by a
 * launch that carries the bump (see dv_counters_add2); c == NULL: unused slot */
/* y-marginalisation riding on the classifier-head launch (dv_smalln_linear_fwd): the arguments of dv_ymarg_fwdbwd
 * (src/DrVAE.py:503-534); fp_ptr == NULL: none */
typedef struct dv_ymarg {
    const int32_t* label;
    const int32_t* fp_ptr;
    const float* klfp;
    float log_prior;
    const float* log_prior_v;
    const float* c_kld;
    const float* c_yl;
    float* yl;
    float* kld;
    float* cfp;
    float* dqy;
    int64_t lddq;
} dv_ymarg;

/* The classifier's data gradient riding on the classifier-head launch (dv_smalln_linear_fwd with a dv_ymarg argument;
 * train step): the wave that owns row r has stored dqy[r]; it forms the row's d logits from (dqy[r], probs[r]) as
 * dv_smalln_linear_bwd_data does and writes, for up to two destinations t < n,
 *   dst_t[r, c] = beta_t*dst_t[r, c] + sum_j dlogit[r,j] * (alpha_t*W[j, col0_t + c] + alpha2_t*W[j, col1_t + c]),  c < ncol_t
 * (the arithmetic of that launch without its `seg` start: same bits).  n == 0: none */
typedef struct dv_clf_dgrad {
    float* dst[2];
    int64_t ld[2];
    int32_t col0[2];
    int32_t ncol[2];
    float alpha[2];
    float beta[2];
    int32_t col1[2];
    float alpha2[2];
    int32_t n;
} dv_clf_dgrad;

typedef struct dv_bump {
    int32_t* c[2];
    int32_t n[2];
    int64_t inc[2];
} dv_bump;

/* ------------------------------------------------------------------ GEMM family
 * C[M,N] = epilogue( alpha * sum_k Aop[m,k] * Bop[k,n] ) + beta*C      (fp32 MFMA,
 * v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fma chain -- no reduced precision).
 *   a_kcontig: Aop[m,k] = A[m*lda + k]   else A[k*lda + m]
 *   b_kcontig: Bop[k,n] = B[n*ldb + k]   else B[k*ldb + n]
 * which covers the three products of a Linear layer y = x W^T (+b):
 *   forward      y  = x  W^T      a_kcontig=1 b_kcontig=1   F.linear, src/layers.py:38,
 *                                                            nn.Linear in src/blocks.py:144,278-279,396-397,446
 *   backward dx  dx = dy W        a_kcontig=1 b_kcontig=0   (autograd AddmmBackward in the reference)
 *   backward dW  dW = dy^T x      a_kcontig=0 b_kcontig=0
 * A2/K1: optional second A source for k >= K1 -- `torch.cat(inputs, 1)` of
 *   src/blocks.py:161 without materialising the concat (a_kcontig only).
 * a_kscale: optional per-k multiplier on Aop (WeightNorm backward: dy * g/||W||).
 *
 * epilogue DV_EPI_FWD (per element, col = n):
 *   v = scale[n]*v (WeightNorm g/||W||, src/layers.py:39-40) + bias[n];
 *   v = act(v) + shift, with (act0,shift0) for n < split and (act1,shift1) otherwise
 *       -- dual heads sharing one GEMM: `logvar = lv(h) - 2.` (src/blocks.py:296,360),
 *          `std = softplus(sg(h)) + 1e-3` (src/blocks.py:401,415);
 *   v += resid[m*ldr+n] for n < resid_cols  -- `mu = x + F.linear(x,W_mu) + b` (src/blocks.py:357).
 * epilogue DV_EPI_BWD: v *= act'(yref[m*ldy+n] - shift) with the same (split, act, shift)
 * epilogue DV_EPI_KLQ (round 5): the product is d/dz of a reparameterised sample z = mu + eps * exp(logvar / 2) of q rows that
 *   also carry a prior term coef[m] * max(KL(q_m || N(0,I)), kl_min): with Z = split, for columns n < Z the launch writes the
 *   gradient w.r.t. (mu | logvar) instead of v -- C[m, n] = c_m * mu + v, C[m, Z + n] = c_m * (e^logvar - 1) / 2 +
 *   v * eps[m, n] * e^(logvar / 2) / 2, c_m = coef[m] * gate(raw[m]) (1 above kl_min, 1/2 on a tie, 0 below) -- what
 *   dv_kl_rows_bwd(dz = v, eps) computes in a launch of its own; columns n >= Z are dropped.  Operands travel in fields this
 *   epilogue does not otherwise use: yref / ldy = the q rows (mu | logvar), resid / ldr = eps, bias = coef (per ROW),
 *   scale = raw (per ROW), shift0 = kl_min; ldc >= 2 Z, beta = 0.
 *   selection: the activation backward of the layer BELOW fused into the dx GEMM.
 */
/* Per-call steering of the GEMM dispatcher (ABI 9; replaces the process-global dv_gemm_force_tiling / dv_gemm_set_option
 * hooks of ABI <= 8).  tiling: see dv_gemm_has_tiling.  opt[0] = workgroup -> tile map (-1 by tiling, 0 linear, 1 XCD
 * chunk-major, >= 2 bands of that many tile rows); opt[1] extra dynamic LDS of the chip-filling 32x32 launches; opt[2] = 1:
 * no fused form of dv_gemm_pair; opt[3]: tiles of 64x64 from which the 64x64 tiling runs (-1: never the hand-pipelined
 * LDS-DMA kernels); opt[4] heads kernel variant (dv_gemm_heads): 0 = by rule -- a sample-mode launch with few 32-row tiles and a
 * long K runs on 16 x (8 + 8) tiles, the same bits (csrc/heads_route.h) --, 3 = the seven-per-CU kernel at any size, 4 = the
 * 16-row tile wherever it can run (sample mode, operands fit for the LDS-DMA ring; otherwise as 0), 5 = never the 16-row
 * tile; opt[5] > 0 (opt-in, tuning): the 128x256 tiling's second resident workgroup of a CU starts that many percent of an estimated half tile late under a plain epilogue; opt[6] = -1: a chip-filling plain product with a ragged last column of
 * 128x256 tiles is NOT split into [full tiles | narrow rest] (dv_gemm: two launches where that saves a tile per CU); opt[7]: the latency-bound 32x32x64 launches (dv_gemm, dv_gemm_heads, the fused dv_gemm_pair): 0 = the LDS-DMA ring's depth by rule --
 * three slots of one 64-deep K tile for long reductions on grids of at most 192 workgroups, otherwise two; every depth stores the same
 * bits (csrc/ring_route.h) --, 1 = four-wave K split for the k-contiguous layouts (ring of two), 2 = four ring slots wherever these
 * kernels run, 3 = three slots, 4 = never a deeper ring (two slots everywhere); opt[8]: tiles of
 * 32x32 from which the seven-per-CU tiling runs; opt[9] = 1: chip-filling dW || dX as two launches */
typedef struct dv_gemm_tune {
    int32_t tiling;
    int32_t opt[10];
} dv_gemm_tune;

typedef struct dv_gemm_desc {
    int32_t M, N, K;
    int32_t a_kcontig, b_kcontig;
    const float* A;
    int64_t lda;
    const float* A2;
    int64_t lda2;
    int32_t K1;
    const float* a_kscale;
    const float* B;
    int64_t ldb;
    float* C;
    int64_t ldc;
    float alpha, beta;
    int32_t epilogue;
    const float* scale;
    const float* bias;
    int32_t split;
    int32_t act0, act1;
    float shift0, shift1;
    const float* resid;
    int64_t ldr;
    int32_t resid_cols;
    const float* yref;
    int64_t ldy;
    /* optional fused bias gradient (a_kcontig == 0 only, i.e. the dW product where
     * Aop[m,k] = dy[k, m]):  a_colsum[m] = colsum_beta*a_colsum[m] + sum_k Aop[m,k]
     * -- `db = dy.sum(0)` computed from the dy tiles the dW GEMM stages anyway. */
    float* a_colsum;
    float colsum_beta;
    /* bit0 / bit1: reading up to 3 floats past the END OF ANY ROW of A / B stays inside the
     * caller's allocation (rows padded to 4 floats, or followed by more of the same buffer).
     * Lets edge tiles of row-contiguous operands use aligned 16-B loads (the over-read values
     * only feed output elements that are never stored).  0 = never over-read (default). */
    int32_t flags;
    /* optional: on kernel ENTRY (i.e. once everything before this launch in its stream is complete)
     * publish pub_flag[0] = pub_ctr[0] + pub_add like dv_flag_publish -- saves the separate launch. */
    int32_t* pub_flag;
    const int32_t* pub_ctr;
    int32_t pub_add;
    /* optional (tests / tuning; NULL = the dispatcher's heuristics): read on the host at launch time, per call */
    const struct dv_gemm_tune* tune;
} dv_gemm_desc;

int dv_gemm(const dv_gemm_desc* desc, dv_stream_t stream);
/* Two independent products in one launch when both take the 32x32 K-split tiling with the
 * (dy^T x) and (dy W) layouts -- the weight- and data-gradient of one Linear layer, which both
 * only need dy; otherwise exactly dv_gemm(d1) followed by dv_gemm(d2).  At most ONE of the two descriptors may
 * carry a publish (pub_flag): the launch publishes once, on entry (DV_ERR_ARG when both do). */
int dv_gemm_pair(const dv_gemm_desc* d1, const dv_gemm_desc* d2, dv_stream_t stream);
/* OPT-IN split-bf16 product ("dtype: bf16x3"; drvae_amd/csrc/gemm_x3.hip): the same descriptor, C = epilogue(alpha * Aop Bop)
 * + beta * C, on the bf16 matrix pipe.  Every fp32 operand element a is split as hi = bf16_rn(a), mid = bf16_rn(a - hi),
 * lo = bf16_rn(a - hi - mid); a product a * b is the sum of the six terms hi hi, hi mid, mid hi, hi lo, lo hi, mid mid
 * (exact in fp32 each); accumulation is fp32, no atomics, a fixed order of summation: bitwise reproducible.  Part of that
 * order: every output element has two fp32 accumulators -- the hi hi terms in one, the five correction terms in the other,
 * k ascending in both -- which are added once, in front of the epilogue.  A non-finite
 * operand element makes every output element it feeds non-finite (an inf may come out as NaN).  Nothing routes here on
 * its own: dv_gemm and every other entry point stay fp32 MFMA.
 * Runs: the three Linear layouts, alpha / beta, DV_EPI_PLAIN and DV_EPI_BWD, a_colsum on the dy^T x layout (a dv_colsum
 * launch in front), any M and N, K % 4 == 0, 16-B aligned operand rows (A, B and lda, ldb multiples of 4 floats); it then
 * never reads past the end of a row, whatever `flags` allows, and ignores `tune`.  K % 4 != 0 runs only where `flags` lets
 * every k-contiguous operand's row ends be over-read (bit 0 for A, bit 1 for B): the 16-B chunk that straddles K is
 * loaded whole and its elements past K count as zeros.  Everything else -- A2, a_kscale, DV_EPI_FWD, DV_EPI_KLQ, pub_flag,
 * misaligned rows, K % 4 != 0 without that word -- returns DV_ERR_UNSUPPORTED and touches nothing; a NULL descriptor,
 * M < 0, N < 0, K < 1, or a NULL A, B, C (yref with DV_EPI_BWD) of a non-empty product returns DV_ERR_ARG.  One launch of
 * 128 x 128 output tiles (K tile 32, 48 KiB of LDS: three bf16 planes per operand, two workgroups per CU).  dv_gemm_x3_ok: a pure function, 1 where dv_gemm_x3 would run the descriptor, 0 otherwise. */
int dv_gemm_x3(const dv_gemm_desc* desc, dv_stream_t stream);
int dv_gemm_x3_ok(const dv_gemm_desc* desc);
/* The precision ladder of the split-bf16 product (OPT-IN, as dv_gemm_x3): `parts` = P bf16 parts per operand element, the
 * FIRST P of hi, mid, lo above.  parts = 3 is dv_gemm_x3 ("dtype: bf16x3").  parts = 2 ("dtype: bf16x2"): the three terms
 * hi hi, hi mid, mid hi (mid mid is dropped: the size of the residuals dropped already; <= (3 2^-16 + 2^-30) sum |a||b|
 * from the exact product before accumulation), hi hi in one accumulator, the two correction terms in the other.  parts = 1
 * ("dtype: bf16x1"): the one term hi hi in one accumulator, i.e. a bf16 product of the rounded operands with fp32
 * accumulation (<= (2^-7 + 2^-16) sum |a||b|): NOT an fp32 product, label it.  Everything else -- what runs and what is
 * refused, epilogues, alpha / beta, a_colsum, K tail, over-read, non-finite operands, bitwise reproducibility -- is
 * dv_gemm_x3's.  parts outside 1..3: DV_ERR_ARG (dv_gemm_split_ok: 0). */
int dv_gemm_split(const dv_gemm_desc* desc, int32_t parts, dv_stream_t stream);
int dv_gemm_split_ok(const dv_gemm_desc* desc, int32_t parts);
/* Dual-head Linear with the ROW work that consumes both heads fused into the epilogue (SURVEY.md K2+K3 /
 * K2+K5): y = x W^T with W = [W_head0 ; W_head1] (desc->split = rows of head 0, desc->N = 2*split), forward
 * layout (a_kcontig = b_kcontig = 1), epilogue DV_EPI_FWD exactly as dv_gemm (scale / bias / act0,shift0 |
 * act1,shift1 / resid).  Each workgroup computes the tile of head-0 columns [c, c+32) TOGETHER with the
 * head-1 columns [split+c, split+c+32) of the same rows, so element (m, c) sees a0 = head0(m,c) and
 * a1 = head1(m,c) and neither has to round-trip through HBM for the per-element work that follows:
 *
 *  DV_HEADS_SAMPLE  (a0 = mu, a1 = logvar: `DiagGaussianModule.forward` + `sample`, src/blocks.py:291-301,
 *    170-174; `DiagGaussianModuleLinear`, src/blocks.py:349-361): C = (mu | logvar) is written as by dv_gemm,
 *    and for every destination row s of source row m (seg_rows[seg_ptr[m] .. seg_ptr[m+1]); seg_ptr == NULL:
 *    s = m; rows m >= n_src emit nothing):   z = eps[s,c]*exp(logvar/2) + mu;   out[s,c] = z;
 *    out2[s,c] = z - sub[s,c] (optional);  out3[out3_idx[s], c] = z where out3_idx[s] >= 0 (optional)
 *    -- the L Monte-Carlo samples of a row (and the z2 samples of a pair, src/DrVAE.py:421-427) leave the
 *    encoder-heads launch directly.
 *  DV_HEADS_NLL  (a0 = mu, a1 = std = act1(.) + shift1: `DiagGaussianSigmaModule.forward` + `logp_perx`,
 *    src/blocks.py:410-416, 233-234), train step only: with xv = x[xidx ? xidx[m] : m, c]
 *      part[m*n_tiles + t] = -1/2 sum_{c in tile t} [log 2pi + log std^2 + (xv-mu)^2/std^2]   (row NLL = sum_t)
 *      C[m, c]       = coef[m] * (xv-mu)/std^2                                   = d/d mu
 *      C[m, split+c] = coef[m] * (-1/std + (xv-mu)^2/std^3) * act1'(.)           = d/d(pre-activation of std)
 *    i.e. C receives the GRADIENTS (the loss is linear in the row terms with coefficients known up front);
 *    mu / std themselves are never stored.  n_tiles = ceil(split/32) (dv_gemm_heads_tiles). */
enum { DV_HEADS_SAMPLE = 1, DV_HEADS_NLL = 2 };
typedef struct dv_heads_epi {
    int32_t mode;
    /* SAMPLE */
    const int32_t* seg_ptr;
    const int32_t* seg_rows;
    int32_t n_src;
    const float* eps;
    int64_t lde;
    float* out;
    int64_t ldo;
    const float* sub;
    int64_t lds;
    float* out2;
    int64_t ldo2;
    float* out3;
    int64_t ldo3;
    const int32_t* out3_idx;
    float* out4;               /* optional: sample row s is also copied to rows [out4_ptr[s], out4_ptr[s+1]) of out4 */
    int64_t ldo4;              /* (the z1 columns of the fprop rows of that sample, src/DrVAE.py:337-341) */
    const int32_t* out4_ptr;
    /* NLL */
    const float* x;
    int64_t ldx;
    const int32_t* xidx;
    const float* coef;
    float* part;
} dv_heads_epi;
int dv_gemm_heads(const dv_gemm_desc* desc, const dv_heads_epi* epi, dv_stream_t stream);
int dv_gemm_heads_tiles(int32_t split);
/* Does this build of the library carry tiling code t (dv_gemm_tune.tiling)?  0 = heuristic, 1 = 64x64, 2 = 32x32 K-split,
 * 3 = 128x128, 17 = 32x32x32 seven-per-CU, 40 = 128x256x16 hand-pipelined LDS-DMA ring, 46 = 64x64x32 pipelined; any
 * other code names a lab tiling of the tuning build (-DDV_LAB).  A pure function: the library keeps NO tuning state --
 * tests and tools pass a dv_gemm_tune with the descriptor of the call they want to steer. */
int dv_gemm_has_tiling(int tiling);

/* out[n] = beta*out[n] + sum_m X[m*ldx+n]            (bias gradient) */
int dv_colsum(const float* X, int64_t ldx, int32_t M, int32_t N, float* out, float beta, dv_stream_t stream);

/* dY[m,n] *= act'(Y[m,n]-shift), (act,shift) chosen by n<split as in DV_EPI_FWD */
int dv_act_bwd(float* dY, int64_t ldd, const float* Y, int64_t ldy, int32_t M, int32_t N, int32_t split,
               int32_t act0, int32_t act1, float shift0, float shift1, dv_stream_t stream);

/* WeightNorm (src/layers.py:39): norm[n] = ||W[n,:]||_2, scale[n] = g[n]/norm[n] */
int dv_wn_scale(const float* W, int64_t ldw, const float* g, int32_t N, int32_t K, float* scale, float* norm,
                dv_stream_t stream);
/* WeightNorm backward from dWraw = dpre^T x (dpre NOT yet multiplied by scale):
 *   dot = <W[n,:], dWraw[n,:]>;  dg[n] = beta*dg[n] + dot/norm[n]
 *   dW[n,k] = beta*dW[n,k] + scale[n]*dWraw[n,k] - dot*g[n]/norm[n]^3 * W[n,k] */
int dv_wn_bwd(const float* dWraw, int64_t ldr, const float* W, int64_t ldw, const float* g, const float* norm,
              int32_t N, int32_t K, float* dW, int64_t ldd, float* dg, float beta, dv_stream_t stream);

/* ------------------------------------------------------- reparameterisation (K3)
 * out row r = l*n + j (l < reps, j < n) samples from q row qi = src_idx ? src_idx[j] : j:
 *   out[r,d] = mu[qi,d] + eps[r,d] * (mode==LOGVAR ? exp(0.5*sd[qi,d]) : sd[qi,d])
 * (src/blocks.py:170-174, 208-211; eps is explicit so parity tests can inject it).
 * Optional out2[r,d] = out[r,d] - sub[r,d]   (`z2Fz1_sample - z1_sample`, src/DrVAE.py:495).
 * Optional out3[out3_idx[r], d] = out[r,d] for out3_idx[r] >= 0 (a second, scattered copy:
 * the z2Fz1 samples of paired rows also feed the decoder, src/DrVAE.py:455-459).
 * backward: dmu[qi] = beta*dmu[qi] + sum_l dz[l*n+j]; dsd likewise with the chain factor. */
int dv_reparam_fwd(const float* mu, const float* sd, int64_t ldq, const int32_t* src_idx, int32_t n, int32_t reps,
                   int32_t Z, const float* eps, int64_t lde, int32_t mode, float* out, int64_t ldo,
                   const float* sub, int64_t lds, float* out2, int64_t ldo2, float* out3, int64_t ldo3,
                   const int32_t* out3_idx, dv_stream_t stream);
int dv_reparam_bwd(const float* dz, int64_t ldz, const float* eps, int64_t lde, const float* sd, int64_t ldq,
                   const int32_t* src_idx, int32_t n, int32_t reps, int32_t Z, int32_t mode, float* dmu, float* dsd,
                   int64_t lddq, float beta, dv_stream_t stream);
/* CSR form of the backward: q row i (nq rows) sums the sample rows seg_rows[seg_ptr[i]..seg_ptr[i+1])
 * of dz/eps (any number of draws per q row), and optionally the row-aligned (dmu|dsd) contributions
 * `extra[ex_rows[t], :2Z]`, t in [ex_ptr[i], ex_ptr[i+1]).  dmu/dsd[i] = beta*old + sums.
 * `add` (optional, ABI 10): a second gradient source for the first add->n sample rows, g[r] = dz[r] + add->dz[r] for
 * r < add->n (VFAE: the classifier / fprop chain's share of d/dz1, which used to be summed into dz by a launch of its
 * own); `park` (optional): the launch parks on another chain's flag first, like dv_z2f_post_bwd. */
/* KL(q || N(0, I)) of the launch's OWN q rows with per-row free bits (PVAE's prior term, src/PVAE.py): its gradient w.r.t.
 * (mu, logvar) -- coef[i] * gate(raw[i]) * (mu, (e^logvar - 1) / 2) -- is added to the row's result on the way out instead
 * of a dv_kl_rows_bwd launch behind it (round 5).  LOGVAR parameterisation; the log-variances are the launch's own operand. */
typedef struct dv_prior_kl {
    const float* coef;       /* (rows) dLoss / d KL */
    const float* raw;        /* (rows) raw KL of the forward (the free-bits gate) */
    float kl_min;
    const float* mu;         /* (rows, ld) the rows' means; NULL where the launch has them already (dv_z2f_post_bwd: q2) */
    int64_t ld;
} dv_prior_kl;
typedef struct dv_seg_add {
    const float* dz;
    int64_t ld;
    int32_t n;
} dv_seg_add;
int dv_reparam_bwd_seg(const float* dz, int64_t ldz, const float* eps, int64_t lde, const float* sd, int64_t ldq,
                       const int32_t* seg_ptr, const int32_t* seg_rows, int32_t nq, int32_t Z, int32_t mode,
                       const float* extra, int64_t ldx, const int32_t* ex_ptr, const int32_t* ex_rows, float* dmu,
                       float* dsd, int64_t lddq, float beta, const dv_bump* bump, const dv_seg_add* add,
                       const dv_wait* park, const dv_prior_kl* prior, dv_stream_t stream);
/* `prior` (optional, round 5): the prior-KL gradient of q row i is added to (dmu, dsd)[i], see dv_prior_kl */
/* Backward of everything hanging on the z2Fz1 samples (src/DrVAE.py:431-433, 459-487) in one pass
 * over (row i < B, dim d < Z), looping the L samples r = l*B + i; jp = pair_slot[i] (-1: singleton):
 *   g       = dz2f[r] (0 when dz2f == NULL: a model without a classifier) + (jp >= 0 ? dzdec_pert[l*Np + jp] : 0)
 *   dp2[r]  = (g | g*eps*0.5*exp(0.5*lv2)) + [jp >= 0] d KL(q2[jp] || p2[r]) / d p2 * coef[l*Np+jp]*mask
 *   dz1[r] += dp2[r].mu (residual mu2 = z1 + ..., src/blocks.py:357) + (dz1b ? dz1b[r] : 0)
 *   dq2[jp] = sum_l d KL / d q2 * coef*mask                      (mask = free-bits gate on raw)      */
/* One wave per batch row i, lanes over d; with kl_out / raw_out the row sum of KL(q2[jp] || p2[r]) is formed first, with
 * the lane mapping and the reduction tree of dv_kl_rows_fwd (same bits), and gates the gradients (weight 1/2 on raw ==
 * kl_min); with seg_src / z1_dz2f:
 *   dz1[r] += dp2[r].mu + (((dz1b ? dz1b[r] : 0) + seg_beta * sum_t seg_src[t]) + z1_dz2f * dz2f[r])
 * -- with seg_beta = 1, z1_dz2f = -1 the bits of dv_smalln_linear_bwd_data's (seg + dlogit W1) - dlogit W2.             */
/* ABI 11: the operands travel in a descriptor (28 positional arguments before); shapes in the comments */
typedef struct dv_z2f_desc {
    const float* dz2f;       /* (L*B, Z) or NULL */
    int64_t ld_dz2f;
    const float* dzdec_pert; /* (L*Np, Z) gradient of the decoded z2Fz1 copies, or NULL */
    int64_t ld_pert;
    const int32_t* pair_slot; /* (B) jp or -1 */
    const float* eps;        /* (L*B, Z) */
    int64_t lde;
    const float* p2;         /* (L*B, 2Z) mu2 | lv2 */
    int64_t ldp2;
    const float* q2;         /* (Np, 2Z) mu | lv of q(z2|x2) */
    int64_t ldq2;
    const float* coef;       /* (L*Np) KL coefficients */
    const float* raw;        /* (L*Np) raw KL (free bits) */
    float kl_min;
    const float* dz1b;       /* (L*B, Z) or NULL */
    int64_t ld_dz1b;
    float* dp2;              /* (L*B, 2Z) out */
    int64_t ld_dp2;
    float* dz1;              /* (L*B, Z) in/out (+=) */
    int64_t ld_dz1;
    float* dq2;              /* (Np, 2Z) out, or NULL */
    int64_t ld_dq2;
    int32_t L;
    int32_t B;
    int32_t Np;
    int32_t Z;
    const float* prior_coef; /* (Np) or NULL (with prior_raw): the prior-KL gradient of q2 row jp is added to dq2[jp], */
    const float* prior_raw;  /* see dv_prior_kl (kl_min as above) */
    /* trailing fields (ABI 12, zero = as before): the launch forms the pairs' KL rows itself, and sums fprop rows */
    float* kl_out;           /* (L*Np) out or NULL (with raw_out): max(raw, kl_min), what dv_kl_rows_fwd(free_bits) writes */
    float* raw_out;          /* (L*Np) out or NULL: the raw KL; when set the gate reads the launch's own sum, `raw` is unused */
    const float* seg_src;    /* (rows, >= Z) or NULL (with seg_ptr): a second share of d/dz1, summed per sample row */
    int64_t ld_seg;
    const int32_t* seg_ptr;  /* (L*B + 1) row r sums seg_src rows [seg_ptr[r], seg_ptr[r+1]) in index order */
    float seg_beta;
    float z1_dz2f;           /* dz1[r] also gets z1_dz2f * dz2f[r]: a classifier on [z1, z2Fz1 - z1] sends -dz2f to z1 */
} dv_z2f_desc;
int dv_z2f_post_bwd(const dv_z2f_desc* d, const dv_wait* park, dv_stream_t stream);

/* ------------------------------------------------ diagonal-Gaussian KL per row (K4)
 * row r = l*n + j: q row = qidx ? qidx[j] : j ; p row = pidx ? pidx[r] : r, or the
 * scalar prior (prior_mu, prior_sd) when mu_p == NULL (prior_sd is a log-variance in
 * LOGVAR mode, a std in SIGMA mode).
 *   LOGVAR: raw = -1/2 sum_d [1 - lv_p + lv_q - ((mu_q-mu_p)^2 + e^lv_q)/e^lv_p]   src/blocks.py:180-182
 *   SIGMA : same with log(std^2), std^2                                              src/blocks.py:217-220
 *   out = free_bits ? max(raw, kl_min) : raw      (per-ROW free bits, src/DGMMixin.py:68-75)
 *   out[r] += add[r] (optional);  zout[r,d] = mu_q + eps[r,d]*std_q (optional): the reparameterised
 *   sample of q drawn in the same row pass (q(z3|z1,y): src/DrVAE.py:341-347).
 *   mu2 != NULL: a second term of the same row, KL(N(mu2[r], sd2[r]) || the scalar prior) over Z2 columns, with its
 *   own free bits: out[r] += max(raw2, kl_min), raw2_out[r] = raw2 (the z3 term of an fprop row, src/DrVAE.py:347,358,
 *   evaluated next to the z1 term instead of in a launch of its own).
 * backward: coef[r] = dLoss/d out[r]; gradients are written ROW-ALIGNED (row r of
 * dq_* / dp_*); callers reduce duplicates with dv_rows_segment_sum.  With dz != NULL the
 * backward of that fused sample (dq_mu += dz, dq_sd += dz*eps*dstd/dsd) rides along. */
/* ABI 11: the forward's operands travel in a descriptor (29 positional arguments before: one transposed int64 away
 * from silent corruption); field names as in the comment above */
typedef struct dv_kl_rows_desc {
    const float* mu_q;
    const float* sd_q;
    int64_t ldq;
    const int32_t* qidx;
    const float* mu_p;
    const float* sd_p;
    int64_t ldp;
    const int32_t* pidx;
    float prior_mu;
    float prior_sd;
    int32_t n;
    int32_t reps;
    int32_t Z;
    int32_t mode;
    int32_t free_bits;
    float kl_min;
    float* raw_out;
    float* out;
    const float* add;
    const float* eps;
    int64_t lde;
    float* zout;
    int64_t ldz;
    const float* mu2;
    const float* sd2;
    int64_t ld2;
    int32_t Z2;
    float* raw2_out;
} dv_kl_rows_desc;
int dv_kl_rows_fwd(const dv_kl_rows_desc* d, const dv_wait* park, dv_stream_t stream);
/* two independent sets of plain KL rows (no fused sample, no second term) in ONE launch -- PVAE's prior term and the pairs' term
 * sit back to back on its main chain (round 5) */
int dv_kl_rows_fwd_pair(const dv_kl_rows_desc* d1, const dv_kl_rows_desc* d2, dv_stream_t stream);
/* the backward reads the forward's descriptor -- operands, n / reps / Z / mode, free_bits, kl_min, eps / lde, and raw_out
 * as the raw KL the forward stored (required with free_bits); out / add / zout / mu2.. are not looked at -- plus its own
 * outputs (30 positional arguments before ABI 11) */
typedef struct dv_kl_rows_grad {
    const float* coef;       /* (n*reps) dLoss / d out */
    float* dq_mu;
    float* dq_sd;
    int64_t lddq;
    float* dp_mu;            /* NULL (with dp_sd): no gradient towards p */
    float* dp_sd;
    int64_t lddp;
    float beta;              /* outputs = beta * old + gradient */
    const float* dz;         /* gradient of the fused sample, or NULL */
    int64_t ldz;
} dv_kl_rows_grad;
int dv_kl_rows_bwd(const dv_kl_rows_desc* d, const dv_kl_rows_grad* g, dv_stream_t stream);

/* ------------------------------------- Gaussian log-likelihood over genes per row (K5)
 * out[r] = -1/2 sum_g [log 2pi + log var + (x-mu)^2/var], x row = xidx ? xidx[r] : r
 *   SIGMA : var = sd^2  (src/blocks.py:233-234, the reconstruction term of src/DrVAE.py:442,452,460)
 *   LOGVAR: var = e^sd  (src/blocks.py:195-196)
 * backward: coef[r] = dLoss/d out[r]; writes d/dmu and d/d(sd) -- the latter chained
 * through sd = sd_act(pre) + sd_shift when sd_act != IDENTITY, i.e. directly the
 * gradient w.r.t. the head's pre-activation (src/blocks.py:415).  dx optional. */
int dv_gauss_nll_rows_fwd(const float* x, int64_t ldx, const int32_t* xidx, const float* mu, const float* sd,
                          int64_t ldp, int32_t M, int32_t X, int32_t mode, float* out, const float* bias_mu,
                          const float* bias_sd, float sd_shift, dv_stream_t stream);
/* bias_mu / bias_sd (both or neither, SIGMA mode; ABI 11): mu / sd hold the heads' RAW products and the pass finishes them
 * on its way (mu + bias_mu, softplus(sd + bias_sd) + sd_shift) -- evaluation passes behind a plain heads product */
int dv_gauss_nll_rows_bwd(const float* coef, const float* x, int64_t ldx, const int32_t* xidx, const float* mu,
                          const float* sd, int64_t ldp, int32_t M, int32_t X, int32_t mode, int32_t sd_act,
                          float sd_shift, float* dmu, float* dsd, int64_t ldd, float* dx, int64_t lddx, float beta,
                          dv_stream_t stream);

/* EXTENSION: log-likelihood rows of the Bernoulli / Poisson data decoders that src/DrVAE.py:124-129
 * names (`type_rec='binary'` / `'poisson'`; the reference ships neither class).  v = the head's post-activation output
 * (probability = sigmoid(a), or rate = softplus(a) + shift); x row = xidx ? xidx[r] : r.
 *   out[r] = sum_g log p(x[.,g] | v[r,g]);  coef != NULL: dpre[r,g] = coef[r] * d log p / d a  (a = pre-activation)
 *   BERNOULLI: pc = clamp(v, 1e-10, 1 - 1e-10); log p = x log pc + (1-x) log(1-pc); d/da = x - v inside the clamp, else 0
 *   POISSON  : log p = x log v - v - lgamma(x+1);  d/da = (x/v - 1) (1 - exp(-(v - shift)))
 * EXTENSION (`type_rec='nb'`, no counterpart in the reference): NEGBIN, the negative binomial with mean mu > 0 and inverse
 * dispersion theta > 0 (Var = mu + mu^2 / theta), two heads over one trunk.  v row r = [mu | theta], 2X columns
 * (ldv >= 2X), mu = softplus(a_m) + shift, theta = softplus(a_t) + DV_NB_THETA_SHIFT; dpre row r =
 * coef[r] * [d/da_m | d/da_t], 2X columns (ldd >= 2X); x counts >= 0 (exact in fp32 up to 2^24):
 *   log p    = [lgamma(x+theta) - lgamma(theta)] - lgamma(x+1) + theta log(theta/(theta+mu)) + x log(mu/(theta+mu))
 *   d/dmu    = x/mu - (x+theta)/(theta+mu);   d/dtheta = [psi(x+theta) - psi(theta)] + log(theta/(theta+mu)) + (mu-x)/(theta+mu)
 *   d/da_*   = d/d(mu, theta) * (1 - exp(-(v - its shift)))
 * The lgamma / digamma pairs and the two log ratios are formed as differences (recurrence + asymptotic series, log1p),
 * never as two large values subtracted: the x = 0 pair is exactly 0, and theta -> inf is the Poisson term.
 * EXTENSION (`library_size=True`): POISSON_LIB / NEGBIN_LIB, the same rows with every mean of row r multiplied by the observed
 * size factor of its target row, s = max(sum_g x[xrow,g], 1) / X; v still holds the UNSCALED heads, m = s v:
 *   POISSON_LIB: log p = x log m - m - lgamma(x+1);  d/da = (x/v - s) (1 - exp(-(v - shift)))
 *   NEGBIN_LIB : log p as NEGBIN at m;  d/da_m = (x - m) / (v (1 + m/theta)) (1 - exp(-(v - shift)))  (the slope is the
 *                unscaled head's);  d/da_t as NEGBIN, at m; theta is not scaled
 * Same signature, same layouts.  The workgroup that owns row r forms s itself in a first sweep over the target row (fixed
 * order: per-thread partials in index order, the wave sum, the four waves as (p0 + p1) + (p2 + p3)); the term loop's second
 * read of the row comes from cache.  For integer counts with a row total below 2^24 every partial sum is exact in fp32 in
 * any order, so s is ONE correctly rounded quotient on every path; a row whose total is X (s = 1) gives the unscaled
 * kind's output bit for bit.
 * EXTENSION (`type_rec='zinb'`, no counterpart in the reference): ZINB / ZINB_LIB, the zero-inflated negative binomial -- a
 * third head, the dropout logit a_d (identity activation), pi = sigmoid(a_d), over the NEGBIN (NEGBIN_LIB) term logNB:
 * v row r = [mu | theta | a_d], 3X columns (ldv >= 3X), the first two blocks as NEGBIN reads them, the third the RAW logit;
 * dpre row r = coef[r] * [d/da_m | d/da_t | d/da_d], 3X columns (ldd >= 3X).  With L0 = logNB(0) = -theta log1p(m/theta) and
 * rho = sigmoid(L0 - a_d), the NB component's responsibility for a zero:
 *   x > 0: log p = -softplus(a_d) + logNB(x);        d/da_d = -pi;  d/da_m, d/da_t as NEGBIN
 *   x = 0: log p = log(pi + (1 - pi) e^{L0});         d/da_d = (1 - rho) (1 - pi) (1 - e^{L0});  d/da_m, d/da_t = rho * NEGBIN's
 * The x = 0 term never adds a vanishing addend to 1: with z = (1 - pi)(-expm1(L0)) it is log1p(-z) for z <= 1/2, else
 * max(u, w) + log1p(exp(-|a_d - L0|)) with u = -softplus(-a_d), w = -softplus(a_d) + L0; its logit gradient is a product of
 * non-negative factors, never a difference of two sigmoids.  theta and the logit are never scaled (ZINB_LIB: m = s mu, the
 * slope of d/da_m the unscaled head's).  Same signature; refusals and the 16-byte / one-gene-per-thread paths as NEGBIN. */
enum { DV_REC_BERNOULLI = 0, DV_REC_POISSON = 1, DV_REC_NEGBIN = 2, DV_REC_POISSON_LIB = 3, DV_REC_NEGBIN_LIB = 4,
       DV_REC_ZINB = 5, DV_REC_ZINB_LIB = 6 };
#define DV_NB_THETA_SHIFT 1e-3f     /* the shift of the NEGBIN theta head (that of the Gaussian decoder's sigma head) */
int dv_rec_nll_rows(int32_t kind, float shift, const float* coef, const float* x, int64_t ldx, const int32_t* xidx,
                    const float* v, int64_t ldv, int32_t M, int32_t X, float* out, float* dpre, int64_t ldd,
                    dv_stream_t stream);

/* The raw-heads forward + backward pass below (dv_gauss_nll_rows_fwdbwd with bias_mu / bias_sd, sigma head = softplus +
 * shift) with the heads' BIAS GRADIENT folded in (wide configuration: saves the separate 1.3-GB column-sum pass over the
 * gradients this kernel writes).  A workgroup owns 1024 genes x 64 rows:
 *   out_part[r, c] = partial log-likelihood of row r over gene chunk c  (M x chunks; out[r] = sum_c out_part[r, c] --
 *                    the loss assembly sums them: dv_loss_term.row_len = chunks)
 *   dmu / dsd      = as dv_gauss_nll_rows_fwdbwd
 *   ws[b, g]          = sum over the rows of row block b of dmu[r, g]        } (row_blocks x ldw; the caller sums the
 *   ws[b, sd_off + g] = the same of dsd[r, g]                                } blocks: dv_colsum(ws, ldw, row_blocks, ..))
 * chunks = dv_nll_raw_cs_chunks(X), row_blocks = dv_nll_raw_cs_row_blocks(M).  X % 4 == 0, 16-B aligned rows.
 * Deterministic (fixed summation order, no atomics).
 * dmu == dsd == ws == NULL (coef unused): FORWARD ONLY -- the row partials of an evaluation pass behind a plain heads
 * product (the whole-set evaluation's loss pass: no activation epilogue in the GEMM, no finished heads written and
 * read back).
 *
 * THE COUNT KINDS WITH A GENE-WISE DISPERSION (trailing fields `kind`, `theta_raw`, `size`; all zero: the Gaussian pass above,
 * bit for bit -- theta_raw and size are not read then).  kind = DV_REC_NEGBIN / DV_REC_NEGBIN_LIB / DV_REC_ZINB /
 * DV_REC_ZINB_LIB: the row terms and gradients of dv_rec_nll_rows' kind of that name, with theta not a head but ONE value
 * per gene, theta_g = softplus(theta_raw[g]) + DV_NB_THETA_SHIFT (theta_raw: X floats; the kernel forms theta itself, in
 * double, rounded once to fp32).  Under a count kind:
 *   mu (row stride ldp) = the FINISHED mean head (softplus + shift);  shift = the mean's shift
 *   sd (same stride)    = the RAW dropout logit for the ZINB kinds; NULL for the NB kinds
 *   coef, x, ldx, xidx  = as dv_rec_nll_rows
 *   dmu / dsd (ldd)     = coef[r] * d/da_m and coef[r] * d/da_d (dsd: ZINB kinds only, NULL otherwise)
 *   out_part            = (M, chunks) row partials, chunks = ceil(X / 1024) -- NOT dv_nll_raw_cs_chunks(X)
 *   ws[b, g]            = sum over the rows of row block b of coef[r] * d/da_t[r, g], ldw >= X (d/da_t: w.r.t. theta_raw);
 *                         the caller sums the blocks: dv_colsum(ws, ldw, row_blocks, X, ..) is the gradient of theta_raw
 *   row_blocks          = the CALLER'S choice in [1, max(M, 1)] (and <= 65535) -- NOT dv_nll_raw_cs_row_blocks(M); block b
 *                         owns the rows [b R, min(M, (b + 1) R)), R = ceil(M / row_blocks) (a block past M owns none and
 *                         writes zeros to its row of ws)
 *   sd_off, bias_mu, bias_sd: unused, must be 0 / NULL
 *   size                = M floats.  The library-scaled kinds need the size factor s[r] = max(sum_g x[xidx[r], g], 1) / X of
 *                         every row.  chunks == 1: the workgroup forms it from the row it reads (and stores it to size when
 *                         size is given).  chunks > 1: REQUIRED -- a small launch in front writes s of every row into it
 *                         (two launches behind this one call), so that no chunk walks the whole target row again.  Either
 *                         way s is the one correctly rounded quotient for integer counts with a total below 2^24.
 *                         The unscaled kinds do not touch it.
 * A workgroup of 256 threads owns one chunk and one row block; a thread owns four genes for all rows of the block (a quad
 * on 16-byte accesses with X % 4 == 0 and aligned rows, else the genes tid + 256 j: any X >= 1, any alignment).  Row
 * partials: per-thread partials in index order, the wave sum, the four waves as (p0 + p1) + (p2 + p3).  ws: ascending row
 * order in registers, stored once.  No atomics; repeated launches give equal bits.
 * Forward only: dmu == dsd == ws == NULL (coef unused).
 * DV_ERR_ARG, before any launch and at M == 0 too: an unknown kind; no theta_raw / x / mu / out_part; a ZINB kind without
 * sd or an NB kind with sd; biases or sd_off given; chunks or row_blocks outside the above; ldx, ldp (, ldd) < X; with dmu:
 * no coef, no ws, ldw < X, dsd not as the kind asks; without dmu: ws or dsd given; a library kind with chunks > 1 and no
 * size.
 *
 * A DISPERSION PER (NUISANCE CLASS, GENE) (trailing fields `n_cls`, `cls`, `cls_src`, `ldth`; all zero: the passes above, bit
 * for bit -- none of them is read then).  n_cls = S >= 1 under a count kind:
 *   theta_raw           = S rows of X floats at stride ldth >= X: theta[k, g] = softplus(theta_raw[k ldth + g]) + shift
 *   class of row r      = cls[cls_src ? cls_src[r] : r]  (cls_src: M int32, the row of `cls` a decoder row reads -- the batch
 *                         row of a sample or pair row, the indexing dv_nuisance_feed documents for sohd)
 *   ws[b, k X + g]      = sum over the rows of row block b that have class k of coef[r] * d/da_t[r, g], ascending rows;
 *                         ldw >= S X; a block without rows of class k writes zeros to that segment.  One
 *                         dv_colsum(ws, ldw, row_blocks, S X, ..) is the whole (S, X) gradient, contiguous
 *   out_part, dmu, dsd, size, chunks, row_blocks: as above
 * The launch is grid(chunks, row_blocks, S): a workgroup owns one chunk, one row block and one class, walks its block's rows
 * in ascending order and skips the rows of other classes (a uniform branch in front of every load of the row), so every
 * output element has one writer and every summation order is the one above: row r's out_part / dmu / dsd / size are, bit
 * for bit, those of the shared-theta launch at theta_raw row cls(r).  A class outside [0, S) is the caller's error with a
 * harmless outcome: no workgroup takes the row, nothing of it is written, nothing is read outside the operands.
 * DV_ERR_ARG, before any launch and at M == 0 too: n_cls != 0 with kind == 0; n_cls < 0 or > 65535; n_cls >= 1 without
 * cls or with ldth < X; with dmu, ldw < n_cls X. */
typedef struct dv_nll_raw_cs_desc {
    const float* coef;
    const float* x;
    int64_t ldx;
    const int32_t* xidx;
    const float* mu;
    const float* sd;
    int64_t ldp;
    int32_t M;
    int32_t X;
    float shift;
    float* out_part;
    int32_t chunks;
    float* dmu;
    float* dsd;
    int64_t ldd;
    const float* bias_mu;
    const float* bias_sd;
    float* ws;
    int64_t ldw;
    int64_t sd_off;
    int32_t row_blocks;
    /* trailing (inside ABI 13): the count kinds with a gene-wise dispersion; all zero = the Gaussian pass as it was */
    int32_t kind;
    const float* theta_raw;
    float* size;
    /* trailing (inside ABI 13): a dispersion per (nuisance class, gene); all zero = the passes as they were */
    int32_t n_cls;
    const int32_t* cls;
    const int32_t* cls_src;
    int64_t ldth;
} dv_nll_raw_cs_desc;
int dv_gauss_nll_rows_raw_cs(const dv_nll_raw_cs_desc* d, dv_stream_t stream);
int dv_nll_raw_cs_chunks(int32_t X);
int dv_nll_raw_cs_row_blocks(int32_t M);

/* forward + backward in one row pass (the loss is linear in the row terms with coefficients
 * known up front): out[r] as _fwd, dmu/dsd[r,:] = coef[r] * d out[r]/d(mu, pre-activation of sd).
 * bias_mu / bias_sd (both or neither; X floats each): mu / sd then hold the heads' RAW products (x W^T without bias and
 * activation) and this pass finishes them on its way: mu = mu_raw + bias_mu, sd = act(sd_raw + bias_sd) + sd_shift --
 * for heads whose product fills the chip, where the plain GEMM epilogue is the faster one (wide configuration). */
int dv_gauss_nll_rows_fwdbwd(const float* coef, const float* x, int64_t ldx, const int32_t* xidx, const float* mu,
                             const float* sd, int64_t ldp, int32_t M, int32_t X, int32_t mode, int32_t sd_act,
                             float sd_shift, float* out, float* dmu, float* dsd, int64_t ldd, const float* bias_mu,
                             const float* bias_sd, dv_stream_t stream);

/* --------------------------------------------------------- categorical head (K6/K7)
 * probs = clamp(softmax(logits), 1e-10, 1-1e-10)   (src/blocks.py:446-463); with
 * sigmoid1 != 0 logits is (M,1) and probs = clamp(cat(1-s, s)) (src/blocks.py:448-451,461-462). */
int dv_softmax_clamp_fwd(const float* logits, int64_t ldl, int32_t M, int32_t Y, int32_t sigmoid1, float* probs,
                         int64_t ldp, dv_stream_t stream);
int dv_softmax_clamp_bwd(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp, int32_t M, int32_t Y,
                         int32_t sigmoid1, float* dlogits, int64_t ldl, float beta, dv_stream_t stream);
/* per-row terms of a categorical q (any may be NULL):
 *   logp[r]   = log probs[r, labels[r]]                               src/blocks.py:473-474
 *   kl[r,j]   = -p (log prior[r,j] - log p)   (elementwise)           src/blocks.py:479-480
 *   ent[r]    = -sum_j p log p                                        src/blocks.py:476-477
 *   best[r]   = argmax_j p                                            src/blocks.py:485-486 */
int dv_cat_terms_fwd(const float* probs, int64_t ldp, int32_t M, int32_t Y, const int32_t* labels,
                     const float* prior, int64_t ldpr, float* logp, float* kl, int64_t ldk, float* ent,
                     int32_t* best, dv_stream_t stream);
/* dprobs[r,j] = beta*dprobs + c_logp[r]*[j==label]/p + g_kl[r,j]*(log p - log prior + 1) - c_ent[r]*(log p + 1) */
int dv_cat_terms_bwd(const float* probs, int64_t ldp, int32_t M, int32_t Y, const int32_t* labels,
                     const float* prior, int64_t ldpr, const float* c_logp, const float* g_kl, int64_t ldg,
                     const float* c_ent, float* dprobs, int64_t lddp, float beta, dv_stream_t stream);

/* Small-N linear head, N <= 8 outputs -- the classifier q(y|z1,z2) when `dim_h_clf=[]`
 * (src/DrVAE.py:165, src/blocks.py:446): logits = [a1|a2] W^T + b, probs = clamp(softmax).
 * One wavefront per row instead of a >90 %-padded MFMA tile.  Either output may be NULL.
 * Backward takes d(probs) (+ probs: chained through clamp+softmax) or, with probs == NULL,
 * d(logits) directly:
 *   bwd_data  : dst_t[r,c] = beta_t*dst_t[r,c] + sum_j dlogit[r,j] (alpha_t W[j,col0_t+c] + alpha2_t W[j,col1_t+c])
 *               for up to 3 destinations; col1/alpha2 may be NULL (the `[z1, z2F - z1]` input of
 *               src/DrVAE.py:495 sends W1 - W2 to z1 and W2 to z2F)
 *   bwd_weight: dW[j,k] = beta*dW + sum_r dlogit[r,j] [a1|a2][r,k];  db[j] likewise (db may be NULL)
 *               seg_src != NULL: destination 0 starts from the segment sum sum_{u in [seg_ptr[r], seg_ptr[r+1])}
 *               seg_src[u, c] instead of beta_0*dst_0[r,c] (the fprop rows' d/dz1 of src/DrVAE.py:337-358 folded into
 *               the classifier's data gradient: one launch instead of dv_rows_segment_sum + this one)
 * The pointer/size arrays of bwd_data are HOST arrays. */
int dv_smalln_linear_fwd(const float* a1, int64_t lda1, int32_t K1, const float* a2, int64_t lda2, int32_t K2,
                         const float* W, int64_t ldw, const float* bias, int32_t M, int32_t N, float* logits,
                         int64_t ldl, float* probs, int64_t ldp, const dv_ymarg* ymarg, const dv_wait* park,
                         const dv_fprop_kl* fprop_kl, const dv_clf_dgrad* dgrad, dv_stream_t stream);
int dv_smalln_linear_bwd_data(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp, const float* W,
                              int64_t ldw, int32_t M, int32_t N, int32_t n_dst, float* const* dst,
                              const int64_t* ld, const int32_t* col0, const int32_t* ncol, const float* alpha,
                              const float* beta, const int32_t* col1, const float* alpha2, const float* seg_src, int64_t ld_seg,
                              const int32_t* seg_ptr, dv_stream_t stream);
int dv_smalln_linear_bwd_weight(const float* dprobs, int64_t lddp, const float* probs, int64_t ldp,
                                const float* a1, int64_t lda1, int32_t K1, const float* a2, int64_t lda2,
                                int32_t K2, int32_t M, int32_t N, float* dW, int64_t ldd, float* db, float beta,
                                const dv_publish* pub, float* ws, int32_t ws_splits, dv_stream_t stream);
/* ws / ws_splits (optional, ABI 11): a workspace of ws_splits x N x (K1 + K2 + 1) floats lets the launch split the rows
 * over up to ws_splits workgroups per block of 16 weight columns (M >= 1024 rows: the wide configuration's 4096) and add
 * the partial sums up in a fixed order with a second tiny launch -- deterministic; without it one workgroup per column
 * block walks all M rows */

/* y-marginalisation of src/DrVAE.py:503-534 / src/VFAE.py:331-390 over the stacked
 * "fprop" rows.  For every (l, i) classifier row r (R rows):
 *   labeled   (fp_ptr[r+1]-fp_ptr[r] == 1): yl[r] = log qy[r, label[r]]; kld[r] = klfp[fp row]
 *   unlabeled (== Y fp rows, class j at fp_ptr[r]+j): yl[r] = 0;
 *       kld[r] = sum_j qy[r,j]*klfp[fp_ptr[r]+j] + sum_j qy[r,j](log qy[r,j] - log prior_j)
 * log prior_j = log_prior_v[j] when log_prior_v != NULL (a class prior given as data, `prior_y` of
 * src/DrVAE.py:83-85,389), else the scalar log_prior ('uniform').
 * backward: c_kld[r], c_yl[r] are dLoss/d kld[r], d yl[r]; writes cfp[fp row] = dLoss/d klfp
 * and dqy (R,Y). */
int dv_ymarg_fwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr, const float* klfp,
                 float log_prior, const float* log_prior_v, int32_t R, int32_t Y, float* yl, float* kld,
                 dv_stream_t stream);
int dv_ymarg_bwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr, const float* klfp,
                 float log_prior, const float* log_prior_v, const float* c_kld, const float* c_yl, int32_t R,
                 int32_t Y, float* cfp, float* dqy, int64_t lddq, dv_stream_t stream);

/* _fwd and _bwd in one launch (the train step knows the coefficients before the forward pass) */
int dv_ymarg_fwdbwd(const float* qy, int64_t ldq, const int32_t* label, const int32_t* fp_ptr, const float* klfp,
                    float log_prior, const float* log_prior_v, const float* c_kld, const float* c_yl, int32_t R,
                    int32_t Y, float* yl, float* kld, float* cfp, float* dqy, int64_t lddq, dv_stream_t stream);

/* Regression head (`type_y='cont'`, src/DrVAE.py:159-169,503-530): q(y|.) = N(sigmoid(.), fixed var).
 * Per classifier row r=(l,i), i = r % B:
 *   labeled   (has_y[i]): yl[r] = log N(ylab[i,:]; mu[r,:], var);  yv = ylab[i,:]
 *   unlabeled            : yl[r] = 0;                               yv = mu + sd*eps[r,:]   (SGVB sample)
 * yv is written into the y columns of both fprop inputs (fpin_y, z3in_y point at column Z of [z | y]).
 * backward: dlogit = dmu * mu(1-mu) with dmu = c_yl*(y-mu)/var (labeled) or the sum of the gradients of
 * the two y columns (unlabeled); called with dlogit == NULL it only writes cfp[r] = c_kld[r]. */
/* sqerr != 0: the labeled rows are scored by squared error instead, yl[r] = -sum_d (y-mu)^2 (VFAE.py:351). */
int dv_ycont_fwd(const float* mu, int64_t ldm, const float* ylab, const int32_t* has_y, const float* eps, int64_t lde,
                 float logvar, int32_t sqerr, int32_t R, int32_t B, int32_t Y, float* yl, float* fpin_y, int64_t ld1,
                 float* z3in_y, int64_t ld2, dv_stream_t stream);
int dv_ycont_bwd(const float* mu, int64_t ldm, const float* ylab, const int32_t* has_y, float logvar, int32_t sqerr,
                 const float* c_yl, const float* c_kld, const float* dfpin_y, int64_t ld1, const float* dz3in_y,
                 int64_t ld2, int32_t R, int32_t B, int32_t Y, float* dlogit, int64_t ldd, float* cfp,
                 dv_stream_t stream);

/* ------------------------------------------- random-Fourier-feature MMD (K10)
 * `mmd_fourier` of src/blocks.py:40-55.  The projections theta = a * x W + 2 pi b (a = sqrt(2/bandwidth)/sqrt(Z))
 * come from dv_gemm (scale/bias epilogue); these finish the statistic:
 *   _fwd: diff[r] = c*(mean_i cos(th1[i,r]) - mean_j cos(th2[j,r])),  mmd2[0] = sum_r diff[r]^2   (c = sqrt(2/R))
 *   _bwd: G[i,r] = coef * gout[0] * (-diff[r]) * sin(th[i,r]) = d mmd2 / d theta for one input when
 *         coef = +-2c/n (sign - for the second input); d/dx follows as a * G W^T (dv_gemm). */
int dv_mmd_rff_fwd(const float* th1, int64_t ld1, int32_t n1, const float* th2, int64_t ld2, int32_t n2, int32_t R,
                   float c, float* diff, float* mmd2, dv_stream_t stream);
int dv_mmd_rff_bwd(const float* th, int64_t ld, int32_t n, int32_t R, const float* diff, const float* gout, float coef,
                   float* G, int64_t ldg, dv_stream_t stream);

/* ------------------------------------------------------------- row movement
 * out[r,:W] = src[idx?idx[r]:r, :W] (+ sigma*noise[r,:W])  -- the group gathers of
 *   src/DrVAE.py:585-608 and the training-noise augmentation of src/DrVAE.py:404-407
 *   (N(0,1)*add_noise_var) in one pass.
 * onehot_cls != NULL additionally writes out[r, W + c] = (c == onehot_cls[r]) for c < Y:
 *   `torch.cat([z, one_hot(y)], 1)` of src/blocks.py:161 + src/blocks.py:78-92. */
int dv_rows_gather(const float* src, int64_t lds, const int32_t* idx, int32_t n, int32_t W, const float* noise,
                   int64_t ldn, float sigma, const int32_t* onehot_cls, int32_t Y, float* out, int64_t ldo,
                   const dv_wait* park, dv_stream_t stream);
/* Graph-resident minibatch feed (input pipeline of src/run_drvae.py:150-166 + the group gathers of
 * src/DrVAE.py:585-608, kept on the device).  `table` holds the dataset row of every slot of every
 * batch of an epoch (n_batches x B, drawn by the weighted sampler on the device); batch
 * b = clamp(ctr[0] - base[0], 0, n_batches-1) is written into the step's buffers:
 *   xin[r]     = x1[table[b,r]]                (r <  B)      } + sigma*noise[r]
 *   xin[B + j] = x2[table[b,pair_rows[j]]]     (j <  Np)     }
 *   label_r[l*B+i] = has_y[i] ? y[table[b,i]] : 0
 *   fp_cls[m]  = fp_lab[m] ? y[table[b,fp_i[m]]] : fp_slot[m];  onehot[m,c] = (c == fp_cls[m])
 *   ylab[i,:]  = yf[table[b,i],:]   (Yc floats per row; regression targets of type_y='cont', or NULL)
 * ctr/base are DEVICE scalars (ctr = the optimiser's step counter), so the launch arguments are
 * constant and the launch can live inside the captured train-step graph. */
/* `masks` (optional): the per-batch masks of a batch-independent plan (dv_batch_masks below, same table / ctr / base /
 * B / L) written by one more workgroup of this launch instead of a launch of their own. */
/* split form (raw-count inputs; `xt` != NULL, trailing fields of the descriptor): the wave that owns row r also writes the
 * RAW row to xt[r,:] (ldt >= X) -- the reconstruction target, without noise -- and xin[r,:] = T(x) + sigma*noise[r] as one
 * fmaf, T = log1p with `transform` == 1 (0: identity).  A compile-time variant of the kernel; with xt == NULL the launch is
 * what it was.  `transform` == 3 (`x_transform='log1p_norm'`, a compile-time variant of the split form): T(x) = log1p(x / s)
 * with s = max(sum_g x[g], 1) / X of that same SOURCE row (the x2 rows of the pairs: x2's own total), summed by the row's wave
 * in front of the transform -- lane partials in index order, then the wave sum, one fixed order -- before and without the noise;
 * x / s is a true division (one rounding).  A row whose total is X (s = 1) gives the bits of code 1, an all-zero row T = 0.
 * For integer counts with a row total below 2^24 the sum is exact in any order, so s is the ONE correctly rounded quotient
 * that dv_rec_nll_rows' _LIB kinds form; for non-integer input s is not guaranteed bit-equal to the decoder's s.  Code 2 is
 * no transform and stays refused.  DV_ERR_ARG, before any launch: `transform` outside {0, 1, 3}, `transform` != 0 without
 * xt, xt not 16-byte aligned.  The step's explicit-batch path runs this form too, over a one-batch identity table with
 * ctr = base = a zero word, x1 / x2 = the two halves of the plan's source rows and no label outputs (y, has_y, label_r,
 * fp_* all NULL: the argument checks never required them without label outputs, so none had to be relaxed), so host-fed
 * and graph-resident steps form their inputs with one kernel and agree bit for bit. */
/* sparse rows (CSR; the six trailing fields csr1_* / csr2_* of the descriptor, all NULL: the launch as it was, bit for bit).
 * With csr1_ptr given, matrix 1 is held as CSR rows instead of a dense x1: `csr1_ptr` = N + 1 int64 row offsets (nnz may
 * exceed 2^31), `csr1_idx` = int32 column indices, strictly increasing inside a row, `csr1_val` = the fp32 values; x1 must
 * then be NULL and ld1 is not read.  csr2_* / x2 / ld2 likewise and independently: one matrix may be dense, the other sparse.
 * The source row of output row r is the same table / pair_rows indexing, and every other output and rider (labels, fp_*,
 * one-hots, ylab, the masks workgroup, park, ctr / base and the batch clamp) is unchanged.  The row's wave stages the row
 * through LDS in chunks of 1024 columns (zeroes its chunk, scatters the row's entries whose column falls inside it, waits
 * for its own LDS writes) and reads from there the very 16-byte groups / scalars the dense launch loads from HBM; all that
 * follows -- the xt store, T, fmaf(sigma, noise, T(x)), the store pattern, both access paths (16-byte when xin / noise / xt
 * rows are 16-byte aligned, scalar for any X >= 1 at any alignment) -- is the dense launch's code, so the outputs are the
 * bits the dense launch writes for the densified matrix.  `transform` == 3: rows of up to 1024 columns are summed from the
 * staged row in the dense launch's order (equal bits for any values); wider rows from the CSR values -- lane partials in
 * index order, then the wave sum: exact, and so bit-equal, for integer counts with a row total below 2^24 (the caveat stated
 * for s above).  Memory contract: the kernel reads ptr[row], ptr[row + 1] and the entries between them, writes exactly the X
 * columns of the output rows, and SKIPS an entry whose column is outside [0, X) -- never stores it; the caller validates the
 * structure once (sorted rows without duplicates, columns in range), the skip only makes a caller's error harmless.  No
 * atomics: repeated launches give equal bits.  16 KiB of static LDS per workgroup, in the sparse instantiations only.
 * DV_ERR_ARG, before any launch and at B == 0 too: an incomplete triple (some but not all of ptr / idx / val), a matrix with
 * both a dense pointer and a triple; and, where rows are read (B > 0; Np > 0 for matrix 2), a matrix with neither. */
/* `park` (optional): the launch first parks like dv_flag_wait -- the first launch of a step waiting for the previous
 * step's other launch chain (DV_ERR_UNSUPPORTED for grids above DV_MAX_PARKED_GRID workgroups). */
typedef struct dv_batch_masks_desc {
    const int32_t* hx;
    const int32_t* hy;
    const int32_t* y;
    int32_t Np;
    float n_tot, kl_rate, pert_rate, yl_rate;
    const float* beta;
    float* c_nll;
    float* c_klz2;
    float* c_yl;
    float* w_recl;
    float* w_pert;
    float* w_yl;
    int32_t* label;
    float* c_klp;
    const int32_t* one_slot;
    const int32_t* gcounts;
    /* annealing schedules (trailing fields; all zero / NULL: the launch as it was).  sched_step != NULL: the launch
     * evaluates the step's schedule record from it = sched_step[0] (the number of finished training iterations, a DEVICE
     * scalar) -- see "annealing schedules" below -- and `beta` is not read */
    const int32_t* sched_step;
    int32_t pert_itermax, pert_offset;
    int32_t kl_itermax;
    int32_t yl_itermax, yl_offset;
    int32_t lr_itermax;
    float mmd_rate;
    float* sched;
    float* c_kld;
    float* w_klz2;
    float* w_klp;
    float* w_elbo;
    float* w_cmpl;
} dv_batch_masks_desc;
/* ABI 11: the feed's operands as a descriptor (names as in the comment above; 37 positional arguments before) */
typedef struct dv_batch_feed_desc {
    const float* x1;
    int64_t ld1;
    const float* x2;
    int64_t ld2;
    const int32_t* y;
    const int32_t* table;
    int32_t n_batches;
    const int32_t* ctr;
    const int32_t* base;
    int32_t B;
    const int32_t* pair_rows;
    int32_t Np;
    int32_t X;
    const float* noise;
    int64_t ldn;
    float sigma;
    float* xin;
    int64_t ldo;
    const int32_t* has_y;
    int32_t L;
    int32_t* label_r;
    const int32_t* fp_i;
    const int32_t* fp_lab;
    const int32_t* fp_slot;
    int32_t Mf;
    int32_t* fp_cls;
    float* onehot;
    int64_t ldh;
    int32_t Y;
    const float* yf;
    float* ylab;
    int32_t Yc;
    float* onehot2;
    int64_t ldh2;
    /* split form (trailing fields; xt == NULL: the launch as it was) -- see "split form" above */
    float* xt;
    int64_t ldt;
    int32_t transform;
    /* sparse rows (trailing fields; all NULL: the launch as it was) -- see "sparse rows" above */
    const int64_t* csr1_ptr;
    const int32_t* csr1_idx;
    const float* csr1_val;
    const int64_t* csr2_ptr;
    const int32_t* csr2_idx;
    const float* csr2_val;
} dv_batch_feed_desc;
int dv_batch_feed(const dv_batch_feed_desc* d, const dv_batch_masks_desc* masks, const dv_wait* park,
                  dv_stream_t stream);
/* dst[di,:W] = beta*dst[di,:W] + sum_{t in [seg_ptr[i],seg_ptr[i+1])} w[t]*src[seg_rows[t],:W],
 * di = dst_idx?dst_idx[i]:i; seg_ptr==NULL: segment i is the single row (seg_rows?seg_rows[i]:i).
 * Deterministic (no atomics): the transpose of every gather above. */
/* Per-batch masks of a batch-independent ("universal") step plan -- every row materialised as a pair with all Y
 * class slots; which rows really are pairs / labeled is DATA: the group split and the per-example normalisers of
 * src/DrVAE.py:565-624 (N_total fixed = n_tot, N_pairs and N_labeled counted per batch, max(1, .)) become
 * coefficient / weight vectors written on the device from the batch's flags.  Row i of the batch is dataset row
 * table[b, i] with b = clamp(ctr[0] - base[0]) (graph-resident epoch feed, as dv_batch_feed) or row i itself
 * (table == NULL: hx / hy / y are batch-local).  With r = l*B + i, px / py = the row is a pair / labeled:
 *   c_nll[r] = -1/(L n_tot);  c_nll[LB + r] = px ? -1/(L n_tot) : 0;  c_nll[2LB + r] = px ? -beta pert_rate/(L N_pairs) : 0
 *   w_recl = |c_nll[0 : 2LB]|;  w_pert[r] = px ? 1/(L N_pairs) : 0;  c_klz2[r] = px ? beta kl_rate/(L n_tot) : 0
 *   c_yl[r] = py ? -yl_rate/(L N_labeled) : 0;  w_yl[r] = 1/(L N_labeled);  label[r] = py ? -2 - y : 0
 *   c_klp[i] = 1/n_tot, c_klp[B + i] = px ? 1/n_tot : 0   (optional; B + B rows: KL to the prior of q(z1|x1) | q(z2|x2))
 * (label <= -2 is what dv_ymarg_* read as "labeled row, all class slots materialised").  hx == NULL / hy == NULL:
 * model without pairs / labels.  beta: DEVICE scalar (perturbation annealing coefficient).  One workgroup.
 * Np <= B: only rows [0, Np) of the batch have pair slots (a plan with fewer x2 / z2 rows for feeds that put a
 * batch's pairs first: DeviceBatcher(mode='sampler', pair_bucket=...)); the pair-indexed vectors then have L*Np
 * entries, slot q = l*Np + j, and sit behind the L*B row entries: c_nll[LB + q], c_nll[LB + L*Np + q], w_recl[LB + q],
 * w_pert[q], c_klz2[q], c_klp[B + j].  Np == B is the layout written out above.
 * one_slot (B flags, optional): rows the plan gives ONE class slot because the feed guarantees they are labeled
 * (DeviceBatcher(label_bucket=...)): label[r] = y, the form dv_ymarg_* read for a single-slot row. */
/* gcounts (optional; data parallelism): the GLOBAL (N_pairs, N_labeled) of batch b as two int32 per batch
 * of the table (table == NULL: one pair) -- every rank draws the same global index table from the shared seed and runs its
 * slice of each batch, so the global counts are table data; with them the normalisers above use the global counts instead
 * of this shard's own (n_tot is then the global number of rows): summed shard gradients == the gradient of the
 * concatenated batch. */
/* annealing schedules (sched_step != NULL; src/DrVAE.py:549-557,619-622, src/DGMMixin.py:77-104).  With it = sched_step[0] and
 *   coef(it, max, off) = it - off > 0 ? min(1, 0.01 + (it - off) / max) : 0.01,   a schedule with itermax <= 0 is OFF (value 1),
 * one thread evaluates, in double from the integers, and stores with one rounding each
 *   sched[0] = beta_pert = coef(it, pert_itermax, pert_offset)      sched[1] = beta_kl = coef(it, kl_itermax, 0)
 *   sched[2] = beta_yr   = coef(it, yl_itermax, yl_offset)          sched[3] = lr_scale = max(0.01, 1 - coef(it, lr_itermax, 0))
 * (16 bytes the optimiser sweeps read through dv_adam_hyper.lr_scale), uses beta_pert where `beta` is read above, folds
 * beta_kl into c_klz2, c_klp and c_kld[r] = beta_kl / (L n_tot) (L*B entries, optional), beta_yr into c_yl, and writes the
 * weights dv_loss_assemble reads:  w_elbo = {1, -beta_kl, hx ? beta_pert pert_rate : 0},
 *   w_cmpl = {0, 0, 0, hy ? -beta_yr yl_rate : 0, mmd_rate != 0 ? -mmd_rate : 0, -1, 0, 0}.
 * w_klz2 / w_klp (optional, laid out as c_klz2 / c_klp): the same vectors WITHOUT beta_kl -- the weights of the reported,
 * unscaled KLD. */
int dv_batch_masks(const dv_batch_masks_desc* m, const int32_t* table, int32_t n_batches, const int32_t* ctr,
                   const int32_t* base, int32_t B, int32_t L, dv_stream_t stream);
int dv_rows_segment_sum(const float* src, int64_t lds, const int32_t* seg_ptr, const int32_t* seg_rows,
                        const float* w, int32_t n, int32_t W, const int32_t* dst_idx, float* dst, int64_t ldd,
                        float beta, const dv_wait* park, dv_stream_t stream);
/* out[0] = beta*out[0] + scale * sum_i w[i]*x[idx?idx[i]:i]   (loss scalars; one workgroup) */
int dv_weighted_sum(const float* x, const float* w, const int32_t* idx, int32_t n, float scale, float* out,
                    float beta, dv_stream_t stream);
/* Reconstruction metrics of `eval_x_reconstruction` (src/DGMMixin.py:128-156), the O(M*X) part:
 *   dv_recon_row_stats: out[i, 0..5] = { sum_g (x-r)^2, mean_g x, mean_g r, sum (x-mx)^2, sum (r-mr)^2,
 *                                        sum (x-mx)(r-mr) }   -> RMSE and the per-row Pearson r
 *   dv_col_moments   : out[b,0,g] = sum_i x, out[b,1,g] = sum_i x^2, out[b,2,g] = sum_i (x-r)^2  (fp64) over the rows i
 *                      of row block b = [b*ceil(M/row_blocks), ...): `out` is (row_blocks, 3, X); the caller adds the
 *                      blocks up (a fixed order: no atomics) -- ABI 9: one workgroup per (64 columns, row block)
 *                      instead of 16 workgroups walking all M rows (8192 x 978: 591 -> ~15 us)
 *                      -> variance-weighted R^2 (sklearn r2_score(multioutput='variance_weighted')) */
int dv_recon_row_stats(const float* x, int64_t ldx, const float* r, int64_t ldr, int32_t M, int32_t X, float* out,
                       dv_stream_t stream);
int dv_col_moments(const float* x, int64_t ldx, const float* r, int64_t ldr, int32_t M, int32_t X, double* out,
                   int32_t row_blocks, const int32_t* sel, const float* r_bias, dv_stream_t stream);
/* `sel` (optional, ABI 11): the M rows that count, as indices into x / r (e.g. the rows with a second profile) */
/* `r_bias` (X, optional, round 5): r holds a RAW heads product, r + r_bias is the reconstruction.
 * dv_recon_rows: dv_recon_row_stats AND the Gaussian log-likelihood rows (dv_gauss_nll_rows_fwd, SIGMA mode) in ONE pass
 * over (x, mu, sd) for rows of up to DV_RECON_ROWS_MAX_X columns -- the whole-set evaluation's 978 genes: a wave holds its
 * row in registers.  Same outputs: rows (M, 6), ll (M, optional) -- bitwise those of dv_recon_row_stats on the dword path
 * (odd X or unaligned rows); rows of even width are read with 8-B loads (a lane owns column pairs: another summation order).  bias_mu / bias_sd (both or neither): mu / sd are the heads' RAW products and are finished on the way
 * (mu + bias_mu, softplus(sd + bias_sd) + sd_shift).  X beyond the limit: DV_ERR_UNSUPPORTED (callers take the two
 * separate passes).
 *
 * The COUNT kinds (trailing fields, ABI 13; all zero / NULL = DV_RECON_GAUSS: the launch above, bit for bit, with its
 * refusals).  kind = DV_RECON_BERNOULLI / _POISSON / _NEGBIN / _ZINB: the whole-set evaluation of the count decoders in one pass
 * per row, ANY X (a workgroup walks a row; 16-byte loads when X % 4 == 0 and every operand's rows are 16-byte aligned):
 *   heads  mu (ldp) = the mean head's POST-activation output, as dv_rec_nll_rows reads it (probability | rate | NB mean);
 *          NEGBIN: sd (row stride ldt >= X, its own) = the theta head; ZINB: a row of sd (row stride ldt >= 2X) holds
 *          [theta | RAW dropout logit] back to back, X columns each, the logit row at sd + i*ldt + X -- the decoder's 3X-wide
 *          heads buffer [mu | theta | a_d] from column X on; else sd is not read.  bias_mu / bias_sd / sd_shift:
 *          NULL / unread (the count heads leave their launch finished)
 *   mean   r = mu without a size source; with size_x (row stride size_ld): r = s * mu, s = max(sum_g size_x[i,g], 1) / X,
 *          ONE rounded product.  size_x may be x itself or another matrix (the prediction of x2 is made at x1's depth);
 *          neither theta nor the logit is ever scaled.  ZINB: r is the negative-binomial mean (the denoised expression),
 *          never (1 - pi) r: rows and rec_out are exactly NEGBIN's
 *   rows   (M, 6): the six statistics of dv_recon_row_stats between x and r -- the centred sums from a second walk over
 *          the row at the means of the first (never from raw moments)
 *   ll     (M, optional): sum_g log p(x | r), the terms of dv_rec_nll_rows (kinds DV_REC_BERNOULLI / _POISSON[_LIB] /
 *          _NEGBIN[_LIB] / _ZINB[_LIB]: the same device functions; ZINB: the zero-inflated log-probability at (r, theta, a_d))
 *   rec_out (row stride rec_ld, optional, WITH a size source only): the finished mean r, for dv_col_moments; may alias
 *          mu (every element is read and written by the same lane).  Without a size source r IS mu: nothing to store,
 *          DV_ERR_ARG
 * No atomics, fixed summation order: equal bits on every launch.  DV_ERR_ARG before any launch: kind outside the five,
 * a size source with BERNOULLI, bias_mu / bias_sd with a count kind, NEGBIN with ldt < X, ZINB with ldt < 2X (both at M = 0
 * too), rec_out without a size source,
 * a row stride below X, a missing operand (M > 0); size_x / rec_out with DV_RECON_GAUSS. */
#define DV_RECON_ROWS_MAX_X 1024
enum { DV_RECON_GAUSS = 0, DV_RECON_BERNOULLI = 1, DV_RECON_POISSON = 2, DV_RECON_NEGBIN = 3, DV_RECON_ZINB = 4 };
typedef struct dv_recon_rows_desc {
    const float* x;
    int64_t ldx;
    const float* mu;
    const float* sd;
    int64_t ldp;
    const float* bias_mu;
    const float* bias_sd;
    float sd_shift;
    int32_t M;
    int32_t X;
    float* rows;
    float* ll;
    int32_t kind;
    int64_t ldt;
    const float* size_x;
    int64_t size_ld;
    float* rec_out;
    int64_t rec_ld;
} dv_recon_rows_desc;
int dv_recon_rows(const dv_recon_rows_desc* d, dv_stream_t stream);

/* Kernel-mixture MMD of `mmd_objective(kernel='poly' | 'rbf')` and the `identity` kernel (src/blocks.py:29-38,59-76; round
 * 5).  The three Gram products x1 x1^T, x2 x2^T, x1 x2^T are dv_gemm calls; on a Gram matrix G (M x N):
 *   dv_mmd_mix_fwd : part[i] = sum_j k_ij, k = 1/nb sum_b f(., gammas[b]) (HOST array, nb <= 8)
 *                    kind 0 poly: f = (gamma G_ij + 1)^2;  kind 1 rbf: f = exp(-gamma d2_ij), d2_ij = sa[i sa_stride] +
 *                    sb[j sb_stride] - 2 G_ij (the squared row norms: the diagonals of the self products)
 *   dv_mmd_mix_bwd : W[i, j] = coef * gout[0] * dk_ij / d(G_ij | d2_ij),  rs[i] = sum_j W[i, j]
 *   dv_mmd_mix_combine: out[0] = m11 - 2 m12 + m22 (MMD^2; m = sum(p) / c), out[1..3] = the means
 *   dv_mmd_identity_fwd: diff[d] = mean_i x1[i, d] - mean_i x2[i, d], out[0] = sum_d diff^2;  _bwd: dx[i, d] = coef gout[0] diff[d] */
int dv_mmd_mix_fwd(const float* G, int64_t ldg, int32_t M, int32_t N, int32_t kind, const float* gammas, int32_t nb,
                   const float* sa, int64_t sa_stride, const float* sb, int64_t sb_stride, float* part, dv_stream_t stream);
int dv_mmd_mix_bwd(const float* G, int64_t ldg, int32_t M, int32_t N, int32_t kind, const float* gammas, int32_t nb,
                   const float* sa, int64_t sa_stride, const float* sb, int64_t sb_stride, const float* gout, float coef,
                   float* W, int64_t ldw, float* rs, dv_stream_t stream);
int dv_mmd_mix_combine(const float* p11, int32_t n11, float c11, const float* p12, int32_t n12, float c12, const float* p22,
                       int32_t n22, float c22, float* out, dv_stream_t stream);
int dv_mmd_identity_fwd(const float* x1, int64_t ld1, int32_t n1, const float* x2, int64_t ld2, int32_t n2, int32_t Z,
                        float* diff, float* out, dv_stream_t stream);
int dv_mmd_identity_bwd(const float* diff, const float* gout, float coef, int32_t n, int32_t Z, float* dx, int64_t ldd,
                        dv_stream_t stream);

/* ------------------------------------------- the nuisance variable s as device data (use_s / use_MMD extension)
 * dv_nuisance_feed: the classes of a batch's rows, gathered like dv_batch_feed gathers the rows themselves --
 * batch b = clamp(ctr[0] - base[0], 0, n_batches-1) of the epoch's index table, c_i = s[table[b, i]] (s: the dataset's
 * column, int32); table == NULL: s is batch-local, c_i = s[i].  One launch, constant arguments (capturable):
 *   cls[i] = c_i                                     (B)
 *   sohe[r, k] = (k == c_i(r)),  k < S:  encoder rows  r <  B: i = r;   r >= B: i = pair_rows[r - B]        (B + Np rows)
 *   sohd[r, k] = (k == c_i(r)):          decoder rows  r < L B: i = r % B;  then L Np + L Np rows of the pairs,
 *                                                      i = pair_rows[j % Np]                          (L B + 2 L Np rows)
 * -- `torch.cat([x, one_hot(s)], 1)` of src/DrVAE.py:134-135,179-180 for the stacked rows of the fused step. */
int dv_nuisance_feed(const int32_t* s, const int32_t* table, int32_t n_batches, const int32_t* ctr, const int32_t* base,
                     int32_t B, const int32_t* pair_rows, int32_t Np, int32_t L, int32_t S, float* sohe, int64_t lde,
                     float* sohd, int64_t ldd, int32_t* cls, dv_stream_t stream);
/* Model-level MMD penalty between the nuisance classes' latent samples (src/DrVAE.py:394-398,537-540; src/DGMMixin.py:42-66)
 * for ALL terms of a step, class membership read from `cls` inside the launch.  A term GROUP g (data group, Monte-Carlo
 * sample, latent z1 | z2) is a constant list of rows of z: entries [grp_ptr[g], grp_ptr[g+1]) of `rows` (row of z) and
 * `src` (batch row of that sample: its class is cls[src]).  For every class k < K (K = S, or 1 when S == 2: the first
 * class against the rest only) there is a term t = g K + k; with n0 / n1 the group's rows inside / outside class k and
 * u_j = [c_j == k] / n0 - [c_j != k] / n1:
 *   kind 1 (rbf_fourier): theta[(k E + e), r] = a z_j . W[t, :, r] + 2 pi b[t, r]   (E = n_entries, e = the row's entry)
 *                         diff[t, r] = c sum_j u_j cos(theta_jr)                     (D = R columns)
 *   kind 0 (identity):    diff[t, d] = sum_j u_j z_j[d]                              (D = Z columns)
 *   m2[t] = sum_d diff[t, d]^2;   value[0] = sum_t -w sqrt(m2[t])
 *   dz[row_j, :] = sum_k d(fac * -w sqrt(m2[t])) / d z_j        (every row of z belongs to exactly ONE group: written, not added)
 * Defined edge cases: a term with an empty side (n0 == 0 or n1 == 0) has diff = 0; a term with m2 == 0 has value 0 and
 * gradient 0 (no division by zero).
 * _fwd writes cnt (n_groups x S: the group's rows per class), theta (kind 1) and diff; _bwd reads them back (theta is read
 * back, not recomputed: half the backward's products for K E R floats that stay in L2) and writes m2, value and dz.
 * No atomics: one writer per element.  _bwd: DV_ERR_UNSUPPORTED when 8 rows of (R + Z) floats do not fit 60 KB of LDS. */
#define DV_MMD_MAX_CLASSES 8
typedef struct dv_mmd_grouped_desc {
    const float* z;
    int64_t ldz;
    int32_t n_z;         /* rows of z / dz */
    int32_t Z;
    int32_t kind;
    int32_t R;
    int32_t n_groups;
    int32_t n_entries;   /* grp_ptr[n_groups] */
    int32_t max_rows;    /* the longest group */
    int32_t S;
    int32_t B;           /* entries of cls */
    const int32_t* grp_ptr;
    const int32_t* rows;
    const int32_t* src;
    const int32_t* cls;
    const float* W;      /* (n_groups K, Z, R) */
    const float* b;      /* (n_groups K, R) */
    float a;
    float c;
    float w;
    float fac;
    float* theta;        /* (K n_entries, R) */
    float* diff;         /* (n_groups K, D) */
    int32_t* cnt;        /* (n_groups, S) */
    float* m2;           /* (n_groups K) */
    float* value;
    float* dz;
    int64_t ldd;
} dv_mmd_grouped_desc;
int dv_mmd_grouped_fwd(const dv_mmd_grouped_desc* d, dv_stream_t stream);
int dv_mmd_grouped_bwd(const dv_mmd_grouped_desc* d, dv_stream_t stream);
/* The same penalty on a batch-independent ("universal") plan: the DATA GROUPS of the batch are data too, read inside the
 * launches the way dv_batch_masks reads them.  One captured step serves every composition of groups and classes.
 * Row lists.  z holds the sample rows of a universal plan with B batch rows, Np <= B pair slots (slot j belongs to batch
 *   row j) and L Monte-Carlo samples: n_z = L (B + Np) rows.  A row list q < n_lists = L (Np > 0 ? 2 : 1) is one (sample,
 *   latent) pair: q < L is the z1 list of sample l = q, rows l B + i of z, i < B, batch row i; q >= L is the z2 list of
 *   sample l = q - L, rows o2 + l Np + j, j < Np, batch row j (o2 = L B).  Every row of z sits in exactly one list.
 * Data group of batch row i.  With r = table[b, i], b = clamp(ctr[0] - base[0], 0, n_batches - 1) (table == NULL: r = i,
 *   batch-local flags), hx = hx[r] != 0 and hy = hy[r] != 0 (hx == NULL / hy == NULL: a model without pairs / without
 *   labels, the flag is 0; r is clamped to [0, n_flags)), the G groups of `model` in the reference's order are
 *     DV_MMD_GROUPS_DRVAE (G = 4): [hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx]     (src/DrVAE.py:585-608)
 *     DV_MMD_GROUPS_PVAE  (G = 2): [~hx, hx]                                    (src/PVAE.py:441-453)
 *     DV_MMD_GROUPS_VFAE  (G = 2): [hy, ~hy]                                    (src/VFAE.py:421-433)
 *   A z2 row exists for the pairs of the batch only: batch row j is a member of a z2 list iff hx, so a z2 list has
 *   members in the groups of pairs only.
 * Terms.  Term group tg = q G + g: the MEMBERS of (list q, data group g) are the list's rows whose batch row is in group
 *   g, in ascending batch row.  For every class k < K (K = S, or 1 when S == 2) there is a term t = tg K + k; n0 / n1 are
 *   the members with cls[batch row] == k / != k.  theta, diff, m2, value and dz are the formulas of dv_mmd_grouped_* above
 *   with the sums over j running over the members; value sums over ALL n_lists G K terms.
 * Layouts (T = n_lists G K terms; D = R for kind 1, Z for kind 0):
 *   W (T, Z, R), b (T, R), diff (T, D), m2 (T)            indexed by the term
 *   theta (K, n_z, R): theta[(k n_z + row), r] of z's row `row` (every row is a member of at most one term group)
 *   cnt (n_lists G, S + 1): members per class, then the number of members of the term group
 *   members (n_lists G, B): the members' batch rows, the first cnt[tg, S] entries of row tg (workspace, _fwd -> _bwd)
 * Defined edge cases: a term without members, with an empty side (n0 == 0 or n1 == 0) or with m2 == 0 has value 0 and
 *   gradient 0; its diff row is written as zeros.  A row of z that belongs to no term -- the z2 row of a pair slot whose
 *   batch row is no pair in this batch -- gets dz written as exact zeros by every launch (the slot may have held a pair
 *   in the batch before).  Rows of theta of such rows and of empty-sided terms are not written.
 * Determinism: one writer per output element, no atomics, no zero-fill launch, fixed summation order (members in
 *   ascending batch row, split over the same 16 row groups / 64 lanes as dv_mmd_grouped_*): two launches on the same
 *   inputs give bit-equal results.
 * _fwd writes members, cnt, theta (kind 1) and diff; _bwd reads them back and writes m2, value and every row of dz.
 * Refusals: S > DV_MMD_MAX_CLASSES, Np > B, a missing operand: -1 before anything is launched.  DV_ERR_UNSUPPORTED: _bwd
 *   when 8 rows of (R + Z) floats do not fit 60 KB of LDS (as dv_mmd_grouped_bwd), either when B ints do not. */
#define DV_MMD_GROUPS_DRVAE 0
#define DV_MMD_GROUPS_PVAE 1
#define DV_MMD_GROUPS_VFAE 2
typedef struct dv_mmd_masked_desc {
    const float* z;
    int64_t ldz;
    int32_t Z;
    int32_t kind;        /* 1 rbf_fourier, 0 identity */
    int32_t R;
    int32_t S;
    int32_t B;           /* batch rows: entries of cls */
    int32_t Np;          /* pair slots */
    int32_t L;
    int32_t model;       /* DV_MMD_GROUPS_* */
    const int32_t* cls;
    const int32_t* hx;
    const int32_t* hy;
    int32_t n_flags;     /* entries of hx / hy */
    const int32_t* table;
    int32_t n_batches;
    const int32_t* ctr;
    const int32_t* base;
    const float* W;
    const float* b;
    float a;
    float c;
    float w;
    float fac;
    float* theta;
    float* diff;
    int32_t* cnt;
    int32_t* members;
    float* m2;
    float* value;
    float* dz;
    int64_t ldd;
} dv_mmd_masked_desc;
int dv_mmd_masked_fwd(const dv_mmd_masked_desc* d, dv_stream_t stream);
int dv_mmd_masked_bwd(const dv_mmd_masked_desc* d, dv_stream_t stream);

/* The tail of a whole-set evaluation (round 5) in three launches instead of ~75 small library ones:
 * dv_recon_finalize: out[0..3] = rmse, variance-weighted R^2, mean per-row Pearson r, mean log-likelihood (float64) from
 *   dv_recon_row_stats' rows (M_all x 6; `sel`: the n rows that count, NULL = rows 0..n-1), dv_col_moments' partials over
 *   the same rows (row_blocks x 3 x X) and the per-row log-likelihoods `ll` (optional: out[3] = nan without) --
 *   `eval_x_reconstruction`, src/DGMMixin.py:128-156.  One workgroup, fixed summation order.
 * dv_rank_metrics: accuracy, ROC-AUC and average precision of `eval_y_prediction` (src/DGMMixin.py:158-190; sklearn's
 *   roc_auc_score / average_precision_score: one threshold per distinct score) WITHOUT a sort: for the n selected rows
 *   (`sel`, NULL = all) and each class c in [c0, c0 + n_cls) the launch counts, per row, how many rows / positives
 *   score above and equal (O(n^2) integer counting spread over the chip; n <= DV_RANK_MAX_ROWS, DV_ERR_UNSUPPORTED
 *   above), then   AUC = sum_{negatives j} (#pos above j + #pos tied with j / 2) / (n_pos n_neg)   (integer sums: exact)
 *                  AP  = 1/n_pos sum_{positives i} #pos(score >= s_i) / #rows(score >= s_i)
 *   positive = binary ? y > 0 : y == c; score = proba[row, c].  out[2c] = AUC (nan: one class only / empty), out[2c + 1]
 *   = AP (0: no positive), out[2 n_cls] = accuracy mean(pred == y), hits / n in fp32 (pred optional: nan without one, as
 *   for n = 0 -- "none given" is not "0 % correct").  `counts` (n_cls x n x 4 int32) must
 *   be zero on entry and is zero again on return.  Deterministic. */
#define DV_RANK_MAX_ROWS 32768
int dv_recon_finalize(const float* rows, const int32_t* sel, int32_t n, int32_t X, const double* cols, int32_t row_blocks,
                      const float* ll, double* out, dv_stream_t stream);
int dv_rank_metrics(const float* proba, int64_t ldp, const int32_t* y, const int32_t* pred, const int32_t* sel, int32_t n,
                    int32_t c0, int32_t n_cls, int32_t binary, int32_t* counts, double* out, dv_stream_t stream);
/* dv_reg_metrics: `eval_y_prediction` for a CONTINUOUS target (src/DGMMixin.py:181-188: numpy / sklearn r2_score / scipy
 *   pearsonr) over the n selected rows (`sel`, NULL = rows 0..n-1) x Y columns of pred / y (fp32), both flattened:
 *     out[0] = sqrt(mean((y-p)^2))
 *     out[1] = 1 - sum((y-p)^2) / sum((y-mean y)^2)                                    (nan: sum((y-mean y)^2) == 0)
 *     out[2] = sum((y-mean y)(p-mean p)) / sqrt(sum((y-mean y)^2) sum((p-mean p)^2))   (nan: zero denominator)
 *   n == 0: all three nan.  Float64 accumulation, TWO passes (means, then centred sums: no cancellation for targets
 *   clustered in (0,1)), one workgroup, fixed summation order, no atomics: two calls give bit-equal results.  (ABI 12,
 *   additive) */
int dv_reg_metrics(const float* pred, int64_t ldp, const float* y, int64_t ldy, const int32_t* sel, int32_t n, int32_t Y,
                   double* out, dv_stream_t stream);

/* All loss scalars of one step in a single launch (src/DrVAE.py:611-624):
 *   loss[0..4] = 0; for each term: loss[out] += scale * sum_i w[i]*x[i]   (w == NULL: plain sum)
 *   loss[5] (ELBO) = <w_elbo[0..2], loss[0..2]>;  loss[6] (CMPL) = <w_cmpl[0..7], loss[0..7]>
 * `terms` is a HOST array (copied into the kernel arguments); x/w are device pointers. */
#define DV_MAX_LOSS_TERMS 8
typedef struct dv_loss_term {
    const float* x;
    const float* w;
    int32_t n;
    float scale;
    int32_t out;     /* 0 RECL, 1 KLD, 2 PERT, 3 YL, 4 MMD */
    int32_t row_len; /* > 1: x is (n / row_len, row_len) and w holds one weight per ROW (w[i / row_len]); else 0 / 1 */
} dv_loss_term;
/* accum (optional, 8 floats): accum[i] += loss[i] in the same launch -- the running sums of a training epoch
 * (src/DrVAE.py:787-795 averages the per-batch objective), read by the host once per epoch */
int dv_loss_assemble(const dv_loss_term* terms, int32_t n_terms, const float* w_elbo, const float* w_cmpl,
                     float* loss, const int32_t* halt, int32_t n_halt, float* accum, dv_stream_t stream);
/* same, but first parks on `wait` (a dv_wait, like dv_flag_wait) inside the launch (the terms of another chain are
 * read only after the wait; saves the separate wait launch), and last advances the counters of `bump` (a dv_bump, like
 * dv_counters_add2; a counter may alias wait->ctr: it is read before; saves the counter launch in front of the
 * optimiser).  With n_terms == 0 `loss` is left untouched: the launch only parks and advances the counters (another
 * chain assembles the scalars).  wait == NULL / wait->flag == NULL: no wait: the launch assembles the scalars and
 * advances the counters; bump == NULL: no counters.  (ABI 11: the wait and the counters were ten positional scalars) */
int dv_loss_assemble_after(const dv_wait* wait, const dv_loss_term* terms, int32_t n_terms, const float* w_elbo,
                           const float* w_cmpl, float* loss, const dv_bump* bump, const int32_t* halt, int32_t n_halt,
                           float* accum, dv_stream_t stream);
/* nn.BatchNorm1d(N, affine=True) over the rows of x (M, N) -- the `batch_norm=True` option of blocks.MLP
 * (src/blocks.py:137-149).  training != 0: batch statistics (biased variance for the normalisation; running_mean /
 * running_var, when given, move by `momentum`, running_var with the unbiased variance, as torch); training == 0: the
 * running statistics.  mean_out / rstd_out (N each) keep what the backward pass needs. */
int dv_bn_fwd(const float* x, int64_t ldx, int32_t M, int32_t N, const float* w, const float* b, float eps,
              float* mean_out, float* rstd_out, float* y, int64_t ldy, float* running_mean, float* running_var,
              float momentum, int32_t training, dv_stream_t stream);
/* dw = sum_i dy*xhat, db = sum_i dy, dx = w*rstd*(dy - db/M - xhat*dw/M) (training) | dy*w*rstd (eval); dx, dw, db
 * optional */
int dv_bn_bwd(const float* dy, int64_t ldd, const float* x, int64_t ldx, const float* mean, const float* rstd,
              const float* w, int32_t M, int32_t N, float* dx, int64_t lddx, float* dw, float* db, int32_t training,
              dv_stream_t stream);
/* y = x * mask * scale: nn.Dropout with its keep mask (forward, and backward on dy) -- hidden-layer dropout of
 * blocks.MLP (src/blocks.py:140-141) */
int dv_mask_scale(const float* x, int64_t ldx, const float* mask, int64_t ldm, float scale, int32_t M, int32_t N,
                  float* y, int64_t ldy, dv_stream_t stream);
/* y[i] = a*x[i] + b*y[i] over n contiguous floats */
int dv_axpby(const float* x, float a, float* y, float b, int64_t n, dv_stream_t stream);

/* ------------------------------------------------------------------ optimiser (K11)
 * torch.optim.Adam as configured by src/DGMMixin.py:36 (coupled L2: g += wd*p), in the
 * arithmetic order of torch 2.x `_single_tensor_adam`, on a flat fp32 arena.
 * step_dev[0] (int32, device) is the 1-based step used for the bias corrections; it is
 * read, not modified (bump it with dv_counter_add so graph replays advance). gscale
 * multiplies g first (1/world_size style scaling; 1.0 for summed gradients).
 * Two options ride on every sweep below through trailing fields of dv_adam_hyper (all zero / NULL: the sweep as it was):
 *   decoupled    AdamW (torch 2.x `_single_tensor_adam` under torch.optim.AdamW): p *= (float)(1 - lr_eff * weight_decay)
 *                first (the factor in double, rounded once; lr_eff the annealed rate), the gradient takes no wd*p term, the
 *                moments and the update follow as ever.  The clip coefficient does not touch the decay.  Adam sweeps only:
 *                dv_adamax_l2 / dv_adamax_l2_clipped return DV_ERR_ARG (torch has no decoupled Adamax)
 *   avg          the exponential moving average of the parameters: after an element's new p is formed,
 *                e = fmaf(w, p_new - e, e) with w = (float)(1.0 - (double)avg_decay); n floats laid out like p (element 0
 *                belongs to p[0] of THIS call), loaded and stored the way p is on each path (it joins the 16-B alignment
 *                test).  A sweep that returns early -- a halt word set, a clipped step skipped for a non-finite gradient, a
 *                parked workgroup whose gate timed out -- touches nothing of it.  avg_decay outside (0, 1) or avg not
 *                4-byte aligned: DV_ERR_ARG before any launch.  9 words of traffic per parameter instead of 7 */
typedef struct dv_adam_hyper {      /* ABI 11: six same-typed scalars travel by name, not by position */
    float lr;
    float beta1;
    float beta2;
    float eps;
    float weight_decay;
    float gscale;
    /* learning-rate annealing (trailing field; NULL: the sweep as it was): a DEVICE scalar, read by the one thread that
     * evaluates the bias corrections; the sweep then runs with lr_eff = (float)((double)lr * (double)lr_scale[0]) where it
     * uses lr (lr_scale[0] == 1.0f: the plain sweep's bits).  Every sweep below honours it, gated and clipped included */
    const float* lr_scale;
    int32_t decoupled;   /* 0: coupled L2 (as ever). 1: AdamW */
    float avg_decay;     /* d of the average; read only when avg != NULL */
    float* avg;          /* NULL: no average. Else n floats laid out like p (element 0 = p[0] of THIS call) */
} dv_adam_hyper;
int dv_adam_l2(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
               const int32_t* step_dev, const int32_t* halt, int32_t n_halt, dv_stream_t stream);
/* same sweep, but the elements [lo, hi) are touched only after another launch chain has published `gate->flag`
 * (flag[0] >= ctr[0] + add, see dv_flag_publish): only the workgroups overlapping the range park (bounded
 * like dv_flag_wait: err[0] = 1 on time-out, err[1] += ticks parked), so gradients that are leaves of
 * the backward pass may still be in flight on the other chain when the optimiser launch starts.  A parked workgroup
 * looks at `halt` again after its wait: with gate->err among the halt words a time-out leaves the elements of the parked
 * workgroups (at least [lo, hi)) as they are while the others have been swept; without it the time-out is only reported */
int dv_adam_l2_gated(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                     const int32_t* step_dev, const dv_wait* gate, int64_t lo, int64_t hi, const int32_t* halt,
                     int32_t n_halt, dv_stream_t stream);
/* torch.optim.Adamax with coupled L2 (the `optim_alg='adamax'` branch of src/DGMMixin.py:37-38):
 * u is the exponentially weighted infinity norm; same conventions as dv_adam_l2. */
int dv_adamax_l2(float* p, const float* g, float* m, float* u, int64_t n, const dv_adam_hyper* h,
                 const int32_t* step_dev, const int32_t* halt, int32_t n_halt, dv_stream_t stream);
/* Global-norm gradient clipping and the non-finite guard of the optimiser sweep (EXTENSION: the reference has no
 * counterpart; semantics of torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) in front of the optimisers above).
 * Three entry points around a dv_clip_state in device memory, 8-byte aligned, owned by the caller and zeroed once but for
 * max_norm: its first word is the step counter the sweeps read (bump it as ever), DV_SUMSQ_PARTIALS(n) doubles of
 * workspace follow it.  Nothing leaves the device.
 *   dv_grad_norm_clip: the NORM PASS over the n contiguous floats at g (n == 0: g may be NULL), two launches.  (1) one double
 *       partial per workgroup = the sum of g[i]^2 over its elements, each element widened to double first;
 *       DV_SUMSQ_PARTIALS(n) workgroups, a function of n alone, at most 1024.  No atomics: the value of every partial is a
 *       function of n and of the pointer's offset within 16 bytes -- bitwise the same from run to run and from rank to rank.
 *       Non-temporal loads from n >= 16 Mi elements on (the streaming sweep's threshold).  g is only read.  (2) sumsq = the
 *       partials summed in index order; norm = |gscale| sqrt(sumsq); coef = min(1, max_norm / (norm + 1e-6)), in double,
 *       stored as fp32.  sumsq not finite (some g[i] is inf or NaN -- finite fp32 inputs cannot overflow the double sum):
 *       skip = 1, coef = 0, n_skipped += 1; else skip = 0.  max_norm > 0; +inf: no clipping (coef = 1), the guard alone.
 *   dv_adam_l2_clipped / dv_adamax_l2_clipped: the sweeps above, counting by st->step and reading st->rec: skip set -> p, m,
 *       v / u are left as they are (not sticky, no halt word is written); else the gradient is scaled by fl32(h->gscale *
 *       coef) where the plain sweep scales by h->gscale (coef == 1.0f: the plain sweep's bits) and the bias corrections use
 *       t = step - n_skipped: a skipped step leaves no trace in the optimiser state.  There is no gated form. */
typedef struct dv_clip_record {
    float norm;                     /* |gscale| * 2-norm of the gradient range of the last norm pass */
    float coef;                     /* its clip coefficient, in [0, 1] */
    int32_t skip;                   /* 1: that gradient held a non-finite element, the sweep reading this record does nothing */
    int32_t n_skipped;              /* running count of such steps */
} dv_clip_record;
typedef struct dv_clip_state {      /* 32 bytes, then the workspace */
    int32_t step;                   /* the 1-based optimiser step (what step_dev[0] is to the plain sweeps) */
    int32_t reserved;
    double max_norm;                /* the threshold, written by the caller */
    dv_clip_record rec;
} dv_clip_state;
#define DV_SUMSQ_PER_BLOCK 8192     /* elements of g per workgroup of the norm pass, below the cap */
#define DV_SUMSQ_MAX_BLOCKS 1024    /* the cap */
#define DV_SUMSQ_PARTIALS(n) ((n) <= DV_SUMSQ_PER_BLOCK ? 1 : (n) > DV_SUMSQ_PER_BLOCK * (int64_t)(DV_SUMSQ_MAX_BLOCKS - 1) ? DV_SUMSQ_MAX_BLOCKS : ((n) + DV_SUMSQ_PER_BLOCK - 1) / DV_SUMSQ_PER_BLOCK)
int dv_grad_norm_clip(const float* g, int64_t n, float gscale, dv_clip_state* st, dv_stream_t stream);
int dv_adam_l2_clipped(float* p, const float* g, float* m, float* v, int64_t n, const dv_adam_hyper* h,
                       const dv_clip_state* st, const int32_t* halt, int32_t n_halt, dv_stream_t stream);
int dv_adamax_l2_clipped(float* p, const float* g, float* m, float* u, int64_t n, const dv_adam_hyper* h,
                         const dv_clip_state* st, const int32_t* halt, int32_t n_halt, dv_stream_t stream);
int dv_counter_add(int32_t* counter_lo_hi, int32_t n_words, int64_t inc, dv_stream_t stream);
/* Joins folded into their consumers: dv_z2f_post_bwd, dv_reparam_bwd_seg and dv_rows_segment_sum take an optional `park`
 * (every workgroup of the launch first parks like dv_flag_wait: the first consumer of another chain's
 * results waits for them itself, no separate wait launch; keep such grids well below the chip's resident
 * capacity), dv_reparam_bwd_seg an optional `bump` (the launch also advances up to two device counters
 * like dv_counters_add2).  `halt` arguments (here and above): n_halt error words at halt[0], halt[2],
 * halt[4] ... (the err[0] of the dv_wait sites of a step, laid out as (err, ticks) pairs); if any is
 * non-zero the loss scalars come out NaN and the optimiser sweep leaves p / m / v untouched. */
/* two device counters in one launch (the optimiser step count and the Philox counter of a train step) */
/* `pub` (optional): published on entry, BEFORE the counters move (its ctr may be one of them) */
int dv_counters_add2(int32_t* c1, int32_t n1, int64_t inc1, int32_t* c2, int32_t n2, int64_t inc2,
                     const dv_publish* pub, dv_stream_t stream);

/* Device-side fork/join between two launch chains that run concurrently (two root branches of one
 * hipGraph; no reference counterpart -- replaces graph edges, which cost ~27 us per fork+join on the
 * ROCm executor): dv_flag_publish stores flag[0] = ctr[0] + add (release) after the kernels before it
 * in its stream; dv_flag_wait parks ONE thread until flag[0] >= ctr[0] + add (acquire), so the kernels
 * after it in ITS stream see the producer's results.  It never hangs: after max_spins polls (~0.1 us
 * each) it sets err[0] = 1 and returns.  err[1] accumulates the time spent parked (wall_clock64 ticks). */
int dv_flag_publish(int32_t* flag, const int32_t* ctr, int32_t add, dv_stream_t stream);
/* (pub, optional: published on entry of the wait launch, before it starts to poll) */
int dv_flag_wait(int32_t* flag, const int32_t* ctr, int32_t add, int32_t* err, int32_t max_spins, const dv_publish* pub,
                 dv_stream_t stream);

/* out[i] ~ N(0,1), Philox4x32-10 keyed by `seed`, counter = ctr_dev[0..1] (uint64 as two
 * int32 words, device) + i/4, Box-Muller on the four outputs.  (the `normal_()` draws of
 * src/blocks.py:172,210 and src/DrVAE.py:405,415 moved on device).
 * Both generators, precisely (tests/philox_ref.py is this paragraph in numpy, tests/test_gpu_philox.py compares every
 * element): a 32-bit word x becomes the uniform u = (float(x) + 0.5f) * 2^-32, evaluated in fp32 -- u is never 0
 * (u(0) = 2^-33, hence |z| <= sqrt(-2 ln 2^-33) < 6.77) and is exactly 1 for x >= 2^32 - 128 (float(x) rounds to 2^32),
 * where the radius and with it that pair of normals is exactly 0.  Output words 0 / 1 are the radius / angle of lanes
 * 0, 1 (r cos a, r sin a with r = sqrt(-2 ln u0), a = 2 pi u1), words 2 / 3 those of lanes 2, 3.
 * dv_fill_normal's counter is (lo, hi, 0, 0) of ctr + i/4 under the key (seed_lo, seed_hi): with ctr + i/4 < 2^32 that
 * is the row-keyed stream below at (global row 0, draw id 0, event 0) under the same seed -- the two forms must not
 * share a seed.  (The train step uses the row-keyed form only.)
 *
 * THE SAMPLER (`draw` != NULL; an optional trailing argument of ABI 13, NULL = the launch above, bit for bit, with its
 * refusals).  One launch draws S posterior-predictive samples of M rows of X genes from FINISHED decoder heads, as float32:
 * out[(k - k0) * sso + r * ldo + g] for sample k = k0 .. k0 + S - 1, row r, gene g.  `out` / `n` are unused; `seed` is the
 * draw's seed and ctr_dev[0..1] its 64-bit EVENT (NULL: event 0).  This paragraph is the specification
 * (tests/count_sample_ref.py is it in numpy, float64).
 *   Stream.  The global row of row r is R = row0 + r, or grow[r] (int32, device; row0 must then be 0).  Block b of element
 *   (k, R, g) is Philox4x32-10(counter = (g, R, (k << 8) | b, event_lo), key = (seed_lo, seed_hi ^ event_hi)), its words w0..w3
 *   mapped to uniforms u(w) as above.  N(b) = sqrt(-2 ln u(w0)) cos(2 pi u(w1)) of block b (lane 0 of the Box-Muller above).  An
 *   element depends on (seed, event, k, R, g) and its own operands only -- not on M, S, the grid, the chunk a row arrives in or
 *   the access path.  The blocks are the row-keyed stream's at (col / 4 = g, global row R, draw id (k << 8) | b): a draw and
 *   the train step's noise must not share a seed.
 *   Operands.  mu[r * ldm + g] always; sd[r * lds + g] (Gaussian); theta[r * ldt + g] (NB / ZINB; ldt == 0: ONE row shared by
 *   all rows, a gene-wise dispersion, nothing expanded); logit[r * ldl + g] (ZINB, the RAW dropout logit); size[r] (optional,
 *   count kinds: the row's size factor s, else s = 1).  m = s * mu, ONE fp32 product.  theta and the logit are never scaled.
 *   All arithmetic below is fp32.
 *   DV_RECON_GAUSS: mu + sd * N(0), plain IEEE arithmetic (NaN / inf propagate).   DV_RECON_BERNOULLI: mu NaN -> NaN; else
 *   1 if u(w0 of block 0) <= mu, else 0.
 *   DV_RECON_POISSON: m NaN -> NaN; m <= 0 -> 0; else P(0, m).
 *   DV_RECON_NEGBIN / _ZINB, in this order: m NaN -> NaN.  theta NaN or theta <= 0 -> NaN.  ZINB: logit NaN -> NaN; u(w0 of
 *   block 16) <= 1 / (1 + exp(-logit)) -> 0 (a dropout).  m <= 0 -> 0.  m = +inf -> FLT_MAX.  Else P(8, lam) with the rate
 *     lam = m if theta = +inf (the Poisson limit), else by Marsaglia-Tsang: a = theta + 1 if theta < 1 else theta, d = a - 1/3,
 *     c = 1 / sqrt(9 d).  Attempt j = 0 .. 7: x = N(j), t = c x; accepted if t > -1 and
 *         ln u(w2 of block j) < x^2 / 2 + d (3 log1p(t) - t (3 + t (3 + t)))
 *     (1 - v + ln v at v = (1 + t)^3, formed from t so that no two values of size d are subtracted); then, with G the Gamma
 *     draw, q = ln(G / theta) = ln(d / theta) + 3 log1p(t) -- the quotient first, so that the logarithm's argument is near 1
 *     for a large theta and no two logarithms of size ln theta are subtracted.  theta < 1: q += ln u(w3 of block 0) / theta
 *     (u^(1 / theta) underflows; its logarithm does not).  lam = m * exp(q).  No attempt accepted: lam = m (the Gamma's mean).
 *     q not finite in fp32 -- a theta so small (a denormal) that d / theta or ln u / theta overflows, +inf, or their difference,
 *     NaN: lam = 0, as for every q below exp's range.
 *   P(b0, lam), the Poisson draw from blocks b0, b0 + 1, ...:
 *     lam >= 2^24 (beyond fp32's exact integers; +inf): min(lam, FLT_MAX), no draw.
 *     lam < 10: inversion from ONE uniform u = u(w0 of block b0): p_0 = F_0 = exp(-lam), p_i = p_(i-1) * (lam / i), F_i = F_(i-1)
 *     + p_i; the result is the smallest i in 0 .. 64 with u <= F_i; none: rint(lam).
 *     lam >= 10: Hoermann's PTRS.  b = 0.931 + 2.53 sqrt(lam), a = -0.059 + 0.02483 b, ia = 1.1239 + 1.1328 / (b - 3.4), vr =
 *     0.9277 - 3.6224 / (b - 2).  Attempt j = 0 .. 15 reads block b0 + j / 2, words (w0, w1) for even j, (w2, w3) for odd j, as
 *     (wU, wV): U = u(wU) - 0.5, V = u(wV), us = 0.5 - |U|, k = floor((2 a / us + b) U + lam + 0.43).  us >= 0.07 and V <= vr:
 *     the result is k.  Else k < 0, or us < 0.013 and V > us: next attempt (us = 0 always lands here).  Else
 *     ln V + ln ia - ln(a / us^2 + b) <= -lam + k ln lam - lgamma(k + 1): the result is k.  No attempt accepted: rint(lam).
 *   Every loop is bounded by the counts above: the launch returns on every input.  No atomics, one writer per element, nothing
 *   is written outside the S x M x X described elements; no operand is written.
 * DV_ERR_ARG, before any launch and at M == 0 or S == 0 too: kind outside the five; M, X, S or k0 < 0; k0 + S > DV_DRAW_MAX_SAMPLES;
 * row0 < 0, row0 + M > DV_DRAW_MAX_ROW, grow with row0 != 0; mu NULL; sd NULL with Gaussian; theta NULL with NB / ZINB; logit
 * NULL with ZINB; size with Gaussian or Bernoulli; ldm / ldo (and lds, ldl of a kind that reads them) below X; ldt below X and
 * not 0; with S > 1 and M > 0 a sample stride sso below (M - 1) ldo + X; out NULL with elements to write.  Operands the kind does
 * not read are ignored.  16-byte loads and stores when X % 4 == 0 and every row of every operand read is 16-byte aligned, scalar
 * ones otherwise: the same values either way. */
#define DV_DRAW_MAX_SAMPLES 16777216        /* 2^24: the sample index shares a counter word with the block index */
#define DV_DRAW_MAX_ROW 2147483648LL        /* 2^31 */
/* THE EFFECT REDUCTION (`draw->fx` != NULL; an optional trailing field of dv_draw_desc inside ABI 13, NULL = the sampler as it
 * was, bit for bit).  One launch reduces two finished mean-head matrices a (baseline, decoded from z1) and b (perturbed,
 * decoded from z2) to per (row block, group, gene) sufficient statistics of the perturbation effect, in float64; it draws
 * nothing.  It rides on the sampler's descriptor because the sampler is the other launch that reads finished heads and
 * because the descriptors of the evaluation launches have their field tails pinned by tests (docs/history/ABI_history.md,
 * round 33).  With fx set the outer descriptor supplies M (rows) and X (genes) and nothing else: every other field of it, and
 * dv_fill_normal's out, n, seed and ctr_dev, must be zero / NULL.
 *   Element.  e(r, g) = log2f(b + c) - log2f(a + c) with a = a[r * lda + g], b = b[r * ldb + g], c = pseudo (mode 0, the count
 *   decoders: a log2 fold change; the row's size factor would cancel, the heads are taken UNSCALED), or e = b - a (mode 1,
 *   Gaussian; c must be 0) -- fp32: one add per side (c != 0), two log2f, one subtraction.  The element is VALID when e is
 *   finite; an invalid element (a NaN or infinite head, a + c <= 0, ...) adds to no statistic.
 *   Rows.  Row block q owns rows [q R, min(M, (q + 1) R)), R = ceil(M / row_blocks).  grp[r] (int32, device; NULL: every row in
 *   group 0) is the row's group; a value outside [0, n_grp), negatives included, leaves the row out: it is not read.
 *   Output.  out[((q * n_grp + k) * 7 + t) * X + g], float64, EVERY element written (zeros where block q has no row of group k
 *   or lies past M).  Statistic t over the valid elements of block q's rows of group k: 0 their number n, 1 sum e, 2 sum e^2,
 *   3 #{e > delta}, 4 #{e < -delta} (strict), 5 sum a, 6 sum b.  Counts are exact integers.  Every sum is accumulated in double
 *   from the fp32 element (e^2 is the exact double product) in one fixed order, whatever the access path: no atomics, one writer
 *   per element, two launches give equal bits; a and b may alias each other and may be column views of a wider buffer.
 *   Geometry.  A workgroup of 256 threads owns 64 genes x one row block x one group (grid = ceil(X / 64) x row_blocks x n_grp):
 *   thread t holds genes 4 (t % 16) .. + 3 and walks rows q R + t / 16, + 16, ... of its group; its sixteen row slots are added
 *   as ((s0 + s1) + (s2 + s3)) inside a wave and the four waves as ((w0 + w1) + (w2 + w3)).  16-byte loads where X % 4 == 0
 *   and both matrices' rows are 16-byte aligned, scalar ones otherwise -- any X >= 1, any alignment, the same bits.
 * DV_ERR_ARG before any launch, at M == 0 too: another outer field or dv_fill_normal argument set; M < 0, X < 1 or X > 2^31 - 64; n_grp < 1 or
 * > 65535; row_blocks outside [1, max(M, 1)] or > 65535; lda or ldb < X; a, b or out NULL with M > 0; mode outside {0, 1};
 * delta < 0 or NaN; pseudo < 0 or not finite; mode 1 with pseudo != 0.  M == 0 with a valid descriptor: DV_OK, no launch,
 * nothing written. */
typedef struct dv_effect_desc {
    const float* a;
    int64_t lda;
    const float* b;
    int64_t ldb;
    int32_t mode;                 /* 0: log2(b + c) - log2(a + c); 1: b - a */
    float delta, pseudo;
    double* out;                  /* (row_blocks, n_grp, 7, X) */
    int32_t row_blocks, n_grp;
    const int32_t* grp;
} dv_effect_desc;
typedef struct dv_draw_desc {
    int32_t kind, M, X, S;        /* DV_RECON_*; rows, genes, samples */
    const float* mu;
    int64_t ldm;
    const float* sd;
    int64_t lds;
    const float* theta;
    int64_t ldt;
    const float* logit;
    int64_t ldl;
    const float* size;
    float* out;
    int64_t ldo, sso;             /* row stride, sample stride */
    int64_t row0;
    const int32_t* grow;
    int32_t k0;                   /* the sample index of out's first sample */
    const dv_effect_desc* fx;     /* trailing: THE EFFECT REDUCTION above (NULL: the sampler as it was) */
} dv_draw_desc;
int dv_fill_normal(float* out, int64_t n, uint64_t seed, const int32_t* ctr_dev, dv_stream_t stream,
                   const dv_draw_desc* draw);
/* Row-keyed form for the train step's noise arena (SURVEY.md 8(e) "RNG under DP": results must not depend
 * on the number of ranks).  desc = n_rows x {offset into arena (floats), width, draw id, GLOBAL minibatch
 * row} (int32 x 4, 16-B aligned); element (row, col) = Philox(key = seed (^ ctr_dev[1] in the high word),
 * counter = (col/4, global row, draw id, ctr_dev[0]))[col % 4] through Box-Muller.  ctr_dev counts draw
 * EVENTS (one per train step: advance it by 1), so every rank holds the same value; a rank that owns rows
 * [rB, (r+1)B) of the global minibatch draws exactly the values a single process would draw for them.  n_rows == 0: no launch. */
int dv_fill_normal_rows(float* arena, const int32_t* desc, int32_t n_rows, uint64_t seed, const int32_t* ctr_dev,
                        const dv_wait* park, dv_stream_t stream);
/* The noise arena of a step with hidden-layer dropout: `table` = n_rows descriptor rows as above that END in KEEP rows, and one
 * more row behind them, the trailer {n_keep, keep_thr (the uint32's bits), 0, 0}: how many, counted from the table's end (so
 * the table may be handed over from any row on).  The rows in front of the keep rows are written as dv_fill_normal_rows
 * writes them, bit for bit (another kernel).  Element (row, col) of a keep row is 1.0f if word col % 4 of Philox4x32-10(counter
 * = (col/4, global row, draw id, ctr_dev[0]), key = (seed_lo, seed_hi ^ ctr_dev[1])) -- counter and key laid out as for the
 * normals -- is < keep_thr (unsigned compare), else 0.0f.  keep_thr = floor((1 - dropout_rate) * 2^32) as uint32, computed by
 * the HOST in double: the keep probability is exactly keep_thr / 2^32, no float uniform is involved (tests/philox_ref.py
 * reproduces a mask exactly).  Same launch shape, same `park`; the counter is read behind the wait.  The trailer is DEVICE
 * memory: the host cannot validate it.  The kernel clamps n_keep to [0, n_rows]; a wrong count or threshold inside that range
 * draws rows of the wrong kind, it writes nothing outside the described elements. */
int dv_fill_noise_rows(float* arena, const int32_t* table, int32_t n_rows, uint64_t seed, const int32_t* ctr_dev,
                       const dv_wait* park, dv_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* DRVAE_HIP_H */
