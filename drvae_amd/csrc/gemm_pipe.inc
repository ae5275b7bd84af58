// Hand-pipelined main loop of the fp32-MFMA GEMM family (gfx950), included by gemm.hip inside its anonymous namespace.
//
// What it changes against gemm_body's compiler-scheduled [barrier -> fragment reads -> MFMA chain -> stage] loop:
//   * staging is LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction): no staging registers, no ds_write;
//     an S-deep ring of K tiles in LDS, S - 1 tiles in flight behind the one being multiplied, retired by COUNTED
//     s_waitcnt vmcnt(N) and a RAW s_barrier (one per K tile; a __syncthreads() would drain the DMA queue);
//   * the MFMA fragments are software-pipelined in register groups of four k-steps: the ds_reads of group q + 1 are
//     issued in front of the MFMAs of group q (two register sets), so a wave's matrix pipe never waits for LDS;
//   * k-contiguous operands live in LDS as unpadded [row][BK] images with the 16-B chunks XOR-swizzled (applied to
//     the per-lane SOURCE address of the DMA, which writes lane-linearly, and again on the ds_read_b128);
//     row-contiguous operands live as plain [k][row] images and are read T consecutive rows per lane
//     (ds_read_b64 / _b128 for T = 2 / 4): MFMA tile i of a wave then owns the rows {T*l + i} -- a permutation of the
//     wave's rows that only the epilogue's index map has to know -- instead of one scalar ds_read_b32 per element;
//     the k-contiguous images hold their rows in the matching order (the DMA's source address is per lane), so every
//     layout ends with T adjacent output columns per lane: 16-B stores.
// Preconditions (checked by the dispatcher, else the register-staged kernel runs): 16-B aligned operand rows, K % 4 == 0
// for k-contiguous operands, row-contiguous operands over-readable or a multiple of 4 wide, one A source, no k-scale.

template <int BM, int BN, int BK, int WM, int WN, int KS, int S, bool AKC, bool BKC>
struct PipeGeom {
    static constexpr int NW = WM * WN * KS, NT = 64 * NW;
    static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;      // 32x32 MFMA tiles per wave
    static constexpr int KW = BK / KS, KH = KW / 2, G = KH / 4;      // k per wave / per lane half; groups of 4 k-steps
    static constexpr int A_FL = BM * BK, B_FL = BN * BK, STAGE_FL = A_FL + B_FL;
    static constexpr int PA = A_FL / 256, PB = B_FL / 256, P = (PA + PB) / NW;   // 1-KiB pieces (per wave: P)
    static constexpr int CPR = BK / 4;                              // 16-B chunks per row of a k-contiguous image
    static constexpr int RED_FL = (KS > 1) ? KS * BM * (BN + 1) : 0;
    static constexpr int SMEM_FL = S * STAGE_FL > RED_FL ? S * STAGE_FL : RED_FL;
    static_assert(KH % 4 == 0 && G >= 1, "a lane half holds whole 16-B chunks of k");
    static_assert((PA + PB) % NW == 0 && P >= 1, "pieces divide over the waves");
    static_assert(CPR == 4 || CPR == 8 || CPR == 16, "BK = 16, 32 or 64");
    static_assert(TM == 1 || TM == 2 || TM == 4, "row-contiguous reads are 4, 8 or 16 B");
    static_assert(TN == 1 || TN == 2 || TN == 4, "row-contiguous reads are 4, 8 or 16 B");
    static_assert(AKC || (256 % BM == 0 && BM <= 256), "row-contiguous A: whole k lines per piece");
    static_assert(BKC || (256 % BN == 0 && BN <= 256), "row-contiguous B: whole k lines per piece");
    static_assert((S - 2) * P <= 63 && S >= 2, "vmcnt is a 6-bit counter");
};

// chunk swizzle of a k-contiguous image: chunk c of row r sits at chunk position c ^ pipe_sw(r)
template <int CPR>
__device__ __forceinline__ int pipe_sw(int row) {
    return (row / (16 / CPR)) & (CPR - 1);
}

template <int N>
__device__ __forceinline__ void pipe_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The K loop: on return acc[i][j] holds the wave's partial product (over its K share when KS > 1).
// row_of_line(l): global line (row of the k-contiguous matrix) staged as line l of the A / B tile, already clamped.
// ONES (dy^T x layout): with DV_FLAG_ONES_COL the 16-B chunk of B columns [N4, N4 + 4), N4 = N + DV_ONES_OFF(g), holds ones
// in every k line of every ring slot -- written once, up front, and left out of the DMA (the lanes that would fetch it
// sit the instruction out) -- so that accumulator column N4 comes out as sum_k A[k, m], the bias gradient.
template <int BM, int BN, int BK, int WM, int WN, int KS, int S, bool AKC, bool BKC, bool ONES = false, typename LineA,
          typename LineB>
__device__ __forceinline__ void pipe_loop(const dv_gemm_desc& g, float* smem, int m0, int n0, LineA a_line,
                                          LineB b_line, f32x16 (&acc)[BM / WM / 32][BN / WN / 32]) {
    using PG = PipeGeom<BM, BN, BK, WM, WN, KS, S, AKC, BKC>;
    constexpr int TM = PG::TM, TN = PG::TN, G = PG::G, P = PG::P, CPR = PG::CPR, NW = PG::NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int ks_id = wave / (WM * WN), wm = (wave % (WM * WN)) / WN, wn = wave % WN;

    // ---- this wave's DMA pieces: piece q = wave + i*NW of the stage's PA + PB pieces (A first).  A piece is addressed
    // as [wave-uniform 64-bit base of the operand at the K tile, in SGPRs] + [this lane's 32-bit byte offset, fixed for
    // the whole loop]: measured (tools/mfma_probe.hip), the 64-bit-per-lane address form of global_load_lds costs the
    // issuing SIMD so much more that a loop of this shape drops from 148 to 119 TFLOP/s.
    unsigned voff[P];              // byte offset of this lane's chunk from the operand's base at K tile 0
    int kofs[P];                   // k index (inside a K tile) of this lane's chunk
    bool live[P];                  // this lane takes part in the piece (false: its chunk is the ones column's)
    const bool ones_on = ONES && (g.flags & DV_FLAG_ONES_COL) != 0;
    const int n_ones = g.N + DV_ONES_OFF(g);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int q = wave + i * NW;
        const bool isA = q < PG::PA;
        const int pq = isA ? q : q - PG::PA;
        const bool kc = isA ? AKC : BKC;
        const int64_t ld = isA ? g.lda : g.ldb;
        live[i] = true;
        if (kc) {
            const int row_t = pq * (64 / CPR) + lane / CPR;          // row POSITION in the LDS image
            const int c = (lane % CPR) ^ pipe_sw<CPR>(row_t);
            // position w*T*32 + j*32 + l holds tile row w*T*32 + T*l + j: MFMA tile j of a wave owns the rows {T*l + j}
            // for k-contiguous operands too (the permutation is free here: the DMA source address is per lane), so the
            // epilogue has ONE index map and every layout stores T adjacent columns per lane
            const int T = isA ? TM : TN, wq = row_t / (T * 32), jq = (row_t / 32) % T, lq = row_t % 32;
            const int line = isA ? a_line(wq * T * 32 + T * lq + jq) : b_line(wq * T * 32 + T * lq + jq);
            kofs[i] = c * 4;
            voff[i] = (unsigned)(((int64_t)line * ld + c * 4) * 4);
        } else {
            const int R = isA ? BM : BN;
            const int line_t = pq * (256 / R) + lane / (R / 4), rc = lane % (R / 4);
            const int r0 = isA ? m0 : n0, lim = isA ? g.M : g.N;
            const int col = r0 + rc * 4 < lim ? r0 + rc * 4 : 0;   // a chunk wholly past the edge: any readable chunk
            kofs[i] = line_t;
            voff[i] = (unsigned)(((int64_t)line_t * ld + col) * 4);
            if (ONES && !isA) live[i] = !(ones_on && r0 + rc * 4 == n_ones);
        }
    }
    const int64_t step_a = (AKC ? (int64_t)BK : (int64_t)BK * g.lda) * 4, step_b = (BKC ? (int64_t)BK : (int64_t)BK * g.ldb) * 4;
    const char* base_a = reinterpret_cast<const char*>(g.A);       // operand bases at the next K tile to issue
    const char* base_b = reinterpret_cast<const char*>(g.B);
    int k_issued = 0;             // first k of the next K tile to issue
    // The DMA is issued from an asm statement ON PURPOSE: hipcc orders every LDS read behind ALL outstanding LDS-DMA
    // it knows of (s_waitcnt vmcnt(0) in front of each group of ds_reads), which would serialise the ring; hidden
    // here, the only waits are the counted ones of this file.  M0 (the LDS destination base) is written in the same
    // statement that uses it.  FULL: the K tile is wholly inside K (every tile of the steady state); otherwise (the
    // ragged last tile, and the ring's tiles past K that keep the counted waits uniform) the chunks at k >= K read a
    // block of zeros through the per-lane address form.
    const unsigned lds0 = (unsigned)(uintptr_t)smem;      // LDS byte address of the ring (escapes: the asm writes it)
    auto issue_piece = [&](auto full, int i, unsigned stage_byte) {
        const int q = wave + i * NW;
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + stage_byte + q * 1024);
        const char* base = q < PG::PA ? base_a : base_b;
        if (DV_DBG & 16) return;       // knock-out (tuning builds): no staging behind the prologue
        if constexpr (decltype(full)::value) {
            if (!ONES || live[i])
                asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" ::"v"(voff[i]), "s"(dst), "s"(base) : "memory");
        } else if (!ONES || live[i]) {
            const char* p = kofs[i] < g.K - k_issued ? base + voff[i] : reinterpret_cast<const char*>(dv_zero_chunk);
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(p), "s"(dst) : "memory");
        }
    };
    auto issued = [&]() {          // all pieces of a K tile are out: on to the next one
        base_a += step_a;
        base_b += step_b;
        k_issued += BK;
    };
    // ---- fragment reads of group gi (4 k-steps) of a stage
    const int kb = ks_id * PG::KW + lh * PG::KH;          // this lane's first k inside a K tile
    const int swl = pipe_sw<CPR>(li);
    // a group's reads as a list of single ds_read instructions [0, NR): A's first (TM x b128 along k, or four reads of TM
    // adjacent rows), then B's; read_ops(lo, hi) issues the slice -- the tile loop deals them out between the MFMAs (six
    // ds_read_b128 back to back outlast the 64-cycle shadow of the MFMA in front of them: tools/mfma_probe.hip)
    constexpr int NRA = AKC ? TM : 4, NRB = BKC ? TN : 4, NR = NRA + NRB;
    auto read_ops = [&](const float* stage, int gi, float (&fa)[TM][4], float (&fb)[TN][4], int lo, int hi) {
        const float* sA = stage;
        const float* sB = stage + PG::A_FL;
        const int c = ((kb >> 2) + gi) ^ swl;
#pragma unroll
        for (int r = 0; r < NRA; ++r) {
            if (r < lo || r >= hi) continue;
            if constexpr (AKC) {
                const float4 v = *reinterpret_cast<const float4*>(&sA[(wm * TM * 32 + r * 32 + li) * BK + c * 4]);
                fa[r][0] = v.x; fa[r][1] = v.y; fa[r][2] = v.z; fa[r][3] = v.w;
            } else {
                const float* p = &sA[(kb + gi * 4 + r) * BM + wm * TM * 32 + TM * li];
                if constexpr (TM == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    fa[0][r] = v.x; fa[1][r] = v.y; fa[2][r] = v.z; fa[3][r] = v.w;
                } else if constexpr (TM == 2) {
                    const float2 v = *reinterpret_cast<const float2*>(p);
                    fa[0][r] = v.x; fa[1][r] = v.y;
                } else {
                    fa[0][r] = *p;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NRB; ++r) {
            if (NRA + r < lo || NRA + r >= hi) continue;
            if constexpr (BKC) {
                const float4 v = *reinterpret_cast<const float4*>(&sB[(wn * TN * 32 + r * 32 + li) * BK + c * 4]);
                fb[r][0] = v.x; fb[r][1] = v.y; fb[r][2] = v.z; fb[r][3] = v.w;
            } else {
                const float* p = &sB[(kb + gi * 4 + r) * BN + wn * TN * 32 + TN * li];
                if constexpr (TN == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    fb[0][r] = v.x; fb[1][r] = v.y; fb[2][r] = v.z; fb[3][r] = v.w;
                } else if constexpr (TN == 2) {
                    const float2 v = *reinterpret_cast<const float2*>(p);
                    fb[0][r] = v.x; fb[1][r] = v.y;
                } else {
                    fb[0][r] = *p;
                }
            }
        }
    };
    auto read_group = [&](const float* stage, int gi, float (&fa)[TM][4], float (&fb)[TN][4]) {
        read_ops(stage, gi, fa, fb, 0, NR);
    };
    // MFMAs [lo, hi) of a group's 4*TM*TN (k-step major, then the wave's tiles)
    auto mma = [&](const float (&fa)[TM][4], const float (&fb)[TN][4], int lo, int hi) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = (s * TM + i) * TN + j;
                    if (n >= lo && n < hi) {
                        if (DV_DBG & 32) {     // knock-out (tuning builds): no matrix work, the fragments stay live
                            acc[i][j][0] += fa[i][s] + fb[j][s];
                        } else {
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
                        }
                    }
                }
    };
    constexpr int NM = 4 * TM * TN;                       // MFMAs of a group
    // reads per MFMA gap and the gaps they take: never more slices than the group has MFMAs
    constexpr int RPM = (NR + NM - 1) / NM > 2 ? (NR + NM - 1) / NM : 2, NSL = (NR + RPM - 1) / RPM;
    static_assert(NSL <= NM, "reads dealt out over the group's MFMAs");
    const int nkt = (g.K + BK - 1) / BK;
    if constexpr (ONES) {
        if (ones_on && n0 <= n_ones && n_ones < n0 + BN && tid < S * BK)
            *reinterpret_cast<float4*>(&smem[(tid / BK) * PG::STAGE_FL + PG::A_FL + (tid % BK) * BN + (n_ones - n0)]) =
                make_float4(1.f, 1.f, 1.f, 1.f);
    }
    // prologue: S tiles in flight, the first one landed and visible
#pragma unroll
    for (int t = 0; t < S; ++t) {
        if (k_issued + BK <= g.K) {
#pragma unroll
            for (int i = 0; i < P; ++i) issue_piece(std::true_type{}, i, t * PG::STAGE_FL * 4);
        } else {
#pragma unroll
            for (int i = 0; i < P; ++i) issue_piece(std::false_type{}, i, t * PG::STAGE_FL * 4);
        }
        issued();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pipe_wait_vm<(S - 1) * P>();
    __builtin_amdgcn_s_barrier();
    float fa0[TM][4], fb0[TN][4], fa1[TM][4], fb1[TN][4];
    read_group(smem, 0, fa0, fb0);
    int sc = 0;                                  // ring slot of the tile being multiplied
    // one K tile, entered with its group 0 in (xa, xb); leaves the next tile's group 0 in (xa, xb) when G is even,
    // in (ya, yb) when G is odd.  __builtin_amdgcn_sched_barrier(0) pins the order written here: the fragment reads
    // of the next group behind this group's FIRST MFMA, the DMA pieces spread between the others (a piece costs the
    // issuing wave tens of cycles, an MFMA holds the matrix pipe for 64).  `full`: the tile issued here is wholly inside K
    auto tile = [&](auto full, float (&xa)[TM][4], float (&xb)[TN][4], float (&ya)[TM][4], float (&yb)[TN][4]) {
        const float* cur = smem + sc * PG::STAGE_FL;
        const int sn = sc + 1 == S ? 0 : sc + 1;
        const float* nxt = smem + sn * PG::STAGE_FL;
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            float(&ca)[TM][4] = (gi & 1) ? ya : xa;
            float(&cb)[TN][4] = (gi & 1) ? yb : xb;
            float(&na)[TM][4] = (gi & 1) ? xa : ya;
            float(&nb)[TN][4] = (gi & 1) ? xb : yb;
            if (gi + 1 < G) {
                // (the first MFMA in FRONT of the reads: hipcc waits lgkmcnt(0) for this group's fragments, which must
                // not include the reads issued here)
                // ... and dealt out RPM reads per MFMA
                mma(ca, cb, 0, 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NSL; ++q) {
                    read_ops(cur, gi + 1, na, nb, q * RPM, (q + 1) * RPM);
                    __builtin_amdgcn_sched_barrier(0);
                    if (q + 1 < NSL) {
                        mma(ca, cb, 1 + q, 2 + q);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                mma(ca, cb, NSL, NM);
                __builtin_amdgcn_sched_barrier(0);
            } else {
                // every fragment read of this tile has landed in registers (lgkmcnt(0)), this wave's pieces of the
                // next tile have landed (counted: the S - 2 tiles behind it stay in flight); behind the barrier that
                // holds for every wave: the next tile may be read, this tile's slot may be refilled
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                pipe_wait_vm<(S - 2) * P>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                mma(ca, cb, 0, 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NSL; ++q) {
                    read_ops(nxt, 0, na, nb, q * RPM, (q + 1) * RPM);
                    __builtin_amdgcn_sched_barrier(0);
                    if (q + 1 < NSL) {
                        mma(ca, cb, 1 + q, 2 + q);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                const unsigned sb = sc * PG::STAGE_FL * 4;
                // the DMA pieces share out the MFMAs that are left
                constexpr int M0 = NSL, ML = NM - M0;
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    mma(ca, cb, M0 + i * ML / (P + 1), M0 + (i + 1) * ML / (P + 1));
                    __builtin_amdgcn_sched_barrier(0);
                    issue_piece(full, i, sb);
                    __builtin_amdgcn_sched_barrier(0);
                }
                mma(ca, cb, M0 + P * ML / (P + 1), NM);
                __builtin_amdgcn_sched_barrier(0);
                issued();
            }
        }
        sc = sn;
    };
    // tile kt issues tile kt + S: the steady state runs while that one is a full tile
    const int nfast = g.K / BK - S;
    int kt = 0;
    if constexpr (G % 2 == 0) {
        for (; kt < nfast; ++kt) tile(std::true_type{}, fa0, fb0, fa1, fb1);
        for (; kt < nkt; ++kt) tile(std::false_type{}, fa0, fb0, fa1, fb1);
    } else {
        for (; kt + 1 < nfast; kt += 2) {
            tile(std::true_type{}, fa0, fb0, fa1, fb1);
            tile(std::true_type{}, fa1, fb1, fa0, fb0);
        }
        for (; kt + 1 < nkt; kt += 2) {
            tile(std::false_type{}, fa0, fb0, fa1, fb1);
            tile(std::false_type{}, fa1, fb1, fa0, fb0);
        }
        if (kt < nkt) tile(std::false_type{}, fa0, fb0, fa1, fb1);
    }
    // the ring's last S tiles (past K: zero chunks) are still in flight: nothing may land in LDS after this point
    pipe_wait_vm<0>();
}

// K loop of the paired-heads tile of 16 rows x (8 + 8) columns on v_mfma_f32_16x16x4_f32 (gemm_heads16_kernel): eight
// waves, wave w owns k = [8w, 8w + 8) of every 64 -- the k values, and the order inside the wave's fma chain (0, 4, 1, 5,
// 2, 6, 3, 7 of each eight, the 64-blocks ascending), of the 32-row tile's eight-wave K split on v_mfma_f32_32x32x2_f32:
// there lane half h feeds k = 4h + s to MFMA s = 0 .. 3, here lane group lg = lane / 16 feeds k = 4 (lg & 1) + (lg >> 1) + 2s
// to MFMA s = 0, 1, and the matrix core chains the four k of an instruction in lane-group order.  The accumulators carry
// the same bits.  Staging is the LDS-DMA ring of this file: a K tile of BK = 64 KB k is two unpadded k-contiguous images
// [16 lines][BK] (chunk c of line r at chunk position c ^ (r & 15)), BK / 8 pieces of 1 KiB, KB per wave; S slots.
template <int BK, int S>
struct Heads16Geom {
    static constexpr int BM = 16, BN = 16, KS = 8, NT = 64 * KS;
    static constexpr int KB = BK / 64, CPR = BK / 4;
    static constexpr int OP_FL = 16 * BK, STAGE_FL = 2 * OP_FL;
    static constexpr int PO = OP_FL / 256, P = 2 * PO / KS;          // 1-KiB pieces per operand / per wave and K tile
    static constexpr int RED_FL = KS * BM * (BN + 1);
    static constexpr int SMEM_FL = S * STAGE_FL > RED_FL ? S * STAGE_FL : RED_FL;
    static_assert(BK % 64 == 0 && P == KB && P >= 1, "whole 64-blocks of k; one piece per wave and block");
    static_assert((S - 2) * P <= 63 && S >= 2, "vmcnt is a 6-bit counter");
};

template <int BK, int S, typename LineA, typename LineB>
__device__ __forceinline__ void heads16_loop(const dv_gemm_desc& g, float* smem, LineA a_line, LineB b_line, f32x4& acc) {
    using HG = Heads16Geom<BK, S>;
    constexpr int P = HG::P, CPR = HG::CPR, KB = HG::KB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    // this wave's pieces: piece q = wave + 8 i of the stage's 2 PO (A's first); per lane the address of its chunk at K tile 0
    const float* src[P];
    int kofs[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int q = wave + i * HG::KS;
        const bool isA = q < HG::PO;
        const int pq = isA ? q : q - HG::PO;
        const int row_t = pq * (64 / CPR) + lane / CPR, c = (lane % CPR) ^ (row_t & 15);
        kofs[i] = c * 4;
        src[i] = isA ? g.A + (int64_t)a_line(row_t) * g.lda + c * 4 : g.B + (int64_t)b_line(row_t) * g.ldb + c * 4;
    }
    const unsigned lds0 = (unsigned)(uintptr_t)smem;
    int k_issued = 0;
    // (issued from an asm statement, M0 written in the same statement: see pipe_loop.  Chunks at k >= K read zeros)
    auto issue_tile = [&](int slot) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((slot * HG::STAGE_FL + (wave + i * HG::KS) * 256) * 4));
            const float* p = k_issued + kofs[i] < g.K ? src[i] + k_issued : dv_zero_chunk;
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(p), "s"(dst) : "memory");
        }
        k_issued += BK;
    };
#pragma unroll
    for (int t = 0; t < S; ++t) issue_tile(t);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pipe_wait_vm<(S - 1) * P>();
    __builtin_amdgcn_s_barrier();
    const int nkt = (g.K + BK - 1) / BK;
    const int e0 = lg >> 1;                                 // element of the wave's chunk (lg & 1) that MFMA 0 takes; MFMA 1: + 2
    int sc = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const float* sA = smem + sc * HG::STAGE_FL;
        const float* sB = sA + HG::OP_FL;
        float4 va[KB], vb[KB];
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            const int pos = ((b * 16 + 2 * wave + (lg & 1)) ^ li) * 4;
            va[b] = *reinterpret_cast<const float4*>(&sA[li * BK + pos]);
            vb[b] = *reinterpret_cast<const float4*>(&sB[li * BK + pos]);
        }
        // the fragments are in registers, this wave's pieces of the next tile have landed; behind the barrier both hold for
        // every wave: the slot is refilled (tiles past K: zeros, so that the counted wait stays uniform)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pipe_wait_vm<(S - 2) * P>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue_tile(sc);
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(e0 ? va[b].y : va[b].x, e0 ? vb[b].y : vb[b].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(e0 ? va[b].w : va[b].z, e0 ? vb[b].w : vb[b].z, acc, 0, 0, 0);
        }
        sc = sc + 1 == S ? 0 : sc + 1;
    }
    pipe_wait_vm<0>();       // (the ring's tiles past K are still in flight: nothing may land in LDS after this point)
}

// Register epilogue of the unsplit-K pipe tilings.  Index map (see the head of this file): tile-row rho of MFMA tile i is
// row TM*rho + i of the wave's rows, tile-column gamma of MFMA tile j is column TN*gamma + j -- in every layout.
template <int BM, int BN, int WM, int WN, bool AKC, bool BKC>
__device__ __forceinline__ void pipe_epilogue(const dv_gemm_desc& g, int m0, int n0,
                                              const f32x16 (&acc)[BM / WM / 32][BN / WN / 32]) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = (wave % (WM * WN)) / WN, wn = wave % WN;
    const int rw = m0 + wm * TM * 32, cw = n0 + wn * TN * 32;
    // plain product, whole tile inside the matrix, columns TN*li .. + TN - 1 of a lane adjacent: vector stores
    // (N a multiple of TN: a lane's column group is wholly inside or wholly outside the matrix)
    const bool vec_ok = TN > 1 && g.epilogue == DV_EPI_PLAIN && g.beta == 0.f && (g.N % TN) == 0 &&
                        (g.ldc % TN) == 0 && (reinterpret_cast<uintptr_t>(g.C) % (4 * TN)) == 0;
    if (vec_ok) {
        if (cw + TN * li >= g.N) return;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int row = rw + TM * rho + i;
                if (row < g.M) {
                    float* p = g.C + (int64_t)row * g.ldc + cw + TN * li;
                    if constexpr (TN == 4) {
                        *reinterpret_cast<float4*>(p) = make_float4(acc[i][0][r] * g.alpha, acc[i][1][r] * g.alpha,
                                                                    acc[i][2][r] * g.alpha, acc[i][3][r] * g.alpha);
                    } else {
                        *reinterpret_cast<float2*>(p) = make_float2(acc[i][0][r] * g.alpha, acc[i][TN - 1][r] * g.alpha);
                    }
                }
            }
        return;
    }
    // the fused epilogues (scale / bias / two-head activation / residual, activation backward, accumulate) on the same
    // 16-B column groups when the whole tile is inside N and every per-element operand is 16-B aligned: one float4 load
    // per operand and one float4 store per (row, 4 columns) instead of four scattered 4-B accesses.  ONE copy of the
    // code, the (tile row, accumulator register) pairs taken in a real loop (wave-uniform index: scalar branches)
    if constexpr (TN == 4) {
        auto al16 = [](const void* q, int64_t ld) { return q == nullptr || ((reinterpret_cast<uintptr_t>(q) & 15) == 0 && (ld & 3) == 0); };
        const bool fwd = g.epilogue == DV_EPI_FWD, bwd = g.epilogue == DV_EPI_BWD;
        const float* exsrc = fwd ? g.resid : (bwd ? g.yref : nullptr);
        const int64_t exld = fwd ? g.ldr : g.ldy;
        const bool use_ex = exsrc != nullptr, use_old = g.beta != 0.f;
        const bool vec4 = g.epilogue != DV_EPI_KLQ && (g.N & 3) == 0 && al16(g.C, g.ldc) && al16(exsrc, exld) && al16(g.scale, 0) && al16(g.bias, 0) &&
                          (!fwd || !use_ex || g.resid_cols >= (n0 + BN < g.N ? n0 + BN : g.N));
        if (vec4) {
            const int col = cw + 4 * li;
            if (col >= g.N) return;
            float sc[4] = {1.f, 1.f, 1.f, 1.f}, bi[4] = {0.f, 0.f, 0.f, 0.f};
            if (fwd && g.scale) {
                const float4 v = *reinterpret_cast<const float4*>(g.scale + col);
                sc[0] = v.x; sc[1] = v.y; sc[2] = v.z; sc[3] = v.w;
            }
            if (fwd && g.bias) {
                const float4 v = *reinterpret_cast<const float4*>(g.bias + col);
                bi[0] = v.x; bi[1] = v.y; bi[2] = v.z; bi[3] = v.w;
            }
            // the activation of a column depends on which side of `split` it is: wave-uniform unless the wave's 128 columns
            // straddle the split -- then it is chosen ONCE, outside the loops (a per-lane `switch` inside them is a ladder
            // of exec-mask branches per element: 18 us per 128 x 256 tile, as much as a quarter of a K = 600 product).
            // ACT: >= 0 the activation itself (the three the models use), -1 wave-uniform but a run-time value, -2 per lane
            const int cwu = __builtin_amdgcn_readfirstlane(cw);
            const bool uni = cwu + 128 <= g.split || cwu >= g.split;
            const int act_u = cwu < g.split ? g.act0 : g.act1;
            const float shift_u = cwu < g.split ? g.shift0 : g.shift1;
            auto body = [&](auto ACT) {
                constexpr int A = decltype(ACT)::value;
#pragma clang loop unroll(disable)
                for (int t = 0; t < TM * 4; ++t) {      // (MFMA tile row i, register quad rq): 4 rows x 4 columns per lane
                    float a16[4][4];
#pragma unroll
                    for (int n = 0; n < TM * 4; ++n)
                        if (t == n) {
#pragma unroll
                            for (int rl = 0; rl < 4; ++rl)
#pragma unroll
                                for (int j = 0; j < 4; ++j) a16[rl][j] = acc[n / 4][j][(n % 4) * 4 + rl];
                        }
                    const int i = t / 4, rq = t % 4;
                    float ex[4][4], old[4][4];
#pragma unroll
                    for (int rl = 0; rl < 4; ++rl) {          // every load of the step in front of its first store
                        const int row = rw + TM * (rl + 8 * rq + 4 * lh) + i, rc = row < g.M ? row : g.M - 1;
                        const float4 e = use_ex ? *reinterpret_cast<const float4*>(exsrc + (int64_t)rc * exld + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float4 c = use_old ? *reinterpret_cast<const float4*>(g.C + (int64_t)rc * g.ldc + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                        ex[rl][0] = e.x; ex[rl][1] = e.y; ex[rl][2] = e.z; ex[rl][3] = e.w;
                        old[rl][0] = c.x; old[rl][1] = c.y; old[rl][2] = c.z; old[rl][3] = c.w;
                    }
#pragma unroll
                    for (int rl = 0; rl < 4; ++rl) {
                        const int row = rw + TM * (rl + 8 * rq + 4 * lh) + i;
                        float o[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            int act;
                            float shift;
                            if constexpr (A == -2) {
                                const bool first = col + j < g.split;
                                act = first ? g.act0 : g.act1;
                                shift = first ? g.shift0 : g.shift1;
                            } else {
                                act = A >= 0 ? A : act_u;
                                shift = shift_u;
                            }
                            float v = a16[rl][j] * g.alpha;
                            if (fwd) {
                                v = dv_act(act, v * sc[j] + bi[j]) + shift;
                                if (use_ex) v += ex[rl][j];
                            } else if (bwd) {
                                v *= dv_dact_from_y(act, ex[rl][j] - shift);
                            }
                            if (use_old) v += g.beta * old[rl][j];
                            o[j] = v;
                        }
                        if (row < g.M) *reinterpret_cast<float4*>(g.C + (int64_t)row * g.ldc + col) = make_float4(o[0], o[1], o[2], o[3]);
                    }
                }
            };
            if (!uni) body(std::integral_constant<int, -2>{});
            else if (act_u == DV_ACT_IDENTITY) body(std::integral_constant<int, DV_ACT_IDENTITY>{});
            else if (act_u == DV_ACT_ELU) body(std::integral_constant<int, DV_ACT_ELU>{});
            else if (act_u == DV_ACT_SOFTPLUS) body(std::integral_constant<int, DV_ACT_SOFTPLUS>{});
            else body(std::integral_constant<int, -1>{});
            return;
        }
    }
    // every other case: ONE copy of the column epilogue's code, the wave's MFMA tiles taken in a real loop (the tile
    // index is wave-uniform: a scalar branch selects which accumulator is copied out)
#pragma clang loop unroll(disable)
    for (int t = 0; t < TM * TN; ++t) {
        float a16[16];
#pragma unroll
        for (int n = 0; n < TM * TN; ++n)
            if (t == n) {
#pragma unroll
                for (int r = 0; r < 16; ++r) a16[r] = acc[n / TN][n % TN][r];
            }
        const int i = t / TN, j = t % TN;
        const int col = cw + TN * li + j;
        epi_store_col<16, false>(g, a16, col, [rw, lh, i](int r) {
            const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
            return rw + TM * rho + i;
        });
    }
}

template <int BM, int BN, int BK, int WM, int WN, int S, bool AKC, bool BKC, int WGPC>
__global__ __launch_bounds__(64 * WM * WN, WGPC * WM * WN / 4) void gemm_pipe_kernel(const dv_gemm_desc g, const LoadCfg lc) {
    using PG = PipeGeom<BM, BN, BK, WM, WN, 1, S, AKC, BKC>;
    __shared__ __attribute__((aligned(1024))) float smem[PG::SMEM_FL];
    publish_on_entry(g);
    if (WGPC == 2 && lc.stagger > 0 && blockIdx.x >= 256 && blockIdx.x < 512) {
        // blocks b and b + 256 of the first dispatch round share a CU: the second one starts half a tile late, and the
        // phase shift stays (a slot is refilled when ITS tile ends) -- one workgroup's store epilogue and prologue run
        // under the other's K loop instead of both at the same time (plain epilogues: see pipe_stagger_ticks)
        const uint64_t t0 = wall_clock64();
        while (wall_clock64() - t0 < (uint64_t)lc.stagger) __builtin_amdgcn_s_sleep(64);
    }
    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = (g.N + BN - 1) / BN;
    int tm, tn;
    tile_of_block(blockIdx.x, gridDim.x, tiles_m, tiles_n, lc.map, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    f32x16 acc[PG::TM][PG::TN];
#pragma unroll
    for (int i = 0; i < PG::TM; ++i)
#pragma unroll
        for (int j = 0; j < PG::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    pipe_loop<BM, BN, BK, WM, WN, 1, S, AKC, BKC>(
        g, smem, m0, n0, [&](int l) { return m0 + l < g.M ? m0 + l : g.M - 1; },
        [&](int l) { return n0 + l < g.N ? n0 + l : g.N - 1; }, acc);
    pipe_epilogue<BM, BN, WM, WN, AKC, BKC>(g, m0, n0, acc);
}

// may this product run on the pipe family?  (see the preconditions at the head of this file)
inline bool pipe_ok(const dv_gemm_desc& g, const LoadCfg& lc) {
    if (g.A2 != nullptr || g.a_kscale != nullptr || lc.vecA != 4 || lc.vecB != 4) return false;
    if ((g.a_kcontig || g.b_kcontig) && (g.K & 3)) return false;
    if (!g.a_kcontig && (g.M & 3) && !(g.flags & 1)) return false;
    if (!g.b_kcontig && (g.N & 3) && !(g.flags & 2)) return false;
    // per-lane offsets from the operand bases are 32-bit byte offsets
    const int64_t ra = g.a_kcontig ? g.M : g.K, rb = g.b_kcontig ? g.N : g.K;
    if (ra * g.lda * 4 >= (int64_t(1) << 32) || rb * g.ldb * 4 >= (int64_t(1) << 32)) return false;
    return true;
}

template <int BM, int BN, int BK, int WM, int WN, int S, int WGPC>
int launch_pipe(const dv_gemm_desc& g, const LoadCfg& lc, hipStream_t st) {
    const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
    dim3 grid(tiles), block(64 * WM * WN);
    if (g.a_kcontig && g.b_kcontig)
        hipLaunchKernelGGL((gemm_pipe_kernel<BM, BN, BK, WM, WN, S, true, true, WGPC>), grid, block, 0, st, g, lc);
    else if (g.a_kcontig && !g.b_kcontig)
        hipLaunchKernelGGL((gemm_pipe_kernel<BM, BN, BK, WM, WN, S, true, false, WGPC>), grid, block, 0, st, g, lc);
    else if (!g.a_kcontig && !g.b_kcontig)
        hipLaunchKernelGGL((gemm_pipe_kernel<BM, BN, BK, WM, WN, S, false, false, WGPC>), grid, block, 0, st, g, lc);
    else
        return DV_ERR_UNSUPPORTED;
    DV_RETURN_LAUNCH();
}
