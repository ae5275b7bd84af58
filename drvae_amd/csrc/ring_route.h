// How many slots the LDS-DMA ring of a latency-bound 32 x 32 K-split launch has (gemm_pipe.inc: S; S - 1 K tiles of 64 in
// flight behind the one being multiplied): plain host code, no device and no HIP header needed -- gemm.hip includes it, and
// tests/test_ring_route.py compiles it into a small program of its own.  The depth changes neither which wave owns which k
// nor the order of any sum: every depth stores the same bits.
#pragma once

enum {
    DV_RING_FAMILY_GEMM = 0,     // dv_gemm on the 32 x 32 x 64 K-split tiling (gemm_kpipe_kernel, four or eight waves)
    DV_RING_FAMILY_HEADS = 1,    // dv_gemm_heads on 32 x (16 + 16) tiles, eight waves (gemm_heads_pipe_kernel)
    DV_RING_FAMILY_PAIR = 2      // dv_gemm_pair, fused dW || dX on four waves (gemm_pair_pipe_kernel); K: the longer of the two
};

// dv_gemm_tune.opt[7] values the rule knows (include/drvae_hip.h); 0: by rule, 1: the four-wave K split for the k-contiguous
// layouts on the ring of two (as before)
#define DV_RING_OPT_FOUR_WAVE 1
#define DV_RING_OPT_DEPTH4 2      // four slots wherever the kernels of this file's families run
#define DV_RING_OPT_DEPTH3 3      // three slots wherever ...
#define DV_RING_OPT_FORBID 4      // two slots everywhere: the route of the builds before the deeper rings

// A ring slot is 16 KiB: three slots are 48 KiB of static LDS per workgroup, and three such workgroups fit a CU's 160 KiB
// (four slots: 64 KiB, two per CU).  A grid that is resident in one round with the ring of two must stay so with the deeper
// one on the smallest partition it usually runs on -- the side chain's 64 CUs -- so the rule deepens the ring up to 3 x 64
// workgroups only.
#define DV_RING_D3_MAX_TILES32 192

// From this many K tiles of 64 on the rule runs three slots.  Measured on MI355X on COLD operands (tools/gemm_cold_bench.py:
// every launch of the timed graph on its own copy of every operand, the copies together 68 MiB -- past twice the aggregate
// L2 --, min .. max in us over 15 replays in alternating rounds; profiles/r21_ring_depth.md holds every figure, the warm ones
// included).  A (shape class, depth) pair moves when every cold replay of the deeper ring lies below every cold replay of
// the ring of two.  Two / three / four slots:
//   plain product (x W^T, bias, ELU): 224 x 800 x 980, 175 workgroups, 16 K tiles: 11.63 .. 11.86 / 8.91 .. 9.14 / 9.01 .. 9.23:
//     moved.  596 x 600 x 100 and 450 x 200 x 104 (2 K tiles): 6.04 .. 6.13 / 6.21 .. 6.27 / 6.43 .. 6.47 and 4.65 .. 4.69 /
//     4.71 .. 4.74 / 4.82 .. 4.85: slower (the ring's tiles past K are issued all the same), stay.  Nothing in between was timed;
//     the threshold sits halfway in K tiles.
//   fused pair dW || dX, by the longer reduction: 596 rows, 600 -> 100 wide (10 K tiles, 152 workgroups): 9.75 .. 9.95 /
//     8.82 .. 8.89 / 8.95 .. 9.26: moved.  450 rows, 200 -> 104 and 200 -> 200 wide (8 K tiles, 88 and 154 workgroups): 8.39 .. 8.43 /
//     7.76 .. 7.83 / 7.98 .. 8.05 and 8.39 .. 8.45 / 7.83 .. 7.89 / 8.10 .. 8.14: moved.  300 rows, 200 -> 100 (5 K tiles, 60
//     workgroups): 6.81 .. 6.95 / 6.66 .. 6.81 / 6.90 .. 7.04: the ranges touch, stays.  224 rows, 200 -> 800 (4 K tiles, 357
//     workgroups): 8.20 .. 8.34 / 8.46 .. 8.59 / 8.94 .. 9.11: slower, stays.  The threshold is the shortest K that moved.
//   paired heads, sample mode: 450 x (100 + 100) x 200 (4 K tiles, 105 workgroups): 7.05 .. 7.09 / 6.90 .. 6.96 / 6.89 .. 6.96:
//     moved, by 0.1 us.  No other shape of the family was timed; shorter K stays (see the plain product's two K tiles).
// Four slots beat three nowhere, so the rule never hands them out; dv_gemm_tune.opt[7] = 2 still runs them.
#define DV_RING_MIN_KTILES_GEMM 8
#define DV_RING_MIN_KTILES_HEADS 4
#define DV_RING_MIN_KTILES_PAIR 8

// family: DV_RING_FAMILY_*; tiles32: workgroups of the launch (both products of a pair); K: the reduction length (the longer
// one of a pair); a_kcontig / b_kcontig: the layout (of a pair: its first product); opt7: dv_gemm_tune.opt[7].
// The chip-filling seven-per-CU kernels never come here: LDS caps their occupancy, depth would trade for it one for one.
static inline int dv_ring_depth(int family, int tiles32, int K, int a_kcontig, int b_kcontig, int opt7) {
    (void)a_kcontig;
    (void)b_kcontig;
    if (opt7 == DV_RING_OPT_DEPTH4) return 4;
    if (opt7 == DV_RING_OPT_DEPTH3) return 3;
    if (opt7 != 0) return 2;         // forbidden, or the four-wave split of before
    const int ktiles = (K + 63) / 64;
    const int min_kt = family == DV_RING_FAMILY_HEADS ? DV_RING_MIN_KTILES_HEADS
                                                      : (family == DV_RING_FAMILY_PAIR ? DV_RING_MIN_KTILES_PAIR : DV_RING_MIN_KTILES_GEMM);
    return ktiles >= min_kt && tiles32 <= DV_RING_D3_MAX_TILES32 ? 3 : 2;
}
