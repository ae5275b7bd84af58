// Which kernel a paired-heads launch (dv_gemm_heads) runs on: plain host code, no device and no HIP header needed --
// gemm.hip includes it, and tests/test_heads_route.py compiles it into a small program of its own.
#pragma once

enum {
    DV_HEADS_ROUTE_KS8 = 0,      // 32 x (16 + 16) tiles, eight waves split each 64-deep K tile
    DV_HEADS_ROUTE_DENSE = 1,    // 32 x (16 + 16) tiles, four waves, seven workgroups per CU: the chip-filling grids
    DV_HEADS_ROUTE_T16 = 2       // 16 x (8 + 8) tiles on v_mfma_f32_16x16x4_f32, eight waves (sample mode, LDS-DMA ring)
};

// dv_gemm_tune.opt[4] values the rule knows (include/drvae_hip.h)
#define DV_HEADS_OPT_DENSE 3
#define DV_HEADS_OPT_T16 4
#define DV_HEADS_OPT_NO_T16 5

// From this K on a sample-mode launch whose 32-row tiles leave most of the chip idle moves to the 16-row tile (four times
// the workgroups, a quarter of the matrix work each), and up to this many 32-row tiles.  Measured on MI355X
// (`tools/heads_bench.py tiles`, min .. max over 15 replays each, profiles/r17_enc_heads.md): 224 x (100 + 100) x 800 -- 49
// tiles -- 7.90 .. 9.12 us on the 32-row tile, 6.30 .. 7.02 on the 16-row tile: moved.  300 x (100 + 100) x 100 -- 70 tiles --
// 5.01 .. 6.04 against 4.38 .. 5.08: the ranges overlap, stays.  450 x (100 + 100) x 200 -- 105 tiles -- 5.67 .. 6.71 against
// 5.89 .. 6.69: nothing, stays.  Both numbers sit between the shape that moved and the two that did not; the 16-row tile
// reads its operands from the L2 twice as often, which is what a short K or a larger grid does not pay back.
#define DV_HEADS_T16_MIN_K 512
#define DV_HEADS_T16_MAX_TILES32 64

// tiles32: workgroups of the 32-row tiling, ceil(M / 32) * ceil(split / 16); sample: DV_HEADS_SAMPLE; ring_ok: the operands
// allow the LDS-DMA ring (16-B aligned rows, K % 4 == 0) and it is not switched off; opt4: dv_gemm_tune.opt[4];
// dense_min: tiles from which the chip-filling route runs
static inline int dv_heads_route(int tiles32, int K, int sample, int ring_ok, int opt4, int dense_min) {
    if (opt4 == DV_HEADS_OPT_DENSE) return DV_HEADS_ROUTE_DENSE;
    const int t16_can = sample && ring_ok;     // (otherwise a forced 16-row tile falls back to the default rule)
    if (opt4 == DV_HEADS_OPT_T16 && t16_can) return DV_HEADS_ROUTE_T16;
    const int dflt = opt4 == 0 || opt4 == DV_HEADS_OPT_T16 || opt4 == DV_HEADS_OPT_NO_T16;
    if (dflt && tiles32 >= dense_min) return DV_HEADS_ROUTE_DENSE;
    if (opt4 == 0 && t16_can && K >= DV_HEADS_T16_MIN_K && tiles32 <= DV_HEADS_T16_MAX_TILES32) return DV_HEADS_ROUTE_T16;
    return DV_HEADS_ROUTE_KS8;
}
