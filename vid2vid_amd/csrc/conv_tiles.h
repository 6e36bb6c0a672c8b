// The conv tile table: what every tile id of v2v_conv_desc.tile IS -- kernel family, tile geometry, the weight packing it reads and
// what it may be asked to do.  The ONE listing: build_conv / ConvOp::launch (conv_igemm.hip) dispatch and validate on a row, the
// launch_*_typed switches take their geometry template arguments from it (V2V_TILE_GEOM / V2V_TILE_BMBN), and the Python engine reads
// the rows through v2v_conv_tile_info (include/v2v_hip.h).  Adding or retiring a tile: one row here + its case in the family's switch.
// Host-side only: no kernel reads the table.
#pragma once
#include "../../include/v2v_hip.h"

namespace v2v {

struct ConvTile {
    int id;
    int family;          // V2V_TILE_FAMILY_*: the launcher ConvOp::launch picks and the validation block of build_conv
    int bm, bn;          // output pixels (transposed stride-2 tiles: input positions) x output channels of a workgroup's tile
    int th, tw;          // bm = th x tw pixels for every family but the implicit GEMM (0, 0: bm consecutive pixels of a class)
    int korder;          // v2v_conv_desc.w_korder the tile reads (paired-x layers hand the persistent tiles korder 3, see build_conv)
    int flags;           // V2V_TILE_*
};

namespace tiles {
constexpr int GRP = V2V_TILE_GROUPED, NORM = V2V_TILE_FUSED_NORM, PAD2 = V2V_TILE_PAD2, ONECH = V2V_TILE_SINGLE_CHUNK,
              PERS = V2V_TILE_PERSISTENT, HELP = V2V_TILE_HELPER, BF16 = V2V_TILE_BF16_ONLY, ABL = V2V_TILE_ABLATION,
              EXP = V2V_TILE_EXPERIMENT, FULLN = V2V_TILE_EXACT_BN;
constexpr ConvTile gemm(int id, int bm, int bn, int flags = 0) { return {id, V2V_TILE_FAMILY_IGEMM, bm, bn, 0, 0, 0, flags}; }
constexpr ConvTile px(int id, int family, int th, int tw, int bn, int korder, int flags = 0) { return {id, family, th * tw, bn, th, tw, korder, flags}; }
constexpr ConvTile patch(int id, int th, int tw, int bn, int flags = 0) { return px(id, V2V_TILE_FAMILY_PATCH, th, tw, bn, 1, flags); }
constexpr ConvTile pp(int id, int th, int tw, int bn) { return px(id, V2V_TILE_FAMILY_PP, th, tw, bn, 1); }
constexpr ConvTile pp2(int id, int th, int tw, int bn, int flags = 0) { return px(id, V2V_TILE_FAMILY_PP2, th, tw, bn, 1, GRP | flags); }
constexpr ConvTile pp3(int id, int th, int tw, int bn, int flags) { return px(id, V2V_TILE_FAMILY_PP3, th, tw, bn, 1, flags); }
constexpr int FULL3 = GRP | PAD2 | NORM;      // the regular single-phase tiles

inline constexpr ConvTile kConvTiles[] = {
    // ---- implicit GEMM (conv_igemm_kernel.h): any conv / transposed conv, BM x BN tiles, tap-major (korder 0) class matrices.
    //      HELP: the tile has an instance with the weight-prefetch helper wave (v2v_conv_desc.prefetch)
    gemm(1, 128, 128), gemm(2, 128, 64, HELP), gemm(3, 64, 64, HELP), gemm(4, 128, 32), gemm(5, 64, 128, HELP), gemm(6, 256, 64),
    gemm(7, 128, 64, HELP), gemm(8, 128, 128),                                                   // deeper LDS-DMA rings of 2 / 1
    gemm(9, 64, 64, HELP), gemm(10, 64, 64), gemm(11, 128, 64, HELP), gemm(12, 64, 128, HELP),   // occupancy / depth variants of 3, 2, 5
    gemm(13, 128, 64, HELP), gemm(14, 128, 128), gemm(15, 128, 128), gemm(16, 256, 64), gemm(17, 64, 128, HELP),     // 8-wave workgroups
    // wave tiles >= 64x64 (LDS-read efficient); meant to be combined with split-K on small-M layers
    gemm(18, 256, 128), gemm(19, 256, 128), gemm(20, 128, 256), gemm(21, 128, 128), gemm(22, 256, 128), gemm(23, 128, 256),
    // ---- LDS-resident-patch 3x3 kernel (conv3x3_patch_kernel.h): 3x3 / stride 1 / pad 1 Conv2d whose channel stride is a whole number of
    //      128-byte chunks, TH x TW output pixels x BN channels, weights channel-chunk major (korder 1) -- as every 3x3 family below
    patch(32, 2, 64, 64, HELP), patch(33, 4, 64, 64, HELP), patch(34, 2, 64, 128, HELP), patch(35, 4, 32, 64, HELP), patch(36, 8, 32, 64, HELP),
    patch(37, 4, 32, 128, HELP),
    // the same tiles with 2 dedicated loader waves; 46, 47: 8 compute waves (2 per SIMD) + 2 loader waves; 48: 256 x 128 tile
    patch(40, 2, 64, 64), patch(41, 4, 64, 64), patch(42, 2, 64, 128), patch(43, 4, 32, 64), patch(44, 8, 32, 64), patch(45, 4, 32, 128),
    patch(46, 4, 64, 64), patch(47, 2, 64, 128), patch(48, 4, 64, 128),
    // ---- ping-pong wave groups (conv3x3_pp_kernel.h)
    pp(50, 4, 64, 128), pp(51, 4, 64, 64), pp(52, 2, 64, 128), pp(53, 8, 32, 128), pp(54, 8, 32, 64), pp(55, 4, 32, 128), pp(56, 8, 32, 64),
    pp(57, 4, 64, 64),
    // ---- 7x7 heads and stems on halo patches (conv7x7_head_kernel.h), tap-major weights, all output channels in one tile (n_tiles = 1).
    //      60: <= 32 output channels, 8 x 32 pixels; 61: pixels of exactly 16 bytes (the 6-channel previous-frame stems, the heads'
    //      backward-data); 62: the generator heads as row GEMM + shifted sum, 10 x 32 pixels
    px(60, V2V_TILE_FAMILY_HEAD, 8, 32, 4, 0), px(61, V2V_TILE_FAMILY_C8, 8, 32, 4, 0), px(62, V2V_TILE_FAMILY_ROWSUM, 10, 32, 4, 0, BF16),
    // ---- ping-pong, second schedule: LDS-DMA issued between the MFMAs (conv3x3_pp2_kernel.h).  From here to 93: GRP, the tiles
    //      v2v_conv2d_pair launches as one grid of two members.  78 / 79: instrumented copies of 71 / 70 (scripts/pp2_ablate.py)
    pp2(70, 8, 32, 64), pp2(71, 8, 32, 128), pp2(72, 8, 32, 64), pp2(73, 4, 64, 64), pp2(74, 4, 64, 64), pp2(75, 4, 32, 128),
    pp2(78, 8, 32, 128, ABL), pp2(79, 8, 32, 64, ABL),
    // ---- single-phase software-pipelined schedule (conv3x3_pp3_kernel.h): two fragment register sets, ONE barrier per step.
    //      PAD2: also the "full" 3x3 convolution (zero pad 2: backward-data behind a ReflectionPad2d); NORM: V2V_OUT_NORM_ACT_NHWC
    pp3(80, 8, 32, 64, FULL3), pp3(81, 8, 32, 128, FULL3), pp3(82, 8, 32, 64, FULL3), pp3(83, 4, 64, 64, FULL3), pp3(84, 4, 32, 128, FULL3),
    pp3(85, 4, 64, 128, FULL3), pp3(86, 4, 32, 128, FULL3), pp3(87, 2, 64, 128, FULL3),     // 86 / 87: 4 waves (2 x 2), 64 x 64 wave tiles
    pp3(88, 8, 32, 128, GRP | PAD2 | ABL), pp3(89, 8, 32, 64, GRP | PAD2 | ABL),            // ablation instances of 81 / 80
    pp3(90, 8, 32, 64, FULL3), pp3(91, 4, 64, 64, FULL3),      // 82 / 83 with K pairs: 4 x 1 wave tiles of 64 x 64, two K halves (8 fragment reads per 8 MFMAs)
    pp3(92, 8, 32, 64, FULL3), pp3(93, 4, 64, 64, FULL3),      // K quads: 2 x 1 wave tiles of 128 x 64, four K quarters (6 reads per 8 MFMAs)
    // ONECH: single-chunk layers (64 bf16 input channels = one 128-byte chunk), one patch buffer, 3 weight stages (72 / 80 KiB), single
    // launches only; 96: FOUR waves (2 x 2, 64 x 32 wave tiles), 52 KiB: the tile that really puts two workgroups on a CU
    pp3(94, 8, 32, 64, ONECH | BF16), pp3(95, 4, 64, 64, ONECH | BF16), pp3(96, 4, 32, 64, ONECH | BF16),
    // (the round-5 experiment tiles 97-99 / 130-132 on tile 90's geometry and 142 -- all bit-identical to the tiles they varied, none
    //  faster, DESIGN 3.1 -- were removed in round 6; the FLAGS parameter of the body that built them stays)
    // ---- stride-2 3x3 convolutions on the plane-resident patch kernel (conv3x3_s2_kernel.h): (TH, TW) of the OUTPUT tile
    px(100, V2V_TILE_FAMILY_S2, 4, 32, 64, 1), px(101, V2V_TILE_FAMILY_S2, 4, 32, 128, 1), px(102, V2V_TILE_FAMILY_S2, 4, 32, 64, 1),
    px(103, V2V_TILE_FAMILY_S2, 4, 32, 128, 1),
    // ---- ConvTranspose2d(3x3, stride 2) with all four output-parity classes per workgroup (conv3x3_t2_kernel.h): (TH, TW) = tile of
    //      INPUT positions, the full-tap chunk-major matrix (korder 2).  114: persistent, weights resident, single chunk (64 input
    //      channels), <= 32 output channels (conv3x3_one_kernel.h, conv3x3_t2_one_kernel)
    px(110, V2V_TILE_FAMILY_T2, 4, 32, 64, 2), px(111, V2V_TILE_FAMILY_T2, 4, 32, 128, 2), px(112, V2V_TILE_FAMILY_T2, 8, 32, 64, 2),
    px(113, V2V_TILE_FAMILY_T2, 4, 32, 64, 2), px(114, V2V_TILE_FAMILY_T2_ONE, 8, 32, 32, 2, PERS | BF16),
    // ---- dense 7x7 / stride 1 / pad 3 on the single-phase kernel with a 7x7 window (conv3x3_pp3_kernel.h, KK = 7): 10 x 38 pixel patch
    px(120, V2V_TILE_FAMILY_S7, 4, 32, 64, 1, BF16), px(121, V2V_TILE_FAMILY_S7, 4, 32, 128, 1, BF16),
    // ---- conv3x3_one_kernel.h: PERSISTENT, weights-resident tile for single-chunk layers with <= 64 output channels (one workgroup per
    //      CU walks its tiles; no barrier / DMA / wait inside a tile's 9 steps).  140: bit-identical to tile 94 and 18-20 % faster; 141 (two
    //      patch buffers): another 5 % on the 2048-tile layer, 5-7 % slower on the small ones (profiles/r05_v6_stagger.txt) -- both are
    //      offered, the search decides per shape; 143: 141 with its stores left in flight (experiment; FULLN: exactly bn output channels)
    px(140, V2V_TILE_FAMILY_ONE, 8, 32, 64, 1, ONECH | PERS | BF16), px(141, V2V_TILE_FAMILY_ONE, 8, 32, 64, 1, ONECH | PERS | BF16),
    px(143, V2V_TILE_FAMILY_ONE, 8, 32, 64, 1, ONECH | PERS | BF16 | EXP | FULLN),
};
}  // namespace tiles
using tiles::kConvTiles;
inline constexpr int kNumConvTiles = sizeof(kConvTiles) / sizeof(kConvTiles[0]);

// row of a tile id, nullptr for an id the library cannot launch
constexpr const ConvTile* find_conv_tile(int id) {
    for (const ConvTile& t : kConvTiles)
        if (t.id == id) return &t;
    return nullptr;
}
// ... for an id known at compile time: a missing row does not compile (null dereference in a constant expression)
constexpr const ConvTile& conv_tile(int id) { return *find_conv_tile(id); }

// geometry template arguments of the launch_*_typed switches, straight from the row
#define V2V_TILE_GEOM(id) ::v2v::conv_tile(id).th, ::v2v::conv_tile(id).tw, ::v2v::conv_tile(id).bn
#define V2V_TILE_BMBN(id) ::v2v::conv_tile(id).bm, ::v2v::conv_tile(id).bn

}  // namespace v2v
