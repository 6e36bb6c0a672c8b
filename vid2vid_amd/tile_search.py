"""Which conv tiles a launch may try: the tile-table views, the eligibility predicates and the candidate lists of the measured
search.  Policy only -- pure functions of (descriptor, dtype, module, environment), no torch.cuda and no Engine state, so "what
would the tuner try for this layer" has an answer on a CPU host.  Engine._autotune / _autotune_pair time what is listed here;
scripts/tile_search_record.py freezes the lists (tests/data/tile_search_candidates.json)."""
import os

import torch.nn as nn

from . import lib as L

# What a tile id is -- kernel family, geometry, weight packing, capabilities -- is written down once, in the library's tile table
# (csrc/conv_tiles.h, read through v2v_conv_tile_info); the names below are views of it.
_TILES = L.conv_tiles()


def _geom(pick):
    return {t: (r.th, r.tw, r.bn) for t, r in sorted(_TILES.items()) if pick(r)}


def _ids(pick):
    return tuple(t for t, r in sorted(_TILES.items()) if pick(r))


def _flag(t, bit):
    """Flag `bit` of tile id t; False for 0 (auto) and ids the library does not know (it refuses them)."""
    return t in _TILES and bool(_TILES[t].flags & bit)


# implicit-GEMM tiles: id -> (BM, BN, has a prefetch-helper instance)
TILE_CFGS = {t: (r.bm, r.bn, bool(r.flags & L.TILE_HELPER)) for t, r in sorted(_TILES.items()) if r.family == L.TILE_IGEMM}
# id -> (TH, TW, BN) of the tiles each search walks: the 3x3 / stride 1 families, stride 2, transposed stride 2, the 7x7 window
PATCH_CFGS = _geom(lambda r: r.family in (L.TILE_PATCH, L.TILE_PP, L.TILE_PP2, L.TILE_PP3, L.TILE_ONE) and not r.flags & L.TILE_ABLATION)
S2_CFGS = _geom(lambda r: r.family == L.TILE_S2)
T2_CFGS = _geom(lambda r: r.family in (L.TILE_T2, L.TILE_T2_ONE))
# (the 7x7 window tiles are offered to the tile search unless V2V_S7_PATCH=0)
S7_CFGS = _geom(lambda r: r.family == L.TILE_S7)
ABLATION_TILES = _geom(lambda r: r.flags & L.TILE_ABLATION)     # never auto-selected
# paired launches the engine searches: the library also pairs the ablation instances, the engine never offers them
PAIR_TILES = _ids(lambda r: r.flags & L.TILE_GROUPED and not r.flags & L.TILE_ABLATION)
# backward-data as a "full" (pad 2) 3x3 convolution: same rule
BWD_PATCH_TILES = _ids(lambda r: r.flags & L.TILE_PAD2 and not r.flags & L.TILE_ABLATION)
ONE_TILES = _ids(lambda r: r.family == L.TILE_ONE)
T2_ONE_TILES = _ids(lambda r: r.family == L.TILE_T2_ONE)
PERSISTENT_TILES = ONE_TILES + T2_ONE_TILES                     # ONE statistics row per workgroup, finalize in the launch at any size
ONE_FIN = os.environ.get("V2V_ONE_FIN", "1") != "0"             # ... finalize their <= 256 statistics rows in the launch (0: separate bn_finalize launch, for A/B)
EXP_TILES = _ids(lambda r: r.flags & L.TILE_EXPERIMENT)
if os.environ.get("V2V_EXP_TILES", "0") == "1":
    PAIR_TILES = PAIR_TILES + EXP_TILES
# families the frame-wide search treats as "ping-pong" (every LDS-patch schedule after the first patch kernel)
_PP_FAMILIES = (L.TILE_PP, L.TILE_PP2, L.TILE_PP3, L.TILE_S7, L.TILE_S2, L.TILE_T2, L.TILE_ONE, L.TILE_T2_ONE)

# ids the table has no flag for
HEAD_TILE, C8_TILE, ROWSUM_TILE = 60, 61, 62      # the 7x7 halo-patch kernels: conv7x7_head_kernel, conv7x7_c8_kernel (16-byte pixels), conv7x7_rowsum_kernel
IGEMM_NARROW_TILE = 4                             # the 128 x 32 implicit-GEMM tile: only for layers of <= 32 output channels
IGEMM_LARGE_FROM = 18                             # implicit-GEMM ids from here up have wave tiles >= 64x64: unsplit only where they fill the chip
PAIR_TILE_RAGGED, PAIR_TILE_W64 = 80, 83          # untuned paired launches: the 8 x 32 tile, the 4 x 64 one where the rows are whole 64-pixel tiles


def tile_korder(t):
    """Weight packing a tile id reads: 0 tap-major class matrices (implicit-GEMM tiles, 7x7 kernels), 1 channel-chunk-major (patch
    kernels, stride-2 patch kernel), 2 the full-tap chunk-major matrix of a transposed layer (conv3x3_t2_kernel)."""
    return _TILES[t].korder if t in _TILES else 0


def is_patch_tile(t):
    """Tile ids of the LDS-patch kernels that read channel-chunk-major (korder 1) weights."""
    return tile_korder(t) == 1


def _cfg3(v):
    """tile_override / _tuned values: tile id, or (tile, splitk, prefetch)."""
    return (int(v[0]), int(v[1]), int(v[2])) if isinstance(v, (tuple, list)) else (int(v), 1, 0)


# ---------------- eligibility: may this launch run on that kernel family? ----------------
def _bke(dtype):
    return 64 if dtype == L.BF16 else 32          # elements of one 128-byte K chunk


def _switch(name):
    return os.environ.get(name, "1") != "0"


def _is_conv(mod, k):
    return isinstance(mod, nn.Conv2d) and tuple(mod.kernel_size) == (k, k) and tuple(mod.stride) == (1, 1) and mod.groups == 1


def patch_eligible(d, dtype):
    return not d.transposed and d.KH == 3 and d.KW == 3 and d.stride == 1 and d.pad == 1 and d.cin_stride % _bke(dtype) == 0


def _pairx_layout(d, dtype):
    return (dtype == L.BF16 and d.KH == 3 and d.KW == 3 and d.pad == 1 and d.cin_stride == 32
            and d.out_mode in (L.OUT_RAW_F32_NHWC, L.OUT_RAW_ACT_NHWC) and d.W % 2 == 0 and (d.W // 2) % 32 == 0 and d.H % 8 == 0
            and _switch("V2V_PAIRX"))


def pairx_eligible(d, dtype):
    """Persistent single-chunk tiles 140 / 141 (/ 143) on a layer with 64-byte pixels (<= 32 -> 32 channels, bf16, raw fp32 output): the
    paired-x view (PairedXConv) -- pairs of pixels as one 128-byte pixel of a 64 -> 64 layer."""
    return not d.transposed and d.stride == 1 and d.cout == 32 and _pairx_layout(d, dtype)


def pairx_t_eligible(d, dtype):
    """Persistent transposed tile 114 on a layer with 64-byte pixels (<= 32 -> 16 channels): the paired-x view (PairedXConvT)."""
    return bool(d.transposed) and d.stride == 2 and d.cout == 16 and d.OH == 2 * d.H and d.OW == 2 * d.W and _pairx_layout(d, dtype)


def s7_eligible(d, dtype):
    """7x7-window tiles 120 / 121: dense bf16 7x7 / stride 1 / pad 3 Conv2d whose channel stride is a whole number of 128-byte chunks
    (the stems on the pooled label encodings, edge2face's 45 -> 128 stem; 1.1-1.7x there: profiles/r05_v1_stem7_bench.txt)."""
    return (dtype == L.BF16 and not d.transposed and d.KH == 7 and d.KW == 7 and d.stride == 1 and d.pad == 3
            and d.cin_stride % 64 == 0 and d.out_mode != L.OUT_NORM_ACT_NHWC and _switch("V2V_S7_PATCH"))


def s2_eligible(d, dtype):
    """conv3x3_s2_kernel: 3x3 / stride 2 / zero pad 1 Conv2d whose channel stride is a whole 128-byte chunk."""
    return (not d.transposed and d.KH == 3 and d.KW == 3 and d.stride == 2 and d.pad == 1 and d.pad_mode == L.PAD_ZERO
            and d.cin_stride % _bke(dtype) == 0 and d.out_mode != L.OUT_NORM_ACT_NHWC and _switch("V2V_S2_PATCH"))


def t2_eligible(d, dtype):
    """conv3x3_t2_kernel: ConvTranspose2d(3x3, stride 2, padding 1) whose channel stride is a whole 128-byte chunk."""
    return (bool(d.transposed) and d.KH == 3 and d.KW == 3 and d.stride == 2 and d.pad == 1
            and d.cin_stride % _bke(dtype) == 0 and d.out_mode != L.OUT_NORM_ACT_NHWC and _switch("V2V_T2_PATCH"))


def bwd_patch_eligible(d, dtype, mod):
    """Backward-data of a 3x3 / stride 1 Conv2d on the single-phase 3x3 tiles (round 6): the operator IS a 3x3 convolution of the
    output gradient with the role-swapped, tap-flipped weights (PackedConv korder 4) and pad 2 - p -- behind a ReflectionPad2d
    (p = 0) a "full" convolution onto the padded grid, which reflect_pad_fold then folds.  The generic tiles ran these at
    62 us for the 1024 -> 1024 layers (the forward, same FLOP, takes 44 on tile 90: profiles/r06_v17_train_by_grid.txt)."""
    return (_is_conv(mod, 3) and d.cin_stride % _bke(dtype) == 0 and d.out_mode == L.OUT_ACT_NHWC and _switch("V2V_BWD_PATCH"))


def bwd_c8_eligible(d, dtype, mod):
    """Backward-data of the 7x7 heads (ngf -> 3 behind ReflectionPad2d(3): models/networks.py:178-183) on conv7x7_c8_kernel
    (tile 61): the output gradient is ONE 16-byte vector per pixel, the operator a 7x7 convolution of it with the role-swapped,
    tap-flipped weights (PackedConv korder 5) and zero padding 6 - p.  The generic tiles walk it in 128-byte K chunks that are
    7/8 padding: 816 us per head at 2048x1024 (profiles/r06_v14_train_hires_by_grid.txt)."""
    vec = 8 if dtype == L.BF16 else 4
    return (_is_conv(mod, 7) and d.cin_stride == vec and mod.in_channels <= 128 and mod.in_channels % vec == 0
            and d.cout_stride % vec == 0 and d.out_mode == L.OUT_ACT_NHWC and _switch("V2V_BWD_C8"))


# ---------------- candidate lists ----------------
def _splits(tiles, splits, chunks, max_wgs=1024, min_tiles=64):
    """The fill rule.  Of the split-K factors `splits`, those a launch of `tiles` workgroups may try: unsplit only where it has
    min_tiles workgroups (fewer leave the chip idle), split S only within max_wgs workgroups and `chunks` K chunks (one per split)."""
    return [S for S in splits if (tiles >= min_tiles if S == 1 else tiles * S <= max_wgs and chunks >= S)]


def _grid(d, cout, geom, OH=None, OW=None):
    th, tw, bn = geom
    return d.N * -(-(d.OH if OH is None else OH) // th) * -(-(d.OW if OW is None else OW) // tw) * -(-cout // bn)


def conv_candidates(d, dtype, cout, mod=None, role="fwd", rowsum_heads=True):
    """[(tile, split-K, prefetch)] Engine._autotune times for descriptor `d` (role 'bwd': a backward-data operator of `mod`), in
    the order it times them.  (Prefetch-helper variants never won a sweep: not searched.)"""
    bf16 = dtype == L.BF16
    exp = os.environ.get("V2V_EXP_TILES", "0") == "1"
    ncc = d.cin_stride // _bke(dtype)
    cands = []
    def offer(t, tiles, splits=(1,), chunks=1, **rule):
        cands.extend((t, S, 0) for S in _splits(tiles, splits, chunks, **rule))

    M = d.N * (d.H * d.W if d.transposed else d.OH * d.OW)
    ncls = 4 if (d.transposed and d.stride == 2) else 1
    nk = (d.KH * d.KW * d.cin_stride * (2 if bf16 else 4)) // 128 // ncls
    for t, (bm, bn, _) in sorted(TILE_CFGS.items()):
        if t == IGEMM_NARROW_TILE and cout > 32:
            continue
        # (every split keeps four 128-byte K chunks; the large tiles cannot fill the chip without split-K)
        offer(t, -(-M // (bm * ncls)) * -(-cout // bn) * ncls, (1, 2, 3, 4, 6, 8), nk // 4, min_tiles=96 if t >= IGEMM_LARGE_FROM else 0)
    halo7 = (not d.transposed and d.KH == 7 and d.KW == 7 and d.stride == 1 and d.pad == 3 and not d.fin_counter
             and d.out_mode in (L.OUT_F32_NCHW, L.OUT_RAW_F32_NHWC))
    if halo7 and cout <= 32 and d.cin_stride % (32 if bf16 else 16) == 0:       # whole 64-byte half chunks (HC = 1)
        cands.append((HEAD_TILE, 1, 0))       # LDS patch + 16-wide MFMA
        if rowsum_heads and bf16 and cout <= 4 and d.out_mode == L.OUT_F32_NCHW and d.cin_stride % 32 == 0 and not d.stats:
            cands.append((ROWSUM_TILE, 1, 0))     # row GEMM + shifted sum
    if halo7 and cout <= 128 and d.cin_stride * (2 if bf16 else 4) == 16:
        cands.append((C8_TILE, 1, 0))         # 16-byte pixels (the 6-channel previous-frame stems), four taps per MFMA step
    if mod is None:
        return cands
    if role == "fwd" and patch_eligible(d, dtype):
        for t, geom in sorted(PATCH_CFGS.items()):        # (ragged tiles are legal, just wasteful; the timing decides)
            if t not in EXP_TILES or exp:
                offer(t, _grid(d, cout, geom), (1, 2, 3, 4, 8), ncc)
    if role == "bwd" and bwd_c8_eligible(d, dtype, mod):
        cands.append((C8_TILE, 1, 0))         # on the tap-flipped role-swapped weights (full convolution of the head's output gradient)
    if role == "bwd" and bwd_patch_eligible(d, dtype, mod):
        for t in BWD_PATCH_TILES:
            offer(t, _grid(d, cout, PATCH_CFGS[t]), (1, 2), ncc)
    paired_wgs = d.N * (d.H // 8) * (d.W // 64)           # workgroups of the persistent tiles in the paired-x view
    if role == "fwd" and pairx_eligible(d, dtype):
        for t in ONE_TILES:
            if t not in EXP_TILES or exp:
                offer(t, paired_wgs)
    if role == "fwd" and pairx_t_eligible(d, dtype):
        for t in T2_ONE_TILES:
            offer(t, paired_wgs, min_tiles=48)
    if role == "fwd" and s7_eligible(d, dtype):
        for t, geom in sorted(S7_CFGS.items()):
            if geom[2] <= 64 or cout > 64:
                offer(t, _grid(d, cout, geom))
    if s2_eligible(d, dtype):
        for t, geom in sorted(S2_CFGS.items()):
            offer(t, _grid(d, cout, geom))
    if t2_eligible(d, dtype):
        for t, geom in sorted(T2_CFGS.items()):           # (TH, TW): a tile of INPUT positions
            offer(t, _grid(d, cout, geom, (d.OH + 1) // 2, (d.OW + 1) // 2), min_tiles=48)
    return cands


def pair_candidates(N, H, W, cin_stride, cout, dtype):
    """[(tile, split-K, 0)] Engine._autotune_pair times for a paired 3x3 launch: every pair tile, unsplit and split 2 (a launch of two
    members: half the workgroup budget each, two K chunks per split)."""
    ncc, cands = cin_stride // _bke(dtype), []
    for t in PAIR_TILES:
        th, tw, bn = PATCH_CFGS[t]
        tiles = N * -(-H // th) * -(-W // tw) * -(-cout // bn)
        cands.extend((t, S, 0) for S in _splits(tiles, (1, 2), ncc // 2, max_wgs=512, min_tiles=0))
    return cands


def default_pair_tile(W):
    """Tile of a paired launch nobody measured."""
    return PAIR_TILE_RAGGED if W % 64 else PAIR_TILE_W64


def runners_up(timed, best):
    """(alts, wide) of an isolated search for the whole-frame search of the frame plan (models/vid2vid_model_G._FramePlan._frame_tune).
    timed: [(ms, cfg)] sorted; best: the configuration selected."""
    # the fastest few in isolation plus the fastest unsplit ones (split-K fills an idle chip; beside concurrent lanes it only adds slab traffic)
    unsplit = [cfg for _, cfg in timed if cfg[1] <= 1]
    pp_ = lambda t: _TILES[t].family in _PP_FAMILIES
    alts = ([cfg for _, cfg in timed[:3]] + unsplit[:3]
            + [cfg for _, cfg in timed if cfg[0] == best[0] and cfg[1] <= 2]          # the winner's tile, less split
            + [cfg for cfg in unsplit if pp_(cfg[0])][:1])                             # the best unsplit ping-pong tile
    alts = [c for i, c in enumerate(alts) if c != best and c not in alts[:i]][:7]
    # for the heaviest shapes of a frame the whole-frame search also walks every lightly split configuration that was not hopeless in isolation
    wide = ([cfg for ms, cfg in timed if pp_(cfg[0]) and cfg[1] <= 2 and cfg != best]      # every ping-pong tile
            + [cfg for ms, cfg in timed if not pp_(cfg[0]) and cfg[1] <= 2 and ms <= 1.7 * timed[0][0] and cfg != best][:10])
    return alts, wide
