"""The conv tile table (csrc/conv_tiles.h -> v2v_conv_tile_info -> vid2vid_amd.engine): the engine's views of it are frozen against the
literals they replaced, and what the library accepts, refuses and sizes per (tile id, descriptor) is frozen against a matrix recorded
before the table existed (tests/data/conv_tile_acceptance.json, scripts/conv_tile_acceptance.py).  No GPU: dry-run library."""
import ctypes as C
import json
import os
import sys

from conftest import ROOT

# ---- the module-level names of vid2vid_amd/engine.py as they were written out by hand before the table
TILE_CFGS = {1: (128, 128, False), 2: (128, 64, True), 3: (64, 64, True), 4: (128, 32, False), 5: (64, 128, True),
             6: (256, 64, False), 7: (128, 64, True), 8: (128, 128, False), 9: (64, 64, True), 10: (64, 64, False),
             11: (128, 64, True), 12: (64, 128, True), 13: (128, 64, True), 14: (128, 128, False),
             15: (128, 128, False), 16: (256, 64, False), 17: (64, 128, True), 18: (256, 128, False),
             19: (256, 128, False), 20: (128, 256, False), 21: (128, 128, False), 22: (256, 128, False),
             23: (128, 256, False)}
PATCH_CFGS = {32: (2, 64, 64), 33: (4, 64, 64), 34: (2, 64, 128), 35: (4, 32, 64), 36: (8, 32, 64), 37: (4, 32, 128),
              40: (2, 64, 64), 41: (4, 64, 64), 42: (2, 64, 128), 43: (4, 32, 64), 44: (8, 32, 64), 45: (4, 32, 128),
              46: (4, 64, 64), 47: (2, 64, 128), 48: (4, 64, 128),
              50: (4, 64, 128), 51: (4, 64, 64), 52: (2, 64, 128), 53: (8, 32, 128), 54: (8, 32, 64), 55: (4, 32, 128),
              56: (8, 32, 64), 57: (4, 64, 64),
              70: (8, 32, 64), 71: (8, 32, 128), 72: (8, 32, 64), 73: (4, 64, 64), 74: (4, 64, 64), 75: (4, 32, 128),
              80: (8, 32, 64), 81: (8, 32, 128), 82: (8, 32, 64), 83: (4, 64, 64), 84: (4, 32, 128), 85: (4, 64, 128),
              86: (4, 32, 128), 87: (2, 64, 128),
              90: (8, 32, 64), 91: (4, 64, 64),
              92: (8, 32, 64), 93: (4, 64, 64),
              94: (8, 32, 64), 95: (4, 64, 64), 96: (4, 32, 64),
              140: (8, 32, 64), 141: (8, 32, 64), 143: (8, 32, 64)}
S2_CFGS = {100: (4, 32, 64), 101: (4, 32, 128), 102: (4, 32, 64), 103: (4, 32, 128)}
T2_CFGS = {110: (4, 32, 64), 111: (4, 32, 128), 112: (8, 32, 64), 113: (4, 32, 64),
           114: (8, 32, 32)}
S7_CFGS = {120: (4, 32, 64), 121: (4, 32, 128)}
ABLATION_TILES = {78: (8, 32, 128), 79: (8, 32, 64), 88: (8, 32, 128), 89: (8, 32, 64)}
PAIR_TILES = (70, 71, 72, 73, 74, 75, 80, 81, 82, 83, 84, 85, 86, 87, 90, 91, 92, 93)
ONE_TILES = (140, 141, 143)
PERSISTENT_TILES = ONE_TILES + (114,)
EXP_TILES = (143,)
if os.environ.get("V2V_EXP_TILES", "0") == "1":
    PAIR_TILES = PAIR_TILES + EXP_TILES
BWD_PATCH_TILES = (80, 81, 82, 83, 84, 85, 86, 87, 90, 91, 92, 93)          # was a literal inside Engine._autotune


def _is_patch_tile(t):
    return 32 <= t < 60 or 70 <= t < 110 or 120 <= t < 150


def _tile_korder(t):
    return 2 if 110 <= t < 120 else 1 if _is_patch_tile(t) else 0


def _rows():
    from vid2vid_amd.lib import lib, ConvTileInfo
    rows = []
    for i in range(lib.v2v_conv_tile_count()):
        r = ConvTileInfo()
        assert lib.v2v_conv_tile_info(i, C.byref(r)) == 0
        rows.append(r)
    return rows


def test_engine_names_equal_the_literals_they_replaced():
    from vid2vid_amd import engine as E
    for name in ("TILE_CFGS", "PATCH_CFGS", "S2_CFGS", "T2_CFGS", "S7_CFGS", "ABLATION_TILES", "PAIR_TILES", "ONE_TILES",
                 "PERSISTENT_TILES", "EXP_TILES", "BWD_PATCH_TILES"):
        got, want = getattr(E, name), globals()[name]
        assert type(got) is type(want) and got == want, name
        if isinstance(want, dict):
            assert all(type(v) is tuple and [type(x) for x in v] == [type(x) for x in want[k]] for k, v in got.items()), name


def test_table_rows_are_unique_and_cover_every_listed_id():
    from vid2vid_amd.lib import lib, ConvTileInfo
    rows = _rows()
    ids = [r.id for r in rows]
    assert len(set(ids)) == len(ids) == lib.v2v_conv_tile_count() > 0
    listed = set(TILE_CFGS) | set(PATCH_CFGS) | set(S2_CFGS) | set(T2_CFGS) | set(S7_CFGS) | set(ABLATION_TILES) | {60, 61, 62}
    assert set(ids) == listed
    assert all(0 < t <= 150 for t in ids)                       # the acceptance matrix below sweeps 0 ... 150
    out = ConvTileInfo()
    assert lib.v2v_conv_tile_info(-1, C.byref(out)) != 0 and lib.v2v_conv_tile_info(len(rows), C.byref(out)) != 0
    assert lib.v2v_conv_tile_info(0, None) != 0


def test_patch_and_korder_lookups_equal_the_range_formulas():
    from vid2vid_amd.engine import is_patch_tile, tile_korder
    for r in _rows():
        assert bool(is_patch_tile(r.id)) == _is_patch_tile(r.id), r.id
        assert tile_korder(r.id) == _tile_korder(r.id) == r.korder, r.id
    for t in (0, -1, 24, 39, 97, 142, 150, 1000):               # auto and ids outside the table: the library refuses them, not the engine
        assert not is_patch_tile(t) and tile_korder(t) == 0, t


def test_acceptance_matrix_equals_the_recorded_one():
    """Every return code and number of v2v_conv_tile_config / _stats_rows / _splitk_workspace (+ tickets) / v2v_conv2d /
    v2v_conv2d_pair, tile ids 0 ... 150 x the generator's descriptors, against the matrix recorded from the build before the table."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import conv_tile_acceptance as A
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "data", "conv_tile_acceptance.json")) as f:
        want = json.load(f)
    got = A.compute()
    assert list(got) == list(want) == [name for name, _ in A.DESCRIPTORS] and len(got) >= 20
    bad = [(name, t, got[name][i], want[name][i]) for name in want for i, t in enumerate(A.TILE_IDS) if got[name][i] != want[name][i]]
    assert all(len(got[name]) == len(want[name]) == 151 for name in want)
    assert not bad, "%d combinations differ, first (descriptor, tile, got, recorded): %s" % (len(bad), bad[:5])
    # the matrix is worth something only if every family is accepted somewhere in it
    launched = {t for name in want for t, r in zip(A.TILE_IDS, want[name]) if r[4] == 0}
    assert launched == {0} | {r.id for r in _rows()}
