"""The conv tile search's policy (vid2vid_amd/tile_search.py) against the lists recorded from the code it was lifted out of
(tests/data/tile_search_candidates.json, scripts/tile_search_record.py): which configurations the tuner times, in which order, and
which runners-up it keeps.  CPU only; nothing is launched."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "tile_search_record.py")

# table ids no recorded list holds, with the reason.  (Every family is reached in dry-run: nothing is named here.)
UNREACHED = {}


@pytest.fixture(scope="module")
def rec():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import tile_search_record as R
    finally:
        sys.path.pop(0)
    return R


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "data", "tile_search_candidates.json")) as f:
        return json.load(f)


def _assert_same_candidates(got, want, which):
    assert list(got) == list(want), which
    for name in want:
        assert got[name]["cands"] == want[name]["cands"], (which, name)
        if "default" in got[name]:          # a pair row: the tile of an untuned launch is one the search offers
            assert got[name]["default"] in [c[0] for c in want[name]["cands"]], (which, name)


def test_candidate_lists_equal_the_recorded_ones(rec, recorded, monkeypatch):
    """(a) conv_candidates / pair_candidates == the first-pass sequence the parent's _autotune / _autotune_pair walked, order and
    duplicates included, for every row of the matrix -- in the default environment and with V2V_S2_PATCH=0 (read at call time)."""
    assert list(recorded) == list(rec.PASSES)
    names = [n for n, _ in rec.FWD + rec.BWD + rec.PAIRS]
    assert all(list(rows) == names for rows in recorded.values()) and len(names) >= 60
    for k in ("V2V_EXP_TILES", "V2V_S2_PATCH", "V2V_PAIRX", "V2V_S7_PATCH", "V2V_T2_PATCH", "V2V_BWD_PATCH", "V2V_BWD_C8", "V2V_HEAD_ROWSUM"):
        monkeypatch.delenv(k, raising=False)
    _assert_same_candidates(rec.compute_direct(), recorded["default"], "default")
    monkeypatch.setenv("V2V_S2_PATCH", "0")
    _assert_same_candidates(rec.compute_direct(), recorded["s2_patch_0"], "s2_patch_0")
    assert any(recorded["s2_patch_0"][n]["cands"] != recorded["default"][n]["cands"] for n in names)


def test_candidate_lists_with_experiment_tiles_equal_the_recorded_ones(rec, recorded):
    """(a), V2V_EXP_TILES=1: the views are built at import, so the enumerator runs in a child process."""
    env = dict(os.environ, **rec.PASSES["exp_tiles"])
    env.pop("V2V_S2_PATCH", None)
    out = subprocess.run([sys.executable, SCRIPT, "--mode", "direct", "--pass", "exp_tiles", "--print"], check=True, env=env,
                         stdout=subprocess.PIPE).stdout
    _assert_same_candidates(json.loads(out), recorded["exp_tiles"], "exp_tiles")
    assert any(c[0] == 143 for row in recorded["exp_tiles"].values() for c in row["cands"])
    assert not any(c[0] == 143 for row in recorded["default"].values() for c in row["cands"])


def test_runners_up_equal_the_recorded_ones(rec, recorded):
    """(b) runners_up on the hand-written times (scripts/tile_search_record.py, MS / SECOND_PASS) == the runner-up lists the
    parent's _autotune left for the same times, for every conv row of every pass."""
    from vid2vid_amd.tile_search import runners_up
    checked = 0
    for which, rows in recorded.items():
        for name, row in rows.items():
            if "wide" not in row:
                continue                    # pair rows: their runners-up are a plain sort inside _autotune_pair
            timed = rec.timed_of(row)
            if not timed:
                assert row["best"] == [0, 1, 0] and row["alts"] == row["wide"] == []
                continue
            assert row["reps"] == [3] and len(row["second_pass"]) == min(6, len(timed))
            alts, wide = runners_up(timed, tuple(row["best"]))
            assert [list(c) for c in alts] == row["alts"] and [list(c) for c in wide] == row["wide"], (which, name)
            assert tuple(row["best"]) not in alts + wide
            checked += 1
    assert checked >= 3 * 60
    # (the stubbed second pass does overturn first-pass leaders: `best` is an input of runners_up, not its fastest entry)
    assert any(tuple(row["best"]) != rec.timed_of(row)[0][1] for row in recorded["default"].values() if "wide" in row)


def test_candidates_are_table_rows_and_cover_the_table(recorded):
    """(c) every candidate's tile id is 0 or a row of the tile table; (d) across the matrix every id of the table that is neither an
    ablation nor an experiment instance appears in some list (the experiment ids: in the V2V_EXP_TILES=1 pass)."""
    from vid2vid_amd import lib as L
    table = L.conv_tiles()
    seen = {which: {c[0] for row in rows.values() for c in row["cands"]} for which, rows in recorded.items()}
    for which, ids in seen.items():
        assert ids <= {0} | set(table), which
    regular = {t for t, r in table.items() if not r.flags & (L.TILE_ABLATION | L.TILE_EXPERIMENT)}
    assert regular - seen["default"] == set(UNREACHED)
    assert not seen["default"] & {t for t, r in table.items() if r.flags & (L.TILE_ABLATION | L.TILE_EXPERIMENT)}
    assert {t for t, r in table.items() if r.flags & L.TILE_EXPERIMENT} <= seen["exp_tiles"]
    launched = {c[0] for rows in recorded.values() for row in rows.values() for c, ok in zip(row["cands"], row["ran"]) if ok}
    assert regular - launched == set(UNREACHED)          # ... and the dry-run library accepted each of them somewhere
