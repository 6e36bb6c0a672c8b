"""Which form of the label stem a launch takes (csrc/onehot_stem.hip, onehot_pick_ppt): two stacked tiles per workgroup where two
tile rows exist and the launch keeps at least 1024 workgroups (four per CU of the MI355X), one tile otherwise; V2V_ONEHOT_PPT=1|2 forces either.  Asked of
the library without a launch (v2v_onehot_conv_ppt), so no GPU is needed."""
import os

import pytest


def _form(N, H, W, cout, prec="bf16", slice_=0, T=3, nc=35, inst=1, env=None):
    from vid2vid_amd import lib as L
    old = os.environ.pop("V2V_ONEHOT_PPT", None)
    try:
        if env is not None:
            os.environ["V2V_ONEHOT_PPT"] = env
        return L.lib.v2v_onehot_conv_ppt(N, T, H, W, nc, inst, cout, L.BF16 if prec == "bf16" else L.F32, slice_)
    finally:
        os.environ.pop("V2V_ONEHOT_PPT", None)
        if old is not None:
            os.environ["V2V_ONEHOT_PPT"] = old


def test_flagship_stems_take_the_pair_form():
    # 512x256: 32 x 16 tiles -> 16 x 16 pairs x 4 slices = 1024 workgroups for 108 -> 128; the 108 -> 64 stem beside it would
    # have 512 and keeps one tile (measured alone: 93 us with one tile, 100 us paired)
    assert _form(1, 256, 512, 128) == 2
    assert _form(1, 256, 512, 64) == 1
    assert _form(1, 256, 512, 128, prec="fp32") == 2
    # 2048x1024 towers: 108 -> 32 and 108 -> 16 (one 16-channel slice)
    assert _form(1, 1024, 2048, 32) == 2
    assert _form(1, 1024, 2048, 16) == 2


@pytest.mark.parametrize("H,W,cout,N", [
    (8, 32, 128, 1),          # one tile row: nothing to pair
    (8, 4096, 128, 1),        # still one tile row, however wide
    (16, 32, 128, 1),         # one pair: 4 workgroups
    (64, 128, 16, 1),         # the smoke run's stem: 16 pairs
    (256, 512, 32, 1),        # 256 workgroups as pairs: below the threshold
    (256, 256, 64, 1),        # 8 x 16 pairs x 2 slices = 256
    (192, 384, 128, 1),       # 12 x 12 pairs x 4 slices = 576 (measured: 117 us with one tile, 124 us paired)
])
def test_small_launches_keep_one_tile(H, W, cout, N):
    assert _form(N, H, W, cout) == 1


def test_threshold_counts_pairs_slices_and_samples():
    assert _form(1, 128, 512, 128) == 1           # 8 pair rows x 16 x 4 slices = 512
    assert _form(2, 128, 512, 128) == 2           # x 2 samples = 1024
    assert _form(2, 256, 512, 64) == 2            # two streams of the 108 -> 64 stem: 16 x 16 x 2 x 2 = 1024
    assert _form(1, 264, 512, 128) == 2           # 33 tile rows -> 17 pair rows x 16 x 4 = 1088 (odd tile rows pair too)
    assert _form(1, 248, 512, 128) == 2           # 31 tile rows -> 16 pair rows x 16 x 4 = 1024
    assert _form(1, 240, 512, 128) == 1           # 30 tile rows -> 15 x 16 x 4 = 960


def test_switch_forces_either_form():
    assert _form(1, 256, 512, 128, env="1") == 1
    assert _form(1, 256, 512, 64, env="1") == 1
    assert _form(1, 8, 32, 128, env="2") == 2     # a lone half: the second one is masked
    assert _form(1, 64, 128, 16, env="2") == 2
    assert _form(2, 24, 40, 64, prec="fp32", T=2, env="2") == 2
    # anything else than 1 or 2 is not a switch
    assert _form(1, 256, 512, 128, env="0") == 2
    assert _form(1, 64, 128, 16, env="22") == 1
    assert _form(1, 64, 128, 16, env="") == 1


def test_64_channel_slices_have_the_one_tile_form_only():
    assert _form(1, 256, 512, 128, slice_=64) == 1
    assert _form(1, 256, 512, 128, slice_=64, env="2") == 1
    assert _form(1, 256, 512, 128, slice_=32) == 2


def test_unsupported_arguments_are_refused():
    assert _form(1, 256, 512, 129) < 0            # cout <= 128
    assert _form(1, 3, 512, 128) < 0              # the 3-pixel mirror needs 4 rows
    assert _form(0, 256, 512, 128) < 0
    assert _form(1, 256, 512, 128, slice_=48) < 0
