"""The measured tile search on the device against the CPU enumerator (vid2vid_amd/tile_search.py): what Engine._autotune /
_autotune_pair select is one of the listed candidates, its runners-up are listed candidates, and the selected configuration
computes what the library's default tile computes.  One search and one launch chain per shape; no timing assertion."""
import os
import sys

import pytest
import torch
import torch.nn as nn

from util import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# two tiles of one bf16 layer: the same products, fp32 sums in another order (tests/test_gpu_kernels.py, "vs the generic tile")
TILE_VS_TILE = 2e-5


@pytest.fixture(scope="module")
def rec():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import tile_search_record as R
    finally:
        sys.path.pop(0)
    return R


@pytest.fixture
def eng(monkeypatch):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine
    monkeypatch.delenv("V2V_TUNE_CACHE", raising=False)
    e = Engine(DEV, L.BF16)
    assert not e._tuned
    return e


def _check_search(cands, best, alts, wide):
    cands = [tuple(c) for c in cands]
    best, alts, wide = tuple(best), [tuple(c) for c in alts], [tuple(c) for c in wide]
    assert cands and best in cands, (best, cands)
    assert set(alts) <= set(cands) and set(wide) <= set(cands) and best not in alts + wide, (best, alts, wide)


# each at the smallest shape at which the enumerator lists the family under test (the fill thresholds prune it below): the
# single-phase / ping-pong 3x3 tiles, conv3x3_s2_kernel (64 output tiles), conv3x3_t2_kernel (48 input tiles), the 7x7 window
FORWARD = [
    ("c3_64to128", dict(H=64, W=128, cout=128), 80),
    ("c3_stride2", dict(H=128, W=128, cout=128, stride=2, pad_mode=0), 100),
    ("t3_stride2", dict(H=48, W=128, cin=128, cs=128, cout=64, transposed=1, stride=2, pad_mode=0), 110),
    ("c7_cs64_stem", dict(H=64, W=128, K=7, pad=3), 120),
]


@pytest.mark.parametrize("case", FORWARD, ids=[c[0] for c in FORWARD])
def test_autotune_selects_a_listed_candidate_that_computes_the_default_tiles_output(case, rec, eng):
    from vid2vid_amd import lib as L
    from vid2vid_amd import tile_search as TS
    name, delta, family_tile = case
    fields, stats, fin, spec = rec.fwd_fields(delta)
    conv = rec.make_module(spec)
    cands = TS.conv_candidates(rec.make_desc(fields, stats, fin, rec.HostMemory()), L.BF16, fields["cout"], conv, "fwd", eng.rowsum_heads)
    assert any(c[0] == family_tile for c in cands), "the shape must reach the family under test"
    torch.manual_seed(len(name))
    conv = conv.to(DEV)
    x = eng.pack(torch.randn(1, fields["cin"], fields["H"], fields["W"], device=DEV))
    args = (x, conv, fields["pad_mode"], fields["pad"], L.OUT_RAW_F32_NHWC)
    n = fields["OH"] * fields["OW"] * fields["cout_stride"]
    with torch.no_grad():
        base = eng.conv(*args, want_stats=True)[0][:n].clone()
        assert eng.conv_log[-1]["tune_key"] not in eng._tuned          # the library's default tile
        eng.autotune = True
        got = eng.conv(*args, want_stats=True)[0][:n].clone()
    key = eng.conv_log[-1]["tune_key"]
    best = eng._tuned[key]
    _check_search(cands, best, eng._tune_alts[key], eng._tune_wide[key])
    assert (eng.conv_log[-1]["tile"], eng.conv_log[-1]["splitk"]) == (best[0], best[1])
    assert_close(got, base, TILE_VS_TILE, "%s: %s vs the default tile" % (name, best))


def test_autotune_pair_selects_a_listed_candidate_that_computes_the_default_tiles_output(eng):
    from vid2vid_amd import lib as L
    from vid2vid_amd import tile_search as TS
    c, H, W = 128, 32, 64
    cands = TS.pair_candidates(1, H, W, c, c, L.BF16)
    torch.manual_seed(3)
    convs = [nn.Conv2d(c, c, 3, padding=0).to(DEV) for _ in range(2)]
    xs = [eng.pack(torch.randn(1, c, H, W, device=DEV)) for _ in range(2)]
    with torch.no_grad():
        base = [eng.conv(x, m, L.PAD_REFLECT, 1, L.OUT_RAW_F32_NHWC, want_stats=True)[0][:H * W * c].clone() for x, m in zip(xs, convs)]
        eng.autotune = True
        (ra, rb), _ = eng.conv_pair(xs[0], convs[0], xs[1], convs[1], L.PAD_REFLECT, 1, (None, None), ("a", "b"))
    key = eng.conv_log[-1]["tune_key"]
    best = eng._tuned[key]
    _check_search(cands, best, eng._tune_alts[key], eng._tune_wide[key])
    assert eng.conv_log[-1]["pair"] and eng.conv_log[-1]["tile"] == best[0]
    assert {(t, S, 0) for _, t, S in eng.pair_tune_log[key]} <= set(cands)
    for raw, want, which in ((ra[0], base[0], "a"), (rb[0], base[1], "b")):
        assert_close(raw[:H * W * c], want, TILE_VS_TILE, "pair member %s: %s vs the default tile" % (which, best))


def test_autotune_backward_data_selects_a_listed_candidate_that_computes_the_default_tiles_output(rec, eng):
    """Backward-data of a 3x3 / stride 1 Conv2d behind zero padding.  dX is stored in the activation dtype, where a sum in another
    order may round to the neighbouring bf16 value; so the operands are small integers and eighths (|dY| <= 3, |w| <= 1: every
    partial sum of the 128 x 9 products is a multiple of 1/8 below 2^12, exact in fp32): the order cannot matter and the two
    tiles must agree to the tolerance of two fp32 tiles."""
    from vid2vid_amd import lib as L
    from vid2vid_amd import autograd as AG
    from vid2vid_amd import tile_search as TS
    c, H, W = 128, 32, 64
    fields, reflect, spec = rec.bwd_fields(dict(H=H, W=W, kind="conv", cin=c, cout=c, K=3, stride=1, pad=1, reflect=False))
    conv = rec.make_module(spec)
    cands = TS.conv_candidates(rec.make_desc(fields, False, False, rec.HostMemory()), L.BF16, fields["cout"], conv, "bwd", eng.rowsum_heads)
    assert any(TS._flag(t, L.TILE_PAD2) for t, _, _ in cands), "the shape must reach the family under test"
    torch.manual_seed(5)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-8, 9, conv.weight.shape) / 8.0)
    conv = conv.to(DEV)
    x = torch.randn(1, c, H, W, device=DEV)
    r = torch.randint(-3, 4, (1, c, H, W), device=DEV).float()

    def dx():
        xg = x.clone().requires_grad_(True)
        y = eng.unpack(AG.conv_group(eng, eng.pack(xg), conv, L.PAD_ZERO, None, None, L.ACT_NONE, 0.0, None, None, False, 1.0, "t"))
        (y * r).sum().backward()
        return xg.grad

    base = dx()
    assert not eng._tuned                                              # the library's default tile
    eng.autotune = True
    got = dx()
    (key, best), = [(k, v) for k, v in eng._tuned.items() if k[0] == -1]
    _check_search(cands, best, eng._tune_alts[key], eng._tune_wide[key])
    assert float(base.abs().max()) > 1.0
    assert_close(got, base, TILE_VS_TILE, "backward-data: %s vs the default tile" % (best,))
