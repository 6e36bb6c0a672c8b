"""Multi-stream inference, checked without a device: the lowering of a B = 2 frame plan in the engine's
record-only mode (every launch is argument-checked by the library, nothing executes), the unchanged B = 1 plan, and the
registration of the new entry points."""
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

NEW_SYMBOLS = ["v2v_conv_stats_rows_per_sample", "v2v_in_finalize_rows_workspace", "v2v_in_finalize_rows",
               "v2v_frame_prologue_batch", "v2v_onehot_conv7x7_batch", "v2v_warp_blend_roll_batch", "v2v_onehot_planar_batch"]


def _toy_model(**kw):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    d = dict(label_nc=35, use_instance=True, fg=True, use_real_img=True, random_init_ok=True, ngf=8, n_blocks=2, n_blocks_local=1,
             n_scales_spatial=1, n_downsample_G=2, loadSize=64, precision="fp32", gpu_ids=[])
    d.update(kw)
    return create_model(make_opt(**d))


def _ops(fp):
    from vid2vid_amd.lib import lib
    return [lib.v2v_plan_op_name(fp.plan.h, i).decode() for i in range(fp.plan.num_ops)]


def _inputs(B, H, W):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(0, 35, (B, 3, 1, H, W), generator=g).float(), torch.zeros(B, 2, 3, H, W),
            torch.randint(0, 20, (B, 3, 1, H, W), generator=g).float())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stream_label_plan_records_with_per_sample_norms(precision):
    from vid2vid_amd import networks as N
    if torch.cuda.is_available():
        pytest.skip("dry-run census is a CPU-host check")
    N.set_record_only(True)
    try:
        m = _toy_model(precision=precision)
        H, W = 32, 64
        fake, last = m.inference(*_inputs(2, H, W))
        assert tuple(fake.shape) == (2, 3, H, W) and tuple(last.shape) == (2, 36, H, W)
        assert [tuple(p.shape) for p in m.fake_B_prev] == [(2, 2, 3, H, W)]
        fp = m._active_plan
        names = [n for n in _ops(fp) if n != "lane_wait"]
        assert names.count("frame_prologue") == 1 and names[0] == "frame_prologue"        # ONE batched head
        assert not any(c.get("pair") or c.get("fused_norm") for c in fp.conv_log)         # no paired / fused-norm launch
        assert not any(n.startswith("bn_") for n in names), names                         # no batch-wide finalize / apply: no fin= conv
        normed = sum(1 for mod in m.netG0.modules() if isinstance(mod, (nn.BatchNorm2d, nn.InstanceNorm2d)))
        assert names.count("in_apply") == normed
        assert names.count("in_finalize_rows") + names.count("in_stats") == normed
        for i, n in enumerate(names):                    # conv -> finalize -> apply, back to back on the conv's lane
            if n == "in_apply":
                assert names[i - 1] in ("in_finalize_rows", "in_stats"), names[i - 3:i + 1]
                assert "conv" in names[i - 2], names[i - 3:i + 1]
        assert names.count("onehot_conv7x7") == 2 and "encode_labels" not in names        # both stems stay gather-sums on the codes
        assert names[-1] == "warp_blend" and "memcpy_d2d" not in names                    # the blend rolls the windows itself
        assert names.count("onehot_planar") == 1
        # changing B inside a sequence is an error, a restart is not
        with pytest.raises(ValueError, match="sequence"):
            m.inference(*_inputs(1, H, W))
        m.fake_B_prev = None
        fake1, last1 = m.inference(*_inputs(1, H, W))
        assert tuple(fake1.shape) == (1, 3, H, W) and tuple(last1.shape) == (36, H, W)
        assert m.engine.per_stream is False
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def test_fallback_plans_record_at_two_streams():
    """n_scales_spatial = 2 and the raw-input (label_nc = 0) model: batch-capable kernels, per-stream encodes and rolls."""
    from vid2vid_amd import networks as N
    if torch.cuda.is_available():
        pytest.skip("dry-run census is a CPU-host check")
    N.set_record_only(True)
    try:
        m = _toy_model(n_scales_spatial=2)
        fake, last = m.inference(*_inputs(2, 32, 64))
        assert tuple(fake.shape) == (2, 3, 32, 64) and tuple(last.shape) == (2, 36, 32, 64)
        assert [tuple(p.shape) for p in m.fake_B_prev] == [(2, 2, 3, 32, 64), (2, 2, 3, 16, 32)]
        names = _ops(m._active_plan)
        assert names.count("encode_labels") == 2 and not any(n.startswith("bn_") for n in names)
        N._ENGINES.clear()
        m = _toy_model(label_nc=0, input_nc=15, use_instance=False, fg=False)
        fake, last = m.inference(torch.rand(2, 3, 15, 32, 32), torch.zeros(2, 2, 3, 32, 32), None)
        assert tuple(fake.shape) == (2, 3, 32, 32) and tuple(last.shape) == (2, 15, 32, 32)
        assert not any(n.startswith("bn_") for n in _ops(m._active_plan))
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def test_single_stream_plan_is_the_pinned_one():
    """B = 1 takes none of the multi-stream lowering: the 512x256 bf16 frame still is the census the boundary tests pin
    (79 convolutions / 2115 GFLOP, 36 of them in 18 paired fused-norm launches), one prologue, and no per-sample launch."""
    from vid2vid_amd import networks as N
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    if torch.cuda.is_available():
        pytest.skip("dry-run census is a CPU-host check")
    N.set_record_only(True)
    try:
        opt = make_opt(label_nc=35, use_instance=True, fg=True, use_real_img=True, random_init_ok=True, precision="bf16", gpu_ids=[])
        m = create_model(opt)
        H, W = 256, 512
        fake, last = m.inference(*_inputs(1, H, W))
        assert tuple(fake.shape) == (1, 3, H, W) and tuple(last.shape) == (36, H, W)
        assert [tuple(p.shape) for p in m.fake_B_prev] == [(2, 3, H, W)]
        fp = m._active_plan
        assert fp.B == 1 and fp.labels.dim() == 3
        assert sum(c.get("convs", 1) for c in fp.conv_log) == 79 and abs(sum(c["flops"] for c in fp.conv_log) / 1e9 - 2115.0) < 0.5
        assert sum(1 for c in fp.conv_log if c.get("pair")) == 36 and sum(1 for c in fp.conv_log if c.get("fused_norm")) == 36
        names = _ops(fp)
        assert names.count("frame_prologue") == 1 and "memcpy_d2d" not in names
        assert not any(n.startswith("in_") for n in names)
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def test_new_entry_points_are_declared_and_registered():
    from vid2vid_amd import lib as L
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    declared = set(re.findall(r"\b(v2v_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in L.PROTOTYPES, name
        assert hasattr(L.lib, name)
    # every entry point the header declares has a prototype (a call without one would pass 64-bit arguments as ints)
    missing = sorted(n for n in declared if n not in L.PROTOTYPES and hasattr(L.lib, n))
    assert not missing, missing
