"""uint8 image inputs for label_nc == 0 models (opt.inputs_u8): what can be checked without a GPU -- the value
tables against an independent restatement of the reference loader's transforms, the option and the ABI, and the record-only
census of the plan's lowering."""
import os
import re
from collections import Counter

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _to_tensor_normalize(byte):
    """transforms.ToTensor then transforms.Normalize(0.5, 0.5) on one byte value, as torchvision computes them in fp32:
    byte -> float, / 255; then (v - mean) / std with mean = std = 0.5 as fp32 tensors."""
    v = torch.tensor([byte], dtype=torch.uint8).to(dtype=torch.float32).div(255)
    mean, std = torch.as_tensor([0.5], dtype=torch.float32), torch.as_tensor([0.5], dtype=torch.float32)
    return (v - mean) / std


def test_default_table_is_totensor_normalize():
    from vid2vid_amd import visual
    lut = visual.input_lut(15)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (15, 256) and lut.is_contiguous()
    want = torch.cat([_to_tensor_normalize(b) for b in range(256)])
    for c in range(15):
        assert torch.equal(lut[c], want), c
    assert float(lut[0, 0]) == -1.0 and float(lut[0, 255]) == 1.0


def test_part_channel_table_is_the_densepose_rescale():
    """data/pose_dataset.py:44 on the loaded channel: Di[2] = ((Di[2] * 0.5 + 0.5) * 255 / 24 - 0.5) / 0.5."""
    from vid2vid_amd import visual
    lut = visual.input_lut(6, densepose_part_channel=2)
    plain = torch.cat([_to_tensor_normalize(b) for b in range(256)])
    part = torch.cat([((_to_tensor_normalize(b) * 0.5 + 0.5) * 255 / 24 - 0.5) / 0.5 for b in range(256)])
    for c in range(6):
        assert torch.equal(lut[c], part if c == 2 else plain), c
    assert not torch.equal(part, plain) and abs(float(part[24]) - 1.0) < 1e-6          # part index 24 is the top of the range
    with pytest.raises(ValueError):
        visual.input_lut(3, densepose_part_channel=3)
    with pytest.raises(ValueError):
        visual.input_lut(0)


def test_decode_inputs_is_the_table_lookup():
    from vid2vid_amd import visual
    g = torch.Generator().manual_seed(3)
    lut = torch.randn(4, 256, generator=g)
    x = torch.randint(0, 256, (2, 3, 5, 7, 4), generator=g, dtype=torch.uint8)
    planes = visual.decode_inputs(x, lut)
    assert tuple(planes.shape) == (2, 3, 4, 5, 7) and planes.dtype == torch.float32
    for (n, t, y, xx, c) in ((0, 0, 0, 0, 0), (1, 2, 4, 6, 3), (0, 1, 2, 3, 1)):
        assert float(planes[n, t, c, y, xx]) == float(lut[c, int(x[n, t, y, xx, c])])


def test_option_defaults_and_abi():
    from vid2vid_amd import lib
    from vid2vid_amd.options import make_opt
    opt = make_opt()
    assert opt.inputs_u8 is False and opt.input_lut is None
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    assert re.search(r"\bint\s+v2v_image_prologue\s*\(", header)
    assert "v2v_image_prologue" in lib.exported_symbols()
    assert lib.lib.v2v_image_prologue.argtypes is not None and len(lib.lib.v2v_image_prologue.argtypes) == 19
    # the argument checks answer on the host: null pointers
    assert lib.lib.v2v_image_prologue(None, None, 1, None, 48, None, 1, 3, 8, 8, 15, None, 0, None, 0, None, 0, 1, None) != 0
    assert b"image_prologue" in lib.lib.v2v_last_error()


def _names(fp):
    from vid2vid_amd.lib import lib
    return Counter(lib.v2v_plan_op_name(fp.plan.h, i).decode() for i in range(fp.plan.num_ops))


def test_inputs_u8_lowering_census_edge2face_512():
    """Record (not run) the per-frame plans of the edge2face 512x512 model with fp32 and with uint8 inputs: the uint8 plan has one
    image_prologue, no pack, no unpack and no copy, and fewer launches; the fp32 plan is what it was (3434.4 GFLOP, its two
    packs, its unpack and the two roll copies)."""
    from vid2vid_amd import networks as N
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    if torch.cuda.is_available():
        pytest.skip("dry-run census is a CPU-host check")
    N.set_record_only(True)
    try:
        opt = make_opt(label_nc=0, input_nc=15, use_instance=False, fg=False, use_real_img=True, random_init_ok=True,
                       dataroot="datasets/face/", precision="bf16", gpu_ids=[])
        m = create_model(opt)
        H = W = 512
        first = torch.zeros(1, 2, 3, H, W)
        fake, last = m.inference(torch.rand(1, 3, 15, H, W), first, None)
        assert fake.shape == (1, 3, H, W) and last.shape == (15, H, W)
        fp32 = m._active_plan
        assert abs(sum(c["flops"] for c in fp32.conv_log) / 1e9 - 3434.4) < 1.0
        base = _names(fp32)
        assert base["pack_nchw_to_nhwc"] == 2 and base["unpack_nhwc_to_nchw"] == 1 and base["memcpy_d2d"] == 2
        assert base["image_prologue"] == 0 and fp32.win_u8 is None and tuple(fp32.raw_in.shape) == (1, 45, H, W)

        m.fake_B_prev = None
        opt.inputs_u8 = True
        frames = torch.randint(0, 256, (1, 3, H, W, 15), dtype=torch.uint8)
        fake, last = m.inference(frames, first, None)
        assert fake.shape == (1, 3, H, W) and last.shape == (15, H, W)
        u8 = m._active_plan
        assert u8 is not fp32 and u8.raw_in is None and tuple(u8.win_u8.shape) == (1, 3, H, W, 15)
        got = _names(u8)
        assert got["image_prologue"] == 1
        assert got["pack_nchw_to_nhwc"] == 0 and got["unpack_nhwc_to_nchw"] == 0 and got["memcpy_d2d"] == 0
        assert u8.plan.num_ops < fp32.plan.num_ops
        assert got["warp_blend"] == base["warp_blend"] == 1
        assert {k: v for k, v in got.items() if "conv" in k} == {k: v for k, v in base.items() if "conv" in k}
        assert abs(sum(c["flops"] for c in u8.conv_log) / 1e9 - 3434.4) < 1.0
        # the next call brings the newest frame alone, on the same plan
        m.inference(frames[:, 2:], None, None)
        assert m._active_plan is u8
        # the option off again: the fp32 plan, unchanged
        opt.inputs_u8 = False
        m.fake_B_prev = None
        m.inference(torch.rand(1, 3, 15, H, W), first, None)
        assert m._active_plan is fp32 and _names(fp32) == base
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def test_inputs_u8_refusals_on_the_host():
    from vid2vid_amd import networks as N
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    if torch.cuda.is_available():
        pytest.skip("dry-run check on a CPU host")
    N.set_record_only(True)
    try:
        opt = make_opt(label_nc=0, input_nc=6, use_instance=False, fg=False, use_real_img=True, random_init_ok=True,
                       precision="bf16", gpu_ids=[], ngf=8, n_blocks=2, n_downsample_G=2, inputs_u8=True)
        m = create_model(opt)
        H, W = 16, 32
        frames = torch.randint(0, 256, (1, 3, H, W, 6), dtype=torch.uint8)
        first = torch.zeros(1, 2, 3, H, W)
        for bad in (frames[:, 2:], frames[:, 1:], frames.float()):
            with pytest.raises(ValueError):
                m.inference(bad, first, None)
            assert getattr(m, "fake_B_prev", None) is None and m._active_plan is None
        with pytest.raises(ValueError):
            m.inference(frames, first, None, active=[0])
        opt.input_lut = torch.zeros(5, 256)
        with pytest.raises(ValueError):
            m.inference(frames, first, None)
        opt.input_lut = None
        m.inference(frames, first, None)
        assert m._active_plan.win_u8 is not None
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()
