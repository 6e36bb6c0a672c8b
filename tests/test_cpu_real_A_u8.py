"""real_A as a uint8 picture written inside the frame plan (opt.real_A_u8), checked without a device.

1. The restatement the GPU tests compare the kernel with (tests/real_A_u8_common.py: label map + instance map -> one-hot and edge
   planes -> first maximum -> palette) against the committed reference results of util.tensor2label, and on the one case where
   the edge plane decides the colour: a label the one-hot has no plane for, on and off an instance edge.
2. The lowering in the engine's record-only mode: with the option on a label plan records exactly one `label_image` and no
   `onehot_planar`, with the same convolutions; off again it is the plan taken before the option was ever set.
3. The option, the entry point's registration and its argument checks on host buffers."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import ROOT
from real_A_u8_common import edges, picture, picture_of_planes, planes_of, planted_maps
from test_cpu_stream_pool import _toy_model, _label_inputs, _raw_inputs, _recording, needs_cpu
from test_cpu_stream_pool import _ops as _all_ops

H, W = 32, 64


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("n", [35, 20, 12])
def test_restated_tensor2label_equals_the_reference_results(golden, n):
    """visual_util.npz holds util.tensor2label of n + 1 planes and of a single plane of stored ids, made by the reference."""
    g = golden("visual_util")
    cmap = g["lab%d.cmap" % n]
    got = picture_of_planes(torch.from_numpy(g["lab%d.x" % n]), n, cmap)
    assert np.array_equal(got.numpy(), g["lab%d.rgb" % n])
    got = picture_of_planes(torch.from_numpy(g["lab%d.ids" % n]), n, cmap)
    assert np.array_equal(got.numpy(), g["lab%d.ids_rgb" % n])


def test_restated_edges_equal_get_edges():
    from vid2vid_amd.models.base_model import BaseModel
    g = torch.Generator().manual_seed(1)
    inst = torch.randint(0, 3, (9, 13), generator=g)
    assert torch.equal(edges(inst).float(), BaseModel.get_edges(None, inst))
    assert not edges(torch.full((4, 5), 7)).any()


@pytest.mark.parametrize("label_nc", [35, 20, 7])
def test_labels_without_a_plane_take_the_edge_planes_colour(label_nc):
    """Pixel by pixel: a label inside the palette has its colour whatever the instance map says; a label >= label_nc is black on an
    instance edge (the edge plane, index label_nc, is the only maximum and has no colour) and cmap[0] off one and without an
    instance map (all planes equal: the first wins)."""
    from vid2vid_amd.visual import labelcolormap
    cmap = torch.from_numpy(labelcolormap(label_nc))
    lab, inst = planted_maps(1, 1, 9, 20, label_nc, seed=label_nc)
    lab, inst = lab[0, 0], inst[0, 0]
    e = edges(inst)
    outside = lab >= label_nc
    assert (outside & e).any() and (outside & ~e).any() and (~outside & e).any() and (~outside & ~e).any()
    assert outside[2, 3] and not e[2, 3] and outside[7, 18] and e[7, 18] and outside[0, 0]
    for maps, got in ((inst, picture(lab, inst, label_nc)), (None, picture(lab, None, label_nc)),
                      (inst.float(), picture(lab.float(), inst.float(), label_nc))):
        for y in range(9):
            for x in range(20):
                v = int(lab[y, x])
                want = cmap[v] if v < label_nc else (torch.zeros(3, dtype=torch.uint8) if maps is not None and e[y, x] else cmap[0])
                assert torch.equal(got[y, x], want), (y, x, v)
    planes = planes_of(lab, inst, label_nc)
    assert tuple(planes.shape) == (label_nc + 1, 9, 20) and torch.equal(planes[label_nc], e.float())
    assert torch.equal(planes[:label_nc].sum(0), (~outside).float())


def test_planted_maps_hold_every_byte_value_and_differ_between_frames():
    lab, inst = planted_maps(2, 3, 32, 64, 35, seed=3)
    assert lab.dtype == torch.uint8 and inst.dtype == torch.int32 and tuple(lab.shape) == (2, 3, 32, 64)
    for n in range(2):
        assert sorted(set(lab[n, 2].view(-1).tolist())) == list(range(256))
        assert not torch.equal(lab[n, 2], lab[n, 1]) and not torch.equal(inst[n, 2], inst[n, 1])
        assert not torch.equal(picture(lab[n, 2], inst[n, 2], 35), picture(lab[n, 1], inst[n, 1], 35))
    assert not torch.equal(inst[0], inst[1])


# ------------------------------------------------------------------ 2. the lowering
KINDS = {
    "plain_b1": (1, {}, {}),
    "plain_b2": (2, {}, {}),
    "generic_s2_b1": (1, dict(n_scales_spatial=2), {}),
    "slots": (3, {}, dict(active=[0, 2])),
    "pool_k1": (3, dict(compact_streams=True), dict(active=[1])),
    "pool_k2": (3, dict(compact_streams=True), dict(active=[0, 2])),
}


def _ops(fp):
    """The launch list without the weight packing, which the first plan a model records carries for all of them."""
    return [n for n in _all_ops(fp) if not n.endswith("pack_weights")]


def _flops(fp):
    return sum(c["flops"] for c in fp.conv_log)


@needs_cpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_label_plans_record_one_label_image_and_no_onehot_planar(kind):
    B, model_kw, call_kw = KINDS[kind]
    S = B
    with _recording():
        m = _toy_model(**model_kw)
        inputs = _label_inputs(B, H, W)
        fake_off, last_off = m.inference(*inputs, **call_kw)
        off = m._active_plan
        (key_off,) = m._plans
        before, flops = _ops(off), _flops(off)
        assert before.count("onehot_planar") == 1 and "label_image" not in before and "real_A_u8" not in key_off
        assert last_off.dtype == torch.float32 and tuple(last_off.shape) == ((36, H, W) if B == 1 else (B, 36, H, W))

        m.opt.real_A_u8 = True
        fake, pic = m.inference(*inputs, **call_kw)
        on = m._active_plan
        names = _ops(on)
        assert on is not off and on.real_A_u8 and not off.real_A_u8
        assert [k for k in m._plans if k != key_off] == [key_off + ("real_A_u8",)]
        assert names.count("label_image") == 1 and "onehot_planar" not in names
        # the launch stands where real_A_last stood: the two lists differ in that one name
        assert [("onehot_planar" if n == "label_image" else n) for n in names] == before
        assert _flops(on) == flops and len(on.conv_log) == len(off.conv_log)
        assert "real_A_last" not in on.out and on.out["real_A_image"].dtype == torch.uint8
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (S, H, W, 3) and pic.is_contiguous()
        assert tuple(on.out["real_A_image"].shape) == (S, H, W, 3) and pic.data_ptr() != on.out["real_A_image"].data_ptr()
        assert fake.dtype == torch.float32 and tuple(fake.shape) == tuple(fake_off.shape)
        assert m.fake_B_prev is on.prev

        m.opt.frames_u8 = True                       # both results as bytes: no fp32 tensor leaves the call
        image, pic = m.inference(*inputs, **call_kw)
        both = m._active_plan
        assert image.dtype == pic.dtype == torch.uint8 and tuple(image.shape) == tuple(pic.shape) == (S, H, W, 3)
        assert [k for k in m._plans if k[-1] == "real_A_u8" and "frames_u8" in k] == [key_off + ("frames_u8", "real_A_u8")]
        assert Counter(_ops(both)) == Counter(names) + Counter(["frames_u8"])
        assert [n for n in _ops(both) if n != "lane_wait"][-1] == "frames_u8"

        m.opt.real_A_u8 = m.opt.frames_u8 = False    # off again: the plan taken before the option was ever set
        _, last = m.inference(*inputs, **call_kw)
        assert m._active_plan is off and _ops(off) == before and last.dtype == torch.float32 and len(m._plans) == 3


@needs_cpu
def test_image_models_convert_the_planes_they_have():
    """label_nc == 0: no new kernel -- the frames_u8 launch without normalisation on the first plane(s) of real_A_last, behind
    a dense copy of them where several streams hold more planes than the picture takes."""
    for B, copies in ((1, 0), (2, 2)):
        with _recording():
            m = _toy_model(label_nc=0, input_nc=15, use_instance=False, fg=False)
            inputs = _raw_inputs(B)
            m.inference(*inputs)
            off = m._active_plan
            before = _ops(off)
            m.opt.real_A_u8 = True
            fake, pic = m.inference(*inputs)
            on = m._active_plan
            names = _ops(on)
            assert pic.dtype == torch.uint8 and tuple(pic.shape) == (B, 32, 32, 1) and fake.dtype == torch.float32
            assert "label_image" not in names and names.count("frames_u8") == 1
            assert Counter(names) == Counter(before) + Counter(["frames_u8"] + ["memcpy_d2d"] * copies)
            assert tuple(on.out["real_A_last"].shape) == tuple(off.out["real_A_last"].shape)      # the planes stay
    with _recording():
        m = _toy_model(label_nc=0, input_nc=3, use_instance=False, fg=False, real_A_u8=True, frames_u8=True)
        image, pic = m.inference(torch.rand(2, 3, 3, 32, 32), torch.zeros(2, 2, 3, 32, 32), None)
        assert tuple(pic.shape) == (2, 32, 32, 3) and tuple(image.shape) == (2, 32, 32, 3)
        assert _ops(m._active_plan).count("frames_u8") == 2


@needs_cpu
def test_calls_without_a_replay_return_zero_pictures():
    with _recording():
        m = _toy_model(real_A_u8=True)
        fake, pic = m.inference(*_label_inputs(1, H, W), active=[False])              # the B == 1 idle shortcut
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (1, H, W, 3) and not pic.any() and not m._plans
        assert fake.dtype == torch.float32 and tuple(fake.shape) == (1, 3, H, W)
    with _recording():
        m = _toy_model(real_A_u8=True, compact_streams=True)
        fake, pic = m.inference(*_label_inputs(3, H, W), active=[])                   # K == 0 in pool mode
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (3, H, W, 3) and not pic.any()
        assert not m._plans and m._active_plan is None and tuple(fake.shape) == (3, 3, H, W)
    with _recording():
        m = _toy_model(label_nc=0, input_nc=15, use_instance=False, fg=False, real_A_u8=True, compact_streams=True)
        _, pic = m.inference(*_raw_inputs(2), active=[False, False])
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (2, 32, 32, 1) and not pic.any()


@needs_cpu
def test_prepare_streams_builds_the_plans_of_the_option_as_it_is():
    with _recording():
        m = _toy_model(compact_streams=True, real_A_u8=True)
        m.prepare_streams(3, H, W, 1, True, counts=[1, 2])
        assert all(k[-1] == "real_A_u8" and k[-2] == ("pool", 3) for k in m._plans) and sorted(k[7] for k in m._plans) == [1, 2]
        built = dict(m._plans)
        _, pic = m.inference(*_label_inputs(3, H, W), active=[0, 2])
        assert m._plans == built and tuple(pic.shape) == (3, H, W, 3)
        assert tuple(m._active_plan.out["real_A_image"].shape) == (3, H, W, 3) and m._active_plan.B == 2


@needs_cpu
def test_engine_op_refuses_wrong_tensors():
    with _recording():
        m = _toy_model()
        eng = m.engine
        lab = torch.zeros(2, 3, 4, 8, dtype=torch.uint8)
        inst = torch.zeros(2, 3, 4, 8, dtype=torch.int32)
        words = torch.zeros(2, dtype=torch.int32)
        out = eng.label_image(lab, inst, 35, words, words, S=4)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 4, 8, 3)
        assert tuple(eng.label_image(lab.float(), None, 7).shape) == (2, 4, 8, 3)
        for bad in (lambda: eng.label_image(lab, inst.float(), 35), lambda: eng.label_image(lab[:, :, :, ::2], None, 35),
                    lambda: eng.label_image(lab, inst, 0), lambda: eng.label_image(lab, inst, 256),
                    lambda: eng.label_image(lab, inst, 35, words.long()), lambda: eng.label_image(lab[0], inst[0], 35),
                    lambda: eng.label_image(lab.to(torch.int16), None, 35)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(RuntimeError, match="K == S"):
            eng.label_image(lab, inst, 35, S=3)


# ------------------------------------------------------------------ 3. option and entry point
def test_option_defaults_off_and_the_entry_point_is_registered():
    from vid2vid_amd import lib as L
    from vid2vid_amd import options
    assert options._DEFAULTS["real_A_u8"] is False and options.make_opt().real_A_u8 is False
    assert options.make_opt(real_A_u8=True).real_A_u8 is True
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    args = re.search(r"\bint\s+v2v_label_image\s*\(([^)]*)\)", header).group(1).split(",")
    assert len(args) == len(L.PROTOTYPES["v2v_label_image"][1]) == 14
    assert "v2v_label_image" in L.exported_symbols()
    makefile = open(os.path.join(ROOT, "vid2vid_amd", "csrc", "Makefile")).read()
    assert "label_image.hip" in makefile and os.path.exists(os.path.join(ROOT, "vid2vid_amd", "csrc", "label_image.hip"))


def test_entry_point_refuses_bad_arguments_and_honours_dry_run():
    """Argument checks run before anything is submitted: host buffers stand in for device pointers."""
    from vid2vid_amd import lib as L
    K, S, T, Hh, Ww, nc = 2, 4, 3, 4, 6, 35
    n = K * T * Hh * Ww
    lab8, inst32 = (C.c_uint8 * n)(), (C.c_int32 * n)()
    labf, instf = (C.c_float * n)(), (C.c_float * n)()
    cmap = (C.c_uint8 * (3 * nc))()
    out = (C.c_uint8 * (S * Hh * Ww * 3))()
    words = (C.c_int32 * K)(3, 1)
    EINVAL = L.lib.v2v_tensor2im(None, None, 1, 1, 1, 1, None)
    assert EINVAL != 0

    def call(lab=lab8, inst=inst32, u8=1, cmap_=cmap, nc_=nc, out_=out, mode=words, rows=words, K_=K, S_=S, T_=T, H_=Hh, W_=Ww):
        return L.lib.v2v_label_image(lab, inst, u8, cmap_, nc_, out_, mode, rows, K_, S_, T_, H_, W_, None)

    def at(buf, off):
        return C.c_void_p(C.addressof(buf) + off)
    bad = [dict(lab=None), dict(cmap_=None), dict(out_=None), dict(nc_=0), dict(nc_=256), dict(nc_=-1), dict(u8=2), dict(K_=0),
           dict(S_=1), dict(S_=65536), dict(T_=0), dict(H_=0), dict(W_=0), dict(rows=None), dict(rows=None, mode=None),
           # misaligned: fp32 labels, either instance map, the words
           dict(lab=at(labf, 2), inst=instf, u8=0), dict(lab=labf, inst=at(instf, 1), u8=0), dict(inst=at(inst32, 2)),
           dict(mode=at(words, 1)), dict(rows=at(words, 2)),
           # out over an input: the labels' first and last byte, the instance map, the palette, the words
           dict(out_=at(lab8, 0)), dict(out_=at(lab8, n - 1)), dict(out_=at(inst32, 4 * n - 1)), dict(out_=at(cmap, 3 * nc - 1)),
           dict(out_=at(words, 4)), dict(lab=at(out, S * Hh * Ww * 3 - 1)), dict(cmap_=at(out, 5))]
    for kw in bad:
        assert call(**kw) == EINVAL and b"label_image" in L.lib.v2v_last_error(), kw
    with pytest.raises(RuntimeError, match="overlap"):
        L.check(call(out_=at(lab8, 8)), "label_image")
    prev = L.lib.v2v_set_dry_run(1)
    try:            # valid calls validate, submit nothing (a launch on host buffers would fault) and return 0
        assert call() == 0 and call(mode=None) == 0 and call(rows=None, K_=S, S_=S, T_=1) == 0 and call(inst=None) == 0
        assert call(lab=labf, inst=instf, u8=0) == 0 and call(lab=labf, inst=None, u8=0) == 0
        assert call(nc_=1) == 0 and call(nc_=255, cmap_=(C.c_uint8 * 765)()) == 0
        assert call(lab=at(lab8, 1), T_=2) == 0 and call(out_=at(out, 1), S_=3) == 0      # byte buffers need no alignment
        assert call(nc_=0) == EINVAL
    finally:
        L.lib.v2v_set_dry_run(prev)
    assert not any(out)
