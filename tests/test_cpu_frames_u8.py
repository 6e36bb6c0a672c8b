"""uint8 frames from the frame plan, checked without a device: the lowering in the engine's record-only mode.  With
opt.frames_u8 off every plan kind records the launches and gets the cache key of a model that never heard of the option; with it
on the same list plus one `frames_u8` as the last launch, and inference returns uint8 (B,H,W,3).  Plus the registration of the
entry point, its argument checks and dry-run behaviour on host buffers."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from test_cpu_stream_pool import _toy_model, _ops, _label_inputs, _recording, needs_cpu

H, W = 32, 64
# plan kind -> (streams in the call, model options, arguments of the call)
KINDS = {
    "plain_b1": (1, {}, {}),
    "plain_b2": (2, {}, {}),
    "slots": (3, {}, dict(active=[0, 2])),
    "pool_k1": (3, dict(compact_streams=True), dict(active=[1])),
    "pool_k2": (3, dict(compact_streams=True), dict(active=[0, 2])),
}


def _call(kind, **opts):
    """(plan key, launch list, outputs, plan) of the first call of a fresh toy model."""
    B, model_kw, call_kw = KINDS[kind]
    kw = dict(model_kw)
    kw.update(opts)
    m = _toy_model(**kw)
    out = m.inference(*_label_inputs(B, H, W), **call_kw)
    (key, fp), = m._plans.items()
    assert fp is m._active_plan
    return key, _ops(fp), out, fp


@needs_cpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_option_off_is_the_plan_of_a_model_without_the_option(kind):
    with _recording():
        key_off, names_off, (fake, _), fp = _call(kind, frames_u8=False)
        assert "image" not in fp.out and not fp.frames_u8
    with _recording():
        B, model_kw, call_kw = KINDS[kind]
        m = _toy_model(**model_kw)
        del m.opt.frames_u8                          # an options object from before the option existed
        fake_old, _ = m.inference(*_label_inputs(B, H, W), **call_kw)
        (key_old, fp_old), = m._plans.items()
        names_old = _ops(fp_old)
    assert names_off == names_old and key_off == key_old
    assert "frames_u8" not in names_off and "frames_u8" not in key_off
    assert fake.dtype == fake_old.dtype == torch.float32 and tuple(fake.shape) == tuple(fake_old.shape) == (B, 3, H, W)


@needs_cpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_option_on_adds_one_launch_at_the_end(kind):
    with _recording():
        key_off, names_off, (_, last_off), _ = _call(kind, frames_u8=False)
    with _recording():
        key_on, names_on, (image, last), fp = _call(kind, frames_u8=True)
    B = KINDS[kind][0]
    assert key_on == key_off + ("frames_u8",)
    assert names_on.count("frames_u8") == 1
    rest = list(names_on)
    rest.remove("frames_u8")
    assert rest == names_off
    assert [n for n in names_on if n != "lane_wait"][-1] == "frames_u8"
    assert names_on.index("frames_u8") > names_on.index("onehot_planar")           # behind real_A_last too
    assert image.dtype == torch.uint8 and tuple(image.shape) == (B, H, W, 3)
    assert last.dtype == torch.float32 and tuple(last.shape) == tuple(last_off.shape)
    assert fp.frames_u8 and fp.out["image"].dtype == torch.uint8 and tuple(fp.out["image"].shape) == (B, H, W, 3)
    assert image.data_ptr() != fp.out["image"].data_ptr()                            # a fresh tensor, not the plan's buffer
    from vid2vid_amd.lib import lib
    i = names_on.index("frames_u8")
    assert lib.v2v_plan_op_lane(fp.plan.h, i) == 0                                   # the lane of the blend that wrote fake_B
    assert fp.out["fake_B"].shape[0] == fp.B                                         # dense rows in, S images out


@needs_cpu
def test_calls_without_a_replay_return_zero_images():
    with _recording():
        m = _toy_model(frames_u8=True)
        image, last = m.inference(*_label_inputs(1, H, W), active=[False])            # the B == 1 idle shortcut
        assert image.dtype == torch.uint8 and tuple(image.shape) == (1, H, W, 3) and not image.any()
        assert tuple(last.shape) == (36, H, W) and not m._plans
    with _recording():
        m = _toy_model(frames_u8=True, compact_streams=True)
        image, last = m.inference(*_label_inputs(3, H, W), active=[])                 # K == 0 in pool mode
        assert image.dtype == torch.uint8 and tuple(image.shape) == (3, H, W, 3) and not image.any()
        assert tuple(last.shape) == (3, 36, H, W) and not m._plans and m._active_plan is None


@needs_cpu
def test_option_is_read_per_call_and_flips_inside_running_sequences():
    with _recording():
        m = _toy_model()
        inp = _label_inputs(2, H, W)
        fake, _ = m.inference(*inp)
        off = m._active_plan
        assert fake.dtype == torch.float32
        m.opt.frames_u8 = True
        image, _ = m.inference(*inp)
        on = m._active_plan
        assert on is not off and on.frames_u8 and image.dtype == torch.uint8 and m.fake_B_prev is on.prev
        m.opt.frames_u8 = False
        fake, _ = m.inference(*inp)
        assert m._active_plan is off and fake.dtype == torch.float32 and len(m._plans) == 2
    with _recording():                               # the pool's windows belong to the model: both plans roll the same ones
        m = _toy_model(compact_streams=True)
        inp = _label_inputs(3, H, W)
        m.inference(*inp, active=[0, 2])
        windows = m.fake_B_prev
        m.opt.frames_u8 = True
        image, _ = m.inference(*inp, active=[0, 2])
        assert image.dtype == torch.uint8 and tuple(image.shape) == (3, H, W, 3)
        assert m.fake_B_prev is windows and m._active_plan.prev is windows and len(m._plans) == 2


@needs_cpu
def test_prepare_streams_builds_the_plans_of_the_option_as_it_is():
    with _recording():
        m = _toy_model(compact_streams=True, frames_u8=True)
        m.prepare_streams(3, H, W, 1, True, counts=[1, 2])
        assert all(k[-1] == "frames_u8" and k[-2] == ("pool", 3) for k in m._plans) and sorted(k[7] for k in m._plans) == [1, 2]
        built = dict(m._plans)
        m.inference(*_label_inputs(3, H, W), active=[0, 2])
        assert m._plans == built
        m.opt.frames_u8 = False
        m.prepare_streams(3, H, W, 1, True, counts=[2])
        assert len(m._plans) == 3 and sum(1 for k in m._plans if k[-1] == ("pool", 3)) == 1


def test_entry_point_is_declared_registered_and_the_option_defaults_off():
    from vid2vid_amd import lib as L
    from vid2vid_amd import options
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    declared = set(re.findall(r"\b(v2v_[a-z0-9_]+)\s*\(", header))
    assert "v2v_frames_u8" in declared and "v2v_frames_u8" in L.PROTOTYPES and hasattr(L.lib, "v2v_frames_u8")
    args = re.search(r"\bv2v_frames_u8\s*\(([^)]*)\)", header).group(1).split(",")
    assert len(args) == len(L.PROTOTYPES["v2v_frames_u8"][1]) == 11
    assert options._DEFAULTS["frames_u8"] is False and options.make_opt().frames_u8 is False
    from vid2vid_amd import visual
    assert callable(visual.tensor2im_batch)


def test_entry_point_refuses_bad_arguments_and_honours_dry_run():
    """Argument checks run before anything is submitted: host buffers stand in for device pointers."""
    from vid2vid_amd import lib as L
    K, S, Cc, Hh, Ww = 2, 4, 3, 4, 4
    frames = (C.c_float * (S * 4 * Hh * Ww))()
    out = (C.c_uint8 * (S * 4 * Hh * Ww))()
    words = (C.c_int32 * S)(3, 1, 0, 2)
    EINVAL = L.lib.v2v_tensor2im(None, None, 1, 1, 1, 1, None)
    assert EINVAL != 0

    def call(frames_=frames, out_=out, mode_=words, rows_=words, K_=K, S_=S, C_=Cc, H_=Hh, W_=Ww):
        return L.lib.v2v_frames_u8(frames_, out_, mode_, rows_, K_, S_, C_, H_, W_, 1, None)
    bad = [dict(frames_=None), dict(out_=None), dict(K_=0), dict(S_=1), dict(C_=0), dict(C_=5), dict(H_=0), dict(W_=0),
           dict(rows_=None), dict(rows_=None, mode_=None)]
    for kw in bad:
        assert call(**kw) == EINVAL and b"frames_u8" in L.lib.v2v_last_error(), kw
    # out inside frames: first byte, last byte, and frames inside out
    fbase, nbytes = C.addressof(frames), 4 * K * Cc * Hh * Ww
    for inside in (fbase, fbase + nbytes - 1, fbase - S * Cc * Hh * Ww + 1):
        assert call(out_=C.c_void_p(inside)) == EINVAL and b"overlap" in L.lib.v2v_last_error(), inside - fbase
    with pytest.raises(RuntimeError, match="overlap"):
        L.check(call(out_=C.c_void_p(fbase + 4)), "frames_u8")
    prev = L.lib.v2v_set_dry_run(1)
    try:            # valid calls validate, submit nothing (a launch on host buffers would fault) and return 0
        assert call() == 0 and call(mode_=None) == 0 and call(rows_=None, K_=S) == 0 and call(rows_=None, mode_=None, K_=S) == 0
        assert call(C_=1) == 0 and call(C_=4) == 0
        assert call(out_=C.c_void_p(fbase + nbytes)) == 0 and call(out_=C.c_void_p(fbase - S * Cc * Hh * Ww)) == 0      # adjacent
        assert call(K_=0) == EINVAL
    finally:
        L.lib.v2v_set_dry_run(prev)
    assert not any(out)
