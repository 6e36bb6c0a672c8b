"""Stream slots, checked without a device: the lowering of slot plans in the engine's record-only mode against
the plain B-stream plans (whose launch lists are pinned in tests/data/stream_slots_plain_plans.json, recorded on the commit
before slot plans existed), and the argument checks of the two new entry points."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ["v2v_warp_blend_slots", "v2v_window_roll_slots"]
PINNED = json.load(open(os.path.join(ROOT, "tests", "data", "stream_slots_plain_plans.json")))
B, TG = 2, 3


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


def _label_inputs(H=32, W=64):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(0, 35, (B, 3, 1, H, W), generator=g).float(), torch.zeros(B, 2, 3, H, W),
            torch.randint(0, 20, (B, 3, 1, H, W), generator=g).float())


def _raw_inputs():
    return torch.rand(B, 3, 15, 32, 32), torch.zeros(B, 2, 3, 32, 32), None


CONFIGS = {"s1": ({}, _label_inputs), "s2": (dict(n_scales_spatial=2), _label_inputs),
           "raw": (dict(label_nc=0, input_nc=15, use_instance=False, fg=False), _raw_inputs)}


def _record(name, **slot_args):
    """Launch list of the first plan a fresh model records for configuration `name`."""
    from vid2vid_amd import networks as N
    N.set_record_only(True)
    try:
        kw, inputs = CONFIGS[name]
        m = _toy_model(**kw)
        fake, _ = m.inference(*inputs(), **slot_args)
        assert fake.shape[0] == B and m.engine.per_stream is False
        return m, _ops(m._active_plan)
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def _substituted(plain):
    """The plain list with the slot plan's substitutions: the blend becomes the slot blend, every run of B * (tG - 1)
    per-stream roll copies (what _roll records) becomes one v2v_window_roll_slots."""
    out, i, run = [], 0, B * (TG - 1)
    while i < len(plain):
        if plain[i] == "warp_blend":
            out.append("warp_blend_slots")
            i += 1
            if plain[i:i + run] == ["memcpy_d2d"] * run:
                out.append("window_roll_slots")
                i += run
        else:
            out.append(plain[i])
            i += 1
    return out


needs_cpu = pytest.mark.skipif(torch.cuda.is_available(), reason="dry-run census is a CPU-host check")


@needs_cpu
@pytest.mark.parametrize("name", ["s1", "s2", "raw"])
def test_plain_plans_are_the_pinned_ones(name):
    _, names = _record(name)
    assert names == PINNED[name]


@needs_cpu
def test_slot_plan_one_scale_blends_and_rolls_in_one_slot_launch():
    m, names = _record("s1", active=[0, 1])
    fp = m._active_plan
    assert fp.slots and fp.B == B and tuple(fp.slot_mode.shape) == (B,) and fp.slot_mode.dtype == torch.int32
    assert names.count("warp_blend_slots") == 1 and names[-1] == "warp_blend_slots"
    assert "memcpy_d2d" not in names and "warp_blend" not in names and "window_roll_slots" not in names
    assert names == _substituted(PINNED["s1"])
    assert [k for k in m._plans if k[-1] == "slots"]


@needs_cpu
@pytest.mark.parametrize("name,scales", [("s2", 2), ("raw", 1)])
def test_slot_plan_off_the_fused_head_rolls_with_the_roll_kernel(name, scales):
    _, names = _record(name, restart=[1])
    assert names.count("warp_blend_slots") == scales and names.count("window_roll_slots") == scales
    assert "warp_blend" not in names
    # the copies that stay are the gather sources (Engine.last_planes: B per scale), none of them a roll
    assert names.count("memcpy_d2d") == B * scales == PINNED[name].count("memcpy_d2d") - scales * B * (TG - 1)
    for i, n in enumerate(names):
        if n == "window_roll_slots":
            assert names[i - 1] == "warp_blend_slots"
    assert names == _substituted(PINNED[name])


@needs_cpu
def test_slot_arguments_are_validated_and_sticky():
    from vid2vid_amd import networks as N
    N.set_record_only(True)
    try:
        m = _toy_model()
        inp = _label_inputs()
        for bad in (dict(restart=[2]), dict(active=[-1]), dict(active=[True]), dict(restart=[True, False, False]),
                    dict(restart=[1], active=[0]), dict(restart=torch.tensor([True, False]), active=torch.tensor([False, True]))):
            with pytest.raises(ValueError):
                m.inference(*inp, **bad)
        assert m._active_plan is None and getattr(m, "fake_B_prev", None) is None      # a refused call changes nothing
        m.inference(*inp)
        plain = m._active_plan
        assert not plain.slots
        m.inference(*inp, active=torch.tensor([True, False]))
        slot = m._active_plan
        assert slot.slots and slot is not plain
        m.inference(*inp)                                   # sticky: no slot argument, still the slot plan
        assert m._active_plan is slot
        m.fake_B_prev = None
        m.inference(*inp)
        assert m._active_plan is plain
    finally:
        N.set_record_only(False)
        N._ENGINES.clear()


def test_new_entry_points_are_declared_and_registered():
    from vid2vid_amd import lib as L
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    declared = set(re.findall(r"\b(v2v_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.PROTOTYPES and hasattr(L.lib, name), name


def test_new_entry_points_refuse_null_mode_and_overlap():
    """Argument checks run before anything is submitted: host buffers stand in for device pointers."""
    from vid2vid_amd import lib as L
    N_, slots, Cc, H, W = 2, 2, 3, 4, 4
    frame = N_ * Cc * H * W
    buf = (C.c_float * (frame * (slots + 4)))()
    mode = (C.c_int32 * N_)()
    base = C.addressof(buf)
    at = lambda k: C.c_void_p(base + 4 * frame * k)      # the k-th frame-sized piece of buf
    window, raw, final, prev = at(0), at(slots), at(slots + 1), at(slots + 2)
    gx, gy = (C.c_float * W)(), (C.c_float * H)()
    EINVAL = L.lib.v2v_warp_blend_roll_batch(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 1, 1, 0, None)
    assert EINVAL != 0

    def blend(mode_, window_, prev_=prev, raw_=raw, final_=final):
        return L.lib.v2v_warp_blend_slots(raw_, at(slots + 3), at(slots + 3), prev_, None, None, final_, None, gx, gy, window_, slots,
                                          mode_, N_, Cc, H, W, 0, None)
    assert blend(None, window) == EINVAL and b"mode" in L.lib.v2v_last_error()
    assert blend(None, None) == EINVAL
    for kw in (dict(prev_=at(1)), dict(raw_=at(0)), dict(final_=C.c_void_p(base + 4 * (frame * slots - 1)))):
        assert blend(mode, window, **kw) == EINVAL and b"overlap" in L.lib.v2v_last_error(), kw
    with pytest.raises(RuntimeError, match="overlap"):
        L.check(blend(mode, window, prev_=at(1)), "warp_blend_slots")

    def roll(mode_, frame_):
        return L.lib.v2v_window_roll_slots(window, frame_, mode_, N_, slots, Cc, H, W, None)
    assert roll(None, raw) == EINVAL and b"mode" in L.lib.v2v_last_error()
    for inside in (at(0), at(1), C.c_void_p(base + 4 * (frame * slots - 1))):
        assert roll(mode, inside) == EINVAL and b"overlap" in L.lib.v2v_last_error()
    assert L.lib.v2v_window_roll_slots(None, raw, mode, N_, slots, Cc, H, W, None) == EINVAL
