"""uint8 image inputs in slot plans and the stream pool (opt.inputs_u8_slots): what can be checked without a GPU --
the option, the ABI of v2v_image_prologue_slots and its argument checks on the host, the record-only census of the slot and pool
plans' lowering, and the interface rules, which raise before any state changes."""
import ctypes as C
import os
import re
from collections import Counter

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_OPS = ("pack_nchw_to_nhwc", "unpack_nhwc_to_nchw", "memcpy_d2d", "window_gather_pool", "window_scatter_pool", "window_roll_slots")


def test_option_exists_and_defaults_to_false():
    from vid2vid_amd.options import make_opt
    opt = make_opt()
    assert opt.inputs_u8_slots is False and opt.inputs_u8 is False
    assert make_opt(inputs_u8_slots=True).inputs_u8_slots is True


def test_entry_point_signature_header_and_export_agree():
    from vid2vid_amd import lib as L
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    args = re.search(r"\bint\s+v2v_image_prologue_slots\s*\(([^)]*)\)", header).group(1).split(",")
    plain = re.search(r"\bint\s+v2v_image_prologue\s*\(([^)]*)\)", header).group(1).split(",")
    assert len(args) == len(L.PROTOTYPES["v2v_image_prologue_slots"][1]) == len(plain) + 4 == 23
    # the arguments of v2v_image_prologue, then the words and the pool sizes
    assert [a.split()[-1].lstrip("*") for a in args[:19]] == [a.split()[-1].lstrip("*") for a in plain]
    assert [a.split()[-1].lstrip("*") for a in args[19:]] == ["slot_mode", "row_slot", "S_win", "S_window"]
    assert L.PROTOTYPES["v2v_image_prologue_slots"][1][:19] == L.PROTOTYPES["v2v_image_prologue"][1]
    assert "v2v_image_prologue_slots" in L.exported_symbols() and hasattr(L.lib, "v2v_image_prologue_slots")


def test_entry_point_argument_checks_answer_on_the_host():
    """Host buffers stand in for device pointers: every refusal comes before anything is submitted; a valid pooled call is
    accepted in dry-run mode (which validates and submits nothing)."""
    from vid2vid_amd import lib as L
    N, S, T, H, W, Cin, win_C = 2, 4, 3, 4, 4, 6, 6
    al = lambda buf: C.c_void_p((C.addressof(buf) + 15) & ~15)
    win = (C.c_uint8 * (S * T * H * W * Cin + 16))()
    lut = (C.c_float * (Cin * 256 + 4))()
    x0 = (C.c_float * (N * H * W * 20 + 4))()
    real_last = (C.c_float * (N * Cin * H * W))()
    window = (C.c_float * (S * win_C * H * W))()
    packed = (C.c_float * (N * H * W * 8 + 4))()
    last = (C.c_float * (N * 3 * H * W))()
    modes, rows = (C.c_int32 * N)(0, 2), (C.c_int32 * N)(3, 1)

    def call(win_=al(win), window_=window, modes_=modes, rows_=rows, S_win=S, S_window=S, N_=N):
        return L.lib.v2v_image_prologue_slots(win_, al(lut), 1, al(x0), 20, real_last, N_, T, H, W, Cin, window_, win_C, al(packed), 8,
                                              last, 3, L.F32, None, modes_, rows_, S_win, S_window)
    EINVAL = L.lib.v2v_image_prologue(None, None, 1, None, 48, None, 1, 3, 8, 8, 15, None, 0, None, 0, None, 0, 1, None)
    assert EINVAL != 0
    assert call(win_=None) == EINVAL and b"image_prologue" in L.lib.v2v_last_error()
    for kw in (dict(rows_=None), dict(S_win=N - 1), dict(S_window=N - 1), dict(S_win=-1), dict(S_win=0, S_window=0),
               dict(window_=None, S_window=S)):
        assert call(**kw) == EINVAL and b"pool" in L.lib.v2v_last_error(), kw
    # overlap against the WHOLE input pool: real_last inside its last slot
    inside = C.c_void_p(((C.addressof(win) + 15) & ~15) + (S - 1) * T * H * W * Cin)

    def overlapping():
        return L.lib.v2v_image_prologue_slots(al(win), al(lut), 1, al(x0), 20, inside, N, T, H, W, Cin, None, 0, None, 0, None, 0,
                                              L.F32, None, modes, rows, S, 0)
    assert overlapping() == EINVAL and b"overlap" in L.lib.v2v_last_error()
    prev = L.lib.v2v_set_dry_run(1)
    try:
        assert call() == 0                                        # pooled input windows, pooled generated windows
        assert call(S_window=0) == 0                              # dense generated windows (their first N rows)
        assert call(rows_=None, S_win=0, S_window=0) == 0         # a slot plan: slot_mode alone
        assert call(modes_=None) == 0
        assert call(modes_=None, rows_=None, S_win=0, S_window=0) == 0        # the plain entry
    finally:
        L.lib.v2v_set_dry_run(prev)


# ------------------------------------------------------------------ the lowering, recorded without a GPU
def _names(fp):
    from vid2vid_amd.lib import lib
    return Counter(lib.v2v_plan_op_name(fp.plan.h, i).decode() for i in range(fp.plan.num_ops))


@pytest.fixture
def record_only():
    from vid2vid_amd import networks as N
    if torch.cuda.is_available():
        pytest.skip("dry-run check on a CPU host")
    N.set_record_only(True)
    yield
    N.set_record_only(False)
    N._ENGINES.clear()


def _pose_model(**kw):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    d = dict(label_nc=0, input_nc=6, use_instance=False, fg=False, use_real_img=True, random_init_ok=True, precision="bf16",
             gpu_ids=[], ngf=8, n_blocks=2, n_downsample_G=2, inputs_u8=True, inputs_u8_slots=True)
    d.update(kw)
    return create_model(make_opt(**d))


H, W, B = 16, 32, 3


def _frames(t=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, t, H, W, 6), generator=g, dtype=torch.uint8)


FIRST = torch.zeros(B, 2, 3, H, W)


def test_slot_plan_records_one_image_prologue_and_no_layout_or_copy_launch(record_only):
    # the fp32 slot plan of the model first (it also records the weight packings): its packs, its unpack, its copies
    m = _pose_model(inputs_u8=False)
    m.inference(torch.rand(B, 3, 6, H, W), FIRST, None, active=[0, 2])
    fp32 = m._active_plan
    base = _names(fp32)
    assert base["image_prologue"] == 0 and base["pack_nchw_to_nhwc"] == 2 and base["unpack_nhwc_to_nchw"] == 1 and fp32.win_u8 is None
    m.fake_B_prev = None
    m.opt.inputs_u8 = True
    fake, last = m.inference(_frames(), FIRST, None, active=[0, 2])
    fp = m._active_plan
    assert fp.slots and fp.pool is None and fp.raw_in is None and tuple(fp.win_u8.shape) == (B, 3, H, W, 6)
    assert tuple(fake.shape) == (B, 3, H, W) and tuple(last.shape) == (B, 6, H, W)
    got = _names(fp)
    assert got["image_prologue"] == 1 and got["warp_blend_slots"] == 1
    assert not [n for n in NO_OPS if got[n]], got
    assert fp.plan.num_ops - got["pack_weights"] < fp32.plan.num_ops - base["pack_weights"]
    assert {k: v for k, v in got.items() if "conv" in k} == {k: v for k, v in base.items() if "conv" in k}


@pytest.mark.parametrize("active", [[0, 2], [1]])
def test_pool_plan_records_one_image_prologue_and_no_gather_scatter_or_copy(record_only, active):
    m = _pose_model(compact_streams=True)
    fake, last = m.inference(_frames(), FIRST, None, active=active)
    fp = m._active_plan
    pool = fp.pool
    assert pool is not None and fp.B == len(active) and fp.raw_in is None
    assert fp.win_u8 is pool.inputs[6] and tuple(fp.win_u8.shape) == (B, 3, H, W, 6) and fp.win_u8.dtype == torch.uint8
    assert tuple(fake.shape) == (B, 3, H, W) and tuple(last.shape) == (B, 6, H, W)
    got = _names(fp)
    assert got["image_prologue"] == 1 and got["warp_blend_pool"] == 1
    assert not [n for n in NO_OPS if got[n]], got
    # another active count: another plan on the same input windows
    m.inference(_frames(1), None, None, active=[0, 1, 2] if len(active) == 1 else [2])
    assert m._active_plan is not fp and m._active_plan.win_u8 is fp.win_u8


def test_pool_plan_off_the_rolling_blend_gathers_the_generated_windows_only(record_only):
    """no_flow: no blend launch to roll in -- the dense lowering on gathered generated windows, the uint8 windows still in place."""
    m = _pose_model(compact_streams=True, no_flow=True)
    m.inference(_frames(), FIRST, None, active=[0, 2])
    got = _names(m._active_plan)
    assert got["image_prologue"] == 1 and got["window_gather_pool"] == 1 and got["window_scatter_pool"] == 1
    assert got["pack_nchw_to_nhwc"] == 0 and got["unpack_nhwc_to_nchw"] == 0


def test_option_off_refuses_as_before_and_alone_changes_nothing(record_only):
    m = _pose_model(inputs_u8_slots=False)
    for kw in (dict(active=[0, 2]), dict(restart=[1])):
        with pytest.raises(ValueError, match="fp32 inputs"):
            m.inference(_frames(), FIRST, None, **kw)
    m.opt.compact_streams = True
    with pytest.raises(ValueError, match="fp32 inputs"):
        m.inference(_frames(), FIRST, None)
    assert getattr(m, "fake_B_prev", None) is None and m._active_plan is None
    # inputs_u8_slots without inputs_u8: the fp32 path
    m.opt.compact_streams = False
    m.opt.inputs_u8, m.opt.inputs_u8_slots = False, True
    m.inference(torch.rand(B, 3, 6, H, W), FIRST, None, active=[0, 2])
    assert m._active_plan.win_u8 is None and m._active_plan.raw_in is not None and _names(m._active_plan)["image_prologue"] == 0


@pytest.mark.parametrize("pool", [False, True])
def test_interface_rules_raise_before_state_changes(record_only, pool):
    m = _pose_model(compact_streams=pool)
    frames = _frames()

    def refused(*args, **kw):
        plan, prev = m._active_plan, getattr(m, "fake_B_prev", None)
        keep = None if plan is None or plan.win_u8 is None else plan.win_u8.clone()
        with pytest.raises(ValueError):
            m.inference(*args, **kw)
        assert m._active_plan is plan and getattr(m, "fake_B_prev", None) is prev
        assert keep is None or torch.equal(plan.win_u8, keep)

    # no running sequence: the newest frame alone starts nothing
    refused(frames[:, 2:], FIRST, None, active=[0, 2])
    refused(frames[:, 1:], FIRST, None, active=[0, 2])
    refused(frames.float(), FIRST, None, active=[0, 2])
    assert m._active_plan is None
    m.inference(frames, FIRST, None, active=[0, 2])
    m.inference(frames[:, 2:], None, None, active=[0, 2])                      # t = 1 continues
    refused(frames[:, 2:], FIRST, None, restart=[1], active=[0, 1, 2])          # a restart brings its whole window
    refused(frames[:, 1:], None, None, active=[0])                              # t = 2
    refused(frames, None, None, restart=[1], active=[0, 2])                     # restarted and idle
    refused(frames, None, None, active=[3])
    m.inference(frames, FIRST, None, restart=[1], active=[0, 1, 2])
    # a sequence fed with fp32 so far is not continued by a uint8 slot or pool call
    m.fake_B_prev = None
    m.opt.inputs_u8 = False
    m.inference(torch.rand(B, 3, 6, H, W), FIRST, None, active=[0, 2])
    m.opt.inputs_u8 = True
    refused(frames, None, None, active=[0, 2])
    refused(frames[:, 2:], None, None, active=[0, 2])
