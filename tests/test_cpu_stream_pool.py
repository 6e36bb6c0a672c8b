"""Stream pool, checked without a device: the lowering of pool plans in the engine's record-only mode (row
counts, the batch-1 body at one active stream, which paths gather / scatter), the unchanged plans with the option off, the
argument checks of the four new entry points and prepare_streams."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ["v2v_frame_prologue_pool", "v2v_warp_blend_pool", "v2v_window_gather_pool", "v2v_window_scatter_pool"]
PINNED = json.load(open(os.path.join(ROOT, "tests", "data", "stream_slots_plain_plans.json")))
TG = 3


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


def _label_inputs(B, H=32, W=64):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(0, 35, (B, 3, 1, H, W), generator=g).float(), torch.zeros(B, 2, 3, H, W),
            torch.randint(0, 20, (B, 3, 1, H, W), generator=g).float())


def _raw_inputs(B):
    return torch.rand(B, 3, 15, 32, 32), torch.zeros(B, 2, 3, 32, 32), None


CONFIGS = {"s1": ({}, _label_inputs), "s2": (dict(n_scales_spatial=2), _label_inputs),
           "raw": (dict(label_nc=0, input_nc=15, use_instance=False, fg=False), _raw_inputs)}


class _recording:
    """Engines in record-only mode for the block (and none left behind it)."""

    def __enter__(self):
        from vid2vid_amd import networks as N
        N.set_record_only(True)

    def __exit__(self, *exc):
        from vid2vid_amd import networks as N
        N.set_record_only(False)
        N._ENGINES.clear()


def _record(name, B, compact=True, **slot_args):
    """(model, outputs, launch list) of the first call of a fresh model of configuration `name` with B streams."""
    with _recording():
        kw, inputs = CONFIGS[name]
        m = _toy_model(compact_streams=compact, **kw)
        out = m.inference(*inputs(B), **slot_args)
        assert m.engine.per_stream is False
        return m, out, (None if m._active_plan is None else _ops(m._active_plan))


needs_cpu = pytest.mark.skipif(torch.cuda.is_available(), reason="dry-run census is a CPU-host check")
POOL_OPS = ("frame_prologue_pool", "warp_blend_pool", "window_gather_pool", "window_scatter_pool")


@needs_cpu
def test_two_active_of_four_record_a_two_row_plan():
    m, (fake, last), names = _record("s1", 4, active=[1, 3])
    fp = m._active_plan
    assert fp.pool is not None and fp.pool.S == 4 and fp.B == 2 and not fp.slots
    assert fp.conv_log and all(c["N"] == 2 for c in fp.conv_log)            # convolutions and gather-sum stems alike
    assert any(c.get("onehot") for c in fp.conv_log)
    assert tuple(fp.row_slot.shape) == tuple(fp.slot_mode.shape) == (2,) and fp.row_slot.dtype == torch.int32
    assert fp.row_slot.tolist() == [1, 3] and m._pools[(4, 32, 64)].idle == [0, 2]
    assert tuple(fake.shape) == (4, 3, 32, 64) and tuple(last.shape) == (4, 36, 32, 64)
    assert [tuple(w.shape) for w in m.fake_B_prev] == [(4, TG - 1, 3, 32, 64)]
    assert [k for k in m._plans] == [k for k in m._plans if k[-1] == ("pool", 4) and k[7] == 2]
    # the per-stream body of the plain 2-stream plan between the pooled head and tail; no copy of any window
    assert names[0] == "frame_prologue_pool" and names[-1] == "warp_blend_pool"
    assert names[1:-1] == PINNED["s1"][1:PINNED["s1"].index("warp_blend")]
    assert not {"window_gather_pool", "window_scatter_pool", "memcpy_d2d", "frame_prologue", "warp_blend"} & set(names)


@needs_cpu
def test_one_active_stream_records_the_batch_1_body():
    m, _, names = _record("s1", 4, active=[2])
    fp = m._active_plan
    assert fp.B == 1 and fp.pool.S == 4 and all(c["N"] == 1 for c in fp.conv_log)
    assert any(c.get("pair") for c in fp.conv_log)                          # the twin launches: not the per-stream lowering
    _, _, plain = _record("s1", 1, compact=False)
    assert plain[0] == "frame_prologue" and plain[-1] == "warp_blend"
    assert names == ["frame_prologue_pool"] + plain[1:-1] + ["warp_blend_pool"]


@needs_cpu
def test_no_active_stream_records_nothing_and_returns_zeros():
    m, (fake, last), names = _record("s1", 4, active=[])
    assert names is None and not m._plans and getattr(m, "fake_B_prev", None) is None
    assert tuple(fake.shape) == (4, 3, 32, 64) and tuple(last.shape) == (4, 36, 32, 64)
    assert not fake.any() and not last.any()
    _, (fake, last), _ = _record("raw", 2, active=[False, False])
    assert tuple(fake.shape) == (2, 3, 32, 32) and tuple(last.shape) == (2, 15, 32, 32) and not fake.any() and not last.any()


@needs_cpu
@pytest.mark.parametrize("name,scales", [("s2", 2), ("raw", 1)])
@pytest.mark.parametrize("active", [[0, 1], [1]])
def test_paths_off_the_rolling_blend_gather_and_scatter_once_per_scale(name, scales, active):
    m, _, names = _record(name, 2, active=active)
    K = len(active)
    assert m._active_plan.B == K
    assert names.count("window_gather_pool") == scales and names.count("window_scatter_pool") == scales
    assert names.count("window_roll_slots") == scales and names.count("warp_blend_slots") == scales
    assert "warp_blend_pool" not in names and "frame_prologue_pool" not in names
    # the copies that stay are the gather sources (Engine.last_planes: K per scale at K > 1, a view at K = 1), none a roll
    assert names.count("memcpy_d2d") == (K * scales if K > 1 else 0)
    for i, n in enumerate(names):
        if n == "window_scatter_pool":
            assert names[i - 1] == "window_roll_slots"
    if K == 2:          # the dense lowering is the slot plan's, between a gather and a scatter per scale
        slot = [n for n in names if n not in ("window_gather_pool", "window_scatter_pool")]
        _, _, ref = _record(name, 2, compact=False, active=active)
        assert slot == ref


@needs_cpu
@pytest.mark.parametrize("name", ["s1", "s2", "raw"])
def test_option_off_records_the_pinned_plain_plans_and_the_slot_plans(name):
    m, _, names = _record(name, 2, compact=False)
    assert names == PINNED[name] and not m._pools and m._active_plan.pool is None
    m, _, names = _record(name, 2, compact=False, active=[0, 1])
    assert m._active_plan.slots and m._active_plan.pool is None and not m._pools and not set(POOL_OPS) & set(names)
    assert all(k[-1] == "slots" for k in m._plans)
    run, out, i = 2 * (TG - 1), [], 0
    plain = PINNED[name]
    while i < len(plain):                   # the substitutions of a slot plan (tests/test_cpu_stream_slots.py)
        if plain[i] == "warp_blend":
            out.append("warp_blend_slots")
            i += 1
            if plain[i:i + run] == ["memcpy_d2d"] * run:
                out.append("window_roll_slots")
                i += run
        else:
            out.append(plain[i])
            i += 1
    assert names == out
    # one stream: no pool whatever the option says
    m, _, names = _record(name, 1, compact=True)
    assert not m._pools and m._active_plan.pool is None and not set(POOL_OPS) & set(names)


@needs_cpu
def test_calls_follow_the_active_count_and_refused_calls_change_nothing():
    with _recording():
        m = _toy_model(compact_streams=True)
        inp = _label_inputs(3)
        for bad in (dict(restart=[3]), dict(active=[-1]), dict(active=[True]), dict(restart=[1], active=[0, 2])):
            with pytest.raises(ValueError):
                m.inference(*inp, **bad)
        assert m._active_plan is None and getattr(m, "fake_B_prev", None) is None and not m._plans
        m.inference(*inp)
        windows = m.fake_B_prev
        assert m._active_plan.B == 3
        m.inference(*inp, active=[0, 2])
        assert m._active_plan.B == 2 and m._active_plan.row_slot.tolist() == [0, 2] and m.fake_B_prev is windows
        m.inference(*inp, active=[1], restart=[1])
        assert m._active_plan.B == 1 and m._active_plan.row_slot.tolist() == [1]
        assert all(p.prev is windows for p in m._plans.values())
        with pytest.raises(ValueError):
            m.inference(*_label_inputs(2))                  # another slot count inside the sequences
        m.fake_B_prev = None
        m.inference(*inp, active=[2])
        assert m.fake_B_prev is windows and len(m._plans) == 3


@needs_cpu
def test_switching_the_option_inside_running_sequences():
    """On: a ValueError before anything changes (the windows are the running plan's own).  Off: the sequences continue on the slot
    or plain plan, which takes the pool's windows over."""
    with _recording():
        m = _toy_model(compact_streams=False)
        inp = _label_inputs(3)
        m.inference(*inp, active=[0, 1, 2])
        running, windows = m._active_plan, m.fake_B_prev
        m.opt.compact_streams = True
        with pytest.raises(ValueError):
            m.inference(*inp, active=[0, 2])
        assert m._active_plan is running and m.fake_B_prev is windows and not m._pools[(3, 32, 64)].windows[0].any()
        m.fake_B_prev = None
        m.inference(*inp, active=[0, 2])
        pool = m._pools[(3, 32, 64)]
        assert m._active_plan.pool is pool and m.fake_B_prev is pool.windows and pool.idle == [1]
        pool.windows[0].fill_(0.25)
        m.opt.compact_streams = False
        m.inference(*inp, active=[0, 2])
        assert m._active_plan is running and m.fake_B_prev is running.prev and bool((running.prev[0] == 0.25).all())


@needs_cpu
def test_prepare_streams_builds_exactly_the_requested_plans():
    with _recording():
        m = _toy_model(compact_streams=True)
        m.prepare_streams(4, 32, 64, 1, True, counts=[1, 3])
        assert sorted(k[7] for k in m._plans) == [1, 3] and all(k[-1] == ("pool", 4) for k in m._plans)
        built = dict(m._plans)
        inp = _label_inputs(4)
        m.inference(*inp, active=[0, 1, 3])
        assert m._plans == built and m._active_plan is built[[k for k in built if k[7] == 3][0]]
        m.prepare_streams(4, 32, 64, 1, True)
        assert sorted(k[7] for k in m._plans) == [1, 2, 3, 4] and all(m._plans[k] is built[k] for k in built)
        for bad in ([0], [5], []):
            with pytest.raises(ValueError):
                m.prepare_streams(4, 32, 64, 1, True, counts=bad)
        # uint8 label maps: plans of their own (key field 6), the ones a call with uint8 input_A / int32 inst_A replays
        m.prepare_streams(4, 32, 64, 1, True, u8=True, counts=[2])
        u8_plans = {k: v for k, v in m._plans.items() if k[6]}
        assert [k[7] for k in u8_plans] == [2] and len(m._plans) == 5
        fp = list(u8_plans.values())[0]
        assert fp.labels.dtype == torch.uint8 and fp.inst.dtype == torch.int32 and _ops(fp)[0] == "frame_prologue_pool"
        m.fake_B_prev = None
        m.inference(inp[0].to(torch.uint8), inp[1], inp[2].to(torch.int32), active=[1, 2])
        assert m._active_plan is fp and len(m._plans) == 5


def test_new_entry_points_are_declared_and_registered():
    from vid2vid_amd import lib as L
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    declared = set(re.findall(r"\b(v2v_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.PROTOTYPES and hasattr(L.lib, name), name


def test_new_entry_points_refuse_null_pointers_and_overlap():
    """Argument checks run before anything is submitted: host buffers stand in for device pointers."""
    from vid2vid_amd import lib as L
    K, S, slots, Cc, H, W = 2, 4, 2, 3, 4, 4
    frame = K * Cc * H * W                                # the K rows of one frame buffer
    pool_frames = S * slots * Cc * H * W // frame         # the pool, in such pieces
    buf = (C.c_float * (frame * (pool_frames + 6)))()
    base = C.addressof(buf)
    at = lambda k: C.c_void_p(base + 4 * frame * k)
    pool, raw, final, prev, other = at(0), at(pool_frames), at(pool_frames + 1), at(pool_frames + 2), at(pool_frames + 3)
    words = (C.c_int32 * K)(0, 1)
    gx, gy = (C.c_float * W)(), (C.c_float * H)()
    EINVAL = L.lib.v2v_warp_blend_roll_batch(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 1, 1, 0, None)
    assert EINVAL != 0

    def blend(mode_=words, rows_=words, pool_=pool, prev_=prev, raw_=raw, final_=final):
        return L.lib.v2v_warp_blend_pool(raw_, other, other, prev_, None, None, final_, None, gx, gy, pool_, slots, mode_, rows_,
                                         K, S, Cc, H, W, 0, None)
    assert blend(mode_=None) == EINVAL and b"mode" in L.lib.v2v_last_error()
    assert blend(rows_=None) == EINVAL and b"row_slot" in L.lib.v2v_last_error()
    assert blend(pool_=None) == EINVAL and blend(raw_=None) == EINVAL and blend(final_=None) == EINVAL
    # against the WHOLE pool: the last slot is as forbidden as the first
    for kw in (dict(prev_=at(pool_frames - 1)), dict(raw_=at(0)), dict(final_=C.c_void_p(base + 4 * (frame * pool_frames - 1)))):
        assert blend(**kw) == EINVAL and b"overlap" in L.lib.v2v_last_error(), kw
    with pytest.raises(RuntimeError, match="overlap"):
        L.check(blend(prev_=at(1)), "warp_blend_pool")

    labels, codes = (C.c_float * (K * TG * H * W))(), (C.c_uint8 * (K * TG * H * W))()
    packed = (C.c_float * (K * H * W * 8 + 4))()
    packed_p = C.c_void_p((C.addressof(packed) + 15) & ~15)

    def prologue(labels_=labels, codes_=codes, pool_=pool, rows_=words, packed_=packed_p, K_=K, S_=S):
        return L.lib.v2v_frame_prologue_pool(labels_, None, 0, codes_, None, None, 0, K_, TG, H, W, 35, pool_, S_, rows_, 6,
                                             packed_, 8, prev, 3, L.F32, None)
    assert prologue(rows_=None) == EINVAL and b"row_slot" in L.lib.v2v_last_error()
    assert prologue(pool_=None) == EINVAL and b"window" in L.lib.v2v_last_error()
    for kw in (dict(labels_=None), dict(codes_=None), dict(packed_=None), dict(K_=0), dict(S_=0)):
        assert prologue(**kw) == EINVAL, kw

    dense = at(pool_frames)
    for fn, args in ((L.lib.v2v_window_gather_pool, lambda d, p, r: (d, p, r)),
                     (L.lib.v2v_window_scatter_pool, lambda d, p, r: (p, d, r))):
        call = lambda d=dense, p=pool, r=words: fn(*args(d, p, r), K, S, slots, Cc, H, W, None)
        assert call(d=None) == EINVAL and call(p=None) == EINVAL and call(r=None) == EINVAL
        for inside in (at(0), at(pool_frames - 1), C.c_void_p(base + 4 * (frame * pool_frames - 1))):
            assert call(d=inside) == EINVAL and b"overlap" in L.lib.v2v_last_error()


def test_new_entry_points_honour_dry_run():
    """In dry-run mode a valid call validates, submits nothing and returns 0 (host buffers: a launch would fault)."""
    from vid2vid_amd import lib as L
    K, S, slots, Cc, H, W = 2, 3, 2, 3, 4, 4
    elems = slots * Cc * H * W
    pool, dense = (C.c_float * (S * elems))(), (C.c_float * (K * elems))()
    raw, final = (C.c_float * (K * Cc * H * W))(), (C.c_float * (K * Cc * H * W))()
    words = (C.c_int32 * K)(2, 0)
    prev = L.lib.v2v_set_dry_run(1)
    try:
        assert L.lib.v2v_window_gather_pool(dense, pool, words, K, S, slots, Cc, H, W, None) == 0
        assert L.lib.v2v_window_scatter_pool(pool, dense, words, K, S, slots, Cc, H, W, None) == 0
        assert L.lib.v2v_warp_blend_pool(raw, None, None, None, None, None, final, None, None, None, pool, slots, words, words,
                                         K, S, Cc, H, W, 0, None) == 0
        labels, labels_u8 = (C.c_float * (K * TG * H * W))(), (C.c_uint8 * (K * TG * H * W))()
        inst_i32, codes = (C.c_int32 * (K * TG * H * W))(), (C.c_uint8 * (K * TG * H * W))()
        packed = (C.c_float * (K * H * W * 8 + 4))()
        packed_p = C.c_void_p((C.addressof(packed) + 15) & ~15)
        for maps, inst, u8 in ((labels, None, 0), (labels_u8, inst_i32, 1)):
            assert L.lib.v2v_frame_prologue_pool(maps, inst, u8, codes, None, None, 0, K, TG, H, W, 35, pool, S, words, slots * Cc,
                                                 packed_p, 8, raw, Cc, L.F32, None) == 0
    finally:
        L.lib.v2v_set_dry_run(prev)
