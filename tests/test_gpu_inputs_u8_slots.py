"""uint8 image inputs in slot plans and the stream pool (opt.inputs_u8_slots) on the GPU.

Kernel level, bit exact: v2v_image_prologue_slots against torch indexing -- lut[c][win[row_slot]] packed by Engine.pack, the window
pack of the named slots, a torch roll of the named non-idle slots for the advance; the words are read when a recorded launch runs;
with NULL words the entry is v2v_image_prologue.
Model level, bit exact: one schedule (late start, a pause of two calls, a restart, a retire, a one-stream call and an empty call)
fed uint8 frames against the same model object fed visual.decode_inputs of them as fp32 planes with the option off -- slot plan
and pool plan, fp32 and bf16, uint8 results, the lowering off the fused head -- tile searches off so both runs pick the same tiles.
The interface's refusals leave every state as it is."""
import pytest
import torch

from test_gpu_multi_stream import _model
from test_gpu_inputs_u8 import _engine, _u8_stream, _edge2face

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TG = 3


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ 1. the kernel against torch indexing
S_, ROWS, MODES = 5, [4, 0, 2], [0, 2, 1]


def _reference(eng, win0, lut, rows, modes, window_rows, precision):
    """(x0 bytes, real_last, packed bytes or None, last or None, the input pool after the launch)."""
    from vid2vid_amd import visual
    N_, T = len(rows), win0.shape[1]
    planes = visual.decode_inputs(win0[rows], lut)                              # (N, T, Cin, H, W): lut[c][win[row_slot]]
    x0 = eng.pack(planes.reshape(N_, -1, *planes.shape[-2:]).contiguous())
    newest = planes[:, T - 1] if precision == "fp32" else planes[:, T - 1].bfloat16().float()
    packed = last = None
    if window_rows is not None:
        packed, last = eng.pack(window_rows.contiguous()).t.clone(), window_rows[:, -3:].clone()
    win = win0.clone()
    for s, md in zip(rows, modes):
        if md != 2:                                                             # torch.roll, the newest frame kept in its place
            win[s] = torch.cat([torch.roll(win0[s], -1, 0)[:T - 1], win0[s, T - 1:]])
    return x0.t.clone(), newest, packed, last, win


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("window", ["none", "dense", "pooled"])
@pytest.mark.parametrize("HWC", [(5, 7, 3), (8, 8, 6), (24, 40, 15)])
def test_kernel_equals_torch_indexing(HWC, window, T, precision):
    """(5,7,3): a frame is no multiple of 16 bytes (the byte path of the advance); (8,8,6): it is (the granule path); (24,40,15):
    three full 256-pixel runs and a partial one.  Row 1 is idle; slots 1 and 3 are not named."""
    eng = _engine(precision)
    H, W, Cin = HWC
    g = torch.Generator().manual_seed(H * W * Cin + T)
    lut = torch.randn(Cin, 256, generator=g).to(DEV)
    win0 = torch.randint(0, 256, (S_, T, H, W, Cin), generator=g, dtype=torch.uint8).to(DEV)
    gen = torch.randn(S_ if window == "pooled" else len(ROWS), 6, H, W, generator=g).to(DEV) if window != "none" else None
    gen_rows = None if gen is None else (gen[ROWS] if window == "pooled" else gen)
    want = _reference(eng, win0, lut, ROWS, MODES, gen_rows, precision)
    win, gen0 = win0.clone(), None if gen is None else gen.clone()
    x0, real_last, packed, last = eng.image_prologue(win, lut, window=gen, last_C=3 if gen is not None else 0,
                                                     slot_mode=_i32(MODES), row_slot=_i32(ROWS), pooled_window=window == "pooled")
    torch.cuda.synchronize()
    assert x0.N == len(ROWS) and x0.C == T * Cin and tuple(real_last.shape) == (len(ROWS), Cin, H, W)
    assert torch.equal(x0.t.view(torch.uint8), want[0].view(torch.uint8))       # every row, pad channels included
    assert torch.equal(real_last, want[1])
    if gen is None:
        assert packed is None and last is None
    else:
        assert torch.equal(packed.t.view(torch.uint8), want[2].view(torch.uint8)) and torch.equal(last, want[3])
        assert torch.equal(gen, gen0)
    for s, md in zip(ROWS, MODES):                                              # the named non-idle slots moved on
        if md != 2 and T > 1:
            assert torch.equal(win[s, :T - 1], win0[s, 1:]) and torch.equal(win[s, T - 1], win0[s, T - 1]), s
    for s in (0, 1, 3):                                                         # the idle slot and the slots not named: untouched
        assert torch.equal(win[s], win0[s]), s
    assert torch.equal(win, want[4])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_words_are_read_when_the_recorded_launch_runs(precision):
    from vid2vid_amd.engine import Plan
    eng = _engine(precision)
    T, H, W, Cin = 3, 8, 8, 6
    g = torch.Generator().manual_seed(9)
    lut = torch.randn(Cin, 256, generator=g).to(DEV)
    win0 = torch.randint(0, 256, (S_, T, H, W, Cin), generator=g, dtype=torch.uint8).to(DEV)
    gen = torch.randn(S_, 6, H, W, generator=g).to(DEV)
    win, modes, rows = win0.clone(), _i32(MODES), _i32(ROWS)
    plan = Plan()
    eng.plan = plan
    try:
        with plan:
            x0, real_last, packed, last = eng.image_prologue(win, lut, window=gen, last_C=3, slot_mode=modes, row_slot=rows,
                                                             pooled_window=True)
    finally:
        eng.plan = None
    assert torch.equal(win, win0)                                               # recorded, not run
    state = win0
    for r, m in ((ROWS, MODES), ([1, 3, 0], [2, 0, 0]), ([3, 4, 1], [1, 2, 2])):
        rows.copy_(_i32(r))
        modes.copy_(_i32(m))
        want = _reference(eng, state, lut, r, m, gen[r], precision)
        plan.run()
        torch.cuda.synchronize()
        assert torch.equal(x0.t.view(torch.uint8), want[0].view(torch.uint8)) and torch.equal(real_last, want[1]), r
        assert torch.equal(packed.t.view(torch.uint8), want[2].view(torch.uint8)) and torch.equal(last, want[3]), r
        assert torch.equal(win, want[4]), r
        state = want[4]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_entry_with_null_words_is_the_plain_entry(precision):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    eng = _engine(precision)
    N_, T, H, W, Cin = 2, 3, 5, 7, 3
    g = torch.Generator().manual_seed(4)
    lut = torch.randn(Cin, 256, generator=g).to(DEV)
    win0 = torch.randint(0, 256, (N_, T, H, W, Cin), generator=g, dtype=torch.uint8).to(DEV)
    gen = torch.randn(N_, 6, H, W, generator=g).to(DEV)
    win_a = win0.clone()
    x0, real_last, packed, last = eng.image_prologue(win_a, lut, window=gen, last_C=3)
    win_b = win0.clone()
    x0_b, real_b, packed_b, last_b = (torch.full_like(t, 7) for t in (x0.t, real_last, packed.t, last))
    L.check(L.lib.v2v_image_prologue_slots(_ptr(win_b), _ptr(lut), 1, _ptr(x0_b), x0.Cs, _ptr(real_b), N_, T, H, W, Cin, _ptr(gen), 6,
                                           _ptr(packed_b), packed.Cs, _ptr(last_b), 3, eng.dtype, _stream(), None, None, 0, 0),
            "image_prologue_slots")
    torch.cuda.synchronize()
    assert torch.equal(x0_b.view(torch.uint8), x0.t.view(torch.uint8)) and torch.equal(real_b, real_last)
    assert torch.equal(packed_b.view(torch.uint8), packed.t.view(torch.uint8)) and torch.equal(last_b, last)
    assert torch.equal(win_a, win_b) and not torch.equal(win_a, win0)
    # the engine's argument rules
    with pytest.raises(ValueError):
        eng.image_prologue(win0.clone(), lut, row_slot=_i32([0, 1, 1]))                   # more rows than slots
    with pytest.raises(ValueError):
        eng.image_prologue(win0.clone(), lut, row_slot=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        eng.image_prologue(win0.clone(), lut, slot_mode=_i32([0]))
    with pytest.raises(ValueError):
        eng.image_prologue(win0.clone(), lut, window=gen, last_C=3, pooled_window=True)   # a pooled window without row_slot


# ------------------------------------------------------------------ 2. the model against its own fp32 path
N_CLIP = 12


def _sched():
    """B = 3, 11 calls; row[slot] = (clip, local frame, restart) or None (idle).  Slot 0 runs clip 0 and retires after call 5;
    slot 1 starts late (call 2) on clip 1 and is restarted on clip 2 at call 5; slot 2 runs clip 3, pauses at calls 3-4 and
    resumes at call 5.  Call 8 has one active stream, call 9 none, call 10 two again.  Active counts 2 2 3 2 2 3 2 2 1 0 2."""
    rows = []
    for c in range(11):
        s0 = (0, c, c == 0) if c < 6 else None
        s1 = None if c < 2 or c == 9 else ((1, c - 2, c == 2) if c < 5 else (2, c - 5 - int(c > 9), c == 5))
        s2 = (3, c, c == 0) if c < 3 else (None if c in (3, 4, 8, 9) else (3, c - 2 - int(c > 8) - int(c > 9), False))
        rows.append([s0, s1, s2])
    return rows


def _call_inputs(clips, row, u8, lut=None):
    """input_A and input_B of one call.  u8: bytes (B,t,H,W,C), t = 1 where no stream is restarted; where one is, t = tG and the
    OLDER frames of the other streams are 0xAA, as are an idle stream's rows.  Not u8: the decoded true frames, fp32 planes."""
    from vid2vid_amd import visual
    Bn = len(row)
    shape = clips[0][0].shape[2:]                                                # (H, W, C)
    any_restart = any(r is not None and r[2] for r in row)
    A = torch.full((Bn, TG) + tuple(shape), 0xAA, dtype=torch.uint8)
    Bf = torch.zeros((Bn, TG - 1) + tuple(clips[0][1].shape[2:]))
    for b, r in enumerate(row):
        if r is not None:
            c, t, restart = r
            if restart or not u8:
                A[b] = clips[c][0][0, t:t + TG]
            else:
                A[b, TG - 1] = clips[c][0][0, t + TG - 1]
            if restart:
                Bf[b] = clips[c][1][0, :TG - 1]
    if not u8:
        A = visual.decode_inputs(A, lut)
        for b, r in enumerate(row):
            if r is None:
                A[b] = 0
    elif not any_restart:
        A = A[:, TG - 1:].contiguous()
    return A, (Bf if any_restart else None)


def _run(model, sched, clips, u8, lut=None, watch=None):
    """[(first result, second result, [windows])] per call.  watch(call, model): called after every call of the uint8 run."""
    model.fake_B_prev = None
    model.opt.inputs_u8 = model.opt.inputs_u8_slots = bool(u8)
    outs = []
    try:
        for call, row in enumerate(sched):
            A, Bf = _call_inputs(clips, row, u8, lut)
            first, second = model.inference(A, Bf, None, restart=[r is not None and r[2] for r in row],
                                            active=[r is not None for r in row])
            outs.append((first, second, None if model.fake_B_prev is None else [p.clone() for p in model.fake_B_prev]))
            if watch is not None:
                watch(call, model)
    finally:
        model.opt.inputs_u8 = model.opt.inputs_u8_slots = False
    return outs


def _assert_schedule_equal(got, want, sched, what, second_rows=True):
    assert len(got) == len(want) == len(sched)
    for call, (row, (f, l, w), (rf, rl, rw)) in enumerate(zip(sched, got, want)):
        assert f.dtype == rf.dtype and l.dtype == rl.dtype and f.shape == rf.shape and l.shape == rl.shape, (what, call)
        for b, r in enumerate(row):
            if r is None:
                assert not f[b].any(), "%s call %d: idle stream %d has a non-zero first result" % (what, call, b)
                continue
            assert torch.equal(f[b], rf[b]), "%s call %d stream %d first result" % (what, call, b)
            assert torch.equal(l[b], rl[b]), "%s call %d stream %d second result" % (what, call, b)
            for si in range(len(w)):
                assert torch.equal(w[si][b], rw[si][b]), "%s call %d stream %d fake_B_prev[%d]" % (what, call, b, si)
        if f.is_floating_point():
            assert torch.isfinite(f).all()


def _watch_idle(kind, sched, seen):
    """After every call: the idle streams' uint8 windows (and generated windows) are what they were before it."""
    def watch(call, model):
        fp = model._active_plan
        if fp is None:
            return
        assert fp.win_u8 is not None and fp.raw_in is None and (fp.pool is not None) == (kind == "pool") and (fp.slots == (kind == "slots"))
        if kind == "pool":
            assert fp.win_u8 is fp.pool.inputs[fp.win_u8.shape[-1]] and fp.B == max(1, sum(r is not None for r in sched[call]))
        now = (fp.win_u8.clone(), [p.clone() for p in model.fake_B_prev])
        before = seen.get("state")
        if before is not None:
            for b, r in enumerate(sched[call]):
                if r is None:
                    assert torch.equal(now[0][b], before[0][b]), "call %d: idle stream %d: uint8 window changed" % (call, b)
                    for si, p in enumerate(now[1]):
                        assert torch.equal(p[b], before[1][si][b]), "call %d: idle stream %d: window %d changed" % (call, b, si)
        seen["state"] = now
        seen[call] = now
    return watch


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["slots", "pool"])
def test_schedule_equals_the_fp32_path_on_the_decoded_inputs(golden, kind, precision):
    from vid2vid_amd import visual
    model = _edge2face(golden, precision, compact_streams=kind == "pool")
    clips = [_u8_stream(700 + c, n=N_CLIP) for c in range(4)]
    sched = _sched()
    assert [sum(r is not None for r in row) for row in sched] == [2, 2, 3, 2, 2, 3, 2, 2, 1, 0, 2]
    lut = visual.input_lut(15)
    want = _run(model, sched, clips, u8=False, lut=lut)
    assert model._active_plan.win_u8 is None and model._active_plan.raw_in is not None
    seen = {}
    got = _run(model, sched, clips, u8=True, watch=_watch_idle(kind, sched, seen))
    _assert_schedule_equal(got, want, sched, "%s %s" % (kind, precision))
    # the paused stream (slot 2, idle at calls 3 and 4): uint8 window and generated windows as the call before the pause left them
    assert torch.equal(seen[4][0][2], seen[2][0][2]) and all(torch.equal(a[2], b[2]) for a, b in zip(seen[4][1], seen[2][1]))
    assert not torch.equal(seen[5][0][2], seen[4][0][2])
    # after resuming, its frames are those of the same clip run without a pause (the other slots arranged so that every frame
    # of the clip is generated beside as many active streams as in the schedule: the same pool plan per frame)
    straight = [[(0, t, t == 0), (1, t - 2, t == 2) if t in (2, 3) else None, (3, t, t == 0)] for t in range(7)]
    frames_of_3 = [r[2][1] for r in sched if r[2] is not None]
    assert frames_of_3 == list(range(7))
    assert [sum(r is not None for r in row) for row in straight] == \
        [sum(r is not None for r in row) for row in sched if row[2] is not None]
    alone = _run(model, straight, clips, u8=True)
    for call in (5, 6, 7, 10):
        t = sched[call][2][1]
        assert torch.equal(got[call][0][2], alone[t][0][2]) and torch.equal(got[call][1][2], alone[t][1][2]), call
    if kind == "pool":
        assert sorted(k[7] for k in model._plans if "inputs_u8" in k and ("pool", 3) in k) == [1, 2, 3]


def test_uint8_in_and_uint8_out_in_the_pool_and_the_slot_plan(golden):
    """frames_u8 + real_A_u8 with uint8 inputs: both results are uint8 and equal the fp32-input path's, slot plan and pool plan."""
    from vid2vid_amd import visual
    sched = _sched()[:7]
    clips = [_u8_stream(700 + c, n=N_CLIP) for c in range(4)]
    for kind in ("slots", "pool"):
        model = _edge2face(golden, "bf16", compact_streams=kind == "pool", frames_u8=True, real_A_u8=True)
        want = _run(model, sched, clips, u8=False, lut=visual.input_lut(15))
        got = _run(model, sched, clips, u8=True)
        assert got[0][0].dtype == torch.uint8 and tuple(got[0][0].shape) == (3, 32, 32, 3)
        assert got[0][1].dtype == torch.uint8 and tuple(got[0][1].shape) == (3, 32, 32, 1)
        _assert_schedule_equal(got, want, sched, kind + " uint8 out")
        for call, row in enumerate(sched):
            for b, r in enumerate(row):
                if r is None:
                    assert not got[call][1][b].any(), (kind, call, b)


def test_carries_plain_slot_and_pool_to_slot(golden):
    """The uint8 window follows the sequences: plain plan -> slot plan -> plain plan, and pool -> slot when compact_streams is
    cleared; t = 1 calls throughout, against the fp32 path making the same switches."""
    from vid2vid_amd import visual
    clips = [_u8_stream(700 + c, n=N_CLIP) for c in range(4)]
    lut = visual.input_lut(15)
    # calls 0-1 without slot arguments (a plain plan, or the pool with every stream active), from call 2 on with active=: the
    # slot plan, compact_streams cleared; stream 1 is idle at call 3 and goes on with its next frame at call 4
    rows = [[(0, t, t == 0), None if t == 3 else (1, t - int(t > 3), t == 0), (3, t, t == 0)] for t in range(6)]

    def run(u8, start_in_pool):
        model.fake_B_prev = None
        model.opt.inputs_u8 = model.opt.inputs_u8_slots = u8
        model.opt.compact_streams = start_in_pool
        outs = []
        try:
            for t, row in enumerate(rows):
                A, Bf = _call_inputs(clips, row, u8, lut)
                if t == 2:
                    model.opt.compact_streams = False
                slot_kw = dict(active=[r is not None for r in row]) if t >= 2 else {}
                f, l = model.inference(A, Bf, None, **slot_kw)
                outs.append((f, l, [p.clone() for p in model.fake_B_prev], model._active_plan))
        finally:
            model.opt.inputs_u8 = model.opt.inputs_u8_slots = model.opt.compact_streams = False
        return outs

    model = _edge2face(golden, "fp32")
    for start_in_pool in (False, True):
        want, got = run(False, start_in_pool), run(True, start_in_pool)
        kinds = [("pool" if o[3].pool is not None else "slots" if o[3].slots else "plain") for o in got]
        assert kinds == (["pool", "pool"] + ["slots"] * 4 if start_in_pool else ["plain", "plain"] + ["slots"] * 4), kinds
        assert all(o[3].win_u8 is not None for o in got) and all(o[3].win_u8 is None for o in want)
        for t, (g_, w_) in enumerate(zip(got, want)):
            for b in range(3):
                if rows[t][b] is None:
                    assert not g_[0][b].any()
                    continue
                assert torch.equal(g_[0][b], w_[0][b]) and torch.equal(g_[1][b], w_[1][b]) and torch.equal(g_[2][0][b], w_[2][0][b]), \
                    (start_in_pool, t, b)


def test_two_spatial_scales_and_fg_take_the_lowering_off_the_fused_head():
    """A toy pose model: S = 2, --fg (the mask from input channel 1), 6 input channels with the DensePose part-index table, 32x64,
    seeded random weights.  image_prologue without `window` in front of the dense slot lowering."""
    from vid2vid_amd import visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    from vid2vid_amd.lib import lib
    torch.manual_seed(23)
    opt = make_opt(label_nc=0, input_nc=6, use_instance=False, fg=True, fg_labels=[1], use_real_img=True, random_init_ok=True, ngf=8,
                   n_blocks=2, n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, loadSize=64, precision="fp32", gpu_ids=[0])
    model = create_model(opt)
    opt.autotune = False
    opt.frame_tune = 0
    lut = visual.input_lut(6, densepose_part_channel=2)
    opt.input_lut = lut.to(DEV)
    clips = [_u8_stream(800 + c, H=32, W=64, in_ch=6, n=N_CLIP) for c in range(4)]
    sched = _sched()[:7]
    want = _run(model, sched, clips, u8=False, lut=lut)
    got = _run(model, sched, clips, u8=True)
    fp = model._active_plan
    names = [lib.v2v_plan_op_name(fp.plan.h, i).decode() for i in range(fp.plan.num_ops)]
    assert fp.slots and fp.win_u8 is not None and names.count("image_prologue") == 1 and "pack_nchw_to_nhwc" in names
    assert model.n_scales == 2 and len(got[0][2]) == 2
    _assert_schedule_equal(got, want, sched, "S = 2 with fg")


# ------------------------------------------------------------------ 3. the interface
@pytest.mark.parametrize("kind", ["slots", "pool"])
def test_refusals_leave_every_state_untouched(golden, kind):
    from vid2vid_amd import visual
    model = _edge2face(golden, "fp32", compact_streams=kind == "pool")
    opt = model.opt
    clips = [_u8_stream(700 + c, n=N_CLIP) for c in range(4)]
    sched = _sched()[:5]
    want = _run(model, sched, clips, u8=True)

    def refused(*args, **kw):
        plan, prev = model._active_plan, model.fake_B_prev
        keep = None if prev is None else ([p.clone() for p in prev], None if plan.win_u8 is None else plan.win_u8.clone())
        with pytest.raises(ValueError):
            model.inference(*args, **kw)
        assert model._active_plan is plan and model.fake_B_prev is prev
        if keep is not None:
            assert all(torch.equal(a, b) for a, b in zip(prev, keep[0])) and (keep[1] is None or torch.equal(plan.win_u8, keep[1]))

    model.fake_B_prev = None
    opt.inputs_u8 = opt.inputs_u8_slots = True
    full, Bf = _call_inputs(clips, sched[0], True)
    refused(full[:, 2:], Bf, None, active=[0, 2])                               # no running sequence: t = 1 starts nothing
    assert model.fake_B_prev is None
    for call in range(4):
        A, Bf = _call_inputs(clips, sched[call], True)
        model.inference(A, Bf, None, restart=[r is not None and r[2] for r in sched[call]], active=[r is not None for r in sched[call]])
    A, _ = _call_inputs(clips, sched[4], True)                                   # t = 1
    whole = torch.cat([A, A, A], 1)
    refused(A, None, None, restart=[1], active=[0, 1])                           # restart together with t = 1
    refused(whole[:, 1:], None, None, active=[0, 1])                             # t = 2
    refused(visual.decode_inputs(whole, visual.input_lut(15)), None, None, active=[0, 1])
    refused(whole, None, None, restart=[2], active=[0, 1])                       # restarted and idle
    refused(whole, None, None, active=[0, 3])
    refused(whole[:2], None, None, active=[0, 1])                                # another B
    opt.input_lut = torch.zeros(14, 256)
    refused(A, None, None, active=[0, 1])
    opt.input_lut = None
    opt.inputs_u8_slots = False                                                  # the option off: today's refusals
    refused(A, None, None, active=[0, 1])
    opt.inputs_u8_slots = True
    f, l = model.inference(A, None, None, active=[0, 1])                         # call 4 as in the undisturbed run
    assert torch.equal(f, want[4][0]) and torch.equal(l[:2], want[4][1][:2])
    # a sequence fed with fp32 so far is not continued by a uint8 slot or pool call
    opt.inputs_u8 = opt.inputs_u8_slots = False
    model.fake_B_prev = None
    lut = visual.input_lut(15)
    for call in range(2):
        A32, Bf = _call_inputs(clips, sched[call], False, lut)
        model.inference(A32, Bf, None, restart=[r is not None and r[2] for r in sched[call]], active=[r is not None for r in sched[call]])
    opt.inputs_u8 = opt.inputs_u8_slots = True
    refused(whole, None, None, active=[0, 2])
    refused(A, None, None, active=[0, 2])
    # inputs_u8_slots alone, without inputs_u8, changes nothing: the fp32 call goes on
    opt.inputs_u8 = False
    plan = model._active_plan
    A32, Bf = _call_inputs(clips, sched[2], False, lut)
    model.inference(A32, Bf, None, restart=[False, True, False], active=[True, True, True])
    assert model._active_plan.win_u8 is None and model._active_plan.raw_in is not None
    assert (model._active_plan is plan) == (kind == "slots")
    opt.inputs_u8_slots = False
