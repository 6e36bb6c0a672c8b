"""Stream slots on the GPU: restart, pause and retire one stream of a B-stream frame plan.

The definition under test: under any schedule of restart / idle / resume, a slot that is active in a call produces what a
batch-1 model with the same weights produces on that slot's clip alone (fake_B_prev = None at each restart, no call while the
slot is idle).  Model level: a schedule against the pinned CPU oracle stepped per clip (the 1e-3 per-pixel bar) and against
this library's batch-1 plan (2e-3: two paths that each meet 1e-3 against the oracle), idle slots that nothing reads and
nothing writes (bit equality), the plain path bit for bit.  Kernel level, bit exact: v2v_warp_blend_slots against the batched
and the batch-1 rolling blend per mode, v2v_window_roll_slots against torch indexing."""
import os
import tempfile

import pytest
import torch

from util import sd_from_npz, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CALLS = 7
TG = 3


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


# ------------------------------------------------------------------ models, clips, schedules
def _model(g, S=1, precision="fp32", **kw):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "g"))
    for s in range(S):
        torch.save(sd_from_npz(g, "sd%d." % s), os.path.join(ck, "g", "latest_net_G%d.pth" % s))
    d = dict(name="g", checkpoints_dir=ck, label_nc=35, use_instance=True, fg=True, use_real_img=True, ngf=8, n_blocks=2,
             n_blocks_local=1, n_scales_spatial=S, n_downsample_G=2, loadSize=64, precision=precision)
    d.update(kw)
    return create_model(make_opt(**d))


def _raw_model(g, precision="fp32", **kw):
    return _model(g, 1, precision, label_nc=0, input_nc=15, use_instance=False, fg=False, **kw)


def _label_clip(seed, H=32, W=64, n=CALLS + 2):
    from vid2vid_amd import synthetic
    return synthetic.label2city_sequence(n, H, W, seed=seed, cell=8)


def _raw_clip(seed, n=CALLS + 2):
    from vid2vid_amd import synthetic
    return synthetic.edge2face_sequence(n, 32, 32, seed=seed)


def _label_inputs(clips, row, fill=0.0):
    """Inputs of one call.  row[slot] = (clip, local frame, restart) or None for an idle slot, whose rows hold `fill`."""
    H, W = next(c for c in clips if c is not None)[0].shape[-2:]
    nB = len(row)
    A = torch.full((nB, TG, 1, H, W), fill)
    I = torch.full((nB, TG, 1, H, W), fill)
    Bf = torch.zeros(nB, TG - 1, 3, H, W)
    for b, r in enumerate(row):
        if r is not None:
            c, t, restart = r
            A[b, :, 0], I[b, :, 0] = clips[c][0][t:t + TG], clips[c][1][t:t + TG]
            if restart:
                Bf[b] = clips[c][2][0, :TG - 1]
    return A, (Bf if any(r is not None and r[2] for r in row) else None), I


def _raw_inputs(clips, row, fill=0.0):
    nB = len(row)
    A = torch.full((nB, TG, 15, 32, 32), fill)
    Bf = torch.zeros(nB, TG - 1, 3, 32, 32)
    for b, r in enumerate(row):
        if r is not None:
            c, t, restart = r
            A[b] = clips[c][0][0, t:t + TG]
            if restart:
                Bf[b] = clips[c][1][0, :TG - 1]
    return A, (Bf if any(r is not None and r[2] for r in row) else None), None


def _sched3():
    """B = 3, 7 calls: slot 0 runs clip 0 straight through; slot 1 runs clip 1 and restarts on clip 2 at call 3; slot 2 runs
    clip 3, is idle at calls 2-3 and resumes at call 4."""
    rows = []
    for c in range(CALLS):
        s1 = (1, c, c == 0) if c < 3 else (2, c - 3, c == 3)
        s2 = (3, c, c == 0) if c < 2 else (None if c < 4 else (3, c - 2, False))
        rows.append([(0, c, c == 0), s1, s2])
    return rows


def _sched2():
    """The same shape at B = 2 (slots 1 and 2 of _sched3): slot 0 runs clip 1 and restarts on clip 2 at call 3; slot 1 runs
    clip 3, is idle at calls 2-3 and resumes at call 4."""
    return [[r[1], r[2]] for r in _sched3()]


def _run_schedule(model, sched, clips, inputs, slot_args=True):
    model.fake_B_prev = None
    outs = []
    for row in sched:
        kw = dict(restart=[r is not None and r[2] for r in row], active=[r is not None for r in row]) if slot_args else {}
        fake, _ = model.inference(*inputs(clips, row), **kw)
        outs.append((fake, [p.clone() for p in model.fake_B_prev]))
    return outs


def _clip_steps(sched):
    """{clip: number of frames the schedule generates from it}"""
    n = {}
    for row in sched:
        for r in row:
            if r is not None:
                n[r[0]] = max(n.get(r[0], 0), r[1] + 1)
    return n


def _alone(step, windows, reset, clips, sched, inputs):
    """{clip: [(fake_B, window per scale)] per local frame} of a batch-1 generator stepped on each clip alone."""
    ref = {}
    for c, steps in sorted(_clip_steps(sched).items()):
        reset()
        ref[c] = []
        for t in range(steps):
            fake = step(*inputs(clips, [(c, t, t == 0)]))
            ref[c].append((fake.clone(), [p.clone() for p in windows()]))
    return ref


def _check_schedule(outs, sched, ref, S, tol, what):
    worst = 0.0
    for call, (row, (fake, window)) in enumerate(zip(sched, outs)):
        for b, r in enumerate(row):
            if r is None:
                assert not fake[b].any(), "%s call %d: idle slot %d has a non-zero fake_B row" % (what, call, b)
                continue
            rf, rw = ref[r[0]][r[1]]
            worst = max(worst, assert_close(fake[b:b + 1], rf, tol, "%s call %d slot %d fake_B" % (what, call, b)))
            for si in range(S):
                assert_close(window[si][b], rw[si], tol, "%s call %d slot %d fake_B_prev[%d]" % (what, call, b, si))
    print("%s: worst per-pixel relative error of fake_B %.2e" % (what, worst))


# ------------------------------------------------------------------ 1. the schedule against the oracle
def test_schedule_of_three_slots_matches_the_oracle_per_clip(golden):
    from oracle import vid2vid_oracle as O
    g = golden("inference_label2city_s1_32x64")
    clips = [_label_clip(400 + c) for c in range(4)]
    sched = _sched3()
    sd = sd_from_npz(g, "sd0.")
    box = {}

    def reset():
        box["o"] = O.InferenceOracle([sd], 35, True, True, [26], 2, 2, 1)
    ref = _alone(lambda *a: box["o"].step(*a)[0], lambda: box["o"].fake_B_prev, reset, clips, sched, _label_inputs)
    model = _model(g, 1)
    outs = _run_schedule(model, sched, clips, _label_inputs)
    assert model._active_plan.slots and model._active_plan.B == 3
    _check_schedule(outs, sched, ref, 1, 1e-3, "S=1 B=3 schedule")


# ------------------------------------------------------------------ 2. the schedule against this library's batch-1 plan
def _against_batch_one(model, S, clips, inputs, what):
    sched = _sched2()

    def reset():
        model.fake_B_prev = None
    ref = _alone(lambda *a: model.inference(*a)[0], lambda: model.fake_B_prev, reset, clips, sched, inputs)
    outs = _run_schedule(model, sched, clips, inputs)
    assert model._active_plan.slots and model._active_plan.B == 2
    _check_schedule(outs, sched, ref, S, 2e-3, what)


def test_schedule_two_spatial_scales_matches_batch_one(golden):
    g = golden("inference_label2city_s2_32x64")
    clips = [None] + [_label_clip(420 + c) for c in range(3)]
    _against_batch_one(_model(g, 2), 2, clips, _label_inputs, "S=2 B=2 schedule")


def test_schedule_raw_inputs_matches_batch_one(golden):
    g = golden("inference_edge2face_s1_32x32")
    clips = [None] + [_raw_clip(440 + c) for c in range(3)]
    _against_batch_one(_raw_model(g), 1, clips, _raw_inputs, "raw B=2 schedule")


# ------------------------------------------------------------------ 3. no_first_img: the raw-only frame of one slot
def test_no_first_img_restart_is_raw_only_for_that_slot_alone(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1, use_real_img=False, no_first_img=True)
    clips = [_label_clip(460 + c) for c in range(3)]
    base = [[(0, c, c == 0), (1, c, c == 0)] for c in range(4)]
    with_restart = [list(r) for r in base]
    with_restart[3][1] = (2, 0, True)
    plain = _run_schedule(model, base, clips, _label_inputs)
    outs = _run_schedule(model, with_restart, clips, _label_inputs)
    assert model._active_plan.slots and not model._active_plan.use_raw_only
    for c in range(4):      # slot 0 never sees what slot 1 does
        assert torch.equal(outs[c][0][0], plain[c][0][0]) and torch.equal(outs[c][1][0][0], plain[c][1][0][0]), c
    assert not torch.equal(outs[3][0][1], plain[3][0][1])
    model.fake_B_prev = None
    first, _ = model.inference(*_label_inputs(clips, [(2, 0, True)]))          # batch 1: the raw-only first-frame plan
    assert model._active_plan.use_raw_only and model._active_plan.B == 1
    assert_close(outs[3][0][1:2], first, 2e-3, "restarted slot against the batch-1 raw-only first frame")
    assert_close(outs[3][1][0][1], model.fake_B_prev[0], 2e-3, "its window")
    assert not outs[3][1][0][1][0].any()                                         # oldest slot of a fresh window: zeros


# ------------------------------------------------------------------ 4. an idle slot is neither read nor written
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["label", "raw"])
def test_idle_slot_is_isolated(golden, precision, mode):
    if mode == "label":
        model = _model(golden("inference_label2city_s1_32x64"), 1, precision=precision)
        clips, inputs, garbage = [_label_clip(480 + c) for c in range(3)], _label_inputs, 255.0
    else:
        model = _raw_model(golden("inference_edge2face_s1_32x32"), precision=precision)
        clips, inputs, garbage = [_raw_clip(480 + c) for c in range(3)], _raw_inputs, float("nan")
    sched = [[(0, c, c == 0), (1, c, c == 0) if c < 2 or c == 4 else None, (2, c, c == 0)] for c in range(5)]
    sched[4][1] = (1, 2, False)                      # slot 1 pauses at calls 2-3 and resumes with its third frame

    def run(fill):
        model.fake_B_prev = None
        outs, windows = [], []
        for row in sched:
            before = None if model.fake_B_prev is None else model.fake_B_prev[0][1].clone()
            A, Bf, I = inputs(clips, row, fill)
            if row[1] is None and fill != fill:
                assert torch.isnan(A[1]).all()
            fake, _ = model.inference(A, Bf, I, restart=[r is not None and r[2] for r in row], active=[r is not None for r in row])
            if row[1] is None:
                assert torch.equal(model.fake_B_prev[0][1], before), "the idle slot's window changed"
                assert not fake[1].any() and torch.isfinite(fake).all()
            outs.append(fake)
            windows.append(model.fake_B_prev[0].clone())
        return outs, windows
    clean, wclean = run(0.0)             # idle rows hold valid data (label 0 / zeros)
    dirty, wdirty = run(garbage)         # idle rows hold label 255 / NaN
    for c in range(5):
        assert torch.equal(clean[c], dirty[c]) and torch.equal(wclean[c], wdirty[c]), "call %d" % c
    assert clean[4][1].any()


# ------------------------------------------------------------------ 5. the plain path, bit for bit
def test_slot_plan_with_every_stream_steady_equals_the_plain_plan(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1)
    clips = [_label_clip(500 + c) for c in range(3)]
    sched = [[(b, c, c == 0) for b in range(3)] for c in range(4)]
    plain = _run_schedule(model, sched, clips, _label_inputs, slot_args=False)
    assert not model._active_plan.slots
    model.fake_B_prev = None
    for c, row in enumerate(sched):
        fake, _ = model.inference(*_label_inputs(clips, row), **(dict(active=[0, 1, 2]) if c else {}))
        assert model._active_plan.slots == bool(c)
        assert torch.equal(fake, plain[c][0]), "frame %d" % c
        assert torch.equal(model.fake_B_prev[0], plain[c][1][0]), "window after frame %d" % c


# ------------------------------------------------------------------ 6. v2v_warp_blend_slots
def _engine(precision="fp32"):
    from vid2vid_amd import networks as N
    N.set_precision(precision)
    return N.get_engine(DEV)


def _blend_slots(eng, raw, flow, wgt, prev, fg, mask, win, modes, final, warp):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    N_, Cc, H, W = raw.shape
    gx, gy = eng.grid(H, W)
    md = torch.tensor(modes, dtype=torch.int32, device=DEV)
    L.check(L.lib.v2v_warp_blend_slots(_ptr(raw), _ptr(flow), _ptr(wgt), _ptr(prev), _ptr(fg), _ptr(mask), _ptr(final), _ptr(warp),
                                       _ptr(gx), _ptr(gy), _ptr(win), 0 if win is None else win.shape[1], _ptr(md), N_, Cc, H, W,
                                       int(eng.align_corners), _stream()), "warp_blend_slots")
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_fg", [True, False])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("HW", [(24, 40), (8, 8)])
def test_warp_blend_slots_per_mode(HW, B, with_fg):
    eng = _engine()
    (H, W), slots = HW, 2
    g = torch.Generator().manual_seed(B * 100 + H)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    raw0, flow0, wgt, prev, fg = r(B, 3, H, W), 3.0 * r(B, 2, H, W), torch.sigmoid(r(B, 1, H, W)), r(B, 3, H, W), r(B, 3, H, W)
    mask = (r(B, 1, H, W) > 0.5).float()
    win0 = r(B, slots, 3, H, W)
    fg_, mask_ = (fg, mask) if with_fg else (None, None)
    SENT = 7.0
    # every mode 0: the batched rolling blend, every output and the window
    raw_a, win_a = raw0.clone(), win0.clone()
    final_a, warp_a = eng.warp_blend(raw_a, flow0, wgt, prev, fg_, mask_, want_warp=True, roll=win_a)
    raw_b, win_b = raw0.clone(), win0.clone()
    final_b, warp_b = torch.full_like(raw0, SENT), torch.full_like(raw0, SENT)
    _blend_slots(eng, raw_b, flow0, wgt, prev, fg_, mask_, win_b, [0] * B, final_b, warp_b)
    assert torch.equal(final_a, final_b) and torch.equal(raw_a, raw_b) and torch.equal(warp_a, warp_b) and torch.equal(win_a, win_b)
    # the same through Engine.warp_blend(slot_mode=...)
    raw_c, win_c = raw0.clone(), win0.clone()
    final_c, _ = eng.warp_blend(raw_c, flow0, wgt, prev, fg_, mask_, roll=win_c, slot_mode=torch.zeros(B, dtype=torch.int32, device=DEV))
    assert torch.equal(final_a, final_c) and torch.equal(win_a, win_c)
    # mixed modes, sample by sample
    for rot in range(3):
        modes = [(b + rot) % 3 for b in range(B)]
        raw, flow, win = raw0.clone(), flow0.clone(), win0.clone()
        for b in range(B):
            if modes[b] == 2:                           # an idle sample's inputs may hold anything
                raw[b], flow[b] = float("nan"), float("nan")
        raw_in = raw.clone()
        final, warp = torch.full_like(raw0, SENT), torch.full_like(raw0, SENT)
        _blend_slots(eng, raw, flow, wgt, prev, fg_, mask_, win, modes, final, warp)
        for b in range(B):
            sl = lambda t: None if t is None else t[b:b + 1].contiguous()
            if modes[b] == 2:
                assert not final[b].any()
                assert torch.equal(win[b], win0[b]) and bool(torch.isnan(raw[b]).all()) and bool((warp[b] == SENT).all())
                continue
            raw1, win1 = raw0[b:b + 1].clone(), win0[b].clone()
            steady = modes[b] == 0
            f1, w1 = eng.warp_blend(raw1, sl(flow0) if steady else None, sl(wgt) if steady else None, sl(prev) if steady else None,
                                    sl(fg_), sl(mask_), want_warp=True, roll=win1)
            assert torch.equal(final[b], f1[0]) and torch.equal(raw[b], raw1[0]) and torch.equal(win[b], win1), (modes, b)
            assert torch.equal(warp[b], w1[0]) if steady else bool((warp[b] == SENT).all())
            assert torch.equal(win[b, 0], win0[b, 1]) and torch.equal(win[b, 1], final[b])
            if not steady and not with_fg:
                assert torch.equal(final[b], raw_in[b])
        # without a window nothing is rolled
        raw, win = raw_in.clone(), win0.clone()
        final2 = torch.full_like(raw0, SENT)
        _blend_slots(eng, raw, flow, wgt, prev, fg_, mask_, None, modes, final2, None)
        assert torch.equal(final2, final)
    with pytest.raises(RuntimeError, match="overlap"):
        w = win0.clone()
        inside = w.view(-1)[3 * H * W:3 * H * W * (B + 1)].view(B, 3, H, W)
        eng.warp_blend(raw0.clone(), flow0, wgt, inside, None, None, roll=w, slot_mode=torch.zeros(B, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ 7. v2v_window_roll_slots
@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("HW", [(8, 8), (5, 7)])
def test_window_roll_slots_equals_indexing(HW, slots):
    eng = _engine()
    (H, W), N_ = HW, 3
    g = torch.Generator().manual_seed(H + slots)
    win0 = torch.randn(N_, slots, 3, H, W, generator=g).to(DEV)
    frame = torch.randn(N_, 3, H, W, generator=g).to(DEV)
    for modes in ([0, 2, 1], [2, 2, 0], [0, 0, 0]):
        win = win0.clone()
        fr = frame.clone()
        for n in range(N_):
            if modes[n] == 2:
                fr[n] = float("nan")
        eng.window_roll(win, fr, torch.tensor(modes, dtype=torch.int32, device=DEV))
        for n in range(N_):
            want = win0[n] if modes[n] == 2 else torch.cat([win0[n, 1:], frame[n:n + 1]])
            assert torch.equal(win[n], want), (modes, n)
    with pytest.raises(RuntimeError, match="overlap"):
        inside = win0.view(-1)[:N_ * 3 * H * W].view(N_, 3, H, W)
        eng.window_roll(win0, inside, torch.zeros(N_, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ 8. interface
def test_interface_errors_single_stream_and_fresh_outputs(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1)
    clips = [_label_clip(520 + c) for c in range(2)]
    two = lambda c: _label_inputs(clips, [(0, c, c == 0), (1, c, c == 0)])
    one = lambda c: _label_inputs(clips, [(0, c, c == 0)])
    for bad in (dict(restart=[2]), dict(active=[0, -1]), dict(active=[True]), dict(restart=torch.tensor([True, False, True])),
                dict(restart=[1], active=[0]), dict(restart=[True, True], active=[True, False])):
        with pytest.raises(ValueError):
            model.inference(*two(0), **bad)
    assert getattr(model, "fake_B_prev", None) is None
    # B == 1: restart=[0] is fake_B_prev = None, active=[False] is no call at all
    f0, _ = model.inference(*one(0))
    f1, _ = model.inference(*one(1))
    z, zl = model.inference(*one(1), active=[False])
    assert tuple(z.shape) == (1, 3, 32, 64) and not z.any() and tuple(zl.shape) == (36, 32, 64)
    assert torch.equal(model.fake_B_prev[0][-1], f1[0]) and not model._active_plan.slots
    f2, _ = model.inference(*one(2))
    r0, _ = model.inference(*one(0), restart=[0])
    assert torch.equal(r0, f0) and not torch.equal(r0, f2) and not model._active_plan.slots
    with pytest.raises(ValueError):
        model.inference(*one(1), restart=[1])
    # B == 2 on the slot plan: fresh tensors per call, the newest window slot is the frame, idle rows are zero
    model.fake_B_prev = None
    fa, la = model.inference(*two(0), active=[0, 1])
    keep = fa.clone()
    fb, lb = model.inference(*two(1), active=torch.tensor([True, False]))
    assert model._active_plan.slots
    assert fa.data_ptr() != fb.data_ptr() and la.data_ptr() != lb.data_ptr() and torch.equal(fa, keep)
    assert not fb[1].any() and fb[0].any() and torch.equal(model.fake_B_prev[0][0, -1], fb[0])
    assert torch.equal(model.fake_B_prev[0][1, -1], fa[1])
