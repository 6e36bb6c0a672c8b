"""Stream pool on the GPU: opt.compact_streams replays a plan with one row per ACTIVE stream of the S slots.

Kernel level, bit exact: the pooled head and tail (v2v_frame_prologue_pool, v2v_warp_blend_pool) per row against the one-sample
calls on the named slot, with the identity against their batched siblings, the guard for a slot index out of range, and
v2v_window_gather_pool / v2v_window_scatter_pool against torch indexing.  Model level: the contract of the stream slots (3.15)
under schedules whose active count changes -- against the pinned CPU oracle stepped per clip (the 1e-3 per-pixel bar), against
this library's batch-1 plan (2e-3 on the paths off the fused head: two paths that each meet 1e-3 against the oracle), bit for
bit against the slot plan (all active) and the batch-1 plan (one active), and isolation of the idle rows."""
import pytest
import torch

from util import sd_from_npz, assert_close, rel_err
from test_gpu_stream_slots import (_model, _raw_model, _label_clip, _raw_clip, _label_inputs, _raw_inputs, _run_schedule, _alone,
                                   _check_schedule, _sched2, _engine, _blend_slots)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TG = 3
SENT = 7.0


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ 1. v2v_frame_prologue_pool
def _prologue_pool(eng, labels, inst, pool, rows, out):
    """The raw entry point on caller-owned outputs `out` = (codes, mask, packed, last): what a row leaves unwritten is seen."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    K, T, H, W = labels.shape
    codes, mask, packed, last = out
    fg, row_slot = eng._fg_labels([26]), _i32(rows)
    u8 = int(labels.dtype == torch.uint8)
    L.check(L.lib.v2v_frame_prologue_pool(_ptr(labels), _ptr(inst), u8, _ptr(codes), _ptr(mask), _ptr(fg), fg.numel(), K, T, H, W, 35,
                                          _ptr(pool), pool.shape[0], _ptr(row_slot), pool.shape[1], _ptr(packed), packed.shape[-1],
                                          _ptr(last), 3, eng.dtype, _stream()), "frame_prologue_pool")
    torch.cuda.synchronize()


def _prologue_outputs(eng, K, T, H, W, win_C):
    cs = eng.empty_act(1, H, W, win_C).Cs
    return (torch.full((K, T, H, W), 99, dtype=torch.uint8, device=DEV), torch.full((K, 1, H, W), SENT, device=DEV),
            torch.full((K, H, W, cs), SENT, device=DEV).to(eng.tdtype), torch.full((K, 3, H, W), SENT, device=DEV))


def _prologue_ref(eng, labels, inst, window):
    """(codes, mask, packed, last) of the existing head: one sample (labels (T,H,W), window (1,C,H,W)) or the batch."""
    from vid2vid_amd.engine import LabelSource
    H, W = labels.shape[-2:]
    src = LabelSource(labels.contiguous(), inst.contiguous(), TG, 35)
    _, mask, packed, last = eng.frame_prologue(src, H, W, [26], True, window=window.contiguous(), last_C=3)
    torch.cuda.synchronize()
    return src.codes, mask, packed.t, last


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("HW", [(8, 16), (5, 7)])
def test_frame_prologue_pool_rows_slots_identity_and_guard(HW, precision):
    eng = _engine(precision)
    (H, W), S, K, slots = HW, 4, 2, 2
    g = torch.Generator().manual_seed(H * 10 + W)
    labels = torch.randint(0, 40, (S, TG, H, W), generator=g).float().to(DEV)         # 35..39: no label plane
    labels[:, :, ::2, ::3] = 26.0                                                    # some foreground
    inst = torch.randint(0, 4, (S, TG, H, W), generator=g).float().to(DEV)
    pool = torch.randn(S, slots * 3, H, W, generator=g).to(DEV)
    pool0 = pool.clone()
    rows = [3, 1]
    out = _prologue_outputs(eng, K, TG, H, W, slots * 3)
    _prologue_pool(eng, labels[:K].contiguous(), inst[:K].contiguous(), pool, rows, out)
    assert torch.equal(pool, pool0)
    for k, s in enumerate(rows):                 # row k: the one-sample head on its maps and on slot s's window
        ref = _prologue_ref(eng, labels[k], inst[k], pool0[s:s + 1])
        for name, got, want in zip(("codes", "mask", "packed", "last"), out, ref):
            assert torch.equal(got[k], want.reshape(got[k].shape)), (name, k)
    # identity, K = S: the batched head
    out = _prologue_outputs(eng, S, TG, H, W, slots * 3)
    _prologue_pool(eng, labels, inst, pool, list(range(S)), out)
    for name, got, want in zip(("codes", "mask", "packed", "last"), out, _prologue_ref(eng, labels, inst, pool0)):
        assert torch.equal(got, want.reshape(got.shape)), name
    # a slot index out of range: that row writes nothing, the other row is what it was
    for bad in (S, -1):
        out2 = _prologue_outputs(eng, K, TG, H, W, slots * 3)
        _prologue_pool(eng, labels[:K].contiguous(), inst[:K].contiguous(), pool, [bad, 1], out2)
        fresh = _prologue_outputs(eng, K, TG, H, W, slots * 3)
        ref = _prologue_ref(eng, labels[1], inst[1], pool0[1:2])
        for name, got, untouched, want in zip(("codes", "mask", "packed", "last"), out2, fresh, ref):
            assert torch.equal(got[0], untouched[0]), (name, bad)
            assert torch.equal(got[1], want.reshape(got[1].shape)), (name, bad)
        assert torch.equal(pool, pool0)
    # through the engine
    from vid2vid_amd.engine import LabelSource
    src = LabelSource(labels[:K].contiguous(), inst[:K].contiguous(), TG, 35)
    _, mask, packed, last = eng.frame_prologue(src, H, W, [26], True, window=pool, last_C=3, row_slot=_i32(rows))
    out = _prologue_outputs(eng, K, TG, H, W, slots * 3)
    _prologue_pool(eng, labels[:K].contiguous(), inst[:K].contiguous(), pool, rows, out)
    assert torch.equal(src.codes, out[0]) and torch.equal(mask, out[1]) and torch.equal(packed.t, out[2]) and torch.equal(last, out[3])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frame_prologue_pool_uint8_labels_int32_instances(precision):
    """The uint8 / int32 instantiations, raw and through the engine: per row the one-sample head on the same maps."""
    from vid2vid_amd.engine import LabelSource
    eng = _engine(precision)
    H, W, S, K, slots = 5, 7, 4, 2, 2
    g = torch.Generator().manual_seed(57)
    labels = torch.randint(0, 40, (K, TG, H, W), generator=g).to(torch.uint8).to(DEV)
    labels[:, :, ::2, ::3] = 26
    blocks = 70000 * (torch.arange(W) // 4)[None, :] + (torch.arange(H) // 3)[:, None]      # ids past 2^16: compared as int32
    inst = (blocks[None, None] + torch.arange(K * TG).view(K, TG, 1, 1)).to(torch.int32).to(DEV)
    pool = torch.randn(S, slots * 3, H, W, generator=g).to(DEV)
    pool0, rows = pool.clone(), [3, 1]
    out = _prologue_outputs(eng, K, TG, H, W, slots * 3)
    _prologue_pool(eng, labels, inst, pool, rows, out)
    assert torch.equal(pool, pool0)
    src = LabelSource(labels, inst, TG, 35)
    _, mask, packed, last = eng.frame_prologue(src, H, W, [26], True, window=pool, last_C=3, row_slot=_i32(rows))
    torch.cuda.synchronize()
    for name, got, want in zip(("codes", "mask", "packed", "last"), out, (src.codes, mask, packed.t, last)):
        assert torch.equal(got, want), name
    for k, s in enumerate(rows):
        ref = _prologue_ref(eng, labels[k], inst[k], pool0[s:s + 1])
        for name, got, want in zip(("codes", "mask", "packed", "last"), out, ref):
            assert torch.equal(got[k], want.reshape(got[k].shape)), (name, k)
    assert bool((out[0] >= 128).any()) and bool((out[0] < 128).any())            # both edge and interior pixels


# ------------------------------------------------------------------ 2. v2v_warp_blend_pool
def _blend_pool(eng, raw, flow, wgt, prev, fg, mask, pool, modes, rows, final, warp):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    K, Cc, H, W = raw.shape
    gx, gy = eng.grid(H, W)
    mode, row_slot = _i32(modes), _i32(rows)                 # two live tensors: a temporary's memory would be handed out again
    L.check(L.lib.v2v_warp_blend_pool(_ptr(raw), _ptr(flow), _ptr(wgt), _ptr(prev), _ptr(fg), _ptr(mask), _ptr(final), _ptr(warp),
                                      _ptr(gx), _ptr(gy), _ptr(pool), pool.shape[1], _ptr(mode), _ptr(row_slot), K,
                                      pool.shape[0], Cc, H, W, int(eng.align_corners), _stream()), "warp_blend_pool")
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_fg", [True, False])
@pytest.mark.parametrize("HW", [(8, 16), (5, 7)])
def test_warp_blend_pool_rows_slots_identity_and_guard(HW, with_fg):
    eng = _engine()
    (H, W), S, K, slots = HW, 4, 2, 2
    g = torch.Generator().manual_seed(H * 10 + W + int(with_fg))
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    raw0, flow, wgt, prev, fg = r(S, 3, H, W), 3.0 * r(S, 2, H, W), torch.sigmoid(r(S, 1, H, W)), r(S, 3, H, W), r(S, 3, H, W)
    mask = (r(S, 1, H, W) > 0.5).float()
    pool0 = r(S, slots, 3, H, W)
    fg_, mask_ = (fg, mask) if with_fg else (None, None)
    d = lambda t: None if t is None else t[:K].contiguous()              # the K dense rows
    rows, modes = [3, 1], [0, 1]

    def one_sample(k, s):
        """Row k by the one-sample rolling blend on slot s's window (mode 1: flow = weight = NULL)."""
        sl = lambda t: None if t is None else t[k:k + 1].contiguous()
        steady = modes[k] == 0
        raw1, win1 = raw0[k:k + 1].clone(), pool0[s].clone()
        f1, w1 = eng.warp_blend(raw1, sl(flow) if steady else None, sl(wgt) if steady else None, sl(prev) if steady else None,
                                sl(fg_), sl(mask_), want_warp=True, roll=win1)
        return f1[0], raw1[0], (w1[0] if steady else None), win1

    raw, pool = d(raw0), pool0.clone()
    final, warp = torch.full_like(raw, SENT), torch.full_like(raw, SENT)
    _blend_pool(eng, raw, d(flow), d(wgt), d(prev), d(fg_), d(mask_), pool, modes, rows, final, warp)
    for k, s in enumerate(rows):
        f1, r1, w1, win1 = one_sample(k, s)
        assert torch.equal(final[k], f1) and torch.equal(raw[k], r1) and torch.equal(pool[s], win1), k
        assert torch.equal(warp[k], w1) if w1 is not None else bool((warp[k] == SENT).all())
        assert torch.equal(pool[s, 0], pool0[s, 1]) and torch.equal(pool[s, 1], final[k])
    assert torch.equal(pool[0], pool0[0]) and torch.equal(pool[2], pool0[2])          # slots not named: bit for bit
    # the same through Engine.warp_blend(row_slot=...)
    raw_e, pool_e = d(raw0), pool0.clone()
    final_e, _ = eng.warp_blend(raw_e, d(flow), d(wgt), d(prev), d(fg_), d(mask_), roll=pool_e, slot_mode=_i32(modes), row_slot=_i32(rows))
    torch.cuda.synchronize()
    assert torch.equal(final_e, final) and torch.equal(raw_e, raw) and torch.equal(pool_e, pool)
    # identity, K = S: v2v_warp_blend_slots on every output and the window
    for all_modes in ([0] * S, [1, 0, 0, 1]):
        raw_a, win_a = raw0.clone(), pool0.clone()
        final_a, warp_a = torch.full_like(raw0, SENT), torch.full_like(raw0, SENT)
        _blend_slots(eng, raw_a, flow, wgt, prev, fg_, mask_, win_a, all_modes, final_a, warp_a)
        raw_b, win_b = raw0.clone(), pool0.clone()
        final_b, warp_b = torch.full_like(raw0, SENT), torch.full_like(raw0, SENT)
        _blend_pool(eng, raw_b, flow, wgt, prev, fg_, mask_, win_b, all_modes, list(range(S)), final_b, warp_b)
        assert torch.equal(final_a, final_b) and torch.equal(raw_a, raw_b) and torch.equal(warp_a, warp_b) and torch.equal(win_a, win_b)
    # a slot index out of range: nothing of that row is written, the other row is what it was
    for bad in (S, -1):
        raw2, pool2 = d(raw0), pool0.clone()
        final2, warp2 = torch.full_like(raw2, SENT), torch.full_like(raw2, SENT)
        _blend_pool(eng, raw2, d(flow), d(wgt), d(prev), d(fg_), d(mask_), pool2, modes, [bad, 1], final2, warp2)
        assert bool((final2[0] == SENT).all()) and bool((warp2[0] == SENT).all()) and torch.equal(raw2[0], raw0[0]), bad
        assert torch.equal(final2[1], final[1]) and torch.equal(raw2[1], raw[1]) and torch.equal(pool2[1], pool[1]), bad
        for s in (0, 2, 3):
            assert torch.equal(pool2[s], pool0[s]), (bad, s)
    with pytest.raises(RuntimeError, match="overlap"):       # against the whole pool: a gather source in the LAST slot
        w = pool0.clone()
        inside = w.view(-1)[-K * 3 * H * W:].view(K, 3, H, W)
        eng.warp_blend(d(raw0), d(flow), d(wgt), inside, None, None, roll=w, slot_mode=_i32(modes), row_slot=_i32(rows))


# ------------------------------------------------------------------ 3. gather / scatter
@pytest.mark.parametrize("HW", [(8, 16), (5, 7)])
def test_window_gather_scatter_round_trip(HW):
    eng = _engine()
    (H, W), S, K, slots = HW, 4, 2, 2
    g = torch.Generator().manual_seed(H + W)
    pool0 = torch.randn(S, slots, 3, H, W, generator=g).to(DEV)
    rows = [3, 1]
    pool, dense = pool0.clone(), torch.full((K, slots, 3, H, W), SENT, device=DEV)
    eng.window_gather(dense, pool, _i32(rows))
    torch.cuda.synchronize()
    assert torch.equal(dense, pool0[rows]) and torch.equal(pool, pool0)
    pool.zero_()
    eng.window_scatter(pool, dense, _i32(rows))                       # gather then scatter: the identity on the named slots
    torch.cuda.synchronize()
    assert torch.equal(pool[rows], pool0[rows]) and not pool[0].any() and not pool[2].any()
    new = torch.randn(K, slots, 3, H, W, generator=g).to(DEV)
    pool = pool0.clone()
    eng.window_scatter(pool, new, _i32(rows))
    torch.cuda.synchronize()
    assert torch.equal(pool[3], new[0]) and torch.equal(pool[1], new[1]) and torch.equal(pool[0], pool0[0]) and torch.equal(pool[2], pool0[2])
    for bad in (S, -1):                      # out of range: the row moves nothing in either direction
        pool, dense = pool0.clone(), torch.full((K, slots, 3, H, W), SENT, device=DEV)
        eng.window_gather(dense, pool, _i32([bad, 1]))
        torch.cuda.synchronize()
        assert bool((dense[0] == SENT).all()) and torch.equal(dense[1], pool0[1])
        eng.window_scatter(pool, new, _i32([bad, 2]))
        torch.cuda.synchronize()
        assert torch.equal(pool[2], new[1]) and all(torch.equal(pool[s], pool0[s]) for s in (0, 1, 3))
    with pytest.raises(RuntimeError, match="overlap"):
        eng.window_gather(pool0.view(-1)[slots * 3 * H * W:][:K * slots * 3 * H * W].view(K, slots, 3, H, W), pool0, _i32(rows))


# ------------------------------------------------------------------ 4. the schedule against the oracle
def _sched_pool():
    """S = 3 slots.  Calls 0-6: slot 0 runs clip 0 straight through; slot 1 runs clip 1 and is restarted on clip 2 at call 3;
    slot 2 runs clip 3, is idle at calls 2-3 and retired from call 6 -- active counts 3, 3, 2, 2, 3, 3, 2.  Two more calls reach
    the one-row plan: slot 1 pauses at call 7 (one active stream) and resumes at call 8."""
    rows = []
    for c in range(9):
        s1 = (1, c, c == 0) if c < 3 else (2, c - 3 - int(c > 7), c == 3)
        if c == 7:
            s1 = None
        s2 = (3, c, c == 0) if c < 2 else (None if c < 4 or c >= 6 else (3, c - 2, False))
        rows.append([(0, c, c == 0), s1, s2])
    return rows


def _run_compact(model, sched, clips, inputs, fill=0.0):
    """_run_schedule with the checks of an idle slot in every call: zero rows, windows bit for bit across the call."""
    model.fake_B_prev = None
    outs = []
    for row in sched:
        before = None if model.fake_B_prev is None else [p.clone() for p in model.fake_B_prev]
        fake, last = model.inference(*inputs(clips, row, fill), restart=[r is not None and r[2] for r in row],
                                     active=[r is not None for r in row])
        fp = model._active_plan
        assert fp.pool is not None and fp.B == sum(r is not None for r in row)
        for b, r in enumerate(row):
            if r is None:
                assert not fake[b].any() and not last[b].any()
                for si, p in enumerate(before or []):
                    assert torch.equal(model.fake_B_prev[si][b], p[b]), "idle slot %d: window %d changed" % (b, si)
        assert torch.isfinite(fake).all()
        outs.append((fake, [p.clone() for p in model.fake_B_prev]))
    return outs


def test_schedule_of_three_slots_matches_the_oracle_per_clip(golden):
    from oracle import vid2vid_oracle as O
    g = golden("inference_label2city_s1_32x64")
    clips = [_label_clip(600 + c, n=11) for c in range(4)]
    sched = _sched_pool()
    assert [sum(r is not None for r in row) for row in sched] == [3, 3, 2, 2, 3, 3, 2, 1, 2]
    sd = sd_from_npz(g, "sd0.")
    box = {}

    def reset():
        box["o"] = O.InferenceOracle([sd], 35, True, True, [26], 2, 2, 1)
    ref = _alone(lambda *a: box["o"].step(*a)[0], lambda: box["o"].fake_B_prev, reset, clips, sched, _label_inputs)
    model = _model(g, 1, compact_streams=True)
    outs = _run_compact(model, sched, clips, _label_inputs)
    assert sorted(k[7] for k in model._plans if k[-1] == ("pool", 3)) == [1, 2, 3]
    _check_schedule(outs, sched, ref, 1, 1e-3, "S=1 pool of 3 schedule")


def test_one_two_row_plan_on_changing_slot_pairs_matches_the_oracle(golden):
    """One K = 2 plan of S = 3 slots sees the rows [0, 1], [1, 2], [0, 2] and [0, 1] again: the non-identity row_slot of a
    plan with more than one row, every active slot at every call against the oracle stepped on its clip alone."""
    from oracle import vid2vid_oracle as O
    g = golden("inference_label2city_s1_32x64")
    clips = [_label_clip(740 + c) for c in range(3)]
    sched = [[(0, 0, True), (1, 0, True), None],
             [None, (1, 1, False), (2, 0, True)],
             [(0, 1, False), None, (2, 1, False)],
             [(0, 2, False), (1, 2, False), None]]
    sd = sd_from_npz(g, "sd0.")
    box = {}

    def reset():
        box["o"] = O.InferenceOracle([sd], 35, True, True, [26], 2, 2, 1)
    ref = _alone(lambda *a: box["o"].step(*a)[0], lambda: box["o"].fake_B_prev, reset, clips, sched, _label_inputs)
    model = _model(g, 1, compact_streams=True)
    outs = _run_compact(model, sched, clips, _label_inputs)
    assert [k[7] for k in model._plans if k[-1] == ("pool", 3)] == [2]
    _check_schedule(outs, sched, ref, 1, 1e-3, "S=1 pool of 3, one two-row plan")


# ------------------------------------------------------------------ 5. the paths off the fused head, against the batch-1 plan
def _against_batch_one(model, S, clips, inputs, what):
    sched = _sched2()

    def reset():
        model.fake_B_prev = None
    ref = _alone(lambda *a: model.inference(*a)[0], lambda: model.fake_B_prev, reset, clips, sched, inputs)
    outs = _run_compact(model, sched, clips, inputs)
    assert sorted(k[7] for k in model._plans if k[-1] == ("pool", 2)) == [1, 2]
    _check_schedule(outs, sched, ref, S, 2e-3, what)


def test_schedule_two_spatial_scales_matches_batch_one(golden):
    g = golden("inference_label2city_s2_32x64")
    clips = [None] + [_label_clip(620 + c) for c in range(3)]
    _against_batch_one(_model(g, 2, compact_streams=True), 2, clips, _label_inputs, "S=2 pool of 2 schedule")


def test_schedule_raw_inputs_matches_batch_one(golden):
    g = golden("inference_edge2face_s1_32x32")
    clips = [None] + [_raw_clip(640 + c) for c in range(3)]
    _against_batch_one(_raw_model(g, compact_streams=True), 1, clips, _raw_inputs, "raw pool of 2 schedule")


def test_no_first_img_restart_is_raw_only_for_that_slot_alone(golden):
    """The restarted row (row_mode 1) against this library's batch-1 raw-only plan at 2e-3, and bit for bit against the slot
    plan's row of the same call (one engine, one tile selection at N = 2).  The raw-only frame runs the image tower on an
    all-zero window: its first norm divides a constant plane by sqrt(0 + eps), which amplifies the rounding of the mean, so
    two lowerings of that frame agree only as far as their summation orders do.  The CPU oracle's frame is O(1) away from all
    of this library's (1.66 measured, pool, slot and batch-1 alike), which is why no oracle bar is set here."""
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1, use_real_img=False, no_first_img=True, compact_streams=True)
    clips = [_label_clip(660 + c) for c in range(3)]
    base = [[(0, c, c == 0), (1, c, c == 0)] for c in range(4)]
    with_restart = [list(r) for r in base]
    with_restart[3][1] = (2, 0, True)
    plain = _run_compact(model, base, clips, _label_inputs)
    outs = _run_compact(model, with_restart, clips, _label_inputs)
    assert model._active_plan.pool is not None and not model._active_plan.use_raw_only
    for c in range(4):      # slot 0 never sees what slot 1 does
        assert torch.equal(outs[c][0][0], plain[c][0][0]) and torch.equal(outs[c][1][0][0], plain[c][1][0][0]), c
    assert not torch.equal(outs[3][0][1], plain[3][0][1])
    model.fake_B_prev = None
    first, _ = model.inference(*_label_inputs(clips, [(2, 0, True)]))          # batch 1: the raw-only first-frame plan
    assert model._active_plan.use_raw_only and model._active_plan.B == 1 and model._active_plan.pool is None
    print("no_first_img restart: pool row %.2e against the batch-1 plan" % rel_err(outs[3][0][1:2].cpu(), first.cpu()))
    assert_close(outs[3][0][1:2], first, 2e-3, "restarted slot against the batch-1 raw-only first frame")
    assert_close(outs[3][1][0][1], model.fake_B_prev[0], 2e-3, "its window")
    assert not outs[3][1][0][1][0].any()                                         # oldest slot of a fresh window: zeros
    model.opt.compact_streams = False                # the slot plan of the same model: slot_mode 1 on the same launches in front
    slot = _run_schedule(model, with_restart, clips, _label_inputs)
    assert model._active_plan.slots and model._active_plan.pool is None
    for c in range(4):
        assert torch.equal(outs[c][0], slot[c][0]) and torch.equal(outs[c][1][0], slot[c][1][0]), c


# ------------------------------------------------------------------ 6. bit contracts at model level
def test_all_active_equals_the_slot_plan_and_one_active_the_batch_1_plan(golden):
    """One model, hence one engine and one tile selection per shape; the option is read per call."""
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1)
    clips = [_label_clip(700 + c) for c in range(3)]
    sched = [[(b, c, c == 0) for b in range(3)] for c in range(4)]
    slot = _run_schedule(model, sched, clips, _label_inputs)
    assert model._active_plan.slots and model._active_plan.pool is None
    model.opt.compact_streams = True
    pooled = _run_schedule(model, sched, clips, _label_inputs)
    assert model._active_plan.pool is not None and model._active_plan.B == 3
    for c in range(4):
        assert torch.equal(pooled[c][0], slot[c][0]), "frame %d" % c
        assert torch.equal(pooled[c][1][0], slot[c][1][0]), "window after frame %d" % c
    # one active stream: slot 1 runs clip 1 alone on the one-row plan; the batch-1 plain plan on that clip
    alone = [[None, (1, c, c == 0), None] for c in range(4)]
    pooled = _run_schedule(model, alone, clips, _label_inputs)
    assert model._active_plan.pool is not None and model._active_plan.B == 1
    model.fake_B_prev = None
    for c in range(4):
        fake, last = model.inference(*_label_inputs(clips, [(1, c, c == 0)]))
        assert model._active_plan.pool is None and model._active_plan.B == 1
        assert torch.equal(pooled[c][0][1:2], fake), "frame %d" % c
        assert torch.equal(pooled[c][1][0][1], model.fake_B_prev[0]), "window after frame %d" % c
        assert not pooled[c][0][0].any() and not pooled[c][0][2].any()


# ------------------------------------------------------------------ 7. isolation
@pytest.mark.parametrize("mode", ["label", "raw"])
def test_idle_rows_of_the_inputs_reach_nothing(golden, mode):
    if mode == "label":
        model = _model(golden("inference_label2city_s1_32x64"), 1, compact_streams=True)
        clips, inputs, garbage = [_label_clip(680 + c) for c in range(3)], _label_inputs, 255.0
    else:
        model = _raw_model(golden("inference_edge2face_s1_32x32"), compact_streams=True)
        clips, inputs, garbage = [_raw_clip(680 + c) for c in range(3)], _raw_inputs, float("nan")
    sched = [[(0, c, c == 0), (1, c, c == 0) if c < 2 or c == 4 else None, (2, c, c == 0) if c != 3 else None] for c in range(5)]
    sched[4][1] = (1, 2, False)                      # slot 1 pauses at calls 2-3 and resumes with its third frame
    sched[4][2] = (2, 3, False)                      # slot 2 pauses at call 3
    clean = _run_compact(model, sched, clips, inputs, 0.0)            # idle rows hold valid data (label 0 / zeros)
    dirty = _run_compact(model, sched, clips, inputs, garbage)        # idle rows hold label 255 / NaN
    for c in range(5):
        assert torch.equal(clean[c][0], dirty[c][0]) and torch.equal(clean[c][1][0], dirty[c][1][0]), "call %d" % c
    assert clean[4][0][1].any()


# ------------------------------------------------------------------ 8. interface
def test_no_active_stream_and_prepare_streams(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1, compact_streams=True)
    clips = [_label_clip(720 + c) for c in range(2)]
    two = lambda c: _label_inputs(clips, [(0, c, c == 0), (1, c, c == 0)])
    model.prepare_streams(2, 32, 64, 1, True, counts=[2])
    assert [k[7] for k in model._plans] == [2]
    z, zl = model.inference(*two(0), active=[])
    assert getattr(model, "fake_B_prev", None) is None and tuple(z.shape) == (2, 3, 32, 64) and tuple(zl.shape) == (2, 36, 32, 64)
    assert not z.any() and not zl.any()
    fa, la = model.inference(*two(0))
    assert [k[7] for k in model._plans] == [2] and fa.any()
    keep, windows = fa.clone(), [p.clone() for p in model.fake_B_prev]
    z, _ = model.inference(*two(1), active=[False, False])
    assert not z.any() and torch.equal(fa, keep) and all(torch.equal(p, q) for p, q in zip(model.fake_B_prev, windows))
    fb, lb = model.inference(*two(1), active=[1])
    assert fa.data_ptr() != fb.data_ptr() and la.data_ptr() != lb.data_ptr() and torch.equal(fa, keep)
    assert not fb[0].any() and fb[1].any() and torch.equal(model.fake_B_prev[0][1, -1], fb[1])
    assert torch.equal(model.fake_B_prev[0][0], windows[0][0]) and lb[1].any() and not lb[0].any()
