"""uint8 inputs at source size (opt.input_geometry) on the GPU.

Kernel level, bit exact: v2v_gather_frames_u8 against the numpy / torch restatement of tests/input_geometry_common.py (which the CPU
tests hold against Pillow) -- upscale and downscale with a vector tail, resize + crop, identity; flip on and off; 1, 3, 6, 15 and 32
channels; five entries over three source frames and two geometries with a repeated source frame and an entry out of range; a
sentinel shows that only the named frames are written.  The tables are read when a recorded launch runs.
Model level, bit exact: a toy pose model fed 45x100 frames with the option on against the same model fed gather(...) of them with
the option off -- one stream, two streams with two geometries, a slot plan with a restart and an idle stream, a pool, uint8 results."""
import pytest
import torch

from input_geometry_common import box, gather

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


def _engine():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    return N.get_engine(DEV)


def _i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _geo_rows(geoms):
    rows = []
    for g in geoms:
        x1, y1, _, _ = box(g)
        rows.append([g["new_size"][0], g["new_size"][1], x1, y1, int(g.get("flip", False)), 0, 0, 0])
    return rows


# ------------------------------------------------------------------ 1. the kernel against the restatement
# name -> (Hs, Ws, geometry without flip, (H, W))
CASES = {
    "up_down_tail": (37, 53, dict(new_size=(40, 24)), (24, 40)),               # rows 37 -> 24, columns 53 -> 40; 40 C is no multiple of 16
    "resize_crop": (90, 160, dict(new_size=(72, 40), crop_size=(64, 32), crop_pos=(5, 3)), (32, 64)),
    "identity": (24, 48, dict(new_size=(48, 24)), (24, 48)),
}
OUT_OF_RANGE = {1: [3, 4, 0, 0], 3: [0, 7, 0, 0], 6: [1, 4, 2, 0], 15: [-1, 4, 0, 0], 32: [0, -2, 1, 0]}


@pytest.mark.parametrize("Cc", [1, 3, 6, 15, 32])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_the_restatement(case, flip, Cc):
    eng = _engine()
    Hs, Ws, geom, (H, W) = CASES[case]
    g0 = dict(geom, flip=flip)
    g1 = dict(geom, flip=not flip)                                             # the second geometry: the same box, mirrored
    assert box(g0)[2:] == (W, H)
    F, D = 3, 7
    gen = torch.Generator().manual_seed(1000 * Cc + Hs + int(flip))
    src = torch.randint(0, 256, (F, Hs, Ws, Cc), generator=gen, dtype=torch.uint8).to(DEV)
    dst = torch.full((D, H, W, Cc), SENTINEL, dtype=torch.uint8, device=DEV)
    # five entries: source frame 1 twice, both geometries, and one entry out of range (aimed at frame 4, which must stay as it is)
    entries = [[0, 0, 0, 0], [1, 2, 1, 0], [1, 3, 0, 0], OUT_OF_RANGE[Cc], [2, 5, 1, 0]]
    eng.gather_frames_u8(src, dst, _i32(entries), _i32(_geo_rows([g0, g1])))
    torch.cuda.synchronize()
    want = {0: gather(src[0], g0), 2: gather(src[1], g1), 3: gather(src[1], g0), 5: gather(src[2], g1)}
    for d in range(D):
        if d in want:
            assert torch.equal(dst[d], want[d]), (case, flip, Cc, d)
        else:
            assert bool((dst[d] == SENTINEL).all()), (case, flip, Cc, d)
    assert not torch.equal(want[2], want[3])
    if case == "identity":                                                     # a copy, or its mirror image
        assert torch.equal(want[0], src[0].flip(1) if flip else src[0])
        assert torch.equal(dst[0], src[0].flip(1) if flip else src[0])


@pytest.mark.parametrize("Cc", [3, 4, 16])
def test_frames_at_odd_addresses(Cc):
    """Neither side 16-byte (nor 4-byte) aligned: the bytes in front of a row's first aligned vector and behind its last one."""
    eng = _engine()
    Hs, Ws, geom, (H, W) = CASES["up_down_tail"]
    geom = dict(geom, flip=True)
    gen = torch.Generator().manual_seed(Cc)
    for so, do in ((1, 3), (4, 8), (0, 13)):
        sbuf = torch.randint(0, 256, (2 * Hs * Ws * Cc + 32,), generator=gen, dtype=torch.uint8).to(DEV)
        dbuf = torch.full((3 * H * W * Cc + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
        src = sbuf[so:so + 2 * Hs * Ws * Cc].view(2, Hs, Ws, Cc)
        dst = dbuf[do:do + 3 * H * W * Cc].view(3, H, W, Cc)
        assert src.data_ptr() % 16 == so and dst.data_ptr() % 16 == do
        eng.gather_frames_u8(src, dst, _i32([[1, 0, 0, 0], [0, 2, 0, 0]]), _i32(_geo_rows([geom])))
        torch.cuda.synchronize()
        assert torch.equal(dst[0], gather(src[1], geom)) and torch.equal(dst[2], gather(src[0], geom)), (Cc, so, do)
        assert bool((dst[1] == SENTINEL).all()) and bool((dbuf[:do] == SENTINEL).all()) and bool((dbuf[do + dst.numel():] == SENTINEL).all())


def test_tables_are_read_when_the_recorded_launch_runs():
    from vid2vid_amd.engine import Plan
    from vid2vid_amd.lib import lib
    eng = _engine()
    Hs, Ws, geom, (H, W) = CASES["resize_crop"]
    gen = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (3, Hs, Ws, 6), generator=gen, dtype=torch.uint8).to(DEV)
    dst = torch.full((4, H, W, 6), SENTINEL, dtype=torch.uint8, device=DEV)
    entries, geoms = _i32([[0, 0, 0, 0], [1, 1, 0, 0]]), _i32(_geo_rows([geom]))
    plan = Plan()
    eng.plan = plan
    try:
        with plan:
            eng.gather_frames_u8(src, dst, entries, geoms)
    finally:
        eng.plan = None
    assert plan.num_ops == 1 and lib.v2v_plan_op_name(plan.h, 0) == b"gather_frames_u8"
    assert bool((dst == SENTINEL).all())                                       # recorded, not run
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(dst[0], gather(src[0], geom)) and torch.equal(dst[1], gather(src[1], geom)) and bool((dst[2:] == SENTINEL).all())
    other = dict(geom, crop_pos=(8, 7), flip=True)
    entries.copy_(_i32([[2, 3, 0, 0], [9, 9, 9, 0]]))
    geoms.copy_(_i32(_geo_rows([other])))
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(dst[3], gather(src[2], other)) and torch.equal(dst[0], gather(src[0], geom)) and bool((dst[2] == SENTINEL).all())
    # a geometry whose box does not lie inside the resized frame does nothing
    dst.fill_(SENTINEL)
    entries.copy_(_i32([[0, 0, 0, 0], [1, 1, 0, 0]]))
    for bad in ([72, 40, 9, 3, 0, 0, 0, 0], [72, 40, 5, 9, 0, 0, 0, 0], [72, 40, -1, 3, 0, 0, 0, 0], [0, 40, 0, 0, 0, 0, 0, 0],
                [72, 16385, 0, 0, 0, 0, 0, 0]):
        geoms.copy_(_i32([bad]))
        plan.run()
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all()), bad


def test_engine_argument_rules_and_resample_u8():
    from vid2vid_amd import visual
    eng = _engine()
    Hs, Ws, geom, (H, W) = CASES["resize_crop"]
    src = torch.randint(0, 256, (2, Hs, Ws, 6), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).to(DEV)
    dst = torch.zeros(2, H, W, 6, dtype=torch.uint8, device=DEV)
    ent, geo = _i32([[0, 0, 0, 0]]), _i32(_geo_rows([geom]))
    with pytest.raises(TypeError):
        eng.gather_frames_u8(src.float(), dst, ent, geo)
    for bad in (dict(dst=dst[..., :5]), dict(dst=torch.zeros(2, H, W, 3, dtype=torch.uint8, device=DEV)), dict(ent=ent.long()),
                dict(ent=ent[:, :3].contiguous()), dict(geo=geo[:, :7].contiguous()), dict(src=src.cpu())):
        a = dict(src=src, dst=dst, ent=ent, geo=geo)
        a.update(bad)
        with pytest.raises(ValueError):
            eng.gather_frames_u8(a["src"], a["dst"], a["ent"], a["geo"])
    with pytest.raises(RuntimeError, match="overlap"):
        eng.gather_frames_u8(dst, dst, ent, _i32(_geo_rows([dict(new_size=(W, H))])))
    eng.gather_frames_u8(src, dst, _i32([]).view(0, 4), geo)                   # E = 0: nothing is launched
    torch.cuda.synchronize()
    assert not dst.any()
    # the launch on its own: frames, and a label map (any bytes, one channel)
    for flip in (False, True):
        g = dict(geom, flip=flip)
        assert visual.geometry_size(g) == (H, W)
        assert torch.equal(visual.resample_u8(src, g), gather(src, g))
        labels = src[..., :1].contiguous() % 35
        out = torch.empty(2, H, W, 1, dtype=torch.uint8, device=DEV)
        assert visual.resample_u8(labels, g, out=out) is out and torch.equal(out, gather(labels, g))
    with pytest.raises(ValueError):
        visual.resample_u8(src.cpu(), geom)


# ------------------------------------------------------------------ 2. the model against itself on host-resized frames
HS, WS, H, W, TG, IN_CH, CALLS = 45, 100, 32, 64, 3, 6, 4
GEOMS = [dict(new_size=(72, 40), crop_size=(64, 32), crop_pos=(5, 3), flip=False),
         dict(new_size=(64, 32), crop_size=(0, 0), crop_pos=(0, 0), flip=True),
         dict(new_size=(100, 45), crop_size=(64, 32), crop_pos=(30, 13), flip=True)]


@pytest.fixture(scope="module")
def pose_model():
    """The toy pose model of tests/test_gpu_inputs_u8.py: one scale pair, 6 input channels with the DensePose table, 32x64."""
    from vid2vid_amd import networks as N
    from vid2vid_amd import visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    N.set_precision("fp32")
    torch.manual_seed(21)
    opt = make_opt(label_nc=0, input_nc=IN_CH, use_instance=False, fg=False, use_real_img=True, random_init_ok=True, ngf=8,
                   n_blocks=2, n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, loadSize=64, precision="fp32", gpu_ids=[0])
    model = create_model(opt)
    opt.autotune = False          # both runs pick the same tiles
    opt.frame_tune = 0
    opt.input_lut = visual.input_lut(IN_CH, densepose_part_channel=2).to(DEV)
    return model


def _clips(n, seed):
    """n clips: (source bytes (CALLS + TG - 1, HS, WS, IN_CH) on the device, first real frames (TG - 1, 3, H, W))."""
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (CALLS + TG - 1, HS, WS, IN_CH), generator=gen, dtype=torch.uint8).to(DEV),
             torch.rand(TG - 1, 3, H, W, generator=gen) * 2 - 1) for _ in range(n)]


def _sizes():
    for g in GEOMS:
        assert box(g)[2:] == (W, H), g


def _call_inputs(clips, call, geoms, on, whole, active, host=False):
    """input_A of one call: every stream's frames call .. call + TG - 1 (whole) or the newest alone; on: at source size, else
    gather(...) of them under the stream's geometry.  An idle stream's rows, and with `whole` the older frames of a stream that is
    not in `whole`, are 0xAA on both sides: they must not be read."""
    rows = []
    for b, (frames, _) in enumerate(clips):
        x = frames[call:call + TG] if whole else frames[call + TG - 1:call + TG]
        x = x if on else gather(x, geoms[b])
        x = x.clone()
        if not active[b]:
            x.fill_(0xAA)
        elif whole and b not in whole:
            x[:TG - 1].fill_(0xAA)
        rows.append(x)
    A = torch.stack(rows)
    return A.cpu() if host else A


def _run(model, clips, geoms, on, sched, host=False, watch=None, **opts):
    """sched: per call (restart list or None, active list or None).  [(first, second, [windows])] per call."""
    opt = model.opt
    B = len(clips)
    model.fake_B_prev = None
    opt.inputs_u8 = opt.inputs_u8_slots = True
    if isinstance(geoms, dict):                                                # one geometry for every stream
        opt.input_geometry, geoms = (geoms if on else None), [geoms] * B
    else:
        opt.input_geometry = (geoms[:B] if B > 1 else geoms[0]) if on else None
    for k, v in opts.items():
        setattr(opt, k, v)
    outs = []
    try:
        for call, (restart, active) in enumerate(sched):
            act = [True] * B if active is None else [b in active for b in range(B)]
            starting = list(range(B)) if call == 0 else (restart or [])
            A = _call_inputs(clips, call, geoms, on, starting, act, host)
            Bf = torch.stack([c[1] for c in clips]) if starting else None
            kw = {}
            if restart is not None or active is not None:
                kw = dict(restart=restart or [], active=[b for b in range(B) if act[b]])
            before = None if model._active_plan is None or call == 0 else model._active_plan.win_u8.clone()
            first, second = model.inference(A, Bf, None, **kw)
            outs.append((first, second, [p.clone() for p in model.fake_B_prev], act))
            if watch is not None:
                watch(call, act, before, model._active_plan)
    finally:
        opt.inputs_u8 = opt.inputs_u8_slots = False
        opt.input_geometry = None
        for k in opts:
            setattr(opt, k, False)
    return outs


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for call, ((f, l, w, act), (rf, rl, rw, _)) in enumerate(zip(got, want)):
        assert f.dtype == rf.dtype and f.shape == rf.shape and l.dtype == rl.dtype and l.shape == rl.shape, (what, call)
        if all(act):
            assert torch.equal(f, rf), "%s call %d: first result" % (what, call)
            assert torch.equal(l, rl), "%s call %d: second result" % (what, call)
            for si, (a, b) in enumerate(zip(w, rw)):
                assert torch.equal(a, b), "%s call %d: fake_B_prev[%d]" % (what, call, si)
            continue
        for b, on in enumerate(act):
            if not on:
                assert not f[b].any(), "%s call %d: idle stream %d" % (what, call, b)
                continue
            assert torch.equal(f[b], rf[b]), "%s call %d stream %d: first result" % (what, call, b)
            assert torch.equal(l[b], rl[b]), "%s call %d stream %d: second result" % (what, call, b)
            for si in range(len(w)):
                assert torch.equal(w[si][b], rw[si][b]), "%s call %d stream %d: fake_B_prev[%d]" % (what, call, b, si)


PLAIN = [(None, None)] * CALLS


def test_one_stream(pose_model):
    _sizes()
    clips = _clips(1, seed=31)
    want = _run(pose_model, clips, GEOMS, False, PLAIN)
    got = _run(pose_model, clips, GEOMS, True, PLAIN)
    fp = pose_model._active_plan
    assert tuple(fp.win_u8.shape) == (1, TG, H, W, IN_CH) and (fp.H, fp.W) == (H, W) and fp.gather_last[0].shape[0] == 1
    assert tuple(got[0][0].shape) == (1, 3, H, W) and tuple(got[0][1].shape) == (IN_CH, H, W)
    _assert_equal(got, want, "B = 1")
    assert not torch.equal(got[0][0], got[1][0]) and torch.isfinite(got[-1][0]).all()
    # the window holds the resized frames, moved on by the plan as with the option off
    assert torch.equal(fp.win_u8[0, TG - 1], gather(clips[0][0][CALLS + TG - 2], GEOMS[0]))
    # frames in host memory go the same way
    _assert_equal(_run(pose_model, clips, GEOMS, True, PLAIN, host=True), want, "B = 1, host frames")
    # another geometry of the same size gives other frames
    other = _run(pose_model, clips, GEOMS[1:], True, PLAIN[:1])
    assert not torch.equal(other[0][0], got[0][0])


def test_two_streams_with_two_geometries(pose_model):
    clips = _clips(2, seed=32)
    want = _run(pose_model, clips, GEOMS, False, PLAIN)
    got = _run(pose_model, clips, GEOMS, True, PLAIN)
    fp = pose_model._active_plan
    assert fp.B == 2 and not fp.slots and fp.pool is None and tuple(fp.gather_last[1].shape) == (2, 8)
    _assert_equal(got, want, "B = 2")
    # one dict serves every stream
    want1 = _run(pose_model, clips, GEOMS[2], False, PLAIN[:2])
    got1 = _run(pose_model, clips, GEOMS[2], True, PLAIN[:2])
    assert tuple(pose_model._active_plan.gather_last[1].shape) == (1, 8)
    _assert_equal(got1, want1, "B = 2, one geometry")


def test_slot_plan_with_a_restart_and_an_idle_stream(pose_model):
    clips = _clips(2, seed=33)
    sched = [([], None), ([], None), ([1], None), ([], [1])]                   # restart=[1] on frame 2, stream 0 idle on frame 3
    seen = {}

    def watch(call, act, before, fp):
        assert fp.slots and fp.win_u8 is not None
        if call == 3:
            assert torch.equal(fp.win_u8[0], before[0]) and not torch.equal(fp.win_u8[1], before[1])
            seen["entries"] = fp.gather_last[0].tolist()
        if call == 2:
            seen["restart"] = fp.gather_last[0].tolist()

    want = _run(pose_model, clips, GEOMS, False, sched)
    got = _run(pose_model, clips, GEOMS, True, sched, watch=watch)
    _assert_equal(got, want, "slot plan")
    assert seen["restart"] == [[2, 2, 0, 0], [3, 3, 1, 0], [4, 4, 1, 0], [5, 5, 1, 0]]      # tG + 1 entries
    assert seen["entries"] == [[1, 5, 1, 0]]                                   # t = 1, nothing for the idle stream


def test_pool_of_three_slots_with_two_active_streams(pose_model):
    clips = _clips(3, seed=34)
    sched = [([], [0, 2])] * CALLS
    want = _run(pose_model, clips, GEOMS, False, sched, compact_streams=True)
    seen = []
    got = _run(pose_model, clips, GEOMS, True, sched, compact_streams=True,
               watch=lambda call, act, before, fp: seen.append((fp.pool is not None, fp.B, tuple(fp.win_u8.shape), fp.gather_last[0].tolist())))
    assert all(s[:3] == (True, 2, (3, TG, H, W, IN_CH)) for s in seen)
    assert seen[0][3] == [[f, f, f // TG, 0] for f in (0, 1, 2, 6, 7, 8)] and seen[1][3] == [[0, 2, 0, 0], [2, 8, 2, 0]]
    _assert_equal(got, want, "pool")
    assert tuple(got[0][0].shape) == (3, 3, H, W)


def test_uint8_in_at_source_size_and_uint8_out(pose_model):
    clips = _clips(2, seed=35)
    want = _run(pose_model, clips, GEOMS, False, PLAIN[:3], frames_u8=True, real_A_u8=True)
    got = _run(pose_model, clips, GEOMS, True, PLAIN[:3], frames_u8=True, real_A_u8=True)
    assert got[0][0].dtype == torch.uint8 and tuple(got[0][0].shape) == (2, H, W, 3)
    assert got[0][1].dtype == torch.uint8 and tuple(got[0][1].shape) == (2, H, W, 1)
    _assert_equal(got, want, "uint8 out")
    assert got[0][0].any() and got[0][1].any()
