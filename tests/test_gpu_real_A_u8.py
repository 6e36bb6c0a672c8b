"""real_A as a uint8 picture written inside the frame plan (opt.real_A_u8) on the GPU.

Kernel level, bit exact: v2v_label_image against the torch restatement of encode_input + get_edges + tensor2label
(tests/real_A_u8_common.py) and against visual.tensor2label of the planes Engine.onehot_planar writes, on caller-owned buffers
pre-filled with 0xAB (what a launch leaves unwritten is seen).  Shapes: 5x7 (runs of 4 pixels with a tail of 3; rows shorter than
a 16-pixel run), 3x16 (exactly one whole 16-pixel run per row), 32x64 (aligned whole runs: the 16-byte stores), 9x130 (rows that
end in a run of 2 pixels and start at every alignment: the dword path with leading and trailing single bytes).  The grid is
capped at 256 workgroups of 256 runs per image, so the grid-stride loop takes a second pass only from 65537 runs on: 1030x1024
(65920 runs) is that case, checked with 7 labels so that its planes stay small.
Model level: a model with the option against a model on the same weights without it, on the same inputs -- the second result is
tensor2label of the other model's real_A_last per stream, the first result and the windows are equal bit for bit; plain plans
on the fused head and on the generic body (two spatial scales), slot and pool plans, an image model, the option flipped inside
a running sequence."""
import ctypes as C

import pytest
import torch

from real_A_u8_common import picture, planted_maps
from test_gpu_stream_slots import _model, _label_clip, _label_inputs
from test_gpu_inputs_u8 import _edge2face, _u8_stream, _decoded, _raw_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xAB


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _cmap(label_nc):
    from vid2vid_amd.visual import labelcolormap
    return torch.from_numpy(labelcolormap(label_nc)[:label_nc].copy()).to(DEV)


def _raw(lab, inst, cmap, label_nc, out, mode, rows, K, S, T, H, W):
    from vid2vid_amd import lib as L
    rc = L.lib.v2v_label_image(_p(lab), _p(inst), int(lab.dtype == torch.uint8), _p(cmap), label_nc, _p(out), _p(mode), _p(rows),
                               K, S, T, H, W, None)
    torch.cuda.synchronize()
    return rc


def _convert(lab, inst, label_nc, mode=None, rows=None, S=None):
    K, T, H, W = lab.shape
    S = K if S is None else S
    out = torch.full((S, H, W, 3), FILL, dtype=torch.uint8, device=DEV)
    assert _raw(lab, inst, _cmap(label_nc), label_nc, out, mode, rows, K, S, T, H, W) == 0
    return out


def _engine():
    from vid2vid_amd import networks as N
    return N.get_engine(torch.device(DEV))


def _by_planes(eng, lab, inst, label_nc):
    """visual.tensor2label of the planes onehot_planar makes of one (H, W) frame on the device."""
    from vid2vid_amd import visual
    H, W = lab.shape
    return visual.tensor2label(eng.onehot_planar(lab.contiguous(), None if inst is None else inst.contiguous(), H, W, label_nc), label_nc)


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("HW", [(5, 7), (3, 16), (32, 64), (9, 130)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("label_nc", [35, 20, 7])
@pytest.mark.parametrize("fp32_maps", [False, True], ids=["u8_i32", "fp32"])
@pytest.mark.parametrize("NT", [(1, 1), (3, 3)], ids=lambda s: "N%dT%d" % s)
def test_kernel_equals_the_restatement_and_tensor2label_of_the_planes(HW, label_nc, fp32_maps, NT):
    (H, W), (N, T) = HW, NT
    eng = _engine()
    lab, inst = planted_maps(N, T, H, W, label_nc, seed=H * W + label_nc + N)
    if H * W >= 1024:
        assert sorted(set(lab[0, T - 1].view(-1).tolist())) == list(range(256))          # every byte value is there
    want = {with_inst: torch.stack([picture(lab[n, T - 1], inst[n, T - 1] if with_inst else None, label_nc) for n in range(N)])
            for with_inst in (True, False)}
    if _cmap(label_nc)[0].any():     # (colour 0 of the 35- and 7-label palettes is black, as an edge pixel without a plane is)
        assert not torch.equal(want[True], want[False])          # the edge plane decides some pixel
    if T > 1:
        assert not torch.equal(want[True][0], picture(lab[0, 0], inst[0, 0], label_nc))         # a wrong frame index would show
    dlab = (lab.float() if fp32_maps else lab).to(DEV)
    dinst = (inst.float() if fp32_maps else inst).to(DEV)
    for with_inst in (True, False):
        got = _convert(dlab, dinst if with_inst else None, label_nc)
        assert torch.equal(got.cpu(), want[with_inst]), "inst %s" % with_inst
        for n in range(N):
            planes = _by_planes(eng, dlab[n, T - 1], dinst[n, T - 1] if with_inst else None, label_nc)
            assert torch.equal(got[n], planes), (n, with_inst)


def test_kernel_at_odd_output_alignment():
    """out one byte into its buffer: the runs of every row start off a dword; the bytes around the images are not touched."""
    H, W, label_nc = 9, 130, 20
    lab, inst = planted_maps(2, 1, H, W, label_nc, seed=11)
    want = torch.stack([picture(lab[n, 0], inst[n, 0], label_nc) for n in range(2)])
    for off in (1, 2, 3):
        buf = torch.full((2 * H * W * 3 + 8,), FILL, dtype=torch.uint8, device=DEV)
        out = buf[off:off + 2 * H * W * 3]
        assert _raw(lab.to(DEV), inst.to(DEV), _cmap(label_nc), label_nc, out, None, None, 2, 2, 1, H, W) == 0
        assert torch.equal(out.view(2, H, W, 3).cpu(), want), off
        assert bool((buf[:off] == FILL).all()) and bool((buf[off + 2 * H * W * 3:] == FILL).all())


def test_kernel_second_pass_of_the_capped_grid():
    """1030 x 1024: 65920 runs of 16 pixels for a grid capped at 256 x 256 threads -- 384 threads take a second run."""
    from vid2vid_amd import visual
    H, W, label_nc = 1030, 1024, 7
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 10, (1, 1, H, W), generator=g, dtype=torch.uint8)         # 7, 8, 9: no plane
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inst = ((yy // 7) * 1000 + xx // 9).to(torch.int32)[None, None]
    want = picture(lab[0, 0], inst[0, 0], label_nc)
    got = _convert(lab.to(DEV), inst.to(DEV), label_nc)
    assert torch.equal(got[0].cpu(), want)
    assert torch.equal(got[0], _by_planes(_engine(), lab[0, 0].to(DEV), inst[0, 0].to(DEV), label_nc))
    assert got[0, H - 1].any() and want[H - 6:].any()


def test_single_plane_colours_the_stored_value():
    """label_nc == 1 without an instance map: tensor2label gets ONE plane and colours its value, not an argmax."""
    lab = torch.tensor([[0, 1, 0, 255, 0, 3, 0]] * 5, dtype=torch.uint8)[None, None]
    got = _convert(lab.to(DEV), None, 1)
    assert torch.equal(got[0], _by_planes(_engine(), lab[0, 0].to(DEV), None, 1))
    inst = torch.arange(35, dtype=torch.int32).view(1, 1, 5, 7)
    got = _convert(lab.to(DEV), inst.to(DEV), 1)
    assert torch.equal(got[0], _by_planes(_engine(), lab[0, 0].to(DEV), inst[0, 0].to(DEV), 1))
    assert torch.equal(got[0].cpu(), picture(lab[0, 0], inst[0, 0], 1))


@pytest.mark.parametrize("HW", [(9, 130), (5, 7)], ids=lambda s: "%dx%d" % s)
def test_rows_slots_modes_and_complete_write(HW):
    H, W = HW
    label_nc, T = 35, 2
    lab, inst = planted_maps(4, T, H, W, label_nc, seed=9)
    pics = torch.stack([picture(lab[n, T - 1], inst[n, T - 1], label_nc) for n in range(4)])
    zero = torch.zeros(H, W, 3, dtype=torch.uint8)
    dlab, dinst = lab.to(DEV), inst.to(DEV)
    # modes of a slot plan: row 1 idle, row 3 an unknown word -> zero bytes, the others their pictures (mode 1 like mode 0)
    got = _convert(dlab, dinst, label_nc, mode=_i32([0, 2, 1, 7])).cpu()
    assert torch.equal(got[0], pics[0]) and torch.equal(got[2], pics[2])
    assert torch.equal(got[1], zero) and torch.equal(got[3], zero)
    # K = 2 rows of S = 4 images: rows 0, 1 -> images 3, 1; the images no row names are written as zeros
    got = _convert(dlab[:2].contiguous(), dinst[:2].contiguous(), label_nc, mode=_i32([0, 1]), rows=_i32([3, 1]), S=4).cpu()
    assert torch.equal(got[3], pics[0]) and torch.equal(got[1], pics[1]) and torch.equal(got[0], zero) and torch.equal(got[2], zero)
    # an idle row's slot is zero too; without mode words every row is live
    got = _convert(dlab[:2].contiguous(), dinst[:2].contiguous(), label_nc, mode=_i32([2, 0]), rows=_i32([0, 2]), S=4).cpu()
    assert torch.equal(got[2], pics[1]) and not got[0].any() and not got[1].any() and not got[3].any()
    got = _convert(dlab[:2].contiguous(), dinst[:2].contiguous(), label_nc, rows=_i32([2, 0]), S=3).cpu()
    assert torch.equal(got[2], pics[0]) and torch.equal(got[0], pics[1]) and not got[1].any()


def test_argument_errors_leave_out_untouched():
    from vid2vid_amd import lib as L
    K, S, T, H, W, nc = 2, 4, 2, 4, 8, 35
    lab = torch.zeros(K, T, H, W, dtype=torch.uint8, device=DEV)
    inst = torch.zeros(K, T, H, W, dtype=torch.int32, device=DEV)
    labf, instf = torch.zeros(K * T * H * W + 1, device=DEV), torch.zeros(K * T * H * W + 1, device=DEV)
    cmap = _cmap(nc)
    out = torch.full((S, H, W, 3), FILL, dtype=torch.uint8, device=DEV)
    words = _i32([3, 1, 0])
    EINVAL = L.lib.v2v_tensor2im(None, None, 1, 1, 1, 1, None)
    assert EINVAL != 0

    def call(lab_=lab, inst_=inst, cmap_=cmap, nc_=nc, out_=out, mode=words[:2], rows=words[:2], K_=K, S_=S, T_=T, H_=H, W_=W):
        return _raw(lab_, inst_, cmap_, nc_, out_, mode, rows, K_, S_, T_, H_, W_)
    odd = lambda t: t.view(-1).view(torch.uint8)[1:]             # a byte view one byte off: a misaligned pointer
    for kw in (dict(cmap_=None), dict(out_=None), dict(nc_=0), dict(nc_=256), dict(K_=0), dict(S_=K - 1), dict(T_=0), dict(H_=0),
               dict(W_=0), dict(rows=None), dict(rows=None, mode=None), dict(inst_=odd(inst)), dict(mode=odd(words)),
               dict(rows=odd(words))):
        assert call(**kw) == EINVAL, kw
        assert b"label_image" in L.lib.v2v_last_error()
        assert bool((out == FILL).all()), kw
    label_image = L.lib.v2v_label_image
    assert label_image(None, _p(inst), 1, _p(cmap), nc, _p(out), None, None, S, S, T, H, W, None) == EINVAL
    # fp32 maps two bytes off
    assert label_image(C.c_void_p(labf.data_ptr() + 2), None, 0, _p(cmap), nc, _p(out), None, None, 1, 1, 1, H, W, None) == EINVAL
    assert label_image(_p(labf), C.c_void_p(instf.data_ptr() + 2), 0, _p(cmap), nc, _p(out), None, None, 1, 1, 1, H, W, None) == EINVAL
    assert label_image(_p(labf), _p(instf), 0, _p(cmap), nc, _p(out), None, None, 1, 1, 1, H, W, None) == 0       # aligned: accepted
    torch.cuda.synchronize()
    assert not bool((out[0] == FILL).any()) and bool((out[1:] == FILL).all())
    out.fill_(FILL)
    # out over the labels (one buffer): refused, nothing written; adjacent is fine
    n_in = K * T * H * W
    both = torch.full((n_in + S * H * W * 3,), FILL, dtype=torch.uint8, device=DEV)
    for off in (0, n_in - 1):
        assert call(lab_=both[:n_in], out_=both[off:]) == EINVAL and b"overlap" in L.lib.v2v_last_error()
        assert bool((both == FILL).all())
    assert call(lab_=both[:n_in], out_=both[n_in:]) == 0
    assert bool((both[:n_in] == FILL).all()) and not bool((both[n_in:] == FILL).all())
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


# ------------------------------------------------------------------ 2. the model
def _pair(golden, precision, S=1, **kw):
    """Two models on the same weights: opt.real_A_u8 off and on."""
    g = golden("inference_label2city_s%d_32x64" % S)
    return _model(g, S, precision, **kw), _model(g, S, precision, real_A_u8=True, **kw)


def _step_both(off, on, inputs, row, frames_u8=False, **kw):
    """One call of both models on the same inputs; the contract of the option."""
    from vid2vid_amd import visual
    first_off, last = off.inference(*inputs, **kw)
    first_on, pic = on.inference(*inputs, **kw)
    nB = len(row)
    H, W = last.shape[-2:]
    last = last.view(nB, -1, H, W)
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (nB, H, W, 3) and pic.is_contiguous()
    for b, r in enumerate(row):
        if r is None:
            assert not pic[b].any(), "idle stream %d" % b
        else:
            assert torch.equal(pic[b], visual.tensor2label(last[b], on.opt.label_nc)), "stream %d" % b
            A, I = inputs[0][b, -1, 0], inputs[2][b, -1, 0]
            assert torch.equal(pic[b].cpu(), picture(A, I, on.opt.label_nc)), "stream %d against its own label map" % b
            assert pic[b].any()
    assert first_on.dtype == first_off.dtype == (torch.uint8 if frames_u8 else torch.float32)
    assert torch.equal(first_on, first_off)
    assert len(on.fake_B_prev) == len(off.fake_B_prev)
    for w_on, w_off in zip(on.fake_B_prev, off.fake_B_prev):
        assert torch.equal(w_on, w_off)
    return pic


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 2], ids=["fused_head", "generic_s2"])
@pytest.mark.parametrize("frames_u8", [False, True], ids=["fp32_frames", "frames_u8"])
def test_plain_plans_return_the_picture_of_real_A_last(golden, precision, B, S, frames_u8):
    off, on = _pair(golden, precision, S, frames_u8=frames_u8)
    clips = [_label_clip(800 + c) for c in range(B)]
    kept = []
    for t in range(4):
        row = [(b, t, t == 0) for b in range(B)]
        pic = _step_both(off, on, _label_inputs(clips, row), row, frames_u8)
        for earlier, copy in kept:                   # returned pictures do not alias the plan's buffer or each other
            assert torch.equal(earlier, copy)
        kept.append((pic, pic.clone()))
    fp = on._active_plan
    assert fp.real_A_u8 and not fp.slots and fp.pool is None and fp.B == B and not off._active_plan.real_A_u8
    assert "real_A_last" not in fp.out and not torch.equal(kept[0][0], kept[1][0])


def test_uint8_labels_in_and_bytes_out(golden):
    """The serving call: uint8 labels and int32 ids in, both results uint8 -- equal to the fp32-encoded call's."""
    off, on = _pair(golden, "bf16", frames_u8=True)
    clips = [_label_clip(820 + c) for c in range(2)]
    for t in range(3):
        row = [(b, t, t == 0) for b in range(2)]
        A, Bf, I = _label_inputs(clips, row)
        image_off, last = off.inference(A, Bf, I)
        image, pic = on.inference(A.to(torch.uint8), Bf, I.to(torch.int32))
        assert image.dtype == pic.dtype == torch.uint8 and torch.equal(image, image_off)
        for b in range(2):
            assert torch.equal(pic[b].cpu(), picture(A[b, -1, 0], I[b, -1, 0], 35))
    assert on._active_plan.labels.dtype == torch.uint8 and on._active_plan.inst.dtype == torch.int32


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_slot_schedule_idle_pictures_are_zero(golden, precision):
    """B = 3: stream 1 idles for two calls and is then restarted on another clip; the idle rows hold label 255 everywhere."""
    off, on = _pair(golden, precision)
    clips = [_label_clip(840 + c) for c in range(4)]
    sched = [[(0, 0, True), (1, 0, True), (2, 0, True)],
             [(0, 1, False), None, (2, 1, False)],
             [(0, 2, False), None, (2, 2, False)],
             [(0, 3, False), (3, 0, True), (2, 3, False)]]
    for row in sched:
        _step_both(off, on, _label_inputs(clips, row, fill=255.0), row,
                   restart=[r is not None and r[2] for r in row], active=[r is not None for r in row])
    assert on._active_plan.slots and on._active_plan.real_A_u8


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("frames_u8", [False, True], ids=["fp32_frames", "frames_u8"])
def test_pool_schedule_delivers_all_slots(golden, precision, frames_u8):
    """S = 3 slots with 3, 1 and 2 of them live: the K-row plans write all S pictures, idle ones zero."""
    off, on = _pair(golden, precision, compact_streams=True, frames_u8=frames_u8)
    clips = [_label_clip(860 + c) for c in range(3)]
    sched = [[(0, 0, True), (1, 0, True), (2, 0, True)],
             [None, (1, 1, False), None],
             [(0, 1, False), None, (2, 1, False)]]
    for row, K in zip(sched, (3, 1, 2)):
        _step_both(off, on, _label_inputs(clips, row, fill=255.0), row, frames_u8,
                   restart=[r is not None and r[2] for r in row], active=[r is not None for r in row])
        fp = on._active_plan
        assert fp.pool is not None and fp.pool.S == 3 and fp.B == K and fp.real_A_u8
        assert tuple(fp.out["real_A_image"].shape) == (3, 32, 64, 3) and "real_A_last" not in fp.out
    first, pic = on.inference(*_label_inputs(clips, sched[0]), active=[])          # nothing live: zeros, no replay
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (3, 32, 64, 3) and not pic.any() and not first.any()
    first, pic = _model(golden("inference_label2city_s1_32x64"), 1, precision, real_A_u8=True).inference(
        *_label_inputs(clips, [(0, 0, True)]), active=[False])
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (1, 32, 64, 3) and not pic.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_image_model_converts_its_first_plane(golden, precision, B):
    """edge2face, 15 input channels: the picture is tensor2im(real_A_last[b][:1], normalize=False), from fp32 and uint8 inputs."""
    from vid2vid_amd import visual
    model = _edge2face(golden, precision)
    streams = [_u8_stream(880 + b) for b in range(B)]
    decoded = _decoded(streams, visual.input_lut(15))
    for u8 in (False, True):
        src = streams if u8 else decoded
        runs = {}
        for pic_on in (False, True):
            model.fake_B_prev = None
            model.opt.inputs_u8, model.opt.real_A_u8 = u8, pic_on
            outs = []
            for t in range(3):
                A, Bf, _ = _raw_inputs(src, t)
                if u8 and t > 0:
                    A = A[:, 2:]
                first, second = model.inference(A, Bf, None)
                outs.append((first, second, [p.clone() for p in model.fake_B_prev]))
            runs[pic_on] = outs
        model.opt.inputs_u8 = model.opt.real_A_u8 = False
        for t, ((f0, last, w0), (f1, pic, w1)) in enumerate(zip(runs[False], runs[True])):
            assert torch.equal(f0, f1) and all(torch.equal(a, b) for a, b in zip(w0, w1)), (u8, t)
            assert pic.dtype == torch.uint8 and tuple(pic.shape) == (B, 32, 32, 1)
            last = last.view(B, 15, 32, 32)
            for b in range(B):
                assert torch.equal(pic[b, ..., 0], visual.tensor2im(last[b][:1], normalize=False)), (u8, t, b)
            assert pic.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_option_flipped_inside_a_running_sequence(golden, precision):
    from vid2vid_amd import visual
    off, flip = _pair(golden, precision)
    flip.opt.real_A_u8 = False
    clips = [_label_clip(900 + c) for c in range(2)]
    for t in range(4):
        row = [(b, t, t == 0) for b in range(2)]
        inputs = _label_inputs(clips, row)
        fake, last = off.inference(*inputs)
        got, second = flip.inference(*inputs)
        assert torch.equal(got, fake), t
        if flip.opt.real_A_u8:
            assert second.dtype == torch.uint8
            for b in range(2):
                assert torch.equal(second[b], visual.tensor2label(last[b], 35)), (t, b)
        else:
            assert torch.equal(second, last)
        assert torch.equal(flip.fake_B_prev[0], off.fake_B_prev[0]), t
        flip.opt.real_A_u8 = t in (0, 1)             # on for frames 1 and 2, off again for frame 3: the windows are carried
    assert len(flip._plans) == 2
