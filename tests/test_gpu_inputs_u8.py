"""uint8 image inputs for label_nc == 0 models (opt.inputs_u8) on the GPU.

Kernel level, bit exact: v2v_image_prologue against the composition of existing ops on the torch-decoded planes -- Engine.pack for
the stem input (pad channels included), the decoded newest frame, Engine.frame_prologue's window part, the window advance.
Model level, bit exact: a model fed uint8 HWC frames (the whole window on the first call, the newest frame alone afterwards)
against the same model's fp32 path on the decoded inputs, tile searches off so both plans run the same tiles; and every stream
against the CPU oracle stepped on its decoded inputs alone at the project's 1e-3 per-pixel bar.  The interface's refusals."""
import pytest
import torch

from util import sd_from_npz
from test_gpu_multi_stream import _model, _oracle_frames, _check_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = 5


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


def _engine(precision):
    from vid2vid_amd import networks as N
    N.set_precision(precision)
    return N.get_engine(DEV)


# ------------------------------------------------------------------ 1. the kernel against existing ops
SHAPES = [(1, 3, 5, 37, 15), (1, 3, 32, 32, 15), (3, 3, 3, 64, 6), (2, 2, 8, 130, 1)]


def _bytes(shape, kind, seed):
    N_, T, H, W, Cin = shape
    if kind == "random":
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    # every byte value in every channel: value (i + 7 c) mod 256 at flat (n, t, y, x) position i; H W T N >= 256 for every shape
    n = N_ * T * H * W
    assert n >= 256
    i = torch.arange(n).view(n, 1) + 7 * torch.arange(Cin).view(1, Cin)
    x = (i % 256).to(torch.uint8).view(shape)
    for c in range(Cin):
        assert len(torch.unique(x[..., c])) == 256
    return x


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["random", "every_byte"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_pack_of_the_decoded_planes(shape, kind, precision):
    from vid2vid_amd import visual
    from vid2vid_amd.engine import LabelSource
    eng = _engine(precision)
    N_, T, H, W, Cin = shape
    g = torch.Generator().manual_seed(sum(shape))
    lut = torch.randn(Cin, 256, generator=g).to(DEV)              # random: a wrong channel -> table mapping shows
    win0 = _bytes(shape, kind, seed=11 + sum(shape)).to(DEV)
    window = torch.randn(N_, 6, H, W, generator=g).to(DEV)
    planes = visual.decode_inputs(win0, lut)                      # (N, T, Cin, H, W)
    assert tuple(planes.shape) == (N_, T, Cin, H, W)
    assert torch.equal(planes[0, T - 1, Cin - 1, H - 1, W - 1], lut[Cin - 1, int(win0[0, T - 1, H - 1, W - 1, Cin - 1])])
    want_x0 = eng.pack(planes.reshape(N_, T * Cin, H, W).contiguous())
    from vid2vid_amd.engine import Act
    want_last_frame = eng.unpack(Act(want_x0.t[..., (T - 1) * Cin:], Cin))
    assert torch.equal(want_last_frame, planes[:, T - 1] if precision == "fp32" else planes[:, T - 1].bfloat16().float())
    lab = torch.zeros(N_, 1, H, W, dtype=torch.uint8, device=DEV)
    _, _, want_packed, want_last = eng.frame_prologue(LabelSource(lab if N_ > 1 else lab[0], None, 1, 35), H, W, (), False,
                                                      window=window, last_C=3)
    assert torch.equal(want_packed.t, eng.pack(window).t) and torch.equal(want_last, window[:, -3:])

    def check(x0, real_last, what):
        assert x0.C == T * Cin and tuple(x0.t.shape) == tuple(want_x0.t.shape) and x0.t.dtype == want_x0.t.dtype, what
        assert torch.equal(x0.t.view(torch.uint8), want_x0.t.view(torch.uint8)), what      # bytes, pad channels included
        assert not x0.t[..., T * Cin:].any(), what
        # the newest frame as the stem input holds it: the existing unpack of those channels (the decoded values; bf16-rounded in
        # a bf16 engine, which is what the fp32-input plan returns as real_A_last)
        assert torch.equal(real_last, want_last_frame), what
        if precision == "fp32":
            assert torch.equal(real_last, planes[:, T - 1]), what

    # with the generated-frame window, advancing
    win = win0.clone()
    x0, real_last, packed, last = eng.image_prologue(win, lut, window=window, last_C=3)
    check(x0, real_last, "window + advance")
    assert torch.equal(packed.t.view(torch.uint8), want_packed.t.view(torch.uint8)) and torch.equal(last, want_last)
    assert torch.equal(win[:, :T - 1], win0[:, 1:]) and torch.equal(win[:, T - 1], win0[:, T - 1])
    # advance=False: the window is not written
    win = win0.clone()
    x0, real_last, packed, last = eng.image_prologue(win, lut, window=window, last_C=3, advance=False)
    check(x0, real_last, "window, no advance")
    assert torch.equal(packed.t.view(torch.uint8), want_packed.t.view(torch.uint8)) and torch.equal(last, want_last)
    assert torch.equal(win, win0)
    # window=None
    win = win0.clone()
    x0, real_last, packed, last = eng.image_prologue(win, lut)
    check(x0, real_last, "no window")
    assert packed is None and last is None
    assert torch.equal(win[:, :T - 1], win0[:, 1:]) and torch.equal(win[:, T - 1], win0[:, T - 1])


def test_kernel_argument_errors():
    eng = _engine("fp32")
    win = torch.zeros(1, 3, 4, 8, 6, dtype=torch.uint8, device=DEV)
    lut = torch.zeros(6, 256, device=DEV)
    with pytest.raises(TypeError):
        eng.image_prologue(win.float(), lut)
    with pytest.raises(TypeError):
        eng.image_prologue(win, lut.double())
    with pytest.raises(ValueError):
        eng.image_prologue(win, lut[:5].contiguous())
    with pytest.raises(ValueError):
        eng.image_prologue(win[..., :5], lut[:5].contiguous())                 # not contiguous
    with pytest.raises(ValueError):
        eng.image_prologue(torch.zeros(1, 3, 4, 8, 33, dtype=torch.uint8, device=DEV), torch.zeros(33, 256, device=DEV))
    with pytest.raises(ValueError):
        eng.image_prologue(win, lut, window=torch.zeros(2, 6, 4, 8, device=DEV), last_C=3)


# ------------------------------------------------------------------ 2. the model against its own fp32 path
def _u8_stream(seed, H=32, W=32, in_ch=15, n=FRAMES + 2):
    """(bytes (1, n, H, W, in_ch), real frames (1, n, 3, H, W)) of one synthetic clip."""
    from vid2vid_amd import synthetic
    A, frames = synthetic.edge2face_sequence(n, H, W, seed=seed, input_nc=in_ch)
    return (A * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous(), frames


def _decoded(streams, lut):
    from vid2vid_amd import visual
    return [(visual.decode_inputs(s[0], lut), s[1]) for s in streams]


def _raw_inputs(streams, t):
    A = torch.cat([s[0][:, t:t + 3] for s in streams])
    return A, (torch.cat([s[1][:, :2] for s in streams]) if t == 0 else None), None


def _run(model, streams, frames, u8, full=False):
    """[(first result, real_A_last, [windows])] of `frames` calls; u8: the whole window on frame 0 (or always), then t = 1."""
    model.fake_B_prev = None
    model.opt.inputs_u8 = bool(u8)
    outs = []
    for t in range(frames):
        A, Bf, _ = _raw_inputs(streams, t)
        if u8 and t > 0 and not full:
            A = A[:, 2:]
        first, last = model.inference(A, Bf, None)
        outs.append((first, last, [p.clone() for p in model.fake_B_prev]))
    model.opt.inputs_u8 = False
    return outs


def _edge2face(golden, precision, **kw):
    m = _model(golden("inference_edge2face_s1_32x32"), 1, precision, label_nc=0, input_nc=15, use_instance=False, fg=False, **kw)
    m.opt.autotune = False          # both plans run the same tiles
    m.opt.frame_tune = 0
    return m


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for t, ((f, l, w), (rf, rl, rw)) in enumerate(zip(got, want)):
        assert torch.equal(f, rf), "%s frame %d fake_B" % (what, t)
        assert torch.equal(l, rl), "%s frame %d real_A_last" % (what, t)
        assert len(w) == len(rw)
        for si, (a, b) in enumerate(zip(w, rw)):
            assert torch.equal(a, b), "%s frame %d fake_B_prev[%d]" % (what, t, si)
        assert torch.isfinite(f).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_model_equals_its_fp32_path_on_the_decoded_inputs(golden, precision, B):
    from vid2vid_amd import visual
    model = _edge2face(golden, precision)
    streams = [_u8_stream(400 + b) for b in range(B)]
    want = _run(model, _decoded(streams, visual.input_lut(15)), FRAMES, u8=False)
    assert model._active_plan.win_u8 is None and model._active_plan.raw_in is not None
    got = _run(model, streams, FRAMES, u8=True)
    fp = model._active_plan
    assert fp.win_u8 is not None and fp.raw_in is None and tuple(fp.win_u8.shape) == (B, 3, 32, 32, 15) and fp.B == B
    _assert_same(got, want, "t = 1 calls")
    assert not torch.equal(got[0][0], got[1][0])
    # the whole window on every call: the same frames
    _assert_same(_run(model, streams, FRAMES, u8=True, full=True), got, "whole window on every call")
    # the streams above are host tensors; frames that are on the device already go the same way
    on_dev = [(s[0].to(DEV), s[1]) for s in streams]
    _assert_same(_run(model, on_dev, 3, u8=True), got[:3], "device inputs")


def test_uint8_in_and_uint8_out(golden):
    from vid2vid_amd import visual
    model = _edge2face(golden, "bf16")
    streams = [_u8_stream(420 + b) for b in range(2)]
    want = _run(model, _decoded(streams, visual.input_lut(15)), 3, u8=False)
    model.opt.frames_u8 = True
    got = _run(model, streams, 3, u8=True)
    model.opt.frames_u8 = False
    for t in range(3):
        image = got[t][0]
        assert image.dtype == torch.uint8 and tuple(image.shape) == (2, 32, 32, 3)
        for b in range(2):
            assert torch.equal(image[b], visual.tensor2im(want[t][0][b])), (t, b)
        assert torch.equal(got[t][1], want[t][1]) and torch.equal(got[t][2][0], want[t][2][0])


def test_two_uint8_streams_match_the_oracle(golden):
    from oracle import vid2vid_oracle as O
    from vid2vid_amd import visual
    g = golden("inference_edge2face_s1_32x32")
    streams = [_u8_stream(300 + b) for b in range(2)]
    sd = sd_from_npz(g, "sd0.")
    ref = _oracle_frames("inputs_u8", lambda: O.InferenceOracle([sd], 0, False, False, [], 2, 2, 1),
                         _decoded(streams, visual.input_lut(15)), FRAMES, _raw_inputs)
    model = _model(g, 1, label_nc=0, input_nc=15, use_instance=False, fg=False)
    outs = _run(model, streams, FRAMES, u8=True)
    assert model._active_plan.win_u8 is not None
    _check_against_oracle(outs, ref, 1, "uint8 inputs B=2")


def test_two_spatial_scales_pose_table():
    """S = 2, seeded random weights, 6 input channels with the DensePose part-index table on channel 2, 32x64, 3 frames."""
    from vid2vid_amd import visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    torch.manual_seed(21)
    opt = make_opt(label_nc=0, input_nc=6, use_instance=False, fg=False, use_real_img=True, random_init_ok=True, ngf=8, n_blocks=2,
                   n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, loadSize=64, precision="fp32", gpu_ids=[0])
    model = create_model(opt)
    opt.autotune = False
    opt.frame_tune = 0
    lut = visual.input_lut(6, densepose_part_channel=2)
    assert not torch.equal(lut[2], lut[1])
    opt.input_lut = lut.to(DEV)
    streams = [_u8_stream(500, H=32, W=64, in_ch=6, n=5)]
    want = _run(model, _decoded(streams, lut), 3, u8=False)
    got = _run(model, streams, 3, u8=True)
    assert model.n_scales == 2 and len(got[0][2]) == 2 and model._active_plan.win_u8 is not None
    _assert_same(got, want, "S = 2")
    assert tuple(got[0][1].shape) == (6, 32, 64)


# ------------------------------------------------------------------ 3. the interface
def test_refusals_leave_the_running_sequence_untouched(golden):
    from vid2vid_amd import visual
    model = _edge2face(golden, "fp32")
    streams = [_u8_stream(440 + b) for b in range(2)]
    want = _run(model, streams[:1], 3, u8=True)
    opt = model.opt

    def refused(*args, **kw):
        with pytest.raises(ValueError):
            model.inference(*args, **kw)

    # no running sequence: t = 1 is refused and starts nothing
    model.fake_B_prev = None
    opt.inputs_u8 = True
    refused(streams[0][0][:, 2:3], None, None)
    assert model.fake_B_prev is None
    # a running sequence: frames 0 and 1, the refusals, then frame 2 as in the undisturbed run
    for t in range(2):
        A, Bf, _ = _raw_inputs(streams[:1], t)
        model.inference(A if t == 0 else A[:, 2:], Bf, None)
    A, _, _ = _raw_inputs(streams[:1], 2)
    keep = [p.clone() for p in model.fake_B_prev]
    plan = model._active_plan
    refused(A[:, 1:], None, None)                                            # t = 2: neither 1 nor tG
    refused(torch.cat([A, A], 1), None, None)                                # t = 6
    refused(visual.decode_inputs(A, visual.input_lut(15)), None, None)       # fp32 input_A with the option on
    refused(A[:, 2:], None, None, restart=[0])
    refused(A[:, 2:], None, None, active=[True])
    refused(torch.zeros(1, 1, 32, 32, 33, dtype=torch.uint8), None, None)    # in_ch > 32
    opt.input_lut = torch.zeros(14, 256)
    refused(A[:, 2:], None, None)                                            # a table of the wrong shape
    opt.input_lut = torch.zeros(15, 256, dtype=torch.float64)
    refused(A[:, 2:], None, None)
    opt.input_lut = None
    opt.compact_streams = True
    refused(torch.cat([A, A]), None, None)                                   # B = 2 in a pool
    opt.compact_streams = False
    assert model._active_plan is plan and all(torch.equal(a, b) for a, b in zip(model.fake_B_prev, keep))
    fake, last = model.inference(A[:, 2:], None, None)
    assert torch.equal(fake, want[2][0]) and torch.equal(last, want[2][1])
    opt.inputs_u8 = False
    # B > 1: the slot and pool arguments
    _run(model, streams, 2, u8=True)
    opt.inputs_u8 = True
    A2, _, _ = _raw_inputs(streams, 2)
    keep = [p.clone() for p in model.fake_B_prev]
    refused(A2[:, 2:], None, None, restart=[1])
    refused(A2[:, 2:], None, None, active=[True, False])
    opt.compact_streams = True
    refused(A2[:, 2:], None, None)
    opt.compact_streams = False
    assert all(torch.equal(a, b) for a, b in zip(model.fake_B_prev, keep))
    model.inference(A2[:, 2:], None, None)
    opt.inputs_u8 = False
    # a label model refuses the option
    lab = _model(golden("inference_label2city_s1_32x64"), 1)
    lab.opt.inputs_u8 = True
    with pytest.raises(ValueError):
        lab.inference(torch.zeros(1, 3, 32, 64, 1, dtype=torch.uint8), torch.zeros(1, 2, 3, 32, 64), None)
    assert getattr(lab, "fake_B_prev", None) is None
