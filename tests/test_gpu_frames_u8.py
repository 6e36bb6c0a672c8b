"""uint8 frames written inside the frame plan on the GPU.

Kernel level, bit exact: v2v_frames_u8 against a numpy fp32 restatement of the formula and against v2v_tensor2im per sample, on
both of its paths (4 pixels per thread where H W is a multiple of 4 and the buffers are aligned, one byte per thread otherwise);
rows, slots and modes with every byte of the output written; the argument checks.  In this implementation a plane is converted
by ONE path (its base is 16-byte aligned for every row and plane only when H W is a multiple of 4), so no size has a scalar tail
behind vectors inside a plane: the ragged sizes are those whose last workgroup of the wide path is partly filled ((3, 20), and
(33, 36): 297 vectors = one full workgroup of 256 and 41 threads of the next) and (3, 22), H W = 66 = 16 vectors + 2 pixels,
which therefore takes the scalar path as a whole.
Model level: a model with opt.frames_u8 against a model with the same weights without it, on the same inputs: every active
stream's image is visual.tensor2im of the other model's fake_B, idle streams are zero bytes, the windows and real_A_last are
bit for bit the same -- plain, slot and pool plans, a generator without a blend launch, the option flipped inside a sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_stream_slots import _model, _label_clip, _label_inputs

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


def _raw(frames, out, mode, rows, K, S, Cc, H, W, normalize=1):
    """The entry point on caller-owned buffers (what a launch leaves unwritten is seen); returns its code."""
    from vid2vid_amd import lib as L
    rc = L.lib.v2v_frames_u8(_p(frames), _p(out), _p(mode), _p(rows), K, S, Cc, H, W, normalize, None)
    torch.cuda.synchronize()
    return rc


def _convert(frames, mode=None, rows=None, S=None, normalize=1):
    K, Cc, H, W = frames.shape
    S = K if S is None else S
    out = torch.full((S, H, W, Cc), FILL, dtype=torch.uint8, device=DEV)
    assert _raw(frames, out, mode, rows, K, S, Cc, H, W, normalize) == 0
    return out


def _scale(x, normalize):
    x = np.asarray(x, dtype=np.float32)
    return ((x + np.float32(1)) / np.float32(2)) * np.float32(255) if normalize else x * np.float32(255)


def _formula(x, normalize):
    """numpy fp32, operation for operation; NaN -> 0 as the kernel defines it; (K,C,H,W) -> (K,H,W,C)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = _scale(x, normalize)
        v = np.where(np.isnan(v), np.float32(0), v)
        v = np.clip(v, np.float32(0), np.float32(255))
    return np.ascontiguousarray(v.astype(np.int32).astype(np.uint8).transpose(0, 2, 3, 1))


def _boundary(n, normalize):
    """The smallest float whose scaled value reaches the integer n, and the float just below it (which truncates to n - 1)."""
    x = np.float32(2.0 * n / 255.0 - 1.0) if normalize else np.float32(n / 255.0)
    down, up = np.float32(-np.inf), np.float32(np.inf)
    while _scale(x, normalize) < n:
        x = np.nextafter(x, up)
    while _scale(np.nextafter(x, down), normalize) >= n:
        x = np.nextafter(x, down)
    assert int(_scale(x, normalize)) == n and int(_scale(np.nextafter(x, down), normalize)) == n - 1
    return [x, np.nextafter(x, down)]


def _planted(K, Cc, H, W, normalize, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(K, Cc, H, W, generator=g) * 3.0 - 1.5).numpy()
    special = [-1.0, 1.0, 0.0, float("inf"), float("-inf"), float("nan")]
    for n in (1, 17, 128, 200, 255):
        special += _boundary(n, normalize)
    flat = x.reshape(-1)
    at = np.linspace(0, flat.size - 1, 3 * len(special)).astype(np.int64)        # every special value three times, spread out
    assert len(set(at.tolist())) == len(at)
    flat[at] = np.asarray(special * 3, dtype=np.float32)
    return torch.from_numpy(x)


# ------------------------------------------------------------------ 1. the formula, v2v_tensor2im, both paths
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("Cc", [3, 1])
@pytest.mark.parametrize("HW", [(5, 7), (8, 16), (3, 22), (3, 20), (33, 36)])
def test_kernel_matches_the_formula_and_tensor2im(HW, Cc, normalize):
    from vid2vid_amd import visual
    (H, W), K = HW, 3
    x = _planted(K, Cc, H, W, normalize, seed=H * 100 + W + Cc)
    want = torch.from_numpy(_formula(x.numpy(), normalize)).to(DEV)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0
    got = _convert(xd, normalize=normalize)
    assert torch.equal(got, want)
    for k in range(K):
        assert torch.equal(got[k].reshape(H, W, Cc), visual.tensor2im(xd[k], bool(normalize)).reshape(H, W, Cc)), k
    assert torch.equal(visual.tensor2im_batch(xd, bool(normalize)), want)
    # frames one float off a 16-byte boundary, then the images one byte off a 4-byte boundary: the scalar path, the same bytes
    shifted = torch.empty(xd.numel() + 4, device=DEV)[1:1 + xd.numel()].view_as(xd)
    shifted.copy_(xd)
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(_convert(shifted, normalize=normalize), want)
    buf = torch.full((want.numel() + 4,), FILL, dtype=torch.uint8, device=DEV)
    out = buf[1:1 + want.numel()].view_as(want)
    assert _raw(xd, out, None, None, K, K, Cc, H, W, normalize) == 0
    assert torch.equal(out, want) and int(buf[0]) == FILL and bool((buf[1 + want.numel():] == FILL).all())


# ------------------------------------------------------------------ 2. rows, slots, modes, complete write
@pytest.mark.parametrize("HW", [(8, 16), (5, 7)])
def test_rows_slots_modes_and_complete_write(HW):
    from vid2vid_amd import visual
    (H, W), K, S, Cc = HW, 2, 4, 3
    g = torch.Generator().manual_seed(H + W)
    x = (torch.rand(K, Cc, H, W, generator=g) * 3.0 - 1.5).to(DEV)
    im = [visual.tensor2im(x[k]) for k in range(K)]
    zero = torch.zeros(H, W, Cc, dtype=torch.uint8, device=DEV)
    assert im[0].any() and im[1].any()

    def expect(out, images, what):
        for s in range(S):
            assert torch.equal(out[s], images.get(s, zero)), (what, s)

    base = _convert(x, None, _i32([3, 1]), S)
    expect(base, {3: im[0], 1: im[1]}, "row_slot [3, 1]")
    assert torch.equal(_convert(x, _i32([0, 0]), _i32([3, 1]), S), base)
    assert torch.equal(_convert(x, _i32([1, 0]), _i32([3, 1]), S), base)                  # mode 1 converts like mode 0
    poisoned = x.clone()
    poisoned[1] = float("nan")
    for frames in (x, poisoned):                                                         # a row of mode 2 is not read
        expect(_convert(frames, _i32([0, 2]), _i32([3, 1]), S), {3: im[0]}, "mode [0, 2]")
    expect(_convert(x, _i32([0, 7]), _i32([3, 1]), S), {3: im[0]}, "mode [0, 7]")         # any other value is idle too
    for bad in (7, -1, S):                                                               # a slot word out of range writes nothing
        expect(_convert(x, None, _i32([3, bad]), S), {3: im[0]}, "row_slot [3, %d]" % bad)
    # identity words, K = S: the call without words
    x4 = (torch.rand(S, Cc, H, W, generator=g) * 3.0 - 1.5).to(DEV)
    plain = _convert(x4)
    assert not (plain == FILL).all() and torch.equal(plain, torch.stack([visual.tensor2im(x4[k]) for k in range(S)]))
    assert torch.equal(_convert(x4, _i32([0] * S), _i32(list(range(S))), S), plain)
    assert torch.equal(_convert(x4, None, _i32(list(range(S))), S), plain)
    # mode alone (a slot plan): row k is image k or zero
    expect(_convert(x4, _i32([0, 2, 1, 2])), {0: plain[0], 2: plain[2]}, "mode alone")


# ------------------------------------------------------------------ 3. argument errors
def test_argument_errors_leave_out_untouched():
    from vid2vid_amd import lib as L
    K, S, Cc, H, W = 2, 4, 3, 4, 8
    x = torch.rand(S, 4, H, W, device=DEV)
    out = torch.full((S, H, W, 4), FILL, dtype=torch.uint8, device=DEV)
    words = _i32([3, 1, 0, 2])
    EINVAL = L.lib.v2v_tensor2im(None, None, 1, 1, 1, 1, None)
    assert EINVAL != 0

    def call(frames=x, out_=out, mode=words, rows=words, K_=K, S_=S, C_=Cc, H_=H, W_=W):
        return _raw(frames, out_, mode, rows, K_, S_, C_, H_, W_)
    for kw in (dict(frames=None), dict(out_=None), dict(K_=0), dict(S_=K - 1), dict(C_=0), dict(C_=5), dict(H_=0), dict(W_=0),
               dict(rows=None), dict(rows=None, mode=None)):
        assert call(**kw) == EINVAL, kw
        assert b"frames_u8" in L.lib.v2v_last_error()
        assert bool((out == FILL).all()), kw
    # out inside frames (one buffer): refused, nothing written
    both = torch.full((4 * K * Cc * H * W + S * Cc * H * W,), FILL, dtype=torch.uint8, device=DEV)
    frames = both[:4 * K * Cc * H * W].view(torch.float32)
    for off in (0, 4 * K * Cc * H * W - 1):
        inside = both[off:]
        assert _raw(frames, inside, words, words, K, S, Cc, H, W) == EINVAL and b"overlap" in L.lib.v2v_last_error()
        assert bool((both == FILL).all())
    assert _raw(frames, both[4 * K * Cc * H * W:], words, words, K, S, Cc, H, W) == 0      # adjacent is fine
    assert bool((both[:4 * K * Cc * H * W] == FILL).all())


# ------------------------------------------------------------------ 4. the model
def _pair(golden, precision, **kw):
    """Two models on the same weights: opt.frames_u8 off and on."""
    g = golden("inference_label2city_s1_32x64")
    return _model(g, 1, precision, **kw), _model(g, 1, precision, frames_u8=True, **kw)


def _step_both(off, on, inputs, row, **kw):
    """One call of both models on the same inputs; checks the contract of the option and returns (fake_B, image)."""
    from vid2vid_amd import visual
    fake, last_off = off.inference(*inputs, **kw)
    image, last_on = on.inference(*inputs, **kw)
    B, _, H, W = fake.shape
    assert image.dtype == torch.uint8 and tuple(image.shape) == (B, H, W, 3) and image.is_contiguous()
    for b, r in enumerate(row):
        if r is None:
            assert not fake[b].any() and not image[b].any(), "idle stream %d" % b
        else:
            assert torch.equal(image[b], visual.tensor2im(fake[b])), "stream %d" % b
            assert image[b].any()
    assert torch.equal(last_on, last_off)
    assert len(on.fake_B_prev) == len(off.fake_B_prev)
    for w_on, w_off in zip(on.fake_B_prev, off.fake_B_prev):
        assert torch.equal(w_on, w_off)
    assert torch.isfinite(fake).all()
    return fake, image


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_plain_plans_return_the_images_of_fake_B(golden, precision, B):
    from vid2vid_amd import visual
    off, on = _pair(golden, precision)
    clips = [_label_clip(700 + c) for c in range(B)]
    kept = []
    for t in range(3):
        row = [(b, t, t == 0) for b in range(B)]
        fake, image = _step_both(off, on, _label_inputs(clips, row), row)
        for earlier, copy in kept:                   # returned images do not alias the plan's buffer or each other
            assert torch.equal(earlier, copy)
        kept.append((image, image.clone()))
        assert torch.equal(visual.tensor2im_batch(fake), torch.stack([visual.tensor2im(fake[b]) for b in range(B)]))
    fp = on._active_plan
    assert fp.frames_u8 and not fp.slots and fp.pool is None and fp.B == B and not off._active_plan.frames_u8
    assert not torch.equal(kept[0][0], kept[1][0])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("blend", [True, False])
def test_slot_schedule_idle_images_are_zero(golden, precision, blend):
    """Stream 1 idles at call 1 and resumes, stream 2 restarts on another clip at call 2.  blend = False: a generator whose
    frame is the image head's output (no flow, no foreground): nothing in front of the image launch zeroes an idle row."""
    off, on = _pair(golden, precision, **({} if blend else dict(no_flow=True, fg=False)))
    clips = [_label_clip(720 + c) for c in range(4)]
    sched = [[(0, 0, True), (1, 0, True), (2, 0, True)],
             [(0, 1, False), None, (2, 1, False)],
             [(0, 2, False), (1, 1, False), (3, 0, True)]]
    for row in sched:
        _step_both(off, on, _label_inputs(clips, row, fill=255.0), row,
                   restart=[r is not None and r[2] for r in row], active=[r is not None for r in row])
    assert on._active_plan.slots and on._active_plan.frames_u8 and on._active_plan.blend_launch == blend


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pool_schedule_delivers_all_slots(golden, precision):
    """S = 3 slots with 3, 1 and 2 of them live: the K-row plans write all S images, idle ones zero."""
    off, on = _pair(golden, precision, compact_streams=True)
    clips = [_label_clip(740 + c) for c in range(3)]
    sched = [[(0, 0, True), (1, 0, True), (2, 0, True)],
             [None, (1, 1, False), None],
             [(0, 1, False), None, (2, 1, False)]]
    for row, K in zip(sched, (3, 1, 2)):
        _step_both(off, on, _label_inputs(clips, row, fill=255.0), row,
                   restart=[r is not None and r[2] for r in row], active=[r is not None for r in row])
        fp = on._active_plan
        assert fp.pool is not None and fp.pool.S == 3 and fp.B == K and fp.frames_u8
        assert tuple(fp.out["image"].shape) == (3, 32, 64, 3) and tuple(fp.out["fake_B"].shape) == (K, 3, 32, 64)
    image, last = on.inference(*_label_inputs(clips, sched[0]), active=[])        # nothing live: zeros, no replay
    assert image.dtype == torch.uint8 and tuple(image.shape) == (3, 32, 64, 3) and not image.any() and not last.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_option_flipped_inside_a_running_sequence(golden, precision):
    from vid2vid_amd import visual
    off, flip = _pair(golden, precision)
    flip.opt.frames_u8 = False
    clips = [_label_clip(760 + c) for c in range(2)]
    for t in range(3):
        row = [(b, t, t == 0) for b in range(2)]
        inputs = _label_inputs(clips, row)
        fake, _ = off.inference(*inputs)
        got, _ = flip.inference(*inputs)
        if t == 0:
            assert torch.equal(got, fake)
            flip.opt.frames_u8 = True                # from frame 2 on: the other plan, on the same windows
        else:
            assert got.dtype == torch.uint8
            for b in range(2):
                assert torch.equal(got[b], visual.tensor2im(fake[b])), (t, b)
        assert torch.equal(flip.fake_B_prev[0], off.fake_B_prev[0]), t
    assert len(flip._plans) == 2 and flip._active_plan.frames_u8
