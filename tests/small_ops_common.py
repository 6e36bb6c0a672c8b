"""fp64 CPU references, case tables, inputs, the guard helper and the comparison shared by tests/test_cpu_small_ops.py and
tests/test_gpu_small_ops.py: the small device ops of csrc/flow_ops.hip (v2v_flownet_normalize, v2v_warp_diff_norm, v2v_resize_planar,
v2v_pack_channels_nhwc, v2v_concat_channels_nhwc), csrc/pointwise.hip (v2v_unpack_channels_nchw, v2v_pack_concat_nhwc,
v2v_fg_mask_nhwc, v2v_avgpool3s2_nhwc, v2v_reflect_pad_fold), csrc/segment_ops.hip (v2v_instance_mean_planar) and the two copies
(v2v_memset_zero, v2v_memcpy_d2d), each restated from its formula in include/v2v_hip.h.

Inputs are seeded and cached: the tensors a maker returns are shared between tests and must not be modified.  Every bound is
derived where it is defined; tests/test_cpu_small_ops.py shows what each of them rejects."""
import functools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
BF16_STEP = 2.0 ** -8     # one round-to-nearest-even step to bf16 (8 significant bits), as DRAW_BOUND of norm_bwd_common
NAN = float("nan")
GUARD = 64                # elements of the guard band on each side of an output
PRECS = ("fp32", "bf16")


def tdt(prec):
    return torch.bfloat16 if prec == "bf16" else torch.float32


def f32(v):
    """The value an fp32 argument of the C ABI carries, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def f32t(v):
    return torch.tensor(v, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison: check() of norm_bwd_common restated with an absolute term and the error / bound ratio as its result
# ---------------------------------------------------------------------------------------------------------------------------
def check(got, ref, rel=0.0, floor=0.0, what="", extra=0.0):
    """Assert |got - ref| <= rel*|ref| + floor*rms(ref) + extra for every element (extra: a number or an fp64 tensor that
    broadcasts to ref, the absolute term of a derived bound; with extra = 0 this is norm_bwd_common.check).  An element of got
    that is not finite fails whatever the bound.  Returns the worst |got - ref| / bound (0 where both are 0): the figure the GPU
    tests print."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    rms = float(ref.pow(2).mean().sqrt())
    err = (got - ref).abs()
    bound = (rel * ref.abs() + floor * rms + extra).expand_as(ref)
    over = err - bound
    over = torch.where(torch.isfinite(got), over, torch.full_like(over, float("inf")))
    worst = int(over.argmax())
    if float(over.reshape(-1)[worst]) > 0:
        where, rest = [], worst
        for size in reversed(ref.shape):
            where.insert(0, rest % size)
            rest //= size
        raise AssertionError("%s: element %s: got %.9g, want %.9g, |diff| %.3e > %.3e; %d of %d elements out of bound"
                             % (what, where, float(got.reshape(-1)[worst]), float(ref.reshape(-1)[worst]),
                                float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]), int((over > 0).sum()), over.numel()))
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------------
# the guard helper.  It only inspects memory the test allocated itself.
# ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    """The bit pattern of t as integers (NaN == NaN here)."""
    t = t.contiguous()
    if not t.dtype.is_floating_point:
        return t
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Guarded:
    """An output of n elements inside a larger allocation: GUARD elements of a fixed pattern in front (plus `lead` more, to move
    the output off the allocation's alignment) and GUARD behind.  The output starts as `fill` (NaN for floating-point outputs, so
    that an element the call does not write fails check()).  finish() compares everything the call must not write, bit for bit,
    with a snapshot taken before the call."""
    PATTERN = {torch.float32: -777.0, torch.bfloat16: -777.0, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A}

    def __init__(self, n, dtype, device="cpu", fill=NAN, lead=0):
        self.lo, self.n = GUARD + lead, n
        self.buf = torch.empty(self.lo + n + GUARD, dtype=dtype, device=device)
        self.buf.fill_(self.PATTERN[dtype])
        self.view = self.buf[self.lo:self.lo + n]
        self.view.fill_(fill)
        self.before = bits(self.buf).clone()

    def ptr(self):
        return self.view.data_ptr()

    def finish(self, written=None, what="output"):
        """written: bool mask over the n elements, True where the call must write (None: everywhere).  Returns the output."""
        now = bits(self.buf)
        lo, n = self.lo, self.n
        assert torch.equal(now[:lo], self.before[:lo]), "%s: the guard band in front of it was overwritten" % what
        assert torch.equal(now[lo + n:], self.before[lo + n:]), "%s: the guard band behind it was overwritten" % what
        if written is None:
            written = torch.ones(n, dtype=torch.bool)
        written = written.reshape(-1).to(self.buf.device)
        assert written.numel() == n
        keep = ~written
        assert torch.equal(now[lo:lo + n][keep], self.before[lo:lo + n][keep]), \
            "%s: an element outside the channels the call writes has changed" % what
        if self.view.dtype.is_floating_point:
            assert not torch.isnan(self.view[written]).any(), "%s: an element the call must write still holds its NaN pre-fill" % what
        return self.view


def channel_mask(P, stride, offset, C):
    """[P][stride] bool: True on channels [offset, offset + C) of every NHWC row."""
    m = torch.zeros(P, stride, dtype=torch.bool)
    m[:, offset:offset + C] = True
    return m


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. v2v_flownet_normalize: x1, x2 = (im1, im2 - mean) / rgb_max, mean per (b, c) over both frames
# ---------------------------------------------------------------------------------------------------------------------------
NORMALIZE_CASES = [(1, 1, 5, 255.0),        # 2*hw = 10 < 64 chunks: 54 empty chunks, one element per chunk
                   (2, 37, 53, 255.0),      # 3922 elements in chunks of 62: chunk 31 straddles im1 / im2, the last chunk holds 16
                   (1, 257, 255, 1.0)]      # 131070 elements in chunks of 2048 > 256: threads loop 8 times, the last chunk holds 2046
NORMALIZE_CHUNKS = 64


@functools.lru_cache(maxsize=None)
def normalize_case(B, H, W, rgb_max):
    """(im1, im2) fp32 [B][3][HW] in [0, rgb_max].  Plane (B - 1, 1) holds at most 0.09 rgb_max except its first pixel of im1 and its
    last pixel of im2, which are rgb_max: the two ends of the range the mean runs over weigh 20 times an average pixel."""
    g = _gen(100 + H * W)
    hw = H * W
    im1 = torch.rand(B, 3, hw, generator=g) * rgb_max
    im2 = torch.rand(B, 3, hw, generator=g) * rgb_max
    im1[B - 1, 1] *= 0.09
    im2[B - 1, 1] *= 0.09
    im1[B - 1, 1, 0] = rgb_max
    im2[B - 1, 1, hw - 1] = rgb_max
    assert float(im1.min()) >= 0 and float(im2.min()) >= 0 and float(im1.max()) <= rgb_max and float(im2.max()) <= rgb_max
    return im1, im2


def ref_normalize(im1, im2, rgb_max):
    both = torch.cat([im1, im2], 2).double()
    mean = both.mean(2, keepdim=True)
    return (im1.double() - mean) / rgb_max, (im2.double() - mean) / rgb_max


def normalize_bound(im1, im2, rgb_max):
    """(rel, extra [B][3][1]).  The kernel sums the 2*hw values of a plane in 64 chunks of per = ceil(2*hw / 64): a thread adds
    ceil(per / 256) values one after the other, an 8-level tree joins the 256 threads, and the second kernel joins the 64 chunk
    sums (one per thread, 0 + s is exact) in another 8-level tree.  No value passes more than d = ceil(per / 256) + 16 roundings
    and all values are >= 0, so |sum' - sum| <= d u sum; the division adds one rounding: |mean' - mean| <= (d + 1) u mean|x|.
    That lands in the output divided by rgb_max (extra).  The output itself takes three more roundings (im - mean, 1 / rgb_max,
    the product): rel = 4 u covers them with their second-order terms.  (The order-free bound (2*hw - 1) u would be 1e-2 of the
    257 x 255 case's mean and hide a dropped pixel, which moves that mean by 1 / (2*hw) = 8e-6 of rgb_max.)"""
    hw = im1.shape[2]
    per = -(-2 * hw // NORMALIZE_CHUNKS)
    depth = -(-per // 256) + 16
    mean_abs = torch.cat([im1, im2], 2).double().abs().mean(2, keepdim=True)
    return 4 * U, (depth + 1) * U * mean_abs / rgb_max


# ---------------------------------------------------------------------------------------------------------------------------
# 2. v2v_warp_diff_norm: warped = Resample2d(img1, flow); out = sqrt(sum_c (img0 - warped)^2) or (that sum < thr)
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (B, C, H, W, halves): halves = img0 / img1 are channels 0..2 / 3..5 of one [B][6][HW] tensor (batch strides 6*HW)
WARP_CASES = {"halves_13x17": (2, 3, 13, 17, True), "row_1x9": (1, 1, 1, 9, False), "dense_8x8": (1, 3, 8, 8, False)}
WARP_OUTPUTS = ("both", "norm_only", "warped_only")
THR_MARGIN = 1e-3


def ref_warp_diff_norm(img0, img1, flow, swap_weights=False, xr_limit=None):
    """(warped [B][C][H][W], r [B][H][W] = sum_c (img0 - warped)^2) in fp64.  xf = fp32(x + dx), yf = fp32(y + dy) as the kernel
    and the reference CUDA form them; the fractional part of an fp32 number is exact, everything from there on is fp64: four
    clamped neighbours, weights from the UNCLAMPED fraction, the sum in the kernel's order.  swap_weights / xr_limit are the
    mutations of tests/test_cpu_small_ops.py (alpha and beta exchanged; xR clamped to xr_limit instead of W - 1)."""
    B, Cc, H, W = img1.shape
    hw = H * W
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    xf, yf = xs[None] + flow[:, 0].float(), ys[None] + flow[:, 1].float()                    # fp32 additions
    fx, fy = torch.floor(xf), torch.floor(yf)
    alpha, beta = xf.double() - fx.double(), yf.double() - fy.double()
    if swap_weights:
        alpha, beta = beta, alpha
    xL, xR = fx.long().clamp(0, W - 1), (fx.long() + 1).clamp(0, W - 1 if xr_limit is None else xr_limit).clamp(min=0)
    yT, yB = fy.long().clamp(0, H - 1), (fy.long() + 1).clamp(0, H - 1)
    flat = img1.double().reshape(B, Cc, hw)
    tap = lambda yy, xx: flat.gather(2, (yy * W + xx).reshape(B, 1, hw).expand(B, Cc, hw)).reshape(B, Cc, H, W)
    a, b = alpha[:, None], beta[:, None]
    val = (1 - a) * (1 - b) * tap(yT, xL)
    val = val + a * (1 - b) * tap(yT, xR)
    val = val + (1 - a) * b * tap(yB, xL)
    val = val + a * b * tap(yB, xR)
    d = img0.double().reshape(B, Cc, H, W) - val
    return val, (d * d).sum(1)


def warp_bounds(img1, Cc):
    """(extra of warped, (rel, extra) of the mode-0 norm).  A tap's weight carries three roundings (1 - alpha, 1 - beta, their
    product), its product with the sample a fourth, and the three additions after the first (0 + t is exact) one each on partial
    sums that stay within max|img1| because the weights are >= 0 and sum to 1: |warped' - warped| <= 7 u max|img1|, taken as 8 u
    for the second-order terms.  (A contraction to fma removes roundings.)  The difference d adds u |d|; as a vector over the
    channels |norm(d') - norm(d)| <= sqrt(C) 8 u max|img1| + u norm(d).  The sum of squares takes at most C roundings per term
    (relative C u, halved by the square root) and the root one more: rel = (C/2 + 2) u, taken as (C/2 + 3) u."""
    e = 8 * U * float(img1.abs().max())
    return e, ((Cc / 2 + 3) * U, math.sqrt(Cc) * e)


@functools.lru_cache(maxsize=None)
def warp_case(name):
    """dict(img0, img1 [B][C][H][W] fp32 (views of x [B][6][HW] when the case says so), x, flow [B][2][H][W], thr, bs = batch
    stride).  Flows: normal with sigma 3; the four corner pixels point 40 pixels outside the image; the middle row holds exact
    integers (alpha == beta == 0; in the one-row case columns 3..5 only).  thr is the fp32 median of r; img0 is then moved where
    r came within 2 THR_MARGIN of it, so that the mode-1 outcome of every pixel is decided well above the kernel's rounding."""
    B, Cc, H, W, halves = WARP_CASES[name]
    g = _gen(200 + H * W)
    hw = H * W
    if halves:
        x = torch.rand(B, 6, hw, generator=g) * 2 - 1
        img0, img1, bs = x[:, :3].view(B, 3, H, W), x[:, 3:].view(B, 3, H, W), 6 * hw
    else:
        x = None
        img0, img1, bs = torch.rand(B, Cc, H, W, generator=g) * 2 - 1, torch.rand(B, Cc, H, W, generator=g) * 2 - 1, Cc * hw
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    cols = slice(None) if H > 1 else slice(3, 6)
    flow[:, :, H // 2, cols] = torch.round(flow[:, :, H // 2, cols])
    for yy, xx, fx, fy in ((0, 0, -40.0, -40.0), (0, W - 1, 40.0, -40.0), (H - 1, 0, -40.0, 40.0), (H - 1, W - 1, 40.0, 40.0)):
        flow[:, 0, yy, xx], flow[:, 1, yy, xx] = fx, fy
    thr = f32(float(ref_warp_diff_norm(img0, img1, flow)[1].median()))
    for _ in range(20):
        r = ref_warp_diff_norm(img0, img1, flow)[1]
        close = (r - thr).abs() < 2 * THR_MARGIN * thr
        if not close.any():
            break
        img0[:, 0][close] += 0.25                               # (writes through to x in the halves case)
    r = ref_warp_diff_norm(img0, img1, flow)[1]
    assert float(((r - thr).abs() / thr).min()) >= THR_MARGIN, "warp_case(%s): a pixel is within %g of the threshold" % (name, THR_MARGIN)
    below = float((r < thr).double().mean())
    assert 0.1 <= below <= 0.9, "warp_case(%s): %.0f %% of the pixels below the threshold" % (name, 100 * below)
    return dict(img0=img0, img1=img1, x=x, flow=flow, thr=thr, bs=bs)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. v2v_resize_planar: nn.Upsample to (OH, OW), bilinear (align_corners False) or nearest, times out_scale
# ---------------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [(3, 5, 7, 20, 28),          # x4, what FlowNet2 does with its flow
                (2, 12, 20, 7, 9),          # non-integer down-scale
                (1, 1, 1, 3, 5),            # one source pixel
                (2, 9, 6, 1, 1),            # one destination pixel
                (1, 10, 6, 6, 10)]          # oy * H / OH = 5 at oy = 3, ox * W / OW = 3 at ox = 5: the fp32 product must not fall short
RESIZE_SCALES = (1.0, 20 * 0.25)


@functools.lru_cache(maxsize=None)
def resize_case(planes, H, W):
    return torch.randn(planes, H, W, generator=_gen(300 + 31 * H + W))


def bilinear_taps(n_in, n_out, half=1):
    """(i0, i1, frac fp64) per destination index: source coordinate ((2 o + 1) n_in - n_out) / (2 n_out) =
    (o + 0.5) n_in / n_out - 0.5 in exact integers, clamped at 0, split by integer division: frac is one correctly rounded
    division.  half = 0 is the mutation that drops the + 0.5."""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = ((2 * o + half) * n_in - n_out).clamp(min=0), 2 * n_out
    i0 = torch.div(num, den, rounding_mode="floor")
    frac = (num - i0 * den).double() / den
    i0 = i0.clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), frac


def nearest_index(n_in, n_out, rounding="floor"):
    """floor(o * n_in / n_out) in exact integers ('round': the mutation)."""
    o = torch.arange(n_out, dtype=torch.int64)
    if rounding == "round":
        return torch.div(2 * o * n_in + n_out, 2 * n_out, rounding_mode="floor").clamp(max=n_in - 1)
    return torch.div(o * n_in, n_out, rounding_mode="floor").clamp(max=n_in - 1)


def nearest_index_fp32(n_in, n_out):
    """The index as the kernel computes it: floor((float)o * ((float)n_in / (float)n_out)), each step one fp32 operation."""
    o = torch.arange(n_out, dtype=torch.float32)
    s = f32t(float(n_in)) / f32t(float(n_out))
    return torch.floor(o * s).long().clamp(max=n_in - 1)


def ref_resize(x, OH, OW, bilinear, out_scale, half=1, rounding="floor"):
    """fp64 [planes][OH][OW] (nearest: the fp32 product x[...] * out_scale widened, one correctly rounded operation like the
    kernel's, so that the GPU comparison is bit exact)."""
    planes, H, W = x.shape
    if not bilinear:
        iy, ix = nearest_index(H, OH, rounding), nearest_index(W, OW, rounding)
        return (x[:, iy][:, :, ix] * f32t(out_scale)).double()
    y0, y1, ly = bilinear_taps(H, OH, half)
    x0, x1, lx = bilinear_taps(W, OW, half)
    xd = x.double()
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * xd[:, y0][:, :, x0] + lx * xd[:, y0][:, :, x1]
    bot = (1 - lx) * xd[:, y1][:, :, x0] + lx * xd[:, y1][:, :, x1]
    return ((1 - ly) * top + ly * bot) * out_scale


def resize_bilinear_extra(x, out_scale):
    """The absolute bound of the bilinear result.  Arithmetic term: each of the two nested blends rounds 1 - l, two products and
    a sum (3 u of values within max|x|), out_scale one more: 7 u max|x|, taken as 8 u.  Coordinate term: the kernel forms the
    source coordinate in fp32 as (n_in / n_out) * (o + 0.5) - 0.5: the quotient, the product and the difference each round a
    number below n_in, so the coordinate is off by at most 3 u n_in, taken as 4 u n_in (an fma removes a rounding).  The
    interpolant is continuous and piecewise linear in each coordinate with a slope of at most the largest difference D between
    adjacent samples along that axis, so a coordinate error moves it by at most 4 u (H Dv + W Dh), also where the error carries
    the coordinate across an integer."""
    planes, H, W = x.shape
    xd = x.double()
    dv = float((xd[:, 1:] - xd[:, :-1]).abs().max()) if H > 1 else 0.0
    dh = float((xd[:, :, 1:] - xd[:, :, :-1]).abs().max()) if W > 1 else 0.0
    return abs(out_scale) * (8 * U * float(xd.abs().max()) + 4 * U * (H * dv + W * dh))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. - 6. the layout ops: bit exact
# ---------------------------------------------------------------------------------------------------------------------------
# v2v_pack_channels_nhwc: (N, C, H, W, stride {prec}, offset, scale, slope)
PACK_CH_CASES = [(2, 3, 5, 7, {"fp32": 16, "bf16": 16}, 5, 0.05, 0.1),
                 (1, 2, 3, 3, {"fp32": 8, "bf16": 8}, 6, 1.0, 1.0),          # offset + C == stride
                 (1, 1, 1, 1, {"fp32": 4, "bf16": 8}, 0, 0.05, 0.1)]
# v2v_concat_channels_nhwc: (P, C, src stride, src offset, dst stride, dst offset)
CONCAT_CASES = [(35, 5, 8, 3, 24, 17), (1, 8, 8, 0, 8, 0), (300, 1, 3, 2, 2, 1)]
# v2v_unpack_channels_nchw: (N, C, H, W, stride, offset)
UNPACK_CASES = [(2, 2, 7, 9, 8, 6),                                          # offset + C == stride: the second operand's gradient
                (2, 2, 7, 9, 8, 0)]
# v2v_pack_concat_nhwc: (N, C0, C1, H, W, stride, scale1)
PACK_CONCAT_CASES = [(2, 3, 0, 5, 7, 8, 1 / 20),                             # x1 == NULL
                     (2, 3, 5, 5, 7, 8, 1 / 20),                             # C0 + C1 == stride
                     (1, 2, 1, 3, 3, 8, 1 / 20)]                             # five pad channels


@functools.lru_cache(maxsize=None)
def planar_case(N, Cc, H, W, seed):
    """fp32 [N][C][HW], both signs, magnitudes around 10."""
    return torch.randn(N, Cc, H * W, generator=_gen(seed)) * 10


@functools.lru_cache(maxsize=None)
def nhwc_case(P, stride, prec, seed):
    """[P][stride] of the activation dtype, every channel different and finite."""
    return torch.randn(P, stride, generator=_gen(seed)).to(tdt(prec))


def to_nhwc(x):
    """planar [N][C][HW] -> [N*HW][C]"""
    N, Cc, hw = x.shape
    return x.permute(0, 2, 1).reshape(N * hw, Cc)


def ref_pack_channels(x, scale, slope, prec):
    """[N*HW][C] of the activation dtype: v = x * scale; v > 0 ? v : v * slope, every step one correctly rounded fp32 operation."""
    v = x * f32t(scale)
    v = torch.where(v > 0, v, v * f32t(slope))
    return to_nhwc(v).to(tdt(prec))


def ref_unpack_channels(y, N, Cc, hw, offset):
    """y [N*HW][stride] activation dtype -> planar fp32 [N][C][HW], the widened values."""
    return y[:, offset:offset + Cc].float().reshape(N, hw, Cc).permute(0, 2, 1).contiguous()


def ref_pack_concat(x0, x1, scale1, stride, prec):
    """[N*HW][stride] of the activation dtype: cat([x0, x1 * scale1], 1), pad channels 0."""
    N, C0, hw = x0.shape
    out = torch.zeros(N * hw, stride)
    out[:, :C0] = to_nhwc(x0)
    if x1 is not None:
        out[:, C0:C0 + x1.shape[1]] = to_nhwc(x1 * f32t(scale1))
    return out.to(tdt(prec))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. v2v_fg_mask_nhwc and 8. v2v_avgpool3s2_nhwc
# ---------------------------------------------------------------------------------------------------------------------------
LABEL_NC = 4                               # a frame = LABEL_NC one-hot channels + the instance-edge channel
FG_STRIDE = 16                             # two frames = 10 channels
FG_SETS = {1: (2,), 3: (1, 3, LABEL_NC)}   # n_fg -> channels; the 3-set includes the edge channel, which is 1 ON TOP of a label
FG_SIZES = {"P1": (1, 1), "P99": (17, 21)}       # full-resolution size; pooled: 1 x 1 and 9 x 11
FG_RAW_SIZES = {"P1": (1, 1), "P99": (9, 11)}
AVGPOOL_SIZES = [(1, 9), (17, 23), (2, 2)]
AVGPOOL_N, AVGPOOL_C, AVGPOOL_STRIDE = 2, 5, 8


@functools.lru_cache(maxsize=None)
def label_frames(H, W):
    """fp32 [H*W][FG_STRIDE]: two frames of one-hot labels plus an edge channel (a third of the pixels), pad channels 0."""
    g = _gen(700 + H * W)
    x = torch.zeros(H * W, FG_STRIDE)
    for t in range(2):
        lab = torch.randint(0, LABEL_NC, (H * W,), generator=g)
        x[torch.arange(H * W), t * (LABEL_NC + 1) + lab] = 1.0
        x[:, t * (LABEL_NC + 1) + LABEL_NC] = (torch.rand(H * W, generator=g) < 0.34).float()
    if H * W == 1:
        x[0, 3], x[0, 0:3] = 1.0, 0.0       # the single pixel: label 3 with an edge in frame 0 (sum 2 for the 3-set)
        x[0, LABEL_NC] = 1.0
    return x


def pooled_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def ref_avgpool3s2(x, N, H, W, include_pad=False):
    """x [N*H*W][stride] (the values the kernel reads) -> fp64 [N*OH*OW][stride]: the in-bounds taps of the 3 x 3 window at
    (2 oy - 1, 2 ox - 1), summed and divided by their number (include_pad: by 9, the mutation)."""
    stride = x.shape[1]
    OH, OW = pooled_size(H, W)
    xd = F.pad(x.double().reshape(N, H, W, stride), (0, 0, 1, 2, 1, 2))
    ones = F.pad(torch.ones(1, H, W, 1, dtype=torch.float64), (0, 0, 1, 2, 1, 2))
    s, cnt = 0, 0
    for dy in range(3):
        for dx in range(3):
            s = s + xd[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2]
            cnt = cnt + ones[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2]
    return (s / (9.0 if include_pad else cnt)).reshape(N * OH * OW, stride)


def avgpool_bound(x, prec):
    """(rel, extra): nine fp32 additions of values within max|x| and one division: |y' - y| <= 9 u max|x| + u |y|; the bf16 store
    adds one round-to-nearest-even step."""
    return (BF16_STEP if prec == "bf16" else 0.0) + 2 * U, 9 * U * float(x.double().abs().max())


@functools.lru_cache(maxsize=None)
def avgpool_case(H, W, prec):
    """[N*H*W][stride] of the activation dtype, both signs, pad channels 0."""
    x = torch.randn(AVGPOOL_N * H * W, AVGPOOL_STRIDE, generator=_gen(800 + 29 * H + W))
    x[:, AVGPOOL_C:] = 0
    return x.to(tdt(prec))


def ref_fg_mask(x, base_ch, fg, clamp=True):
    """x [P][stride] (the values the kernel reads) -> fp64 [P]."""
    m = x.double()[:, [base_ch + f for f in fg]].sum(1)
    return m.clamp(0, 1) if clamp else m


FG_BOUND = (3 * U, 0.0)        # at most three fp32 additions of non-negative values; the clamp is exact


# ---------------------------------------------------------------------------------------------------------------------------
# 9. v2v_reflect_pad_fold: the adjoint of nn.ReflectionPad2d(pad)
# ---------------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(1, 4, 5, 3),                # pad = H - 1, the largest legal value: rows 1 and 2 receive from both borders
              (2, 6, 7, 1),
              (1, 3, 3, 0)]
FOLD_C, FOLD_STRIDE = 5, 8


@functools.lru_cache(maxsize=None)
def fold_case(N, H, W, pad, prec):
    """xp [N*(H+2p)*(W+2p)][stride] of the activation dtype; pad channels 0, as every NHWC buffer of the library keeps them."""
    xp = torch.randn(N * (H + 2 * pad) * (W + 2 * pad), FOLD_STRIDE, generator=_gen(900 + 10 * H + pad))
    xp[:, FOLD_C:] = 0
    return xp.to(tdt(prec))


def ref_reflect_fold(xp, N, H, W, pad):
    """xp [N*HP*WP][stride] -> fp64 [N*H*W][stride]: d/dx of sum(F.pad(x, reflect) * xp), by CPU autograd in fp64."""
    stride = xp.shape[1]
    g = xp.double().reshape(N, H + 2 * pad, W + 2 * pad, stride).permute(0, 3, 1, 2)
    x = torch.zeros(N, stride, H, W, dtype=torch.float64, requires_grad=True)
    y = F.pad(x, (pad, pad, pad, pad), mode="reflect") if pad else x * 1.0
    dx, = torch.autograd.grad((y * g).sum(), [x])
    return dx.permute(0, 2, 3, 1).reshape(N * H * W, stride)


def fold_bound(xp, N, H, W, pad, prec):
    """(rel, extra): a pixel sums at most 3 x 3 sources in fp32: at most 8 roundings of partial sums within the sum of the
    sources' magnitudes, itself the fold of |xp|; the bf16 store adds one rounding step."""
    return (BF16_STEP if prec == "bf16" else 0.0), 8 * U * float(ref_reflect_fold(xp.double().abs(), N, H, W, pad).max())


# ---------------------------------------------------------------------------------------------------------------------------
# 10. v2v_instance_mean_planar: out[c][p] = mean of feat[c][q] over the pixels q with inst[q] == inst[p]
# ---------------------------------------------------------------------------------------------------------------------------
SEG_SLOTS = 4096
INSTANCE_CASES = {"a": (1, 1), "b": (3, 9000), "c": (2, 8192), "d": (2, 10000)}         # name -> (C, HW)
COLLIDING = (7, 26001, -5)                 # case b: id, id + 4096 and id + 8192 of each share a hash bucket
PAIR_GAP = 0.1                             # cases c, d: the two pixels of an id differ by at least this in every channel


def seg_hash(ids):
    """The bucket an id probes first: (uint32(id) * 2654435761) & 4095."""
    return ((ids.long() & 0xFFFFFFFF) * 2654435761) & (SEG_SLOTS - 1)


@functools.lru_cache(maxsize=None)
def instance_case(name):
    """(feat [C][HW] fp32, inst [HW] fp32 holding integers)."""
    Cc, HW = INSTANCE_CASES[name]
    g = _gen(1000 + HW)
    if name == "a":
        return torch.randn(Cc, HW, generator=g), torch.tensor([26001.0])
    if name == "b":
        ids = [0, -1, 26002, 1000, -70000] + [b + k * SEG_SLOTS for b in COLLIDING for k in range(3)]
        extra = torch.randperm(50000, generator=g)[:80] + 30000
        ids += [int(v) for v in extra if int(v) not in ids][:40 - len(ids)]
        ids = torch.tensor(ids)
        assert len(ids) == 40 and len(torch.unique(ids)) == 40
        weight = torch.rand(40, generator=g) ** 3 + 0.01                            # uneven instance sizes
        pick = torch.multinomial(weight, HW, replacement=True, generator=g)
        pick[torch.randperm(HW, generator=g)[:40]] = torch.arange(40)               # every id occurs, in scattered places
        return torch.randn(Cc, HW, generator=g), ids[pick].float()
    n_ids = HW // 2
    ids = torch.randperm(1 << 21, generator=g)[:n_ids] - (1 << 20)                  # distinct, both signs, exact in fp32
    inst = torch.cat([ids, ids])[torch.randperm(HW, generator=g)]
    first = torch.randn(Cc, n_ids, generator=g)
    gap = (PAIR_GAP + 0.05 + torch.rand(Cc, n_ids, generator=g)) * torch.where(torch.rand(Cc, n_ids, generator=g) < 0.5, -1.0, 1.0)
    feat = torch.empty(Cc, HW)
    order = torch.argsort(inst, stable=True)                                        # the two pixels of an id, adjacent
    feat[:, order[0::2]] = first
    feat[:, order[1::2]] = first + gap
    pair = feat[:, order[0::2]].double() - feat[:, order[1::2]].double()
    assert float(pair.abs().min()) >= PAIR_GAP and torch.equal(inst[order[0::2]], inst[order[1::2]])
    return feat, inst.float()


def ref_instance_mean(feat, inst, merge=None):
    """fp64 [C][HW] segmented mean.  merge: a function applied to the ids first (the mutation that merges colliding ids)."""
    ids = inst.long() if merge is None else merge(inst.long())
    _, inv, cnt = torch.unique(ids, return_inverse=True, return_counts=True)
    sums = torch.zeros(feat.shape[0], cnt.numel(), dtype=torch.float64).index_add_(1, inv, feat.double())
    return (sums / cnt)[:, inv]


def instance_mean_extra(feat, inst):
    """The absolute bound per pixel.  Recursive summation of n values in ANY order is off by at most (n - 1) u sum|x| (to first
    order); the kernel adds each instance's values with float atomics in LDS and the per-run sums with atomics in memory, an
    order that changes from run to run but is still some order of at most n additions; the pixel count is exact, the division
    one more rounding: (n + 2) u sum|x| / n, no measured number in it."""
    _, inv, cnt = torch.unique(inst.long(), return_inverse=True, return_counts=True)
    abs_sums = torch.zeros(feat.shape[0], cnt.numel(), dtype=torch.float64).index_add_(1, inv, feat.double().abs())
    return ((cnt + 2) * U * abs_sums / cnt)[:, inv]


# ---------------------------------------------------------------------------------------------------------------------------
# 11. v2v_memset_zero, v2v_memcpy_d2d
# ---------------------------------------------------------------------------------------------------------------------------
COPY_BYTES = (1, 15, 16, 17, 4099)
COPY_BASES = (0, 1)                        # bytes off 16-byte alignment
