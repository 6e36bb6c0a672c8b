"""fp64 CPU references, inputs and the comparison shared by tests/test_cpu_norm_backward.py and tests/test_gpu_norm_backward.py:
v2v_bn_backward, v2v_channel_sum and v2v_act_backward (csrc/norm_act.hip) against the formulas of include/v2v_hip.h."""
import functools

import torch

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID = range(5)
ACT_NAMES = ("none", "relu", "leaky", "tanh", "sigmoid")
SLOPE = 0.2
EPS = 1e-5
PRE_MARGIN = 1e-3         # every pre-activation keeps this distance from 0, where the ReLU / LeakyReLU derivative jumps

# bounds of the GPU tests (|got - ref| <= rel*|ref| + floor*rms(ref)); tests/test_cpu_norm_backward.py shows what they reject
SUM_BOUND = (2e-4, 2e-4)                  # dgamma, dbeta, channel sums: fp32 accumulation, both dtypes
# bf16 outputs: ONE round-to-nearest-even step of the fp32 value v.  bf16 keeps 8 significant bits, so the step is at most half
# an ulp = 2^-8 |v| (reached just above a power of two); the fp32 evaluation error of v itself (~1e-7) falls under the floor.
DRAW_BOUND = {"fp32": (2e-4, 2e-4), "bf16": (2.0 ** -8, 2e-4)}
ACT_BOUND = {"fp32": (1e-6, 1e-6), "bf16": (2.0 ** -8, 1e-6)}     # fp32: elementwise, a handful of roundings

# v2v_bn_backward cases: name -> (P, C, dy stride, raw stride, out stride, element offset of the dy / raw views)
BN_CASES = {
    "a": (1, 1, 4, 4, 4, 0),                  # one pixel, one channel
    "b": (15, 3, 4, 4, 4, 0),                 # empty pixel phases, C % 4 != 0 on the vector path
    "c": (65, 66, 68, 68, 72, 0),             # second slab of 2 channels, 1-pixel last block, pad channels 66..71
    "d": (1000, 130, 136, 132, 132, 0),       # three slabs, all strides different
    "e": (33000, 24, 24, 24, 24, 0),          # block cap: 65 pixels per block, 508 rows, finalizer remainders
    "f": (4160, 2112, 2112, 2112, 2112, 0),   # rebalancing branch: 65 x 33 workgroups > 2048 -> 64 blocks
    "g": (70, 4099, 4100, 4100, 4100, 0),     # 65 slabs: no tickets, the separate finalize launch
    "h1": (130, 70, 70, 72, 72, 0),           # scalar path: dy stride not a multiple of 4
    "h2": (130, 70, 72, 72, 72, 1),           # scalar path: dy and raw one element off 16-byte alignment
}
# activations per case: all three where several slabs and different strides meet, one each elsewhere
BN_ACTS = {"a": (ACT_NONE,), "b": (ACT_LEAKY,), "c": (ACT_NONE, ACT_RELU, ACT_LEAKY), "d": (ACT_NONE, ACT_RELU, ACT_LEAKY),
           "e": (ACT_RELU,), "f": (ACT_LEAKY,), "g": (ACT_NONE,), "h1": (ACT_RELU,), "h2": (ACT_LEAKY,)}
BN_FP32_ONLY = ("f", "g")

# v2v_channel_sum cases: (P, C, stride)
SUM_CASES = [(1, 1, 4), (15, 3, 4), (65, 66, 72), (33000, 24, 24), (70, 4099, 4100), (130, 70, 70)]


def f32(v):
    """The value an fp32 argument of the C ABI carries, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def blocks(P):
    """(pixels per block, partial rows) of the reduce: v2v_bn_backward_rows(P) is the second."""
    nblk = max(1, min(-(-P // 64), 512))
    ppb = -(-P // nblk)
    return ppb, -(-P // ppb)


def bn_blocks(P, C):
    """blocks(P) after v2v_bn_backward's rebalancing (more than 2048 workgroups: fewer, longer pixel blocks)."""
    ppb, nblk = blocks(P)
    slabs = -(-C // 64)
    if nblk * slabs > 2048 and nblk > 64:
        want = max(-(-2048 // slabs), 64)
        if want < nblk:
            ppb = -(-P // want)
            nblk = -(-P // ppb)
    return ppb, nblk


def act_grad_pre(pre, act, slope):
    one = torch.ones_like(pre)
    if act == ACT_RELU:
        return torch.where(pre > 0, one, torch.zeros_like(pre))
    if act == ACT_LEAKY:
        return torch.where(pre > 0, one, one * slope)
    assert act == ACT_NONE
    return one


def ref_bn_backward(dy, raw, stats, act, slope):
    """(draw [P][C], dgamma [C], dbeta [C]) in fp64 from dy [P][C], raw [P][C] and the GIVEN stats [4][C] (scale, shift, mean,
    invstd) as constants -- the formula of include/v2v_hip.h, every operand widened from the dtype the kernel sees."""
    dy, raw, stats = dy.double(), raw.double(), stats.double()
    scale, shift, mean, invstd = stats
    P = dy.shape[0]
    g = dy * act_grad_pre(raw * scale + shift, act, slope)
    xhat = (raw - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    draw = scale * (g - dbeta / P - xhat * (dgamma / P))
    return draw, dgamma, dbeta


def ref_channel_sum(x):
    return x.double().sum(0)


def ref_act_backward(dy, y, act, slope, out_scale):
    """g = dy * act'(.) * out_scale in fp64, with y the SCALED output act(x) * out_scale the kernel is given (None for ACT_NONE)."""
    dy = dy.double()
    s = float(out_scale)
    if act == ACT_NONE:
        return dy * s
    y = y.double()
    if act == ACT_RELU:
        return dy * torch.where(y > 0, torch.full_like(y, s), torch.zeros_like(y))
    if act == ACT_LEAKY:
        return dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)) * s
    t = y / s
    if act == ACT_TANH:
        return dy * ((1 - t * t) * s)
    assert act == ACT_SIGMOID
    return dy * (t * (1 - t) * s)


def batch_stats(raw, gamma, beta, eps=EPS):
    """[4][C] fp64 (scale, shift, mean, invstd) of training-mode BatchNorm2d over the P rows of raw (biased variance)."""
    raw = raw.double()
    mean = raw.mean(0)
    invstd = 1.0 / torch.sqrt(raw.var(0, unbiased=False) + eps)
    scale = gamma * invstd
    return torch.stack([scale, beta - mean * scale, mean, invstd])


@functools.lru_cache(maxsize=None)
def make_case(P, C, act, seed):
    """Inputs of one v2v_bn_backward call: dict(dy [P][C] fp32, raw [P][C] fp32, stats [4][C] fp32, gamma, beta [C] fp64).
    raw has a per-channel mean in [-3, 3] and std in [0.2, 3] (the sums then carry real cancellation); stats are raw's own batch
    statistics with random gamma / beta, cast to fp32.  Every pre-activation raw*scale + shift, evaluated in fp64 from the fp32
    arrays the kernel reads, is at least PRE_MARGIN from 0: the kernel's fp32 pre (off by ~1e-6) picks the same ReLU / LeakyReLU
    branch everywhere, so no element is excluded from any comparison.  Cached: the tensors are shared and must not be modified."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    mean_c = rnd(C) * 6 - 3
    std_c = 0.2 + rnd(C) * 2.8
    raw = (torch.randn(P, C, generator=g, dtype=torch.float64) * std_c + mean_c).float()
    gamma = (0.5 + rnd(C)) * torch.where(rnd(C) < 0.5, -1.0, 1.0)
    beta = (0.05 + 0.95 * rnd(C)) * torch.where(rnd(C) < 0.5, -1.0, 1.0)     # P = 1: pre == beta whatever raw is
    dy = torch.randn(P, C, generator=g)
    for _ in range(50):
        stats = batch_stats(raw, gamma, beta).float()
        scale, shift = stats[0].double(), stats[1].double()
        pre = raw.double() * scale + shift
        close = pre.abs() < PRE_MARGIN
        if not close.any():
            break
        # move the offenders to a pre-activation of +-4 margins (same side), then take the statistics again
        target = torch.where(pre >= 0, 4 * PRE_MARGIN, -4 * PRE_MARGIN)
        raw = torch.where(close, ((target - shift) / scale).float(), raw)
    stats = batch_stats(raw, gamma, beta).float()
    pre = raw.double() * stats[0].double() + stats[1].double()
    assert float(pre.abs().min()) >= PRE_MARGIN, "make_case(%d, %d): a pre-activation is within %g of 0" % (P, C, PRE_MARGIN)
    return dict(dy=dy, raw=raw, stats=stats, gamma=gamma, beta=beta, act=act, slope=f32(SLOPE))


def bn_case(name, act):
    P, C = BN_CASES[name][:2]
    return make_case(P, C, act, 1000 + 17 * sorted(BN_CASES).index(name) + act)


@functools.lru_cache(maxsize=None)
def bn_reference(name, act, prec):
    """(draw, dgamma, dbeta) fp64 of a named case; prec 'bf16': dy as the bf16 values the kernel reads.  Cached, read-only."""
    c = bn_case(name, act)
    dy = c["dy"].bfloat16() if prec == "bf16" else c["dy"]
    return ref_bn_backward(dy, c["raw"], c["stats"], act, c["slope"])


@functools.lru_cache(maxsize=None)
def sum_case(P, C):
    """x [P][C] fp32 for v2v_channel_sum: zero-mean noise with a per-channel scale in [0.5, 2], as the gradients it sums are.  (Around
    a channel mean of 1 the sum of 33000 pixels is 33000 and a dropped pixel would sit inside the 2e-4 bound.)"""
    g = torch.Generator().manual_seed(5000 + P + 7 * C)
    return torch.randn(P, C, generator=g) * (0.5 + 1.5 * torch.rand(C, generator=g))


def rel_err(got, ref):
    """max |got - ref| / (|ref| + rms(ref)): the figure the tests print."""
    got, ref = got.double().cpu(), ref.double()
    rms = float(ref.pow(2).mean().sqrt())
    d = (got - ref).abs()
    if rms == 0.0:
        return float(d.max())
    return float((d / (ref.abs() + rms)).max())


def check(got, ref, rel, floor, what=""):
    """Assert |got - ref| <= rel*|ref| + floor*rms(ref) for every element of a [P][C] or [C] array; the message names the worst
    element's channel and pixel.  Returns rel_err(got, ref)."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    rms = float(ref.pow(2).mean().sqrt())
    err = (got - ref).abs()
    over = err - (rel * ref.abs() + floor * rms)
    over = torch.where(torch.isfinite(got), over, torch.full_like(over, float("inf")))
    worst = int(over.argmax())
    if float(over.reshape(-1)[worst]) > 0:
        Cc = ref.shape[-1]
        pixel, channel = (worst // Cc, worst % Cc) if ref.dim() > 1 else (None, worst)
        raise AssertionError("%s: channel %d%s: got %.9g, want %.9g, |diff| %.3e > %.3e (rel %.3g, floor %.3g x rms %.3e); %d of %d "
                             "elements out of bound" % (what, channel, "" if pixel is None else " pixel %d" % pixel,
                                                        float(got.reshape(-1)[worst]), float(ref.reshape(-1)[worst]),
                                                        float(err.reshape(-1)[worst]),
                                                        rel * abs(float(ref.reshape(-1)[worst])) + floor * rms, rel, floor, rms,
                                                        int((over > 0).sum()), over.numel()))
    return rel_err(got, ref)
