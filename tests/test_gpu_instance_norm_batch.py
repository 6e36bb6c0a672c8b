"""InstanceNorm2d groups at batch > 1 on the GPU (csrc/instance_norm.hip: v2v_in_stats / v2v_in_apply / v2v_in_backward):
per-sample, per-channel statistics exactly as torch.nn.functional.instance_norm defines them -- forward and backward,
fp32 / x3 / bf16, eager and replayed from a plan.

Tolerances are the project's own for the same quantities (util.assert_close, |d| / (|ref| + rms(ref))):
conv + norm + act + residual groups 2e-4 forward / 3e-4 gradients in fp32 and 2e-2 / 4e-2 in bf16
(test_gpu_train_ops.py::test_conv_norm_act_residual_backward), whole networks 1e-3 (north_star), training gradients
2.5e-3 on the norm and 5e-3 on the L2 distance (test_gpu_golden.py::_full_width_train_parity).  The statistics themselves
(v2v_in_stats) are accumulated in fp64 and rounded once to fp32 (2^-24 relative per value, a handful of roundings):
gated at 1e-5.  Kernel-level cases give sample k a scale of 10^k and its own mean, and every sample is compared on its own,
so statistics leaking between samples are an O(1) error, not something a tolerance can hide.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from util import assert_close, sd_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = 0, 1


def _engine(prec="fp32"):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine
    return Engine(DEV, L.BF16 if prec == "bf16" else L.F32)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------
# 1. the group of test_conv_norm_act_residual_backward with InstanceNorm2d at N = 2 and N = 3 (raised NotImplementedError)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["relu", "leaky", "none"])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("affine", [False, True])
def test_conv_instance_norm_act_residual_backward_batched(N, act, prec, affine):
    """ResnetBlock-style group: reflect conv + InstanceNorm2d (training statistics) + activation + two residual adds against
    torch CPU autograd of F.instance_norm.  affine=True is not built by the reference (get_norm_layer) but the engine accepts
    such a norm: dgamma / dbeta are the sums over samples and pixels."""
    from vid2vid_amd import lib as L
    from vid2vid_amd import autograd as AG
    torch.manual_seed(11)
    eng = _engine(prec)
    Cc, H, W = 24, 14, 18
    conv = nn.Conv2d(Cc, Cc, 3)
    norm = nn.InstanceNorm2d(Cc, affine=affine)
    with torch.no_grad():
        conv.weight.normal_(0, 0.2); conv.bias.normal_(0, 0.3)
        if affine:
            norm.weight.normal_(1, 0.2); norm.bias.normal_(0, 0.3)
    rnd = (lambda t: t.bfloat16().float()) if prec == "bf16" else (lambda t: t.clone())
    x, a0, a1 = torch.randn(N, Cc, H, W), torch.randn(N, Cc, H, W), torch.randn(N, Cc, H, W)
    x = x * torch.tensor([1.0, 4.0, 0.25][:N]).view(N, 1, 1, 1) + torch.tensor([0.0, 1.5, -0.5][:N]).view(N, 1, 1, 1)   # samples differ
    xr, a0r, a1r = [rnd(t).requires_grad_(True) for t in (x, a0, a1)]
    cref = nn.Conv2d(Cc, Cc, 3)
    with torch.no_grad():
        cref.weight.copy_(rnd(conv.weight)); cref.bias.copy_(conv.bias)
    raw = cref(F.pad(xr, (1,) * 4, mode="reflect"))
    gam = bet = None
    if affine:
        gam = norm.weight.detach().clone().requires_grad_(True)
        bet = norm.bias.detach().clone().requires_grad_(True)
    h = F.instance_norm(raw, weight=gam, bias=bet, eps=norm.eps)
    h = {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.2), "none": lambda t: t}[act](h)
    yr = h + a0r + a1r
    r = rnd(torch.randn_like(yr))
    (yr * r).sum().backward()

    conv, norm = conv.to(DEV), norm.to(DEV)
    xg, a0g, a1g = [t.to(DEV).requires_grad_(True) for t in (x, a0, a1)]
    code = {"relu": (L.ACT_RELU, 0.0), "leaky": (L.ACT_LEAKY, 0.2), "none": (L.ACT_NONE, 0.0)}[act]
    ya = AG.conv_group(eng, eng.pack(xg), conv, L.PAD_REFLECT, 1, norm, code[0], code[1], eng.pack(a0g), eng.pack(a1g),
                       False, 1.0, "t")
    y = eng.unpack(ya)
    f_tol, g_tol = (2e-4, 3e-4) if prec == "fp32" else (2e-2, 4e-2)
    errs = {"forward": assert_close(y.detach().cpu(), yr.detach(), f_tol, "forward")}
    (y * r.to(DEV)).sum().backward()
    errs["dX"] = assert_close(xg.grad.cpu(), xr.grad, g_tol, "dX")
    errs["d add0"] = assert_close(a0g.grad.cpu(), a0r.grad, g_tol, "d add0")
    errs["d add1"] = assert_close(a1g.grad.cpu(), a1r.grad, g_tol, "d add1")
    errs["dW"] = assert_close(conv.weight.grad.cpu(), cref.weight.grad, g_tol, "dW")
    if affine:
        errs["dgamma"] = assert_close(norm.weight.grad.cpu(), gam.grad, g_tol, "dgamma")
        errs["dbeta"] = assert_close(norm.bias.grad.cpu(), bet.grad, g_tol, "dbeta")
    print("N=%d %s %s affine=%s:" % (N, act, prec, affine), {k: "%.2e" % v for k, v in errs.items()})
    # a conv bias in front of a norm has a mathematically zero gradient: both sides are rounding noise
    assert conv.bias.grad.abs().max().item() < 1e-2 * (conv.weight.grad.abs().max().item() + 1e-6) + 1e-3


# ------------------------------------------------------------------------------------------------------------------
# 2. the three entry points through the C ABI against fp64 numpy
# ------------------------------------------------------------------------------------------------------------------
def _bf16_round(a):
    return torch.from_numpy(a.astype(np.float32)).bfloat16().float().numpy().astype(np.float64)


def _make_raw(N, HW, Cc, raw_bf16, seed):
    """raw [N][HW][cs_raw] on the device (pad channels NaN: nothing may read them into a result) and its fp64 values.
    Sample k: scale 10^k, mean (k + 1) * 2 * scale, so every sample has its own statistics by orders of magnitude."""
    rs = np.random.RandomState(seed)
    cs_raw = (Cc + 7) // 8 * 8 if raw_bf16 else (Cc + 3) // 4 * 4
    x = rs.standard_normal((N, HW, Cc)) * (0.5 + rs.rand(1, 1, Cc))
    scale = (10.0 ** np.arange(N)).reshape(N, 1, 1)
    x = (x + 2.0 * (np.arange(N).reshape(N, 1, 1) + 1)) * scale
    x = _bf16_round(x) if raw_bf16 else x.astype(np.float32).astype(np.float64)
    full = np.full((N, HW, cs_raw), np.nan, dtype=np.float32)
    full[:, :, :Cc] = x
    t = torch.from_numpy(full).to(DEV)
    return (t.bfloat16() if raw_bf16 else t).contiguous(), x, cs_raw


def _ref_stats(x, gamma, beta, eps):
    mean = x.mean(axis=1)                                    # [N][C]
    var = x.var(axis=1)                                      # biased
    invstd = 1.0 / np.sqrt(var + eps)
    g = np.ones_like(mean) if gamma is None else gamma[None].astype(np.float64)
    b = np.zeros_like(mean) if beta is None else beta[None].astype(np.float64)
    sc = g * invstd
    return np.stack([sc, b - mean * sc, mean, invstd], axis=1)   # [N][4][C]


def _act_np(v, act, slope):
    if act == 1: return np.maximum(v, 0.0)
    if act == 2: return np.where(v > 0, v, v * slope)
    if act == 3: return np.tanh(v)
    if act == 4: return 1.0 / (1.0 + np.exp(-v))
    return v


def _workspace(N, HW, Cc):
    from vid2vid_amd.lib import lib
    ws = torch.empty((lib.v2v_in_workspace_bytes(HW, Cc, N) + 7) // 8, dtype=torch.float64, device=DEV)
    tk = torch.zeros(lib.v2v_in_ticket_words(Cc, N), dtype=torch.int32, device=DEV)
    return ws, tk


def _per_sample_close(got, ref, tol, what):
    worst = 0.0
    for n in range(ref.shape[0]):
        worst = max(worst, assert_close(torch.as_tensor(got[n]), torch.from_numpy(np.ascontiguousarray(ref[n])), tol, "%s sample %d" % (what, n)))
    return worst


@pytest.mark.parametrize("raw_bf16", [False, True])
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("HW", [(14, 18), (10, 32), (16, 32)])      # ragged; whole 64-pixel tiles; whole 128 / 256 / 512-pixel tiles
@pytest.mark.parametrize("Cc", [3, 16, 64, 1027])
def test_in_stats_and_apply_against_fp64(Cc, HW, N, raw_bf16):
    from vid2vid_amd.lib import lib, check
    hw = HW[0] * HW[1]
    seed = Cc * 131 + hw * 7 + N + int(raw_bf16)
    raw, x, cs_raw = _make_raw(N, hw, Cc, raw_bf16, seed)
    rs = np.random.RandomState(seed + 1)
    affine = (Cc + N) % 2 == 1
    gamma = (1.0 + 0.2 * rs.standard_normal(Cc)).astype(np.float32) if affine else None
    beta = (0.3 * rs.standard_normal(Cc)).astype(np.float32) if affine else None
    gd = None if gamma is None else torch.from_numpy(gamma).to(DEV)
    bd = None if beta is None else torch.from_numpy(beta).to(DEV)
    eps = 1e-5
    ref_ss = _ref_stats(x, gamma, beta, eps)
    ws, tk = _workspace(N, hw, Cc)
    rdt = BF16 if raw_bf16 else F32
    ss = []
    for run in range(2):
        out = torch.full((N, 4, Cc), float("nan") if run else 7.0, dtype=torch.float32, device=DEV)
        check(lib.v2v_in_stats(_p(raw), rdt, cs_raw, _p(gd), _p(bd), eps, _p(out), _p(ws), _p(tk), N, hw, Cc, None), "in_stats")
        torch.cuda.synchronize()
        ss.append(out)
        assert int(tk.abs().sum().item()) == 0, "ticket words were not re-armed"
    assert torch.equal(ss[0], ss[1]), "v2v_in_stats: two runs differ"
    got = ss[0].cpu().numpy()
    # sample by sample and row by row (scale, shift, mean, invstd), so that no sample hides under another one's magnitude
    e_stats = max(_per_sample_close(got[:, r], ref_ss[:, r], 1e-5, "in_stats row %d" % r) for r in range(4))
    # ---- apply: every activation, with and without residuals, fp32 and bf16 activations ----
    sc, sh = ref_ss[:, 0][:, None, :], ref_ss[:, 1][:, None, :]
    worst = {}
    for dtype in (F32, BF16):
        vec = 8 if dtype == BF16 else 4
        cs = (Cc + vec - 1) // vec * vec
        tdt = torch.bfloat16 if dtype == BF16 else torch.float32
        for act, n_add in ((0, 2), (1, 0), (2, 1), (3, 0), (4, 1)):
            adds = [torch.from_numpy(rs.standard_normal((N, hw, cs)).astype(np.float32)).to(DEV).to(tdt) for _ in range(n_add)] + [None, None]
            ref = _act_np(x * sc + sh, act, 0.2)
            for a in adds[:n_add]:
                ref = ref + a.float().cpu().numpy()[:, :, :Cc].astype(np.float64)
            want_x3 = dtype == F32 and Cc % 4 == 0 and act == 1
            ys = []
            for run in range(2):
                y = torch.full((N, hw, cs), float("nan"), dtype=tdt, device=DEV)
                x3 = torch.zeros((N, hw, 3 * Cc), dtype=torch.bfloat16, device=DEV) if want_x3 else None
                check(lib.v2v_in_apply(_p(raw), rdt, cs_raw, _p(ss[0]), _p(adds[0]), _p(adds[1]), _p(y), _p(x3), N, hw, Cc, cs,
                                       act, 0.2, dtype, None), "in_apply")
                torch.cuda.synchronize()
                ys.append((y, x3))
            assert torch.equal(ys[0][0], ys[1][0]), "v2v_in_apply: two runs differ"
            y, x3 = ys[0]
            if cs > Cc:
                assert float(y[:, :, Cc:].float().abs().max()) == 0.0, "pad channels of y must be zero"
            tol = 2e-2 if dtype == BF16 else 2e-4
            key = ("bf16" if dtype == BF16 else "fp32")
            worst[key] = max(worst.get(key, 0.0), _per_sample_close(y[:, :, :Cc].float().cpu().numpy(), ref, tol, "in_apply act %d" % act))
            if want_x3:                                      # [hi | lo | hi]: hi + lo reproduces y to 2^-16 relative
                hi, lo, hi2 = x3[:, :, :Cc].float(), x3[:, :, Cc:2 * Cc].float(), x3[:, :, 2 * Cc:].float()
                assert torch.equal(hi, hi2) and torch.equal(hi, y.bfloat16().float())
                assert float(((hi + lo) - y).abs().max()) <= 2.0 ** -15 * float(y.abs().max())
    print("C=%d HW=%s N=%d raw %s: stats %.2e apply %s" % (Cc, HW, N, "bf16" if raw_bf16 else "fp32", e_stats,
                                                            {k: "%.2e" % v for k, v in worst.items()}))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("HW", [(14, 18), (10, 32), (16, 32)])
@pytest.mark.parametrize("Cc", [3, 16, 64, 1027])
def test_in_backward_against_fp64(Cc, HW, N, dtype):
    from vid2vid_amd.lib import lib, check
    hw = HW[0] * HW[1]
    seed = Cc * 17 + hw * 3 + N + dtype
    raw, x, cs_raw = _make_raw(N, hw, Cc, False, seed)
    rs = np.random.RandomState(seed + 1)
    gamma = (1.0 + 0.2 * rs.standard_normal(Cc)).astype(np.float32)
    beta = (0.3 * rs.standard_normal(Cc)).astype(np.float32)
    eps = 1e-5
    ws, tk = _workspace(N, hw, Cc)
    ss = torch.empty((N, 4, Cc), dtype=torch.float32, device=DEV)
    check(lib.v2v_in_stats(_p(raw), F32, cs_raw, _p(torch.from_numpy(gamma).to(DEV)), _p(torch.from_numpy(beta).to(DEV)), eps,
                           _p(ss), _p(ws), _p(tk), N, hw, Cc, None), "in_stats")
    st = ss.cpu().numpy().astype(np.float64)                 # the backward pass is checked against the statistics it is given
    sc, sh, mean, inv = [st[:, r][:, None, :] for r in range(4)]
    vec = 8 if dtype == BF16 else 4
    cs = (Cc + vec - 1) // vec * vec
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    tol = 4e-2 if dtype == BF16 else 3e-4
    worst = 0.0
    for act in (0, 1, 2):
        dy_t = torch.from_numpy(rs.standard_normal((N, hw, cs)).astype(np.float32)).to(DEV).to(tdt)
        dy = dy_t.float().cpu().numpy()[:, :, :Cc].astype(np.float64)
        pre = x * sc + sh
        g = dy * {0: np.ones_like(pre), 1: (pre > 0).astype(np.float64), 2: np.where(pre > 0, 1.0, 0.2)}[act]
        xhat = (x - mean) * inv
        ref = sc * (g - g.mean(axis=1, keepdims=True) - xhat * (g * xhat).mean(axis=1, keepdims=True))
        ref_db, ref_dg = g.sum(axis=(0, 1)), (g * xhat).sum(axis=(0, 1))
        outs = []
        for run in range(2):
            dx = torch.full((N, hw, cs), float("nan"), dtype=tdt, device=DEV)
            dg = torch.full((Cc,), 0.5, dtype=torch.float32, device=DEV)
            db = torch.full((Cc,), -0.25, dtype=torch.float32, device=DEV)
            check(lib.v2v_in_backward(_p(dy_t), _p(raw), cs_raw, _p(ss), _p(dx), cs, _p(dg), _p(db), run, _p(ws), _p(tk),
                                      N, hw, Cc, cs, act, 0.2, dtype, None), "in_backward")
            torch.cuda.synchronize()
            assert int(tk.abs().sum().item()) == 0, "ticket words were not re-armed"
            outs.append((dx, dg, db))
        assert torch.equal(outs[0][0], outs[1][0]), "v2v_in_backward: two runs differ"
        dx = outs[0][0]
        if cs > Cc:
            assert float(dx[:, :, Cc:].float().abs().max()) == 0.0, "pad channels of dRaw must be zero"
        worst = max(worst, _per_sample_close(dx[:, :, :Cc].float().cpu().numpy(), ref, tol, "in_backward act %d" % act))
        # run 0 overwrites (accumulate = 0), run 1 adds to what was there
        g_tol = 3e-4 if dtype == F32 else 4e-2
        assert_close(outs[0][1].cpu(), torch.from_numpy(ref_dg), g_tol, "dgamma")
        assert_close(outs[0][2].cpu(), torch.from_numpy(ref_db), g_tol, "dbeta")
        assert_close(outs[1][1].cpu(), torch.from_numpy(ref_dg + 0.5), g_tol, "dgamma (accumulate)")
        assert_close(outs[1][2].cpu(), torch.from_numpy(ref_db - 0.25), g_tol, "dbeta (accumulate)")
    print("C=%d HW=%s N=%d %s: dRaw %.2e" % (Cc, HW, N, "bf16" if dtype == BF16 else "fp32", worst))


# ------------------------------------------------------------------------------------------------------------------
# 3. + 4. whole networks: batch-3 forward == the three batch-1 forwards stacked; batch 2 against the CPU oracle
# ------------------------------------------------------------------------------------------------------------------
def _opt(**kw):
    import types
    d = dict(fp16=False, n_blocks=2, n_blocks_local=1, n_local_enhancers=1, fg=True, no_flow=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.fixture
def precision():
    from vid2vid_amd import networks as N
    def set_(p):
        N.set_precision(p)
        eng = N.get_engine(DEV)
        # the tile selection is pinned: no timing-based search (test_role_split_with_real_networks_equals_single_process pins it the
        # same way, opt.autotune = False), so batch 1 and batch 3 cannot differ by which tile a measurement happened to prefer
        eng.autotune = False
        return eng
    yield set_
    N.set_precision("fp32")


def _first_frame_nets(golden):
    from vid2vid_amd import networks as N
    g = golden("first_frame_nets_32x64")
    gg = N.define_G(11, 3, 0, 8, "global", 2, "instance", 0, [], _opt())
    le = N.define_G(11, 3, 0, 4, "local", 2, "instance", 0, [], _opt())
    gg.load_state_dict(sd_from_npz(g, "sdg.")); le.load_state_dict(sd_from_npz(g, "sdl."))
    torch.manual_seed(5)
    dd = N.define_D(13, 8, 3, "instance", 2, True, [])
    return g, gg.to(DEV), le.to(DEV), dd.to(DEV)


def _inputs(g, n):
    x1 = torch.from_numpy(np.array(g["in.x"]))                       # (1, 11, 32, 64): the golden-pinned sample
    gen = torch.Generator().manual_seed(17)
    xs = [x1] + [x1.roll(7 * k, 3) * (0.5 + 0.5 * k) + 0.3 * k * torch.randn(x1.shape, generator=gen) for k in range(1, n)]
    xd = [torch.randn(1, 13, 64, 96, generator=gen) * (1.0 + k) + 0.5 * k for k in range(n)]
    return torch.cat(xs), torch.cat(xd)


@pytest.mark.parametrize("prec", ["fp32", "x3"])
def test_batch3_forward_equals_three_batch1_forwards(golden, precision, prec):
    """Sample independence: no oracle needed.  Batch 1 is the existing path (golden-pinned in test_gpu_golden.py)."""
    precision(prec)
    g, gg, le, dd = _first_frame_nets(golden)
    x, xd = _inputs(g, 3)
    with torch.no_grad():
        for name, net in (("GlobalGenerator", gg), ("LocalEnhancer", le)):
            whole = net.forward(x.to(DEV)).float().cpu()
            parts = torch.cat([net.forward(x[k:k + 1].to(DEV)).float().cpu() for k in range(3)])
            print(prec, name, "%.2e" % assert_close(whole, parts, 1e-3, "%s batch 3 vs stacked batch 1 (%s)" % (name, prec)))
            if prec == "fp32":
                assert_close(parts[:1], g["out.global" if net is gg else "out.local"], 1e-3, name + " sample 0 vs the reference")
        whole = dd.forward(xd.to(DEV))
        parts = [dd.forward(xd[k:k + 1].to(DEV)) for k in range(3)]
        assert len(whole) == 2 and all(len(f) == 5 for f in whole)
        for i in range(2):
            for j in range(5):                                       # every intermediate feature of every scale
                stacked = torch.cat([parts[k][i][j].float().cpu() for k in range(3)])
                assert_close(whole[i][j].float().cpu(), stacked, 1e-3, "D %d.%d batch 3 vs stacked batch 1 (%s)" % (i, j, prec))


def test_batch2_networks_against_the_cpu_oracle(golden, precision):
    from oracle import vid2vid_oracle as O
    precision("fp32")
    g, gg, le, dd = _first_frame_nets(golden)
    x, xd = _inputs(g, 2)
    cpu = lambda m: {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        e1 = assert_close(gg.forward(x.to(DEV)), O.global_generator(cpu(gg), x, 2, 2), 1e-3, "GlobalGenerator batch 2")
        e2 = assert_close(le.forward(x.to(DEV)), O.local_enhancer(cpu(le), x, 2, 2, 1, 1), 1e-3, "LocalEnhancer batch 2")
        ref = O.multiscale_discriminator(cpu(dd), xd, 3, 2, norm="instance")
        got = dd.forward(xd.to(DEV))
        assert len(got) == len(ref) == 2
        e3 = 0.0
        for i in range(2):
            assert len(got[i]) == len(ref[i]) == 5
            for j in range(5):
                e3 = max(e3, assert_close(got[i][j], ref[i][j], 1e-3, "D %d.%d batch 2" % (i, j)))
    print("batch 2 vs oracle: global %.2e local %.2e D %.2e" % (e1, e2, e3))


@pytest.mark.parametrize("mode", ["x3", "bf16_raw"])
def test_x3_and_bf16_raw_groups_batched(mode):
    """Two chained 64-channel groups (a ResnetBlock's shape) at batch 3.  x3: the fp32 engine's bf16x3 sub-engine runs the
    convolutions and v2v_in_apply writes the next convolution's [hi | lo | hi] operand.  bf16_raw: the conv stores its raw output
    in bf16 (V2V_OUT_RAW_ACT_NHWC) and v2v_in_stats / v2v_in_apply read that.  Against torch CPU, and batch 3 == stacked batch 1."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine
    torch.manual_seed(9)
    if mode == "x3":
        eng, tol = Engine(DEV, L.F32, x3=True), 1e-3
    else:
        eng, tol = Engine(DEV, L.BF16), 2e-2
        eng.raw_bf16 = True
    rnd = (lambda t: t.bfloat16().float()) if mode == "bf16_raw" else (lambda t: t)
    c1, c2 = nn.Conv2d(64, 64, 3), nn.Conv2d(64, 64, 3)
    n1, n2 = nn.InstanceNorm2d(64), nn.InstanceNorm2d(64)
    with torch.no_grad():
        for c in (c1, c2):
            c.weight.normal_(0, 0.1); c.weight.copy_(rnd(c.weight))
    x = rnd(torch.randn(3, 64, 14, 18) * torch.tensor([1.0, 5.0, 0.2]).view(3, 1, 1, 1) + torch.tensor([0.0, 2.0, -1.0]).view(3, 1, 1, 1))
    with torch.no_grad():
        h = F.relu(F.instance_norm(c1(F.pad(x, (1,) * 4, mode="reflect"))))
        want = F.instance_norm(c2(F.pad(rnd(h), (1,) * 4, mode="reflect"))) + x
    c1, c2 = c1.to(DEV), c2.to(DEV)

    def run(xs):
        with torch.no_grad():
            xa = eng.pack(xs.to(DEV))
            ha = eng.conv_group(xa, c1, L.PAD_REFLECT, 1, n1, L.ACT_RELU, 0.0, label="b.c1")
            if mode == "x3":
                assert ha.x3 is not None, "the apply pass did not write the bf16x3 operand"
            return eng.unpack(eng.conv_group(ha, c2, L.PAD_REFLECT, 1, n2, L.ACT_NONE, 0.0, add0=xa, label="b.c2")).float().cpu()
    n0 = len(eng.conv_log)
    whole = run(x)
    if mode == "x3":
        assert all(c.get("x3") for c in eng.conv_log[n0:]) and len(eng.conv_log) == n0 + 2, eng.conv_log[n0:]
    parts = torch.cat([run(x[k:k + 1]) for k in range(3)])
    e1 = assert_close(whole, want, tol, mode + " batch 3 vs torch")
    e2 = assert_close(whole, parts, tol, mode + " batch 3 vs stacked batch 1")
    print(mode, "vs torch %.2e, vs stacked batch 1 %.2e" % (e1, e2))



# ------------------------------------------------------------------------------------------------------------------
# 5. one training step of a CompositeGenerator(norm='instance') at batch 2 + plan / hipGraph replay of the same model
# ------------------------------------------------------------------------------------------------------------------
def test_composite_generator_instance_batch2_training_step_and_replay(precision):
    from oracle import vid2vid_oracle as O
    from vid2vid_amd import lib as L
    from vid2vid_amd import networks as N
    from vid2vid_amd.engine import Plan
    eng = precision("fp32")
    torch.manual_seed(21)
    net = N.define_G(12, 3, 6, 8, "composite", 2, "instance", 0, [], _opt(fg=False))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(4.0)                                              # N(0, 0.02) init: lift the signal through the 7x7 stems
        net.model_final_flow[1].weight.mul_(0.1)
    gen = torch.Generator().manual_seed(3)
    B, H, W = 2, 32, 64
    x = torch.randn(B, 12, H, W, generator=gen) * torch.tensor([1.0, 3.0]).view(B, 1, 1, 1)
    prev = torch.tanh(torch.randn(B, 6, H, W, generator=gen))
    rs = [torch.randn(B, c, H, W, generator=gen) for c in (3, 2, 1)]
    # ---- CPU oracle, differentiable ----
    sd = {k: v.detach().clone().float() for k, v in net.state_dict().items()}
    names = [k for k, _ in net.named_parameters()]
    for k in names:
        sd[k].requires_grad_(True)
    ref = O.composite_generator(sd, x, prev, None, 2, 2, False, norm="instance")
    sum((o * r).sum() for o, r in zip(ref[:3], rs)).backward()
    # ---- product: eager training step ----
    net.to(DEV)
    got = net.forward(x.to(DEV), prev.to(DEV), None, None, None, None, False)
    for name, o, want in zip(["img_final", "flow", "weight"], got[:3], ref[:3]):
        assert_close(o.detach(), want.detach(), 1e-3, name)
    sum((o * r.to(DEV)).sum() for o, r in zip(got[:3], rs)).backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    flat_g = torch.cat([params[k].grad.detach().float().cpu().reshape(-1) for k in names])
    flat_r = torch.cat([sd[k].grad.reshape(-1) if sd[k].grad is not None else torch.zeros(sd[k].numel()) for k in names])
    assert torch.isfinite(flat_g).all() and flat_r.norm() > 0
    norm_err = abs(flat_g.norm().item() - flat_r.norm().item()) / flat_r.norm().item()
    l2_err = (flat_g - flat_r).norm().item() / flat_r.norm().item()
    print("CompositeGenerator(instance) batch 2: gradient norm rel err %.3e, L2 rel err %.3e" % (norm_err, l2_err))
    assert norm_err <= 2.5e-3 and l2_err <= 5e-3, (norm_err, l2_err)
    # ---- the same model under plan recording / graph replay (inference), twin chains allowed as in the frame plan ----
    xd, pd = x.to(DEV), prev.to(DEV)
    with torch.no_grad():
        eager = [o.clone() for o in net.forward(xd, pd, None, None, None, None, False)[:4]]
        eng.twin_enabled = True
        try:
            plan = Plan()
            eng.plan = plan
            try:
                with plan:
                    outs = net.forward(xd, pd, None, None, None, None, False)[:4]
            finally:
                eng.plan = None
        finally:
            eng.twin_enabled = False
        ops = [L.lib.v2v_plan_op_name(plan.h, i).decode() for i in range(plan.num_ops)]
        assert "in_stats" in ops and "in_apply" in ops and "bn_finalize" not in ops, sorted(set(ops))
        plan.instantiate_graph()
        for o in outs:
            o.fill_(float("nan"))
        plan.launch()
        torch.cuda.synchronize()
        for name, a, b in zip(["img_final", "flow", "weight", "img_raw"], outs, eager):
            assert torch.equal(a, b), "%s: graph replay differs from the eager run" % name
        plan.launch()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "second replay differs"


# ------------------------------------------------------------------------------------------------------------------
# 6. N = 1 is unchanged: the launches of one InstanceNorm2d group, as a run of the parent commit recorded them
# ------------------------------------------------------------------------------------------------------------------
N1_PLAN_OPS = {      # (op, label) of the recorded group: the conv finalizes the statistics in its own launch, then bn_apply
    "fp32": [("conv_igemm", "g"), ("bn_apply", "g.apply")],
    "bf16": [("conv_igemm", "g"), ("bn_apply", "g.apply")],
}
N1_CONV_TILE = {"fp32": 4, "bf16": 4}      # conv_log tile of the eager and of the recorded launch


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_batch1_instance_norm_group_keeps_its_launches(prec):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Plan
    torch.manual_seed(3)
    eng = _engine(prec)
    conv = nn.Conv2d(24, 24, 3).to(DEV); norm = nn.InstanceNorm2d(24).to(DEV)
    x = torch.randn(1, 24, 14, 18, device=DEV)
    with torch.no_grad():
        xa = eng.pack(x)
        ref = eng.unpack(eng.conv_group(xa, conv, L.PAD_REFLECT, 1, norm, L.ACT_RELU, 0.0, add0=xa, label="g"))
        plan = Plan(); eng.plan = plan
        try:
            with plan:
                y = eng.conv_group(xa, conv, L.PAD_REFLECT, 1, norm, L.ACT_RELU, 0.0, add0=xa, label="g")
        finally:
            eng.plan = None
    ops = [(L.lib.v2v_plan_op_name(plan.h, i).decode(), L.lib.v2v_plan_op_label(plan.h, i).decode()) for i in range(plan.num_ops)]
    assert ops == N1_PLAN_OPS[prec], ops
    assert [(c["label"], c["tile"]) for c in eng.conv_log] == [("g", N1_CONV_TILE[prec])] * 2, eng.conv_log
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(eng.unpack(y), ref)
    want = F.relu(F.instance_norm(F.conv2d(F.pad(x, (1,) * 4, mode="reflect"), conv.weight, conv.bias), eps=norm.eps)) + x
    assert_close(ref, want.cpu(), 2e-4 if prec == "fp32" else 2e-2, "batch-1 group")
