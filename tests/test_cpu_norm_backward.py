"""CPU-side checks behind tests/test_gpu_norm_backward.py (v2v_bn_backward / v2v_channel_sum / v2v_act_backward, csrc/norm_act.hip):
the fp64 references of tests/norm_bwd_common.py against torch autograd, what the GPU tests' bounds reject, argument validation
and workspace sizing through the library in dry-run mode."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import norm_bwd_common as NB
from norm_bwd_common import ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID

EINVAL = -1
F32, BF16 = 0, 1


# ---------------------------------------------------------------------------------------------------------------------------
# the references against autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _torch_act(x, act, slope):
    return {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LEAKY: lambda t: F.leaky_relu(t, slope),
            ACT_TANH: torch.tanh, ACT_SIGMOID: torch.sigmoid}[act](x)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LEAKY])
@pytest.mark.parametrize("C_", [3, 66])
@pytest.mark.parametrize("nhw", [(1, 3, 5), (1, 5, 13), (2, 20, 25)])
def test_reference_equals_autograd_of_batch_norm(nhw, C_, act):
    """With the true batch statistics ref_bn_backward is the fp64 autograd gradient of F.batch_norm(training=True) + act."""
    N, H, W = nhw
    P = N * H * W
    c = NB.make_case(P, C_, act, 31 + P + C_)
    x = c["raw"].double().reshape(N, H, W, C_).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gamma, beta = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    y = _torch_act(F.batch_norm(x, None, None, gamma, beta, training=True, eps=NB.EPS), act, c["slope"])
    dy = c["dy"].double().reshape(N, H, W, C_).permute(0, 3, 1, 2).contiguous()
    dx, dg, db = torch.autograd.grad((y * dy).sum(), [x, gamma, beta])
    draw, dgamma, dbeta = NB.ref_bn_backward(c["dy"], c["raw"], NB.batch_stats(c["raw"], c["gamma"], c["beta"]), act, c["slope"])
    NB.check(draw, dx.permute(0, 2, 3, 1).reshape(P, C_), 1e-10, 1e-10, "draw")
    NB.check(dgamma, dg, 1e-10, 1e-10, "dgamma")
    NB.check(dbeta, db, 1e-10, 1e-10, "dbeta")


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LEAKY])
def test_reference_equals_autograd_of_instance_norm_batch_1(act):
    """get_norm_layer('instance') at batch 1 shares the kernel: F.instance_norm without affine parameters."""
    H, W, C_ = 5, 13, 66
    P = H * W
    c = NB.make_case(P, C_, act, 77)
    one, zero = torch.ones(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64)
    stats = NB.batch_stats(c["raw"], one, zero)
    pre = c["raw"].double() * stats[0] + stats[1]
    assert float(pre.abs().min()) > 0
    x = c["raw"].double().reshape(1, H, W, C_).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = _torch_act(F.instance_norm(x, eps=NB.EPS), act, c["slope"])
    # (contiguous: torch's CPU instance_norm backward misreads a permuted grad_output)
    dx, = torch.autograd.grad((y * c["dy"].double().reshape(1, H, W, C_).permute(0, 3, 1, 2).contiguous()).sum(), [x])
    draw, _, _ = NB.ref_bn_backward(c["dy"], c["raw"], stats, act, c["slope"])
    NB.check(draw, dx.permute(0, 2, 3, 1).reshape(P, C_), 1e-10, 1e-10, "draw")


@pytest.mark.parametrize("scale", [1.0, 20.0, 0.5])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID])
def test_act_reference_equals_autograd(act, scale):
    g = torch.Generator().manual_seed(act)
    x = (torch.randn(40, 7, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    dy = torch.randn(40, 7, generator=g, dtype=torch.float64)
    y = _torch_act(x, act, NB.SLOPE) * scale
    dx, = torch.autograd.grad((y * dy).sum(), [x])
    got = NB.ref_act_backward(dy, None if act == ACT_NONE else y.detach(), act, NB.SLOPE, scale)
    NB.check(got, dx, 1e-10, 1e-10, NB.ACT_NAMES[act])


def test_make_case_keeps_every_pre_activation_off_the_kink():
    for name in ("a", "b", "c", "e"):
        for act in NB.BN_ACTS[name]:
            c = NB.bn_case(name, act)
            pre = c["raw"].double() * c["stats"][0].double() + c["stats"][1].double()
            assert float(pre.abs().min()) >= NB.PRE_MARGIN
            m = c["raw"].double().mean(0)
            assert c["raw"].dtype == torch.float32 and c["stats"].dtype == torch.float32 and c["stats"].shape == (4, c["raw"].shape[1])
            if c["raw"].shape[0] > 1000:
                assert float(m.abs().max()) > 1.0                      # nonzero means: xhat needs the subtraction


# ---------------------------------------------------------------------------------------------------------------------------
# what the bounds of the GPU tests reject
# ---------------------------------------------------------------------------------------------------------------------------
PERTURBATIONS = ("last_pixel", "last_block", "slab_end_coef", "k_swapped", "slope_zero", "pad_lane_mean")


def _applies(kind, P, C_, act):
    """A perturbation that cannot change anything for a shape is not a gap of the shape: it has nothing to get wrong."""
    if kind == "slab_end_coef":
        return C_ >= 2                       # one channel has no neighbour
    if kind == "slope_zero":
        return act == ACT_LEAKY              # the slope is read by LeakyReLU alone
    if kind == "pad_lane_mean":
        return C_ % 4 >= 2                   # the last 4-channel vector holds pad lanes AND a real channel besides C - 1
    return True


def _perturbed(c, act, kind):
    """ref_bn_backward as a subtly wrong kernel would compute it (fp64)."""
    dy, raw, stats = c["dy"].double(), c["raw"].double(), c["stats"].double()
    scale, shift, mean, invstd = stats
    P, C_ = dy.shape
    slope = 0.0 if kind == "slope_zero" else c["slope"]
    if kind == "pad_lane_mean":              # the clamp `c0 + q < C ? c0 + q : C - 1` applied to the whole last vector
        mean = mean.clone()
        mean[C_ // 4 * 4:] = mean[C_ - 1]
    g = dy * NB.act_grad_pre(raw * scale + shift, act, slope)
    xhat = (raw - mean) * invstd
    keep = P
    if kind == "last_pixel":
        keep = P - 1
    elif kind == "last_block":
        ppb, nblk = NB.bn_blocks(P, C_)
        keep = (nblk - 1) * ppb
    dbeta = g[:keep].sum(0)
    dgamma = (g[:keep] * xhat[:keep]).sum(0)
    k1, k2 = dbeta / P, dgamma / P
    if kind == "k_swapped":
        k1, k2 = k2, k1
    if kind == "slab_end_coef":              # the last channel of every 64-channel slab reads the coefficients one slot early
        last = [c_ for c_ in range(C_) if c_ % 64 == 63 or c_ == C_ - 1]
        k1, k2 = k1.clone(), k2.clone()
        for c_ in last:
            k1[c_], k2[c_] = k1[c_ - 1], k2[c_ - 1]
    return scale * (g - k1 - xhat * k2), dgamma, dbeta


def _rejected(got, ref, bound):
    try:
        NB.check(got, ref, *bound)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", sorted(NB.BN_CASES))
def test_bounds_reject_a_subtly_wrong_bn_backward(name):
    """Every listed slip moves at least one output of every GPU case past the bound that output is held to, under both dtypes'
    bounds.  Case f is drawn at 260 of its 4160 pixels: 33 slabs and a last block remain, the 8.8 M-element arrays add nothing."""
    P, C_ = NB.BN_CASES[name][:2]
    if name == "f":
        P = 260
    for act in NB.BN_ACTS[name]:
        c = NB.make_case(P, C_, act, 1) if name == "f" else NB.bn_case(name, act)
        ref = NB.ref_bn_backward(c["dy"], c["raw"], c["stats"], act, c["slope"])
        assert not any(_rejected(r, r, b) for r, b in zip(ref, (NB.DRAW_BOUND["fp32"], NB.SUM_BOUND, NB.SUM_BOUND)))
        for kind in PERTURBATIONS:
            bad = _perturbed(c, act, kind)
            if not _applies(kind, P, C_, act):
                assert all(torch.equal(b, r) for b, r in zip(bad, ref)), (name, kind)
                continue
            for prec in ("fp32", "bf16") if name not in NB.BN_FP32_ONLY else ("fp32",):
                caught = [_rejected(bad[0], ref[0], NB.DRAW_BOUND[prec]), _rejected(bad[1], ref[1], NB.SUM_BOUND),
                          _rejected(bad[2], ref[2], NB.SUM_BOUND)]
                assert any(caught), "case %s %s: '%s' passes the %s bounds" % (name, NB.ACT_NAMES[act], kind, prec)
                if kind in ("slab_end_coef", "k_swapped"):             # these leave the sums alone: dRaw has to show them
                    assert caught[0], (name, kind, prec)


@pytest.mark.parametrize("case", NB.SUM_CASES)
def test_bounds_reject_a_channel_sum_that_drops_pixels(case):
    P, C_, _ = case
    x = NB.sum_case(P, C_)
    ref = NB.ref_channel_sum(x)
    ppb, nblk = NB.blocks(P)
    for keep in (P - 1, (nblk - 1) * ppb):
        assert _rejected(x[:keep].double().sum(0), ref, NB.SUM_BOUND), (case, keep)


def test_act_bounds_reject_a_dropped_slope_and_an_unscaled_derivative():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(63, 66, generator=g, dtype=torch.float64) * 1.5
    dy = torch.randn(63, 66, generator=g)
    for prec in ("fp32", "bf16"):
        y = F.leaky_relu(x, NB.SLOPE) * 20
        ref = NB.ref_act_backward(dy, y, ACT_LEAKY, NB.f32(NB.SLOPE), 20.0)
        assert _rejected(NB.ref_act_backward(dy, y, ACT_LEAKY, 0.0, 20.0), ref, NB.ACT_BOUND[prec])
        y = torch.tanh(x) * 20
        ref = NB.ref_act_backward(dy, y, ACT_TANH, 0.0, 20.0)
        assert _rejected(dy.double() * (1 - y * y) * 20, ref, NB.ACT_BOUND[prec])       # y taken as the unscaled tanh


# ---------------------------------------------------------------------------------------------------------------------------
# argument validation and workspace sizing (library in dry-run mode: nothing launches)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dry_run():
    from vid2vid_amd.lib import lib
    prev = lib.v2v_set_dry_run(1)
    yield lib
    lib.v2v_set_dry_run(prev)


def _buf():
    t = torch.zeros(1 << 16)
    assert t.data_ptr() % 16 == 0
    return t


def _bn_call(lib, p, **kw):
    a = dict(dy=p, raw=p, cs_raw=16, st=p, dr=p, cs_out=16, dg=p, db=p, acc=0, ws=p, P=252, C=13, cs=16, act=ACT_RELU, dt=F32)
    a.update(kw)
    return lib.v2v_bn_backward(a["dy"], a["raw"], a["cs_raw"], a["st"], a["dr"], a["cs_out"], a["dg"], a["db"], a["acc"], a["ws"],
                               a["P"], a["C"], a["cs"], a["act"], 0.2, a["dt"], None)


def test_bn_backward_validates_its_arguments(dry_run):
    lib = dry_run
    t = _buf()
    p = C.c_void_p(t.data_ptr())
    assert _bn_call(lib, p) == 0, lib.v2v_last_error()
    assert _bn_call(lib, p, dg=None, db=None) == 0 and _bn_call(lib, p, dt=BF16) == 0 and _bn_call(lib, p, cs=13, cs_raw=13) == 0
    for act in (ACT_NONE, ACT_RELU, ACT_LEAKY):
        assert _bn_call(lib, p, act=act) == 0
    off = C.c_void_p(t.data_ptr() + 4)
    for bad in (dict(cs_out=18), dict(cs_out=14, C=13), dict(C=17), dict(C=17, cs=20, cs_out=20), dict(C=17, cs_raw=20, cs_out=20),
                dict(C=17, cs=20, cs_raw=20), dict(dr=off), dict(act=ACT_TANH), dict(act=ACT_SIGMOID), dict(dy=None), dict(raw=None),
                dict(st=None), dict(dr=None), dict(ws=None), dict(P=0), dict(C=0)):
        assert _bn_call(lib, p, **bad) == EINVAL, bad
        assert b"bn_backward" in lib.v2v_last_error(), bad


def _act_call(lib, p, **kw):
    a = dict(dy=p, y=p, g=p, N=1, H=4, W=5, C=3, cs_in=4, cs_out=4, nchw=0, act=ACT_TANH, scale=1.0, dt=F32)
    a.update(kw)
    return lib.v2v_act_backward(a["dy"], a["y"], a["g"], a["N"], a["H"], a["W"], a["C"], a["cs_in"], a["cs_out"], a["nchw"], a["act"],
                                0.2, a["scale"], a["dt"], None)


def test_act_backward_validates_its_arguments(dry_run):
    lib = dry_run
    p = C.c_void_p(_buf().data_ptr())
    assert _act_call(lib, p) == 0, lib.v2v_last_error()
    assert _act_call(lib, p, act=ACT_NONE, y=None) == 0 and _act_call(lib, p, nchw=1) == 0 and _act_call(lib, p, dt=BF16, cs_out=8) == 0
    for bad in (dict(scale=0.0), dict(act=ACT_SIGMOID, scale=0.0), dict(y=None), dict(y=None, act=ACT_RELU), dict(y=None, act=ACT_LEAKY),
                dict(dy=None), dict(g=None), dict(cs_out=6), dict(dt=BF16, cs_out=4), dict(C=5), dict(C=5, cs_out=8)):
        assert _act_call(lib, p, **bad) == EINVAL, bad
        assert b"act_backward" in lib.v2v_last_error(), bad
    assert _act_call(lib, p, act=ACT_RELU, scale=0.0) == 0             # only the activations that divide by out_scale refuse 0


def test_channel_sum_validates_its_arguments(dry_run):
    lib = dry_run
    p = C.c_void_p(_buf().data_ptr())
    assert lib.v2v_channel_sum(p, p, 1, p, 252, 13, 16, F32, None) == 0
    assert lib.v2v_channel_sum(p, p, 0, p, 252, 13, 13, BF16, None) == 0
    for bad in ((None, p, p, 252, 13, 16), (p, None, p, 252, 13, 16), (p, p, None, 252, 13, 16), (p, p, p, 0, 13, 16),
                (p, p, p, 252, 0, 16), (p, p, p, 252, 17, 16)):
        x, out, ws, P, C_, cs = bad
        assert lib.v2v_channel_sum(x, out, 0, ws, P, C_, cs, F32, None) == EINVAL, bad
        assert b"channel_sum" in lib.v2v_last_error()


def test_backward_rows_formula():
    from vid2vid_amd.lib import lib
    ceil = lambda a, b: -(-a // b)
    for P in (1, 63, 64, 65, 4096, 4160, 32768, 32769, 33000, 10 ** 7):
        want = ceil(P, ceil(P, min(ceil(P, 64), 512)))
        assert lib.v2v_bn_backward_rows(P) == want == NB.blocks(P)[1], P
    assert NB.blocks(33000) == (65, 508) and NB.blocks(65) == (33, 2)
    # the rebalancing of v2v_bn_backward only ever lowers the row count the caller sized the workspace for
    assert NB.bn_blocks(4160, 2112) == (65, 64) and NB.blocks(4160) == (64, 65)
    for name, (P, C_) in ((n, v[:2]) for n, v in NB.BN_CASES.items()):
        assert NB.bn_blocks(P, C_)[1] <= NB.blocks(P)[1], name


def test_entry_points_record_under_their_own_names(dry_run):
    lib = dry_run
    p = C.c_void_p(_buf().data_ptr())
    plan = lib.v2v_plan_create()
    try:
        assert lib.v2v_plan_begin_record(plan) == 0
        assert _bn_call(lib, p) == 0
        assert lib.v2v_channel_sum(p, p, 1, p, 252, 13, 16, F32, None) == 0
        assert _act_call(lib, p) == 0
        assert lib.v2v_plan_end_record(plan) == 0
        names = [lib.v2v_plan_op_name(plan, i).decode() for i in range(lib.v2v_plan_num_ops(plan))]
        assert names == ["bn_backward", "channel_sum", "act_backward"]
    finally:
        lib.v2v_plan_destroy(plan)
