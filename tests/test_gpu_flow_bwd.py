"""Backward passes of FlowNet2's three native ops on the MI355X (csrc/flow_ops_bwd.hip, vid2vid_amd/flownet2_ops.py) against
the reference's own backward kernels executed on the host (oracle/ref_ops.py) and torch autograd of the CPU oracle.

Gate: the project's bar for fp32 ops, <= 1e-3 by tests/util.py's per-element relative metric.  Every figure is printed before
it is asserted (run with -s to see them)."""
import ctypes as C

import pytest
import torch

from util import assert_close, rel_err
from flow_bwd_common import (CORR_CASES, FLOWNETC, away_from_integers, randn, autograd_correlation, autograd_resample2d,
                             autograd_channelnorm)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _close(got, ref, what):
    print("%-78s rel err %.3e" % (what, rel_err(got, ref)))
    return assert_close(got, ref, what=what)


def _corr_backward(a, b, go, params, want=(True, True)):
    from vid2vid_amd import lib
    pad, k, md, s1, s2 = params
    n, c, h, w = a.shape
    ad, bd, gd = a.to(DEV), b.to(DEV), go.to(DEV)
    g1 = torch.full(a.shape, float("nan"), device=DEV) if want[0] else None       # NaN: every element must be written
    g2 = torch.full(a.shape, float("nan"), device=DEV) if want[1] else None
    lib.check(lib.lib.v2v_correlation_backward(P(ad), P(bd), P(gd), P(g1), P(g2), n, c, h, w, go.shape[1], go.shape[2], go.shape[3],
                                               pad, k, md, s1, s2, 1, _stream()), "correlation_backward")
    torch.cuda.synchronize()
    return g1, g2


@pytest.mark.parametrize("case", CORR_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_correlation_backward_vs_autograd_of_the_oracle(case):
    """v2v_correlation_backward (C ABI) against torch autograd of the CPU oracle's correlation with a random grad_out: FlowNetC's
    parameter set at C = 256 (the LDS tile kernel; 12x20 and a ragged 13x23), the same class with 5 x 5 displacements, two pixel
    tiles and a ragged channel group, and three generic sets (kernel_size 3, stride1 2, pad != max_displacement).  The forward entry
    is checked on the same inputs, so the pair is an operator and its adjoint.  Both gradients twice: bit-identical (gather form).
    Measured on the MI355X (maximum over the cases): forward 2.2e-6, grad_in1 2.1e-6,
    grad_in2 1.6e-6, all three at C = 256."""
    from vid2vid_amd import lib
    from oracle import vid2vid_oracle as O
    n, c, h, w = case[:4]
    params = case[4:]
    a, b = randn((n, c, h, w), 101), randn((n, c, h, w), 102)
    ref_out = O.correlation(a, b, *params)
    go = randn(tuple(ref_out.shape), 103)
    out = torch.full(ref_out.shape, float("nan"), device=DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    lib.check(lib.lib.v2v_correlation_forward(P(ad), P(bd), P(out), n, c, h, w, *params, 1, _stream()), "correlation_forward")
    _close(out.cpu(), ref_out, "correlation forward %s" % (case,))
    r1, r2 = autograd_correlation(a, b, go, params)
    g1, g2 = _corr_backward(a, b, go, params)
    _close(g1.cpu(), r1, "correlation grad_in1 %s" % (case,))
    _close(g2.cpu(), r2, "correlation grad_in2 %s" % (case,))
    h1, h2 = _corr_backward(a, b, go, params)
    assert torch.equal(g1, h1) and torch.equal(g2, h2), "correlation backward is not bit-identical across two calls"
    # one gradient at a time gives the same bits
    o1, none = _corr_backward(a, b, go, params, want=(True, False))
    assert none is None and torch.equal(o1, g1)
    none, o2 = _corr_backward(a, b, go, params, want=(False, True))
    assert none is None and torch.equal(o2, g2)


def _resample_backward(img, flow, go, k=1, want=(True, True)):
    from vid2vid_amd import lib
    n, c, h, w = img.shape
    oh, ow = flow.shape[2:]
    gi = torch.full(img.shape, float("nan"), device=DEV) if want[0] else None      # zeroed inside the call
    gf = torch.full(flow.shape, float("nan"), device=DEV) if want[1] else None
    imd, fld, gd = img.to(DEV), flow.to(DEV), go.to(DEV)
    lib.check(lib.lib.v2v_resample2d_backward(P(imd), P(fld), P(gd), P(gi), P(gf), n, c, h, w, oh, ow, k, _stream()), "resample2d_backward")
    torch.cuda.synchronize()
    return gi, gf


def _ref_ops():
    from oracle import ref_ops as R
    if not R.available():
        pytest.skip("oracle/_ref/libref_ops.so was not shipped")
    return R


def test_resample2d_backward_vs_autograd_of_the_oracle():
    """grad_img / grad_flow against torch autograd of the CPU oracle's resample2d; flows leave the image on every side and keep
    1e-3 away from integer positions by construction (no element is masked out).  kernel_size 1 (FlowNet2's) and 3 (image two
    rows / columns larger than the flow).  grad_flow is bit-identical across two calls; grad_img (float atomics) is not required to be."""
    for (n, c, h, w, k, seed) in [(2, 3, 13, 17, 1, 7), (1, 8, 32, 48, 1, 8), (2, 3, 9, 11, 3, 9)]:
        img = randn((n, c, h + k - 1, w + k - 1), seed)
        flow = away_from_integers(n, h, w, seed + 50)
        go = randn((n, c, h, w), seed + 100)
        ri, rf = autograd_resample2d(img, flow, go, k)
        gi, gf = _resample_backward(img, flow, go, k)
        _close(gi.cpu(), ri, "resample2d grad_img  k=%d %s" % (k, (n, c, h, w)))
        _close(gf.cpu(), rf, "resample2d grad_flow k=%d %s" % (k, (n, c, h, w)))
        gi2, gf2 = _resample_backward(img, flow, go, k)
        assert torch.equal(gf, gf2), "grad_flow is not bit-identical across two calls"
        _close(gi2.cpu(), ri, "resample2d grad_img, second call into the same kind of buffer")
        none, gf3 = _resample_backward(img, flow, go, k, want=(False, True))
        assert none is None and torch.equal(gf3, gf)
        gi3, none = _resample_backward(img, flow, go, k, want=(True, False))
        assert none is None
        _close(gi3.cpu(), ri, "resample2d grad_img alone")


@pytest.mark.ref_checker
def test_resample2d_and_channelnorm_backward_vs_executed_reference_kernels():
    """Against the reference's OWN backward kernel bodies executed on host cores (oracle/ref_ops.py): resample2d_kernel.cu:67-190
    and channelnorm_kernel.cu:63-96, kernel_size 1 / norm_deg 2 as FlowNet2 uses them."""
    R = _ref_ops()
    from vid2vid_amd import lib
    for (n, c, h, w, seed) in [(2, 3, 13, 17, 21), (1, 8, 32, 48, 22)]:
        img, flow, go = randn((n, c, h, w), seed), away_from_integers(n, h, w, seed + 50), randn((n, c, h, w), seed + 100)
        ri, rf = R.resample2d_backward(img, flow, go, 1)
        gi, gf = _resample_backward(img, flow, go, 1)
        _close(gi.cpu(), ri, "resample2d grad_img  vs the reference kernel %s" % ((n, c, h, w),))
        _close(gf.cpu(), rf, "resample2d grad_flow vs the reference kernel %s" % ((n, c, h, w),))
    for (n, c, h, w, seed) in [(2, 3, 13, 17, 31), (1, 6, 32, 48, 32)]:
        x, go = randn((n, c, h, w), seed), randn((n, 1, h, w), seed + 1)
        out = R.channelnorm(x)
        ref = R.channelnorm_backward(x, out, go)
        g = torch.full(x.shape, float("nan"), device=DEV)
        xd, od, gd = x.to(DEV), out.to(DEV), go.to(DEV)
        lib.check(lib.lib.v2v_channelnorm_backward(P(xd), P(od), P(gd), P(g), n, c, h, w, 2, _stream()), "channelnorm_backward")
        _close(g.cpu(), ref, "channelnorm backward vs the reference kernel %s" % ((n, c, h, w),))


def test_channelnorm_backward_vs_autograd_of_the_oracle():
    from vid2vid_amd import lib
    from oracle import vid2vid_oracle as O
    for (n, c, h, w, seed) in [(2, 3, 13, 17, 41), (1, 6, 32, 48, 42)]:
        x, go = randn((n, c, h, w), seed), randn((n, 1, h, w), seed + 1)
        ref = autograd_channelnorm(x, go)
        g = torch.full(x.shape, float("nan"), device=DEV)
        xd, od, gd = x.to(DEV), O.channelnorm(x).to(DEV), go.to(DEV)
        lib.check(lib.lib.v2v_channelnorm_backward(P(xd), P(od), P(gd), P(g), n, c, h, w, 2, _stream()), "channelnorm_backward")
        _close(g.cpu(), ref, "channelnorm backward vs autograd %s" % ((n, c, h, w),))


def test_modules_autograd_equals_the_oracle():
    """torch.autograd.grad of a scalar loss through Correlation / Resample2d / ChannelNorm (vid2vid_amd.flownet2_ops) equals the
    same through the oracle functions on the CPU; needs_input_grad subsets; a non-contiguous input; a chain of the three."""
    from vid2vid_amd import flownet2_ops as F2
    from oracle import vid2vid_oracle as O
    # Correlation, FlowNetC's set at a small channel count and a generic set
    for (n, c, h, w, params) in [(1, 16, 10, 36, FLOWNETC), (2, 5, 11, 14, (4, 3, 4, 2, 1))]:
        a, b = randn((n, c, h, w), 61), randn((n, c, h, w), 62)
        wgt = randn(tuple(O.correlation(a, b, *params).shape), 63)
        r1, r2 = autograd_correlation(a, b, wgt, params)
        ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        out = F2.Correlation(*params, 1)(ad, bd)
        g1, g2 = torch.autograd.grad((out * wgt.to(DEV)).sum(), [ad, bd])
        _close(g1.cpu(), r1, "Correlation module grad 1 %s" % (params,))
        _close(g2.cpu(), r2, "Correlation module grad 2 %s" % (params,))
        # only the second input asks for a gradient
        ad2 = a.to(DEV)
        out = F2.Correlation(*params, 1)(ad2, bd)
        only2, = torch.autograd.grad((out * wgt.to(DEV)).sum(), [bd])
        assert torch.equal(only2, g2)
        # a non-contiguous first input (a channel slice of a wider tensor)
        wide = torch.cat([a, a], 1).to(DEV)[:, ::2]
        a_nc = torch.cat([a, a], 1)[:, ::2].clone()
        wide.requires_grad_(True)
        assert not wide.is_contiguous()
        out = F2.Correlation(*params, 1)(wide, bd)
        gnc, = torch.autograd.grad((out * wgt.to(DEV)).sum(), [wide])
        rnc, _ = autograd_correlation(a_nc, b, wgt, params)
        _close(gnc.cpu(), rnc, "Correlation module, non-contiguous input %s" % (params,))
    # Resample2d + ChannelNorm: the photometric term |img0 - warp(img1, flow)| that FlowNet2's fusion stage forms
    n, c, h, w = 2, 3, 14, 18
    img0, img1, flow = randn((n, c, h, w), 71), randn((n, c, h, w), 72), away_from_integers(n, h, w, 73)
    wgt = randn((n, 1, h, w), 74)
    i1c, fc = img1.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    loss = (O.channelnorm(img0 - O.resample2d(i1c, fc)) * wgt).sum()
    ri, rf = torch.autograd.grad(loss, [i1c, fc])
    i1d, fd = img1.to(DEV).requires_grad_(True), flow.to(DEV).requires_grad_(True)
    loss_d = (F2.ChannelNorm()(img0.to(DEV) - F2.Resample2d()(i1d, fd)) * wgt.to(DEV)).sum()
    _close(loss_d.detach().cpu(), loss.detach(), "photometric loss value")
    gi, gf = torch.autograd.grad(loss_d, [i1d, fd])
    _close(gi.cpu(), ri, "Resample2d / ChannelNorm chain, grad image")
    _close(gf.cpu(), rf, "Resample2d / ChannelNorm chain, grad flow")
    # flow only (the usual case: the image is data)
    loss_d = (F2.ChannelNorm()(img0.to(DEV) - F2.Resample2d()(img1.to(DEV), fd)) * wgt.to(DEV)).sum()
    gf_only, = torch.autograd.grad(loss_d, [fd])
    assert torch.equal(gf_only, gf)
    with pytest.raises(TypeError, match="float32"):
        F2.ChannelNorm()(img0.to(DEV).double())
    with pytest.raises(TypeError, match="float32"):
        F2.Resample2d()(img1.to(DEV).half(), fd.half())


def test_shim_backward_call_shape():
    """correlation_cuda / resample2d_cuda / channelnorm_cuda .backward in the pybind11 call shape: scratch tensors accepted and
    ignored, empty gradient tensors resized by the callee, return value 1 -- as the reference's wrapper files call them
    (correlation.py:41, resample2d.py:32, channelnorm.py:25)."""
    from vid2vid_amd import flownet2_ops as F2
    from oracle import vid2vid_oracle as O
    params = (4, 1, 4, 1, 2)
    a, b = randn((1, 6, 9, 12), 81), randn((1, 6, 9, 12), 82)
    ad, bd = a.to(DEV), b.to(DEV)
    out = ad.new()
    assert F2.correlation_cuda.forward(ad, bd, ad.new(), bd.new(), out, *params, 1) == 1
    _close(out.cpu(), O.correlation(a, b, *params), "shim correlation forward")
    go = randn(tuple(out.shape), 83)
    g1, g2 = ad.new(), bd.new()
    assert F2.correlation_cuda.backward(ad, bd, ad.new(), bd.new(), go.to(DEV), g1, g2, *params, 1) == 1
    r1, r2 = autograd_correlation(a, b, go, params)
    _close(g1.cpu(), r1, "shim correlation backward grad 1")
    _close(g2.cpu(), r2, "shim correlation backward grad 2")
    with pytest.raises(RuntimeError):
        F2.correlation_cuda.backward(ad, bd, ad.new(), bd.new(), go.to(DEV)[:, :, 1:].contiguous(), g1, g2, *params, 1)
    img, flow, gor = randn((1, 3, 9, 12), 84), away_from_integers(1, 9, 12, 85), randn((1, 3, 9, 12), 86)
    imd, fld = img.to(DEV), flow.to(DEV)
    gi, gf = imd.new(), imd.new()
    assert F2.resample2d_cuda.backward(imd, fld, gor.to(DEV), gi, gf, 1) == 1
    ri, rf = autograd_resample2d(img, flow, gor)
    _close(gi.cpu(), ri, "shim resample2d backward grad image")
    _close(gf.cpu(), rf, "shim resample2d backward grad flow")
    x, gon = randn((1, 3, 9, 12), 87), randn((1, 1, 9, 12), 88)
    xd = x.to(DEV)
    o = xd.new()
    assert F2.channelnorm_cuda.forward(xd, o, 2) == 1
    g = xd.new()
    assert F2.channelnorm_cuda.backward(xd, o, gon.to(DEV), g, 2) == 1
    _close(g.cpu(), autograd_channelnorm(x, gon), "shim channelnorm backward")
