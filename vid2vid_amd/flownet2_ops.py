"""FlowNet2's three native ops as differentiable torch modules on libv2v_hip.so: Correlation, Resample2d, ChannelNorm.

Drop-in for the reference's models/flownet2_pytorch/networks/{correlation,resample2d,channelnorm}_package:
  * `Correlation`, `Resample2d`, `ChannelNorm` (constructor signatures of correlation.py:47, resample2d.py:38, channelnorm.py:31) and
    the `autograd.Function`s behind them (correlation.py:6, resample2d.py:5, channelnorm.py:5), forward AND backward;
  * `correlation_cuda`, `resample2d_cuda`, `channelnorm_cuda`: classes with `forward` / `backward` static methods in the call shape
    of the pybind11 modules (correlation_cuda.cc:170-171, resample2d_cuda.cc:29-30, channelnorm_cuda.cc:28-29), so the reference's
    own wrapper files run unchanged with `from vid2vid_amd.flownet2_ops import correlation_cuda` in place of `import correlation_cuda`.

fp32 CUDA tensors only (the reference's Resample2d is float-only too, resample2d_kernel.cu:209); non-contiguous inputs are made
contiguous; every launch goes to the current stream of the input's device.  A gradient nobody asked for (needs_input_grad) is not
computed.  The reference's ChannelNormFunction.backward calls an undefined name (channelnorm.py:25: `channelnorm.backward`) and
cannot run; the one here simply works.

vid2vid itself keeps FlowNet2 frozen (models/flownet.py) and runs it through the fused engine program (vid2vid_amd/flownet2.py),
which is not differentiable; these modules are for training / fine-tuning FlowNet2 and for losses that warp.
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn.modules.module import Module

from .lib import lib, check

_I = C.c_int32


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _checked(t, what):
    """fp32, on the GPU (or anywhere in the library's dry-run mode, where nothing is launched), contiguous."""
    if not torch.is_tensor(t):
        raise TypeError("%s: expected a tensor, got %s" % (what, type(t).__name__))
    if t.dtype != torch.float32:
        raise TypeError("%s: the HIP kernels are float32-only (as the reference's Resample2d is), got %s -- cast with .float()"
                        % (what, t.dtype))
    if not t.is_cuda and not lib.v2v_get_dry_run():
        raise RuntimeError("%s: expected a CUDA (ROCm) tensor, got one on %s; there is no CPU path" % (what, t.device))
    if t.dim() != 4:
        raise ValueError("%s: expected a 4-D NCHW tensor, got shape %s" % (what, tuple(t.shape)))
    return t.contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def correlation_out_size(h, w, pad_size, kernel_size, max_displacement, stride1, stride2):
    oc, oh, ow = _I(), _I(), _I()
    if stride1 < 1 or stride2 < 1 or kernel_size < 1:
        raise ValueError("correlation: kernel_size, stride1 and stride2 must be positive")
    lib.v2v_correlation_out_size(h, w, pad_size, kernel_size, max_displacement, stride1, stride2, C.byref(oc), C.byref(oh), C.byref(ow))
    return oc.value, oh.value, ow.value


# ---- the pybind11 call shape (callee resizes its outputs, returns 1, raises RuntimeError on failure) ----
class correlation_cuda:
    @staticmethod
    def forward(input1, input2, rInput1, rInput2, output, pad_size, kernel_size, max_displacement, stride1, stride2, corr_type_multiply):
        # rInput1 / rInput2: the reference's padded NHWC scratch copies (correlation_cuda.cc:40-41); accepted, not used
        input1, input2 = _checked(input1, "correlation input1"), _checked(input2, "correlation input2")
        assert input1.shape == input2.shape, "correlation: inputs differ in shape"
        n, c, h, w = input1.shape
        oc, oh, ow = correlation_out_size(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
        output.resize_(n, oc, max(oh, 0), max(ow, 0))
        with torch.cuda.device_of(input1):
            check(lib.v2v_correlation_forward(_p(input1), _p(input2), _p(output), n, c, h, w, pad_size, kernel_size, max_displacement,
                                              stride1, stride2, corr_type_multiply, _stream(input1)), "correlation_forward")
        return 1

    @staticmethod
    def backward(input1, input2, rInput1, rInput2, gradOutput, gradInput1, gradInput2, pad_size, kernel_size, max_displacement,
                 stride1, stride2, corr_type_multiply):
        # gradInput1 / gradInput2: resized and fully written; None skips that gradient (an extension of the reference's shape)
        input1, input2 = _checked(input1, "correlation input1"), _checked(input2, "correlation input2")
        gradOutput = _checked(gradOutput, "correlation gradOutput")
        assert input1.shape == input2.shape, "correlation: inputs differ in shape"
        n, c, h, w = input1.shape
        for g in (gradInput1, gradInput2):
            if g is not None:
                g.resize_(n, c, h, w)
        with torch.cuda.device_of(input1):
            check(lib.v2v_correlation_backward(_p(input1), _p(input2), _p(gradOutput), _p(gradInput1), _p(gradInput2), n, c, h, w,
                                               gradOutput.shape[1], gradOutput.shape[2], gradOutput.shape[3],
                                               pad_size, kernel_size, max_displacement, stride1, stride2, corr_type_multiply,
                                               _stream(input1)), "correlation_backward")
        return 1


class resample2d_cuda:
    @staticmethod
    def forward(input1, input2, output, kernel_size):
        input1, input2 = _checked(input1, "resample2d input1"), _checked(input2, "resample2d input2 (flow)")
        n, c, h, w = input1.shape
        assert input2.shape[0] == n and input2.shape[1] == 2, "resample2d: flow must be (N, 2, OH, OW)"
        oh, ow = input2.shape[2], input2.shape[3]
        output.resize_(n, c, oh, ow)
        with torch.cuda.device_of(input1):
            check(lib.v2v_resample2d_forward(_p(input1), _p(input2), _p(output), n, c, h, w, oh, ow, kernel_size, _stream(input1)),
                  "resample2d_forward")
        return 1

    @staticmethod
    def backward(input1, input2, gradOutput, gradInput1, gradInput2, kernel_size):
        # gradInput1 is zeroed inside the call (it is a scatter); None skips a gradient
        input1, input2 = _checked(input1, "resample2d input1"), _checked(input2, "resample2d input2 (flow)")
        gradOutput = _checked(gradOutput, "resample2d gradOutput")
        n, c, h, w = input1.shape
        oh, ow = input2.shape[2], input2.shape[3]
        assert tuple(gradOutput.shape) == (n, c, oh, ow), "resample2d: gradOutput must have the output's shape"
        if gradInput1 is not None:
            gradInput1.resize_(n, c, h, w)
        if gradInput2 is not None:
            gradInput2.resize_(n, 2, oh, ow)
        with torch.cuda.device_of(input1):
            check(lib.v2v_resample2d_backward(_p(input1), _p(input2), _p(gradOutput), _p(gradInput1), _p(gradInput2), n, c, h, w, oh, ow,
                                              kernel_size, _stream(input1)), "resample2d_backward")
        return 1


class channelnorm_cuda:
    @staticmethod
    def forward(input1, output, norm_deg):
        input1 = _checked(input1, "channelnorm input1")
        n, c, h, w = input1.shape
        output.resize_(n, 1, h, w)
        with torch.cuda.device_of(input1):
            check(lib.v2v_channelnorm_forward(_p(input1), _p(output), n, c, h, w, norm_deg, _stream(input1)), "channelnorm_forward")
        return 1

    @staticmethod
    def backward(input1, output, gradOutput, gradInput1, norm_deg):
        input1, output = _checked(input1, "channelnorm input1"), _checked(output, "channelnorm output")
        gradOutput = _checked(gradOutput, "channelnorm gradOutput")
        n, c, h, w = input1.shape
        assert tuple(output.shape) == (n, 1, h, w) and tuple(gradOutput.shape) == (n, 1, h, w), "channelnorm: output / gradOutput must be (N, 1, H, W)"
        gradInput1.resize_(n, c, h, w)
        with torch.cuda.device_of(input1):
            check(lib.v2v_channelnorm_backward(_p(input1), _p(output), _p(gradOutput), _p(gradInput1), n, c, h, w, norm_deg,
                                               _stream(input1)), "channelnorm_backward")
        return 1


# ---- autograd ----
class CorrelationFunction(Function):
    @staticmethod
    def forward(ctx, input1, input2, pad_size=3, kernel_size=3, max_displacement=20, stride1=1, stride2=2, corr_multiply=1):
        input1, input2 = _checked(input1, "Correlation input1"), _checked(input2, "Correlation input2")
        ctx.save_for_backward(input1, input2)
        ctx.params = (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
        output = input1.new_empty(0)
        correlation_cuda.forward(input1, input2, None, None, output, *ctx.params)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        g1 = input1.new_empty(0) if ctx.needs_input_grad[0] else None
        g2 = input2.new_empty(0) if ctx.needs_input_grad[1] else None
        if g1 is not None or g2 is not None:
            correlation_cuda.backward(input1, input2, None, None, grad_output, g1, g2, *ctx.params)
        return (g1, g2) + (None,) * 6


class Correlation(Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super(Correlation, self).__init__()
        self.pad_size = pad_size
        self.kernel_size = kernel_size
        self.max_displacement = max_displacement
        self.stride1 = stride1
        self.stride2 = stride2
        self.corr_multiply = corr_multiply

    def forward(self, input1, input2):
        return CorrelationFunction.apply(input1, input2, self.pad_size, self.kernel_size, self.max_displacement, self.stride1,
                                         self.stride2, self.corr_multiply)


class Resample2dFunction(Function):
    @staticmethod
    def forward(ctx, input1, input2, kernel_size=1):
        input1, input2 = _checked(input1, "Resample2d input1"), _checked(input2, "Resample2d input2 (flow)")
        ctx.save_for_backward(input1, input2)
        ctx.kernel_size = kernel_size
        output = input1.new_empty(0)
        resample2d_cuda.forward(input1, input2, output, kernel_size)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        g1 = input1.new_empty(0) if ctx.needs_input_grad[0] else None
        g2 = input2.new_empty(0) if ctx.needs_input_grad[1] else None
        if g1 is not None or g2 is not None:
            resample2d_cuda.backward(input1, input2, grad_output, g1, g2, ctx.kernel_size)
        return g1, g2, None


class Resample2d(Module):
    def __init__(self, kernel_size=1):
        super(Resample2d, self).__init__()
        self.kernel_size = kernel_size

    def forward(self, input1, input2):
        return Resample2dFunction.apply(input1, input2, self.kernel_size)


class ChannelNormFunction(Function):
    @staticmethod
    def forward(ctx, input1, norm_deg=2):
        input1 = _checked(input1, "ChannelNorm input1")
        output = input1.new_empty(0)
        channelnorm_cuda.forward(input1, output, norm_deg)
        ctx.save_for_backward(input1, output)
        ctx.norm_deg = norm_deg
        return output

    @staticmethod
    def backward(ctx, grad_output):
        input1, output = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        g = input1.new_empty(0)
        channelnorm_cuda.backward(input1, output, grad_output, g, ctx.norm_deg)
        return g, None


class ChannelNorm(Module):
    def __init__(self, norm_deg=2):
        super(ChannelNorm, self).__init__()
        self.norm_deg = norm_deg

    def forward(self, input1):
        return ChannelNormFunction.apply(input1, self.norm_deg)
