"""CPU-side checks of the backward passes of FlowNet2's three native ops (csrc/flow_ops_bwd.hip): C ABI surface, argument
validation / dry run, and the Python layer (vid2vid_amd/flownet2_ops.py) importing and constructing without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("v2v_correlation_backward", "v2v_resample2d_backward", "v2v_channelnorm_backward")
EINVAL = -1


def test_library_exports_and_header_declares_the_backward_entry_points():
    from vid2vid_amd import lib
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    for name in NEW:
        assert hasattr(lib.lib, name), "libv2v_hip.so does not export %s" % name
        assert name in lib.exported_symbols()
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in include/v2v_hip.h" % name
    # each cites the reference function it replaces, and the list at the top of the header names it
    for cite in ("correlation_cuda.cc:89-167", "resample2d_cuda.cc:15-26", "channelnorm_cuda.cc:16-25"):
        assert header.count(cite) >= 2, cite


@pytest.fixture
def dry_run():
    from vid2vid_amd.lib import lib
    prev = lib.v2v_set_dry_run(1)
    yield lib
    lib.v2v_set_dry_run(prev)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_correlation_backward_validates_geometry(dry_run):
    lib = dry_run
    buf = torch.zeros(1 << 16)
    p = _ptr(buf)
    good = dict(N=1, C=8, H=12, W=20, oc=441, oh=12, ow=20, pad=20, k=1, md=20, s1=1, s2=2, mult=1)

    def call(in1=p, in2=p, go=p, g1=p, g2=p, **kw):
        a = dict(good); a.update(kw)
        return lib.v2v_correlation_backward(in1, in2, go, g1, g2, a["N"], a["C"], a["H"], a["W"], a["oc"], a["oh"], a["ow"],
                                            a["pad"], a["k"], a["md"], a["s1"], a["s2"], a["mult"], None)
    assert call() == 0, lib.v2v_last_error()
    assert call(g1=None) == 0 and call(g2=None) == 0                  # one gradient may be skipped
    assert call(pad=4, k=3, md=4, s1=2, s2=1, H=17, W=23, oc=81, oh=8, ow=11) == 0, lib.v2v_last_error()     # a generic parameter set
    assert call(g1=None, g2=None) == EINVAL                           # nothing to compute
    for bad in (dict(in1=None), dict(in2=None), dict(go=None), dict(N=0), dict(C=0), dict(H=0), dict(W=-3), dict(k=0), dict(k=2),
                dict(s1=0), dict(s2=0), dict(mult=0), dict(oc=440), dict(oh=11), dict(ow=21), dict(md=200, oc=201 * 201),
                dict(pad=0, oc=441, oh=12, ow=20)):                    # pad 0: the forward output would be empty
        assert call(**bad) == EINVAL, bad
    assert b"correlation_backward" in lib.v2v_last_error()


def test_resample2d_and_channelnorm_backward_validate_geometry(dry_run):
    lib = dry_run
    buf = torch.zeros(1 << 14)
    p = _ptr(buf)
    rs = lib.v2v_resample2d_backward
    assert rs(p, p, p, p, p, 2, 3, 9, 14, 9, 14, 1, None) == 0, lib.v2v_last_error()
    assert rs(p, p, p, None, p, 2, 3, 9, 14, 9, 14, 1, None) == 0 and rs(p, p, p, p, None, 2, 3, 9, 14, 9, 14, 1, None) == 0
    assert rs(p, p, p, p, p, 1, 3, 10, 15, 9, 14, 2, None) == 0       # kernel_size 2 needs one more image row / column
    assert rs(p, p, p, p, p, 1, 3, 9, 14, 9, 14, 2, None) == EINVAL
    assert rs(p, p, p, None, None, 2, 3, 9, 14, 9, 14, 1, None) == EINVAL
    assert rs(None, p, p, p, p, 2, 3, 9, 14, 9, 14, 1, None) == EINVAL and rs(p, None, p, p, p, 2, 3, 9, 14, 9, 14, 1, None) == EINVAL
    assert rs(p, p, None, p, p, 2, 3, 9, 14, 9, 14, 1, None) == EINVAL
    assert rs(p, p, p, p, p, 0, 3, 9, 14, 9, 14, 1, None) == EINVAL and rs(p, p, p, p, p, 2, 3, 9, 14, 0, 14, 1, None) == EINVAL
    assert rs(p, p, p, p, p, 2, 3, 9, 14, 9, 14, 0, None) == EINVAL
    cn = lib.v2v_channelnorm_backward
    assert cn(p, p, p, p, 2, 3, 9, 14, 2, None) == 0, lib.v2v_last_error()
    assert cn(p, p, p, p, 2, 3, 9, 14, 1, None) == EINVAL              # the forward entry refuses norm_deg != 2 as well
    assert lib.v2v_channelnorm_forward(p, p, 2, 3, 9, 14, 1, None) == EINVAL
    assert cn(None, p, p, p, 2, 3, 9, 14, 2, None) == EINVAL and cn(p, None, p, p, 2, 3, 9, 14, 2, None) == EINVAL
    assert cn(p, p, None, p, 2, 3, 9, 14, 2, None) == EINVAL and cn(p, p, p, None, 2, 3, 9, 14, 2, None) == EINVAL
    assert cn(p, p, p, p, 2, 0, 9, 14, 2, None) == EINVAL and cn(p, p, p, p, 2, 3, 9, 0, 2, None) == EINVAL


def test_backward_ops_record_into_a_plan(dry_run):
    """Like every other launch entry point they are recordable (bench.py --dry-run's backend records plans on CPU hosts)."""
    lib = dry_run
    buf = torch.zeros(1 << 16)
    p = _ptr(buf)
    plan = lib.v2v_plan_create()
    try:
        assert lib.v2v_plan_begin_record(plan) == 0
        assert lib.v2v_correlation_backward(p, p, p, p, p, 1, 8, 12, 20, 441, 12, 20, 20, 1, 20, 1, 2, 1, None) == 0
        assert lib.v2v_resample2d_backward(p, p, p, p, p, 1, 3, 9, 14, 9, 14, 1, None) == 0
        assert lib.v2v_channelnorm_backward(p, p, p, p, 1, 3, 9, 14, 2, None) == 0
        assert lib.v2v_plan_end_record(plan) == 0
        names = [lib.v2v_plan_op_name(plan, i).decode() for i in range(lib.v2v_plan_num_ops(plan))]
        assert names == ["correlation_backward", "resample2d_backward", "channelnorm_backward"]
    finally:
        lib.v2v_plan_destroy(plan)


def test_python_layer_imports_and_mirrors_the_reference_signatures():
    from vid2vid_amd import flownet2_ops as O
    # constructor signatures of correlation.py:47, resample2d.py:38, channelnorm.py:31
    assert list(inspect.signature(O.Correlation.__init__).parameters)[1:] == [
        "pad_size", "kernel_size", "max_displacement", "stride1", "stride2", "corr_multiply"]
    m = O.Correlation(pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2, corr_multiply=1)     # FlowNetC.py:31
    assert (m.pad_size, m.kernel_size, m.max_displacement, m.stride1, m.stride2, m.corr_multiply) == (20, 1, 20, 1, 2, 1)
    d = O.Correlation()
    assert (d.pad_size, d.kernel_size, d.max_displacement, d.stride1, d.stride2, d.corr_multiply) == (0, 0, 0, 1, 2, 1)
    assert O.Resample2d().kernel_size == 1 and O.Resample2d(kernel_size=2).kernel_size == 2
    assert O.ChannelNorm().norm_deg == 2 and O.ChannelNorm(norm_deg=2).norm_deg == 2
    for fn in (O.CorrelationFunction, O.Resample2dFunction, O.ChannelNormFunction):
        assert issubclass(fn, torch.autograd.Function)
    # the pybind11 call shape: forward and backward, scratch tensors included
    assert list(inspect.signature(O.correlation_cuda.forward).parameters) == [
        "input1", "input2", "rInput1", "rInput2", "output", "pad_size", "kernel_size", "max_displacement", "stride1", "stride2",
        "corr_type_multiply"]
    assert list(inspect.signature(O.correlation_cuda.backward).parameters) == [
        "input1", "input2", "rInput1", "rInput2", "gradOutput", "gradInput1", "gradInput2", "pad_size", "kernel_size",
        "max_displacement", "stride1", "stride2", "corr_type_multiply"]
    assert list(inspect.signature(O.resample2d_cuda.forward).parameters) == ["input1", "input2", "output", "kernel_size"]
    assert list(inspect.signature(O.resample2d_cuda.backward).parameters) == [
        "input1", "input2", "gradOutput", "gradInput1", "gradInput2", "kernel_size"]
    assert list(inspect.signature(O.channelnorm_cuda.forward).parameters) == ["input1", "output", "norm_deg"]
    assert list(inspect.signature(O.channelnorm_cuda.backward).parameters) == ["input1", "output", "gradOutput", "gradInput1", "norm_deg"]


def test_python_layer_refuses_wrong_dtypes_and_cpu_tensors():
    from vid2vid_amd import flownet2_ops as O
    x = torch.randn(1, 4, 6, 8)
    with pytest.raises(TypeError, match="float32"):
        O.ChannelNorm()(x.double())
    with pytest.raises(TypeError, match="float32"):
        O.Resample2d()(x.half(), torch.zeros(1, 2, 6, 8).half())
    with pytest.raises(TypeError, match="float32"):
        O.Correlation(4, 1, 4, 1, 2, 1)(x.double(), x.double())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="CUDA"):
            O.ChannelNorm()(x)


def test_python_layer_runs_forward_and_backward_in_dry_run(dry_run):
    """Dry run: shapes, resizing by the shim and the autograd wiring (needs_input_grad) without a launch."""
    from vid2vid_amd import flownet2_ops as O
    if torch.cuda.is_available():
        pytest.skip("dry-run wiring is a CPU-host check")
    a = torch.randn(2, 8, 12, 20, requires_grad=True)
    b = torch.randn(2, 8, 12, 20)
    out = O.Correlation(20, 1, 20, 1, 2, 1)(a, b)
    assert tuple(out.shape) == (2, 441, 12, 20)
    ga, = torch.autograd.grad(out.sum(), [a])
    assert tuple(ga.shape) == tuple(a.shape)
    flow = torch.zeros(2, 2, 12, 20, requires_grad=True)
    w = O.Resample2d()(b.transpose(2, 3).contiguous().transpose(2, 3), flow)          # a non-contiguous image
    assert tuple(w.shape) == (2, 8, 12, 20)
    gf, = torch.autograd.grad(w.sum(), [flow])
    assert tuple(gf.shape) == (2, 2, 12, 20)
    n = O.ChannelNorm()(a)
    assert tuple(n.shape) == (2, 1, 12, 20)
    gn, = torch.autograd.grad(n.sum(), [a])
    assert tuple(gn.shape) == tuple(a.shape)
    g1, g2 = torch.empty(0), torch.empty(0)
    assert O.correlation_cuda.backward(a.detach(), b, torch.empty(0), torch.empty(0), torch.zeros(2, 441, 12, 20), g1, g2, 20, 1, 20, 1, 2, 1) == 1
    assert tuple(g1.shape) == tuple(g2.shape) == (2, 8, 12, 20)                       # resized by the callee
    with pytest.raises(RuntimeError, match="grad_out"):                             # a gradOutput of the wrong extent
        O.correlation_cuda.backward(a.detach(), b, None, None, torch.zeros(2, 441, 11, 20), g1, g2, 20, 1, 20, 1, 2, 1)


def test_new_module_never_imports_the_oracle():
    """The rule of test_cpu_boundary.py::test_product_never_imports_the_oracle, spelled out for the new files."""
    pat = re.compile(r"^\s*(from|import)\s+\.*oracle\b|oracle\.vid2vid_oracle|/oracle/", re.M)
    for rel in ("vid2vid_amd/flownet2_ops.py", "vid2vid_amd/csrc/flow_ops_bwd.hip"):
        src = open(os.path.join(ROOT, rel)).read()
        assert not pat.search(src), "%s references the oracle" % rel
