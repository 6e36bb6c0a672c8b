"""v2v_bn_backward, v2v_channel_sum and v2v_act_backward (csrc/norm_act.hip) called directly through the C ABI on raw tensors,
against the fp64 references of tests/norm_bwd_common.py (tests/test_cpu_norm_backward.py ties those to autograd and shows what
the bounds reject).  The cases reach what the engine's layers never do: several 64-channel slabs, C % 4 != 0 on the vector
path, three different channel strides, the scalar path, empty pixel phases, short last blocks, the 512-block cap, the
rebalancing branch, the separate finalize launch above 64 slabs, overwrite mode, NULL dgamma / dbeta, re-armed tickets.

Every output (and the workspace, sized exactly as include/v2v_hip.h says) is followed by a 256-element guard that must keep its
bits; outputs start as NaN (overwrite mode must not read them), and so do the pad channels of the operands (never used).

Bounds (norm_bwd_common): sums 2e-4 / 2e-4 in both dtypes, dRaw 2e-4 / 2e-4 (fp32) and 2^-8 / 2e-4 (bf16: one rounding step),
act_backward 1e-6 / 1e-6 (fp32) and 2^-8 / 1e-6 (bf16).  They are ceilings.  Measured on an MI355X, the largest
|got - ref| / (|ref| + rms(ref)) over all cases (each test prints its own):
    v2v_bn_backward    fp32: dRaw 3.2e-07   dgamma 3.1e-07   dbeta 4.0e-07
                       bf16: dRaw 3.5e-03   dgamma 2.7e-07   dbeta 1.4e-07      (dRaw: the bf16 store, at most 2^-8 = 3.9e-03)
    v2v_channel_sum    fp32: 3.9e-07        bf16: 4.6e-08
    v2v_act_backward   fp32: 3.4e-07 (NHWC), 2.1e-07 (NCHW heads)               bf16: 3.2e-03
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import norm_bwd_common as NB
from norm_bwd_common import ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
SENTINEL = -777.0
NAN = float("nan")
F32, BF16 = 0, 1


def _tdt(prec):
    return torch.bfloat16 if prec == "bf16" else torch.float32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(n, dtype, fill=NAN):
    """n elements of `fill` followed by the guard."""
    buf = torch.empty(n + GUARD, dtype=dtype, device=DEV)
    buf[:n] = fill
    buf[n:] = SENTINEL
    assert buf.data_ptr() % 16 == 0
    return buf


def _guard_intact(buf, n):
    return torch.equal(_bits(buf[n:]), _bits(torch.full((GUARD,), SENTINEL, dtype=buf.dtype, device=DEV)))


def _operand(values, stride, dtype, offset=0):
    """[P][stride] device view of `values` [P][C] with NaN pad channels, `offset` elements off the allocation's alignment."""
    P, C_ = values.shape
    host = torch.full((P, stride), NAN)
    host[:, :C_] = values
    buf = torch.empty(P * stride + offset, dtype=dtype, device=DEV)
    view = buf[offset:]
    view.copy_(host.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == (offset * buf.element_size()) % 16
    return view


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _strides(name, prec):
    P, C_, cs, csr, cso, off = NB.BN_CASES[name]
    if prec == "bf16":
        cso = (cso + 7) // 8 * 8
        if name != "h1":                  # h1 IS the dy stride that is no multiple of 4; the scalar path has no alignment need
            cs = (cs + 7) // 8 * 8
    return P, C_, cs, csr, cso, off


class BnCall:
    """One v2v_bn_backward call on guarded buffers.  base: initial dgamma / dbeta of accumulate mode."""

    def __init__(self, name, act, prec, accumulate=0, affine=True, base=None):
        self.P, self.C, self.cs, self.csr, self.cso, off = _strides(name, prec)
        c = NB.bn_case(name, act)
        self.prec, self.act, self.slope, self.accumulate, self.affine, self.base = prec, act, c["slope"], accumulate, affine, base
        self.dy = _operand(c["dy"], self.cs, _tdt(prec), off)
        self.raw = _operand(c["raw"], self.csr, torch.float32, off)
        self.stats = c["stats"].to(DEV).contiguous()
        self.n_ws = NB.blocks(self.P)[1] * 2 * self.C + 2 * self.C
        self.reset()

    def reset(self):
        self.draw = _guarded(self.P * self.cso, _tdt(self.prec))
        self.dgamma = _guarded(self.C, torch.float32)
        self.dbeta = _guarded(self.C, torch.float32)
        if self.accumulate:
            self.dgamma[:self.C] = self.base[0]
            self.dbeta[:self.C] = self.base[1]
        self.ws = _guarded(self.n_ws, torch.float32)

    def submit(self):
        from vid2vid_amd.lib import lib, check
        dg, db = (self.dgamma, self.dbeta) if self.affine else (None, None)
        check(lib.v2v_bn_backward(_ptr(self.dy), _ptr(self.raw), self.csr, _ptr(self.stats), _ptr(self.draw), self.cso, _ptr(dg),
                                  _ptr(db), self.accumulate, _ptr(self.ws), self.P, self.C, self.cs, self.act, self.slope,
                                  BF16 if self.prec == "bf16" else F32, _stream()), "bn_backward")

    def results(self):
        """(dRaw [P][c_stride_out], dgamma [C], dbeta [C]) after the guards and the pad channels were checked."""
        torch.cuda.synchronize()
        assert _guard_intact(self.draw, self.P * self.cso), "dRaw guard overwritten"
        assert _guard_intact(self.dgamma, self.C) and _guard_intact(self.dbeta, self.C), "dgamma / dbeta guard overwritten"
        assert _guard_intact(self.ws, self.n_ws), "workspace guard overwritten"
        draw = self.draw[:self.P * self.cso].view(self.P, self.cso)
        assert not _bits(draw[:, self.C:]).any(), "pad channels of dRaw are not bit-exact 0"
        if not self.affine:
            assert torch.isnan(self.dgamma[:self.C]).all() and torch.isnan(self.dbeta[:self.C]).all(), "NULL dgamma / dbeta written"
        return draw, self.dgamma[:self.C], self.dbeta[:self.C]

    def run(self):
        self.submit()
        return self.results()


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _bn_params():
    out = []
    for name in sorted(NB.BN_CASES):
        for prec in ("fp32",) if name in NB.BN_FP32_ONLY else ("fp32", "bf16"):
            for act in NB.BN_ACTS[name]:
                for acc in (0, 1):
                    out.append(pytest.param(name, prec, act, acc, True, id="%s-%s-%s-acc%d" % (name, prec, NB.ACT_NAMES[act], acc)))
                if name in ("c", "d"):
                    out.append(pytest.param(name, prec, act, 0, False, id="%s-%s-%s-null" % (name, prec, NB.ACT_NAMES[act])))
    return out


@pytest.mark.parametrize("name,prec,act,accumulate,affine", _bn_params())
def test_bn_backward(name, prec, act, accumulate, affine):
    ref_draw, ref_dgamma, ref_dbeta = NB.bn_reference(name, act, prec)
    C_ = ref_draw.shape[1]
    draw, dgamma, dbeta = BnCall(name, act, prec, 0, affine).run()
    e = [NB.check(draw[:, :C_].float(), ref_draw, *NB.DRAW_BOUND[prec], what="dRaw %s" % name), 0.0, 0.0]
    if affine:
        e[1] = NB.check(dgamma, ref_dgamma, *NB.SUM_BOUND, what="dgamma %s" % name)
        e[2] = NB.check(dbeta, ref_dbeta, *NB.SUM_BOUND, what="dbeta %s" % name)
    print("bn_backward %s %s %s: dRaw %.2e dgamma %.2e dbeta %.2e" % (name, prec, NB.ACT_NAMES[act], e[0], e[1], e[2]))
    if not accumulate:
        again = BnCall(name, act, prec, 0, affine).run()           # fixed summation order: the same bits from fresh buffers
        assert _same_bits(again, (draw, dgamma, dbeta)), "a repeated launch differs"
        return
    g = torch.Generator().manual_seed(3)
    base = (torch.randn(C_, generator=g).to(DEV), torch.randn(C_, generator=g).to(DEV))
    adraw, adgamma, adbeta = BnCall(name, act, prec, 1, True, base).run()
    assert torch.equal(_bits(adraw), _bits(draw)), "dRaw depends on accumulate"
    for got, b, over, ref in ((adgamma, base[0], dgamma, ref_dgamma), (adbeta, base[1], dbeta, ref_dbeta)):
        rms = float(ref.pow(2).mean().sqrt())
        assert float((got - (b + over)).abs().max()) <= 1e-6 * rms           # (fp32 sum, as the kernel adds)


# fused-finalize switch: (case, activation, dtype) computed in this process and in a child with V2V_BN_BWD_FUSED=0
SPLIT_CASES = [("c", ACT_RELU, "fp32"), ("c", ACT_LEAKY, "bf16"), ("e", ACT_RELU, "fp32"), ("e", ACT_RELU, "bf16")]


def _split_results():
    out = {}
    for i, (name, act, prec) in enumerate(SPLIT_CASES):
        for key, t in zip(("draw", "dgamma", "dbeta"), BnCall(name, act, prec).run()):
            out["%s%d" % (key, i)] = t.float().cpu()
    return out


def test_fused_and_separate_finalize_give_the_same_bits(tmp_path):
    """The in-launch finalize (last workgroup of a slab) and bn_bwd_finalize_kernel promise the same arithmetic.  The switch is
    read once per process, so the separate launch runs in one fresh child."""
    import numpy as np
    assert os.environ.get("V2V_BN_BWD_FUSED", "1")[:1] != "0", "this process must run the fused finalize"
    mine = _split_results()
    path = str(tmp_path / "separate.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--separate-finalize", path], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, V2V_BN_BWD_FUSED="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = np.load(path)
    assert sorted(theirs.files) == sorted(mine)
    for key, t in mine.items():
        assert torch.equal(t, torch.from_numpy(theirs[key])), key


def test_tickets_rearm_across_plan_replays():
    """A recorded op keeps its ticket words for life: every replay finds them re-armed by the one before."""
    from vid2vid_amd.lib import lib, check
    eager = BnCall("d", ACT_RELU, "fp32").run()
    call = BnCall("d", ACT_RELU, "fp32")
    plan = lib.v2v_plan_create()
    try:
        check(lib.v2v_plan_begin_record(plan), "plan_begin_record")
        try:
            call.submit()
        finally:
            check(lib.v2v_plan_end_record(plan), "plan_end_record")
        assert lib.v2v_plan_num_ops(plan) == 1 and lib.v2v_plan_op_name(plan, 0) == b"bn_backward"
        torch.cuda.synchronize()
        assert torch.isnan(call.draw[:call.P * call.cso]).all(), "recording launched the op"
        for i in range(3):
            for buf, n in ((call.draw, call.P * call.cso), (call.dgamma, call.C), (call.dbeta, call.C), (call.ws, call.n_ws)):
                buf[:n] = NAN
            check(lib.v2v_plan_run(plan, _stream()), "plan_run")
            assert _same_bits(call.results(), eager), "replay %d differs from the eager launch" % i
    finally:
        lib.v2v_plan_destroy(plan)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", NB.SUM_CASES, ids=lambda c: "P%d-C%d-s%d" % c)
def test_channel_sum(case, prec, accumulate):
    from vid2vid_amd.lib import lib, check
    P, C_, cs = case
    if prec == "bf16" and cs % 4 == 0:
        cs = (cs + 7) // 8 * 8                                     # (130, 70, 70) stays the scalar path
    x = NB.sum_case(P, C_)
    xd = _operand(x, cs, _tdt(prec))
    ref = NB.ref_channel_sum(xd.view(P, cs)[:, :C_].cpu())
    n_ws = NB.blocks(P)[1] * 2 * C_
    base = torch.randn(C_, generator=torch.Generator().manual_seed(4)).to(DEV)

    def run(acc):
        out, ws = _guarded(C_, torch.float32), _guarded(n_ws, torch.float32)
        if acc:
            out[:C_] = base
        check(lib.v2v_channel_sum(_ptr(xd), _ptr(out), acc, _ptr(ws), P, C_, cs, BF16 if prec == "bf16" else F32, _stream()), "channel_sum")
        torch.cuda.synchronize()
        assert _guard_intact(out, C_) and _guard_intact(ws, n_ws), "guard overwritten"
        return out[:C_]
    got = run(0)
    e = NB.check(got, ref, *NB.SUM_BOUND, what="channel_sum %s" % str(case))
    print("channel_sum %s %s: %.2e" % (str(case), prec, e))
    if not accumulate:
        assert torch.equal(_bits(run(0)), _bits(got)), "a repeated launch differs"
        return
    acc = run(1)
    rms = float(ref.pow(2).mean().sqrt())
    assert float((acc - (base + got)).abs().max()) <= 1e-6 * rms                # (fp32 sum, as the kernel adds)


# v2v_act_backward: (N, H, W, C, c_stride_in (fp32, bf16), c_stride_out); nchw heads have no input stride
ACT_NHWC = [(1, 1, 9, 3, (4, 8), 8),
            (2, 7, 5, 66, (72, 72), 80),                           # strides differ
            (1, 64, 130, 130, (136, 136), 136)]                    # 1.13 M elements: past the 4096 x 256 grid, the stride loop
ACT_NCHW = [(1, 16, 24, 1), (1, 16, 24, 2), (1, 16, 24, 3)]
ALL_ACTS = [ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID]
OUT_SCALES = (1.0, 20.0, 0.5)


def _act_inputs(NP, C_, act, scale, prec, seed):
    """dy and the scaled output y = act(x) * scale, [NP][C] fp32 holding values of the activation dtype (y from fp64)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(NP, C_, generator=g, dtype=torch.float64) * 1.5
    dy = torch.randn(NP, C_, generator=g)
    y = {ACT_NONE: x, ACT_RELU: x.clamp(min=0), ACT_LEAKY: torch.where(x > 0, x, x * NB.SLOPE), ACT_TANH: torch.tanh(x),
         ACT_SIGMOID: torch.sigmoid(x)}[act] * scale
    return dy.to(_tdt(prec)).float(), y.to(_tdt(prec)).float()


def _check_act(got, dy, y, act, scale, prec, what):
    ref = NB.ref_act_backward(dy, None if act == ACT_NONE else y, act, NB.f32(NB.SLOPE), scale)
    return NB.check(got, ref, *NB.ACT_BOUND[prec], what=what)


@pytest.mark.parametrize("act", ALL_ACTS, ids=lambda a: NB.ACT_NAMES[a])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ACT_NHWC, ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_act_backward_nhwc(shape, prec, act):
    from vid2vid_amd.lib import lib, check
    N, H, W, C_, csi, cso = shape
    csi = csi[1] if prec == "bf16" else csi[0]
    NP = N * H * W
    worst = 0.0
    for scale in OUT_SCALES:
        dy, y = _act_inputs(NP, C_, act, scale, prec, 100 * C_ + act)
        dyd, yd = _operand(dy, csi, _tdt(prec)), _operand(y, csi, _tdt(prec))
        g = _guarded(NP * cso, _tdt(prec))
        check(lib.v2v_act_backward(_ptr(dyd), None if act == ACT_NONE else _ptr(yd), _ptr(g), N, H, W, C_, csi, cso, 0, act,
                                   NB.SLOPE, scale, BF16 if prec == "bf16" else F32, _stream()), "act_backward")
        torch.cuda.synchronize()
        assert _guard_intact(g, NP * cso), "guard overwritten"
        out = g[:NP * cso].view(NP, cso)
        assert not _bits(out[:, C_:]).any(), "pad channels are not bit-exact 0"
        worst = max(worst, _check_act(out[:, :C_].float(), dy, y, act, scale, prec, "%s x%g" % (NB.ACT_NAMES[act], scale)))
    print("act_backward nhwc %s %s %s: %.2e" % (str(shape[:4]), prec, NB.ACT_NAMES[act], worst))


@pytest.mark.parametrize("act", ALL_ACTS, ids=lambda a: NB.ACT_NAMES[a])
@pytest.mark.parametrize("shape", ACT_NCHW, ids=lambda s: "x".join(str(v) for v in s))
def test_act_backward_nchw_heads(shape, act):
    """dy / y planar fp32 [N][C][H][W] (the API-facing heads), g NHWC with channel stride 4."""
    from vid2vid_amd.lib import lib, check
    N, H, W, C_ = shape
    NP, cso = N * H * W, 4
    worst = 0.0
    for scale in OUT_SCALES:
        dy, y = _act_inputs(NP, C_, act, scale, "fp32", 7 * C_ + act)
        planar = lambda t: t.view(N, H * W, C_).permute(0, 2, 1).contiguous().to(DEV)
        dyd, yd = planar(dy), planar(y)
        g = _guarded(NP * cso, torch.float32)
        check(lib.v2v_act_backward(_ptr(dyd), None if act == ACT_NONE else _ptr(yd), _ptr(g), N, H, W, C_, 0, cso, 1, act,
                                   NB.SLOPE, scale, F32, _stream()), "act_backward")
        torch.cuda.synchronize()
        assert _guard_intact(g, NP * cso), "guard overwritten"
        out = g[:NP * cso].view(NP, cso)
        assert not _bits(out[:, C_:]).any(), "pad channels are not bit-exact 0"
        worst = max(worst, _check_act(out[:, :C_], dy, y, act, scale, "fp32", "%s x%g" % (NB.ACT_NAMES[act], scale)))
    print("act_backward nchw %s %s: %.2e" % (str(shape), NB.ACT_NAMES[act], worst))


if __name__ == "__main__":
    # the child of test_fused_and_separate_finalize_give_the_same_bits: SPLIT_CASES -> an .npz
    import numpy as np
    assert sys.argv[1] == "--separate-finalize" and os.environ.get("V2V_BN_BWD_FUSED") == "0"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    np.savez(sys.argv[2], **{k: v.numpy() for k, v in _split_results().items()})
