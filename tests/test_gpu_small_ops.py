"""The small device ops called directly through the C ABI on buffers the test owns, against the fp64 references of
tests/small_ops_common.py (tests/test_cpu_small_ops.py ties those to torch and the oracle and shows what the bounds reject):
v2v_flownet_normalize, v2v_warp_diff_norm, v2v_resize_planar, v2v_pack_channels_nhwc, v2v_concat_channels_nhwc,
v2v_unpack_channels_nchw, v2v_pack_concat_nhwc, v2v_fg_mask_nhwc, v2v_avgpool3s2_nhwc, v2v_reflect_pad_fold,
v2v_instance_mean_planar, v2v_memset_zero, v2v_memcpy_d2d.

Every output lies inside a larger allocation (small_ops_common.Guarded): the guard bands on both sides and, for outputs that
are a channel window of an NHWC row, the channels outside the window keep their bits; outputs start as NaN, so an element the
kernel does not write fails.  Operands carry NaN where the kernel must not read (channels outside the window it is given).
Each test prints the largest |got - ref| / bound it saw; profiles/small_ops_error_ratios.txt keeps one run's figures."""
import ctypes as C

import pytest
import torch

import small_ops_common as S
from small_ops_common import Guarded, NAN, U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = 0, 1
EINVAL = -1


def _dt(prec):
    return BF16 if prec == "bf16" else F32


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    """A contiguous device copy, 16-byte aligned."""
    d = t.contiguous().to(DEV)
    assert d.data_ptr() % 16 == 0
    return d


def _call(name, *args):
    from vid2vid_amd.lib import lib, check
    check(getattr(lib, name)(*args, _stream()), name)
    torch.cuda.synchronize()


@pytest.fixture
def report(request):
    def say(ratio):
        print("\nRATIO %s %.3e" % (request.node.name, ratio))
    return say


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.NORMALIZE_CASES, ids=lambda c: "%dx%dx%d-max%g" % c)
def test_flownet_normalize(case, report):
    B, H, W, rgb_max = case
    hw = H * W
    im1, im2 = S.normalize_case(*case)
    r1, r2 = S.ref_normalize(im1, im2, rgb_max)
    rel, extra = S.normalize_bound(im1, im2, rgb_max)
    d1, d2 = _dev(im1), _dev(im2)
    x1, x2 = Guarded(B * 3 * hw, torch.float32, DEV), Guarded(B * 3 * hw, torch.float32, DEV)
    ws = Guarded(B * 3 * S.NORMALIZE_CHUNKS, torch.float32, DEV)            # the size include/v2v_hip.h names
    _call("v2v_flownet_normalize", _ptr(d1), _ptr(d2), _ptr(x1), _ptr(x2), _ptr(ws), B, H, W, rgb_max)
    ws.finish(what="workspace")
    assert torch.equal(d1.cpu(), im1) and torch.equal(d2.cpu(), im2), "an input was modified"
    e1 = S.check(x1.finish(what="x1").view(B, 3, hw), r1, rel, 0.0, "x1", extra=extra)
    e2 = S.check(x2.finish(what="x2").view(B, 3, hw), r2, rel, 0.0, "x2", extra=extra)
    report(max(e1, e2))


@pytest.mark.parametrize("outputs", S.WARP_OUTPUTS)
@pytest.mark.parametrize("name", sorted(S.WARP_CASES))
def test_warp_diff_norm(name, outputs, report):
    B, Cc, H, W, halves = S.WARP_CASES[name]
    hw = H * W
    c = S.warp_case(name)
    ref_w, ref_r = S.ref_warp_diff_norm(c["img0"], c["img1"], c["flow"])
    e_w, (nrel, nextra) = S.warp_bounds(c["img1"], Cc)
    if halves:
        x = _dev(c["x"])
        p0, p1 = C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr() + 3 * hw * 4)
    else:
        i0, i1 = _dev(c["img0"]), _dev(c["img1"])
        p0, p1 = _ptr(i0), _ptr(i1)
    flow = _dev(c["flow"])
    worst = 0.0
    for mode in (0, 1):
        warped = Guarded(B * Cc * hw, torch.float32, DEV) if outputs != "norm_only" else None
        norm = Guarded(B * hw, torch.float32, DEV) if outputs != "warped_only" else None
        _call("v2v_warp_diff_norm", p0, c["bs"], p1, c["bs"], _ptr(flow), _ptr(warped), _ptr(norm), B, Cc, H, W, mode, c["thr"])
        if warped is not None:
            worst = max(worst, S.check(warped.finish(what="warped").view(B, Cc, H, W), ref_w, U, 0.0, "warped mode %d" % mode, extra=e_w))
        if norm is not None:
            got = norm.finish(what="out_norm").view(B, H, W)
            if mode == 0:
                worst = max(worst, S.check(got, ref_r.sqrt(), nrel, 0.0, "norm", extra=nextra))
            else:
                S.check(got, (ref_r < c["thr"]).double(), what="r < %g" % c["thr"])             # 0 / 1, exact
    report(worst)


@pytest.mark.parametrize("bilinear", [1, 0], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("case", S.RESIZE_CASES, ids=lambda c: "%dx%dx%d-%dx%d" % c)
def test_resize_planar(case, bilinear, report):
    planes, H, W, OH, OW = case
    x = S.resize_case(planes, H, W)
    xd = _dev(x)
    worst = 0.0
    for scale in S.RESIZE_SCALES:
        y = Guarded(planes * OH * OW, torch.float32, DEV)
        _call("v2v_resize_planar", _ptr(xd), _ptr(y), planes, H, W, OH, OW, bilinear, scale)
        got = y.finish(what="y").view(planes, OH, OW)
        ref = S.ref_resize(x, OH, OW, bilinear, scale)
        if bilinear:
            worst = max(worst, S.check(got, ref, U, 0.0, "bilinear x%g" % scale, extra=S.resize_bilinear_extra(x, scale)))
        else:
            worst = max(worst, S.check(got, ref, what="nearest x%g" % scale))                   # bit exact
    report(worst)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("case", S.PACK_CH_CASES, ids=lambda c: "N%dC%d-%dx%d-off%d" % (c[0], c[1], c[2], c[3], c[5]))
def test_pack_channels_nhwc(case, prec, report):
    N, Cc, H, W, strides, off, scale, slope = case
    stride, P = strides[prec], N * H * W
    x = S.planar_case(N, Cc, H, W, 400 + Cc)
    xd = _dev(x)
    y = Guarded(P * stride, S.tdt(prec), DEV)
    _call("v2v_pack_channels_nhwc", _ptr(xd), _ptr(y), N, Cc, H, W, stride, off, scale, slope, _dt(prec))
    got = y.finish(S.channel_mask(P, stride, off, Cc), "y").view(P, stride)[:, off:off + Cc]
    ref = S.ref_pack_channels(x, scale, slope, prec)
    assert torch.equal(S.bits(got.cpu()), S.bits(ref)), "not the bits of leaky_relu(x * scale) in fp32"
    report(S.check(got.float(), ref.double()))


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("case", S.CONCAT_CASES, ids=lambda c: "P%dC%d" % c[:2])
def test_concat_channels_nhwc(case, prec, report):
    P, Cc, ss, so, ds, do = case
    src = S.nhwc_case(P, ss, prec, 500 + P).clone()
    keep = S.channel_mask(P, ss, so, Cc)
    src[~keep] = NAN                                                        # channels the kernel is not given
    sd = _dev(src)
    dst = Guarded(P * ds, S.tdt(prec), DEV)
    _call("v2v_concat_channels_nhwc", _ptr(sd), ss, so, _ptr(dst), ds, do, Cc, P, _dt(prec))
    got = dst.finish(S.channel_mask(P, ds, do, Cc), "dst").view(P, ds)[:, do:do + Cc]
    assert torch.equal(S.bits(got.cpu()), S.bits(src[:, so:so + Cc])), "not a copy"
    report(S.check(got.float(), src[:, so:so + Cc].double()))


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("case", S.UNPACK_CASES, ids=lambda c: "off%d" % c[5])
def test_unpack_channels_nchw(case, prec, report):
    N, Cc, H, W, stride, off = case
    hw = H * W
    y = S.nhwc_case(N * hw, stride, prec, 600 + off).clone()
    y[~S.channel_mask(N * hw, stride, off, Cc)] = NAN
    yd = _dev(y)
    x = Guarded(N * Cc * hw, torch.float32, DEV)
    _call("v2v_unpack_channels_nchw", _ptr(yd), _ptr(x), N, Cc, H, W, stride, off, _dt(prec))
    got = x.finish(what="x").view(N, Cc, hw)
    ref = S.ref_unpack_channels(y, N, Cc, hw, off)
    assert torch.equal(S.bits(got.cpu()), S.bits(ref)), "not the widened values of channels [%d, %d)" % (off, off + Cc)
    report(S.check(got, ref.double()))


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("case", S.PACK_CONCAT_CASES, ids=lambda c: "C%d+%d" % (c[1], c[2]))
def test_pack_concat_nhwc(case, prec, report):
    N, C0, C1, H, W, stride, scale1 = case
    P = N * H * W
    x0 = S.planar_case(N, C0, H, W, 610)
    x1 = S.planar_case(N, C1, H, W, 611) if C1 else None
    d0, d1 = _dev(x0), (_dev(x1) if C1 else None)
    y = Guarded(P * stride, S.tdt(prec), DEV)
    _call("v2v_pack_concat_nhwc", _ptr(d0), C0, _ptr(d1), C1, scale1, _ptr(y), N, H, W, stride, _dt(prec))
    got = y.finish(what="y").view(P, stride)                               # the whole row is written: pad channels are zeros
    assert not S.bits(got[:, C0 + C1:]).any(), "pad channels are not bit-exact 0"
    ref = S.ref_pack_concat(x0, x1, scale1, stride, prec)
    assert torch.equal(S.bits(got.cpu()), S.bits(ref)), "not the bits of cat([x0, x1 * scale1])"
    report(S.check(got.float(), ref.double()))


# ---------------------------------------------------------------------------------------------------------------------------
def _avgpool(xd, N, H, W, stride, prec):
    """v2v_avgpool3s2_nhwc of a device tensor [N*H*W][stride] into a guarded output; returns [N*OH*OW][stride]."""
    OH, OW = S.pooled_size(H, W)
    y = Guarded(N * OH * OW * stride, S.tdt(prec), DEV)
    _call("v2v_avgpool3s2_nhwc", _ptr(xd), _ptr(y), N, H, W, stride, _dt(prec))
    return y.finish(what="pooled").view(N * OH * OW, stride)


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("size", S.AVGPOOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_avgpool3s2_nhwc(size, prec, report):
    H, W = size
    x = S.avgpool_case(H, W, prec)
    got = _avgpool(_dev(x), S.AVGPOOL_N, H, W, S.AVGPOOL_STRIDE, prec)
    assert not S.bits(got[:, S.AVGPOOL_C:]).any(), "pad channels (zeros in x) are not bit-exact 0"
    rel, extra = S.avgpool_bound(x, prec)
    report(S.check(got.float(), S.ref_avgpool3s2(x, S.AVGPOOL_N, H, W), rel, 0.0, "avgpool", extra=extra))


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("n_fg", sorted(S.FG_SETS))
@pytest.mark.parametrize("base_ch", [0, S.LABEL_NC + 1])
@pytest.mark.parametrize("size", sorted(S.FG_SIZES))
@pytest.mark.parametrize("source", ["pooled", "raw"])
def test_fg_mask_nhwc(source, size, base_ch, n_fg, prec, report):
    """x is what the kernel reads on the device: the pooled encoding comes from v2v_avgpool3s2_nhwc itself (fractions, and sums
    above 1 where an edge pixel carries a foreground label), the raw one is the 0 / 1 encoding."""
    if source == "pooled":
        H, W = S.FG_SIZES[size]
        xd = _avgpool(_dev(S.label_frames(H, W).to(S.tdt(prec))), 1, H, W, S.FG_STRIDE, prec).contiguous()
        P = S.pooled_size(H, W)[0] * S.pooled_size(H, W)[1]
    else:
        H, W = S.FG_RAW_SIZES[size]
        xd, P = _dev(S.label_frames(H, W).to(S.tdt(prec))), H * W
    assert P == (1 if size == "P1" else 99)
    fg = S.FG_SETS[n_fg]
    fgd = torch.tensor(fg, dtype=torch.int32, device=DEV)
    mask = Guarded(P, torch.float32, DEV)
    _call("v2v_fg_mask_nhwc", _ptr(xd), _ptr(mask), P, S.FG_STRIDE, base_ch, _ptr(fgd), n_fg, _dt(prec))
    x = xd.cpu()
    unclamped = S.ref_fg_mask(x, base_ch, fg, clamp=False)
    if n_fg == 3 and base_ch == 0:
        assert float(unclamped.max()) > 1, "the input never exceeds 1 before the clamp"
    report(S.check(mask.finish(what="mask"), S.ref_fg_mask(x, base_ch, fg), *S.FG_BOUND, what="mask"))


def test_fg_mask_refuses_bad_arguments():
    from vid2vid_amd.lib import lib
    x, fgd = torch.zeros(16, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    mask = Guarded(1, torch.float32, DEV)
    for args in ((x, mask, fgd, 0), (x, mask, fgd, -1), (None, mask, fgd, 1), (x, None, fgd, 1), (x, mask, None, 1)):
        assert lib.v2v_fg_mask_nhwc(_ptr(args[0]), _ptr(args[1]), 1, 16, 0, _ptr(args[2]), args[3], F32, _stream()) == EINVAL, args[3]
    torch.cuda.synchronize()
    assert bool(torch.isnan(mask.finish(torch.zeros(1, dtype=torch.bool))).all()), "a refused call wrote its output"


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("case", S.FOLD_CASES, ids=lambda c: "N%d-%dx%d-p%d" % c)
def test_reflect_pad_fold(case, prec, report):
    N, H, W, pad = case
    xp = S.fold_case(N, H, W, pad, prec)
    x = Guarded(N * H * W * S.FOLD_STRIDE, S.tdt(prec), DEV)
    _call("v2v_reflect_pad_fold", _ptr(_dev(xp)), _ptr(x), N, H, W, pad, S.FOLD_STRIDE, _dt(prec))
    got = x.finish(what="x").view(N * H * W, S.FOLD_STRIDE)
    # include/v2v_hip.h gives both tensors as [..][cs]: the kernel folds all c_stride channels alike, so the pad channels of x
    # are the fold of xp's pad channels -- zeros, since xp keeps them zero like every NHWC buffer of the library
    assert not S.bits(got[:, S.FOLD_C:]).any(), "pad channels are not bit-exact 0"
    rel, extra = S.fold_bound(xp, N, H, W, pad, prec)
    report(S.check(got.float(), S.ref_reflect_fold(xp, N, H, W, pad), rel, 0.0, "fold", extra=extra))


# ---------------------------------------------------------------------------------------------------------------------------
def _instance_mean(name):
    from vid2vid_amd.lib import lib
    feat, inst = S.instance_case(name)
    Cc, HW = feat.shape
    n_ws = lib.v2v_instance_mean_workspace(Cc, HW)
    assert n_ws == S.SEG_SLOTS * 4 + S.SEG_SLOTS * (Cc + 1) * 4 + HW * 4
    fd, idd = _dev(feat), _dev(inst)
    out, ws = Guarded(Cc * HW, torch.float32, DEV), Guarded(n_ws // 4, torch.int32, DEV, fill=0x5A5A5A5A)
    _call("v2v_instance_mean_planar", _ptr(fd), _ptr(idd), _ptr(out), _ptr(ws), Cc, HW)
    ws.finish(what="workspace")
    assert torch.equal(fd.cpu(), feat) and torch.equal(idd.cpu(), inst), "an input was modified"
    return feat, inst, out.finish(what="out").view(Cc, HW).cpu()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_instance_mean_planar(name, report):
    """a: one pixel.  b: 40 scattered ids (0, negative, three groups that share a hash bucket) over two 8192-pixel runs.
    c: 4096 ids, the table exactly full: every id must still find its slot."""
    feat, inst, got = _instance_mean(name)
    report(S.check(got, S.ref_instance_mean(feat, inst), 0.0, 0.0, "instance mean %s" % name, extra=S.instance_mean_extra(feat, inst)))


def test_instance_mean_planar_overflow(report):
    """d: 5000 ids for 4096 slots, the documented overflow: the excess pixels keep their own value.  A probe fails only if all
    4096 slots were taken when it passed them, and a key never changes once set: so exactly 4096 ids get a slot and
    5000 - 4096 = 904 keep their values, whichever ids lose the race, and the two pixels of an id fare alike."""
    feat, inst, got = _instance_mean("d")
    ref, extra = S.ref_instance_mean(feat, inst), S.instance_mean_extra(feat, inst)
    assert bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs()
    is_mean = (err <= extra).all(0)                                         # per pixel, over the channels
    is_own = (S.bits(got) == S.bits(feat)).all(0)
    assert bool((is_mean ^ is_own).all()), "%d pixels hold neither their instance mean nor their own value" % int((~(is_mean ^ is_own)).sum())
    order = torch.argsort(inst.long(), stable=True)
    assert torch.equal(is_own[order[0::2]], is_own[order[1::2]]), "the two pixels of an id disagree"
    assert int(is_own[order[0::2]].sum()) == 5000 - S.SEG_SLOTS
    report(float((err / extra)[:, is_mean].max()))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", S.COPY_BASES)
@pytest.mark.parametrize("nbytes", S.COPY_BYTES)
def test_memset_zero(nbytes, base, report):
    p = Guarded(nbytes, torch.uint8, DEV, fill=0xA5, lead=base)
    assert p.ptr() % 16 == base
    _call("v2v_memset_zero", _ptr(p), nbytes)
    assert not p.finish(what="memset").any(), "a byte is not 0"
    report(0.0)


@pytest.mark.parametrize("base", S.COPY_BASES)
@pytest.mark.parametrize("nbytes", S.COPY_BYTES)
def test_memcpy_d2d(nbytes, base, report):
    src = torch.randint(1, 256, (nbytes + 1,), dtype=torch.uint8, generator=torch.Generator().manual_seed(nbytes))
    sd = _dev(src)[1 - base:]                                               # the source off alignment where the destination is on it
    dst = Guarded(nbytes, torch.uint8, DEV, fill=0, lead=base)
    assert dst.ptr() % 16 == base and sd.data_ptr() % 16 == 1 - base
    _call("v2v_memcpy_d2d", _ptr(dst), _ptr(sd), nbytes)
    assert torch.equal(dst.finish(what="memcpy").cpu(), src[1 - base:1 - base + nbytes]), "not a copy"
    assert torch.equal(sd.cpu(), src[1 - base:]), "the source was modified"
    report(0.0)
