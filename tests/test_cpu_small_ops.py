"""CPU-side checks behind tests/test_gpu_small_ops.py: the fp64 references of tests/small_ops_common.py against independent
evaluations (torch's own operators, the oracle), the invariants its input makers promise, what the GPU tests' bounds reject
(one deliberately wrong reference per op), the guard helper on host tensors, and the entry points' argument validation with the
library in dry-run mode."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_common as S
from small_ops_common import U

EINVAL = -1
F32, BF16 = 0, 1


def _rejected(wrong, ref, *bound, **kw):
    try:
        S.check(wrong, ref, *bound, **kw)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# the references against independent evaluations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.NORMALIZE_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_normalize_reference_vs_torch(case):
    """models.py:97-102 on doubles: cat, mean over frames and pixels, subtract, divide.  1e-12: fp64 roundings only."""
    B, H, W, rgb_max = case
    im1, im2 = S.normalize_case(*case)
    x = torch.stack([im1, im2], 2).double().reshape(B, 3, 2, H, W)
    mean = x.contiguous().view(B, 3, -1).mean(dim=-1).view(B, 3, 1, 1, 1)
    y = (x - mean) / rgb_max
    r1, r2 = S.ref_normalize(im1, im2, rgb_max)
    S.check(r1.reshape(B, 3, H, W), y[:, :, 0], 1e-12, 1e-12, "x1")
    S.check(r2.reshape(B, 3, H, W), y[:, :, 1], 1e-12, 1e-12, "x2")
    hw = H * W
    assert float(im1[B - 1, 1, 0]) == rgb_max and float(im2[B - 1, 1, hw - 1]) == rgb_max
    rest = torch.cat([im1[B - 1, 1, 1:], im2[B - 1, 1, :hw - 1]])
    assert float(rest.max()) <= 0.1 * rgb_max


@pytest.mark.parametrize("name", sorted(S.WARP_CASES))
def test_warp_reference_vs_oracle(name):
    """O.resample2d + O.channelnorm (vectorised fp32) and the scalar restatement of the CUDA kernel.  Both accumulate in fp32:
    1e-5 relative plus 1e-6 of the rms."""
    from oracle import vid2vid_oracle as O
    from oracle import native_ops_scalar as NS
    c = S.warp_case(name)
    img0, img1, flow = c["img0"].contiguous(), c["img1"].contiguous(), c["flow"]
    warped, r = S.ref_warp_diff_norm(img0, img1, flow)
    ow = O.resample2d(img1, flow)
    S.check(ow, warped, 1e-5, 1e-6, "warped vs oracle")
    S.check(O.channelnorm(img0 - ow)[:, 0], r.sqrt(), 1e-5, 1e-6, "norm vs oracle")
    S.check(torch.from_numpy(NS.resample2d_forward(img1.numpy(), flow.numpy())), warped, 1e-5, 1e-6, "warped vs the scalar restatement")


@pytest.mark.parametrize("case", S.RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c[1:])
def test_resize_reference_vs_interpolate(case):
    planes, H, W, OH, OW = case
    x = S.resize_case(planes, H, W)
    for scale in S.RESIZE_SCALES:
        bil = F.interpolate(x.double()[None], size=(OH, OW), mode="bilinear", align_corners=False)[0] * scale
        S.check(S.ref_resize(x, OH, OW, 1, scale), bil, 1e-12, 1e-12, "bilinear")           # fp64 on both sides
        near = F.interpolate(x[None], size=(OH, OW), mode="nearest")[0] * S.f32t(scale)
        assert torch.equal(S.ref_resize(x, OH, OW, 0, scale), near.double())


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("size", S.AVGPOOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_avgpool_reference_vs_avg_pool2d(size, prec):
    H, W = size
    x = S.avgpool_case(H, W, prec)
    N, cs = S.AVGPOOL_N, S.AVGPOOL_STRIDE
    t = F.avg_pool2d(x.double().reshape(N, H, W, cs).permute(0, 3, 1, 2), 3, stride=2, padding=1, count_include_pad=False)
    OH, OW = S.pooled_size(H, W)
    assert t.shape[2:] == (OH, OW)
    S.check(S.ref_avgpool3s2(x, N, H, W), t.permute(0, 2, 3, 1).reshape(N * OH * OW, cs), 1e-12, 1e-12, "avgpool")


def _fold_by_index(xp, N, H, W, pad, corners=True):
    """The fold as a scatter: padded row i lands on row |i - pad| mirrored at H - 1.  corners=False leaves out the sources that are
    mirrored along BOTH axes (each border counted, their crossing not): the mutation."""
    cs = xp.shape[1]
    HP, WP = H + 2 * pad, W + 2 * pad
    g = xp.double().reshape(N, HP, WP, cs)
    mirror = lambda i, n: (n - 1) - abs((n - 1) - abs(i - pad))
    out = torch.zeros(N, H, W, cs, dtype=torch.float64)
    for i in range(HP):
        for j in range(WP):
            if not corners and not (pad <= i < pad + H) and not (pad <= j < pad + W):
                continue
            out[:, mirror(i, H), mirror(j, W)] += g[:, i, j]
    return out.reshape(N * H * W, cs)


@pytest.mark.parametrize("case", S.FOLD_CASES, ids=lambda c: "%dx%dx%d-p%d" % c)
def test_fold_reference_vs_index_scatter(case):
    N, H, W, pad = case
    xp = S.fold_case(N, H, W, pad, "fp32")
    ref = S.ref_reflect_fold(xp, N, H, W, pad)
    S.check(_fold_by_index(xp, N, H, W, pad), ref, 1e-12, 1e-12, "fold")
    assert float(ref[:, S.FOLD_C:].abs().max()) == 0
    # the adjoint property itself, against a second random tensor: <pad(x), xp> == <x, fold(xp)>
    x = torch.randn(N, S.FOLD_STRIDE, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    y = F.pad(x, (pad,) * 4, mode="reflect") if pad else x
    lhs = float((y.permute(0, 2, 3, 1).reshape(-1, S.FOLD_STRIDE) * xp.double()).sum())
    rhs = float((x.permute(0, 2, 3, 1).reshape(-1, S.FOLD_STRIDE) * ref).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_instance_mean_reference_vs_oracle(name):
    from oracle import vid2vid_oracle as O
    feat, inst = S.instance_case(name)
    Cc, HW = feat.shape
    o = O.instance_mean(feat.double().reshape(1, Cc, 1, HW), inst.reshape(1, 1, 1, HW))
    S.check(S.ref_instance_mean(feat, inst), o.reshape(Cc, HW), 1e-12, 1e-12, "instance mean")    # fp64 on both sides


def test_fg_mask_reference_vs_compute_mask():
    """compute_mask of the reference model: a 0/1 mask per foreground label, summed, clamped."""
    x = S.ref_avgpool3s2(S.label_frames(17, 21), 1, 17, 21)
    for n_fg, fg in S.FG_SETS.items():
        for base in (0, S.LABEL_NC + 1):
            m = torch.zeros(x.shape[0], dtype=torch.float64)
            for f in fg:
                m = m + x[:, base + f]
            assert torch.equal(S.ref_fg_mask(x, base, fg), torch.clamp(m, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# what the input makers promise
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.WARP_CASES))
def test_warp_threshold_margin_and_shares(name):
    c = S.warp_case(name)
    B, Cc, H, W, _ = S.WARP_CASES[name]
    r = S.ref_warp_diff_norm(c["img0"], c["img1"], c["flow"])[1]
    thr = c["thr"]
    assert thr == S.f32(thr) and thr > 0
    assert float(((r - thr).abs() / thr).min()) >= S.THR_MARGIN
    below = float((r < thr).double().mean())
    assert 0.1 <= below <= 0.9
    # the kernel's fp32 sum of squares stays on its side: its error 2 sqrt(r) |e| + (C + 1) u r is below the margin
    e, _ = S.warp_bounds(c["img1"], Cc)
    assert float((2 * r.sqrt() * np.sqrt(Cc) * e + (Cc + 1) * U * r - S.THR_MARGIN * (r - thr).abs()).max()) < 0
    flow = c["flow"]
    assert float(flow[:, :, 0, 0].abs().min()) == 40 and float(flow[:, :, H - 1, W - 1].abs().min()) == 40
    cols = slice(None) if H > 1 else slice(3, 6)
    mid = flow[:, :, H // 2, cols]
    assert torch.equal(mid, torch.round(mid)) and (H == 1 or 0 < H // 2 < H - 1)
    if c["x"] is not None:
        assert c["img0"].data_ptr() == c["x"].data_ptr() and c["img1"].data_ptr() == c["x"].data_ptr() + 3 * H * W * 4


@pytest.mark.parametrize("case", S.RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c[1:])
def test_nearest_index_in_fp32_is_the_exact_one(case):
    _, H, W, OH, OW = case
    assert torch.equal(S.nearest_index_fp32(H, OH), S.nearest_index(H, OH)), "rows"
    assert torch.equal(S.nearest_index_fp32(W, OW), S.nearest_index(W, OW)), "columns"


def test_nearest_case_hits_integers():
    assert 3 * 10 % 6 == 0 and 5 * 6 % 10 == 0 and int(S.nearest_index(10, 6)[3]) == 5 and int(S.nearest_index(6, 10)[5]) == 3


def test_instance_cases_hold_what_they_promise():
    _, inst = S.instance_case("b")
    ids = torch.unique(inst.long())
    assert ids.numel() == 40 and 0 in ids and int(ids.min()) < 0 and 26001 in ids
    assert torch.equal(inst, inst.long().float())
    for base in S.COLLIDING:
        group = torch.tensor([base, base + S.SEG_SLOTS, base + 2 * S.SEG_SLOTS])
        assert all(int(v) in ids for v in group)
        assert len(set(S.seg_hash(group).tolist())) == 1, "ids %s do not share a bucket" % group.tolist()
    # the hash on signed ids is the kernel's unsigned product
    assert int(S.seg_hash(torch.tensor([-5]))[0]) == ((2 ** 32 - 5) * 2654435761) % 2 ** 32 % 4096
    # scattered: the pixels of an id are not one contiguous run
    first = inst.long() == int(inst[0])
    assert int((first[1:] != first[:-1]).sum()) > 2
    assert inst.numel() > 8192
    for name, n_ids in (("c", 4096), ("d", 5000)):
        feat, inst = S.instance_case(name)
        ids, cnt = torch.unique(inst.long(), return_counts=True)
        assert ids.numel() == n_ids and bool((cnt == 2).all()) and torch.equal(inst, inst.long().float())
        order = torch.argsort(inst.long(), stable=True)
        assert float((feat[:, order[0::2]].double() - feat[:, order[1::2]].double()).abs().min()) >= S.PAIR_GAP
        # "mean" and "own value" cannot be confused: they differ by half the gap, the bound is four orders below
        assert float(S.instance_mean_extra(feat, inst).max()) < 1e-5 < S.PAIR_GAP / 2


def test_fg_inputs_exceed_one_and_hold_fractions():
    x = S.ref_avgpool3s2(S.label_frames(17, 21), 1, 17, 21)
    frac = (x > 0) & (x < 1)
    assert bool(frac.any())
    for base in (0, S.LABEL_NC + 1):
        s = S.ref_fg_mask(x, base, S.FG_SETS[3], clamp=False)
        assert float(s.max()) > 1.05 and bool(((s > 0) & (s < 1)).any())
    raw = S.label_frames(9, 11)
    assert float(S.ref_fg_mask(raw, 0, S.FG_SETS[3], clamp=False).max()) == 2
    assert float(S.ref_fg_mask(S.label_frames(1, 1), 0, S.FG_SETS[3], clamp=False)[0]) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# what the bounds reject
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.NORMALIZE_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_normalize_bound_rejects_a_dropped_pixel(case):
    B, H, W, rgb_max = case
    im1, im2 = S.normalize_case(*case)
    r1, r2 = S.ref_normalize(im1, im2, rgb_max)
    rel, extra = S.normalize_bound(im1, im2, rgb_max)
    S.check(r1.float(), r1, rel, 0.0, "x1", extra=extra)                     # the fp32 rounding of the exact result passes
    both = torch.cat([im1, im2], 2).double()
    for lost in (both[:, :, :-1], both[:, :, 1:]):                          # the last pixel of im2, the first of im1
        mean = lost.sum(2, keepdim=True) / (2 * H * W)
        assert _rejected((im1.double() - mean) / rgb_max, r1, rel, 0.0, "x1", extra=extra)
        assert _rejected((im2.double() - mean) / rgb_max, r2, rel, 0.0, "x2", extra=extra)
    # ... on every plane, not only the one with the heavy ends
    mean = both[:, :, :-1].sum(2, keepdim=True) / (2 * H * W)
    for b in range(B):
        for ch in range(3):
            assert _rejected(((im2.double() - mean) / rgb_max)[b, ch], r2[b, ch], rel, 0.0, "x2", extra=extra[b, ch])
    # the order-free bound the issue warns of would let it pass at the large size
    if H * W > 60000:
        loose = (2 * H * W - 1) * U * both.abs().mean(2, keepdim=True) / rgb_max
        assert not _rejected((im2.double() - mean) / rgb_max, r2, rel, 0.0, "x2", extra=loose)


@pytest.mark.parametrize("name", sorted(S.WARP_CASES))
def test_warp_bounds_reject_swapped_weights_and_a_short_clamp(name):
    c = S.warp_case(name)
    B, Cc, H, W, _ = S.WARP_CASES[name]
    warped, r = S.ref_warp_diff_norm(c["img0"], c["img1"], c["flow"])
    e, (nrel, nextra) = S.warp_bounds(c["img1"], Cc)
    S.check(warped.float(), warped, U, 0.0, "warped", extra=e)
    for mut in (dict(swap_weights=True), dict(xr_limit=W - 2)):
        # (one row: yT == yB and beta has no effect, so exchanging the two is "alpha := beta": still a wrong result)
        w2, r2 = S.ref_warp_diff_norm(c["img0"], c["img1"], c["flow"], **mut)
        assert _rejected(w2, warped, 0.0, 0.0, "warped", extra=e), mut
        assert _rejected(r2.sqrt(), r.sqrt(), nrel, 0.0, "norm", extra=nextra), mut
        assert _rejected((r2 < c["thr"]).double(), (r < c["thr"]).double()), mut


@pytest.mark.parametrize("case", S.RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c[1:])
def test_resize_bounds_reject_a_shifted_coordinate_and_rounding(case):
    planes, H, W, OH, OW = case
    x = S.resize_case(planes, H, W)
    ref = S.ref_resize(x, OH, OW, 1, 5.0)
    extra = S.resize_bilinear_extra(x, 5.0)
    S.check(ref.float(), ref, U, 0.0, "bilinear", extra=extra)
    # the kernel's own arithmetic in fp32 (torch, no fma) stays inside the bound
    fy = (S.f32t(float(H)) / S.f32t(float(OH)) * (torch.arange(OH, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
    fx = (S.f32t(float(W)) / S.f32t(float(OW)) * (torch.arange(OW, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
    y0, x0 = fy.long().clamp(max=H - 1), fx.long().clamp(max=W - 1)
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    ly, lx = (fy - y0.float())[None, :, None], (fx - x0.float())[None, None, :]
    v = (1 - ly) * ((1 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]) + ly * ((1 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1])
    S.check(v * S.f32t(5.0), ref, 0.0, 0.0, "bilinear in fp32", extra=extra)
    if H > 1 or W > 1:                                                       # (one source pixel: every coordinate gives that pixel)
        assert _rejected(S.ref_resize(x, OH, OW, 1, 5.0, half=0), ref, 0.0, 0.0, "bilinear", extra=extra)
    if (H > 1 or W > 1) and OH * OW > 1:                                     # (one destination pixel: index 0 either way)
        near = S.ref_resize(x, OH, OW, 0, 5.0)
        assert _rejected(S.ref_resize(x, OH, OW, 0, 5.0, rounding="round"), near)
    assert _rejected(S.ref_resize(x, OH, OW, 1, 1.0), ref, 0.0, 0.0, "bilinear", extra=extra)          # out_scale forgotten


def test_layout_comparisons_reject_an_offset_off_by_one():
    for prec in S.PRECS:
        N, Cc, H, W, strides, off, scale, slope = S.PACK_CH_CASES[0]
        stride = strides[prec]
        x = S.planar_case(N, Cc, H, W, 41)
        ref = torch.full((N * H * W, stride), S.NAN)
        ref[:, off:off + Cc] = S.ref_pack_channels(x, scale, slope, prec).float()
        wrong = torch.full((N * H * W, stride), S.NAN)
        wrong[:, off + 1:off + 1 + Cc] = S.ref_pack_channels(x, scale, slope, prec).float()
        assert _rejected(wrong[:, off:off + Cc], ref[:, off:off + Cc])
        assert _rejected(S.ref_pack_channels(x, scale, 1.0, prec).float(), ref[:, off:off + Cc])           # the slope forgotten
        N, Cc, H, W, stride, off = S.UNPACK_CASES[0]
        y = S.nhwc_case(N * H * W, stride, prec, 43)
        assert _rejected(S.ref_unpack_channels(y, N, Cc, H * W, off - 1), S.ref_unpack_channels(y, N, Cc, H * W, off))
        P, Cc, ss, so, ds, do = S.CONCAT_CASES[0]
        src = S.nhwc_case(P, ss, prec, 44)
        assert _rejected(src[:, so + 1:so + 1 + Cc].float(), src[:, so:so + Cc].float())
        N, C0, C1, H, W, stride, s1 = S.PACK_CONCAT_CASES[1]
        x0, x1 = S.planar_case(N, C0, H, W, 45), S.planar_case(N, C1, H, W, 46)
        ref = S.ref_pack_concat(x0, x1, s1, stride, prec).float()
        assert _rejected(torch.roll(ref, 1, 1), ref) and _rejected(S.ref_pack_concat(x0, x1, 1.0, stride, prec).float(), ref)


def test_fg_mask_bound_rejects_a_missing_clamp():
    x = S.ref_avgpool3s2(S.label_frames(17, 21), 1, 17, 21)
    for base in (0, S.LABEL_NC + 1):
        ref = S.ref_fg_mask(x, base, S.FG_SETS[3])
        S.check(ref.float(), ref, *S.FG_BOUND, what="mask")
        assert _rejected(S.ref_fg_mask(x, base, S.FG_SETS[3], clamp=False), ref, *S.FG_BOUND)
        assert _rejected(S.ref_fg_mask(x, base, S.FG_SETS[3][:2]), ref, *S.FG_BOUND)                  # a label short
    assert _rejected(S.ref_fg_mask(x, 0, S.FG_SETS[1]), S.ref_fg_mask(x, S.LABEL_NC + 1, S.FG_SETS[1]), *S.FG_BOUND)   # the wrong frame


@pytest.mark.parametrize("prec", S.PRECS)
@pytest.mark.parametrize("size", S.AVGPOOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_avgpool_bound_rejects_count_include_pad(size, prec):
    H, W = size
    x = S.avgpool_case(H, W, prec)
    ref = S.ref_avgpool3s2(x, S.AVGPOOL_N, H, W)
    rel, extra = S.avgpool_bound(x, prec)
    S.check(ref.to(S.tdt(prec)).float(), ref, rel, 0.0, "avgpool", extra=extra)          # the stored rounding of the exact result passes
    assert _rejected(S.ref_avgpool3s2(x, S.AVGPOOL_N, H, W, include_pad=True), ref, rel, 0.0, extra=extra)


@pytest.mark.parametrize("prec", S.PRECS)
def test_fold_bound_rejects_corners_counted_once(prec):
    for N, H, W, pad in S.FOLD_CASES:
        xp = S.fold_case(N, H, W, pad, prec)
        ref = S.ref_reflect_fold(xp, N, H, W, pad)
        rel, extra = S.fold_bound(xp, N, H, W, pad, prec)
        S.check(ref.to(S.tdt(prec)).float(), ref, rel, 0.0, "fold", extra=extra)
        if pad:
            assert _rejected(_fold_by_index(xp, N, H, W, pad, corners=False), ref, rel, 0.0, extra=extra)


def test_instance_mean_bound_rejects_merged_ids():
    feat, inst = S.instance_case("b")
    ref, extra = S.ref_instance_mean(feat, inst), S.instance_mean_extra(feat, inst)
    S.check(ref.float(), ref, U, 0.0, "instance mean", extra=extra)
    merged = S.ref_instance_mean(feat, inst, merge=lambda ids: torch.where(ids == 7 + S.SEG_SLOTS, torch.full_like(ids, 7), ids))
    assert _rejected(merged, ref, 0.0, 0.0, extra=extra)
    assert _rejected(feat, ref, 0.0, 0.0, extra=extra)                                   # nothing averaged


# ---------------------------------------------------------------------------------------------------------------------------
# the guard helper and the comparison on host tensors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_helper_sees_stray_writes_and_unwritten_elements(dtype):
    P, stride, off, Cc = 6, 8, 3, 2
    mask = S.channel_mask(P, stride, off, Cc)

    def fresh():
        g = S.Guarded(P * stride, dtype)
        g.view.view(P, stride)[:, off:off + Cc] = 1.5                        # the "kernel"
        return g
    out = fresh().finish(mask)
    assert out.shape == (P * stride,) and bool(torch.isnan(out.view(P, stride)[:, 0]).all())
    with pytest.raises(AssertionError, match="guard band in front"):
        g = fresh(); g.buf[g.lo - 1] = 0.0; g.finish(mask)
    with pytest.raises(AssertionError, match="guard band in front"):
        g = fresh(); g.buf[0] = 0.0; g.finish(mask)
    with pytest.raises(AssertionError, match="guard band behind"):
        g = fresh(); g.buf[g.lo + g.n] = 0.0; g.finish(mask)
    with pytest.raises(AssertionError, match="guard band behind"):
        g = fresh(); g.buf[-1] = 0.0; g.finish(mask)
    with pytest.raises(AssertionError, match="outside the channels"):
        g = fresh(); g.view.view(P, stride)[2, off + Cc] = 1.5; g.finish(mask)     # one channel too far
    with pytest.raises(AssertionError, match="outside the channels"):
        g = fresh(); g.view.view(P, stride)[0, off - 1] = 1.5; g.finish(mask)
    with pytest.raises(AssertionError, match="NaN pre-fill"):
        g = fresh(); g.view.view(P, stride)[P - 1, off + Cc - 1] = S.NAN; g.finish(mask)       # the last pixel not written
    with pytest.raises(AssertionError, match="NaN pre-fill"):
        S.Guarded(4, dtype).finish()
    # a guard rewritten with the same VALUE but other bits (-0.0 over 0.0) counts
    g = S.Guarded(4, dtype, fill=0.0)
    g.view[:] = 1.0
    g.finish()
    g = S.Guarded(4, dtype, fill=0.0)
    g.view[1] = -0.0
    with pytest.raises(AssertionError, match="outside the channels"):
        g.finish(torch.tensor([True, False, True, True]))


def test_guard_helper_on_bytes_and_off_alignment():
    for lead in (0, 1):
        g = S.Guarded(17, torch.uint8, fill=0xA5, lead=lead)
        assert g.ptr() % 16 == lead and g.buf.data_ptr() % 16 == 0
        g.view[:] = 0
        g.finish()
        g.buf[g.lo - 1] = 0
        with pytest.raises(AssertionError, match="guard band in front"):
            g.finish()


def test_check_refuses_unwritten_and_out_of_bound_elements():
    ref = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    assert S.check(ref.clone(), ref) == 0.0
    got = ref.clone(); got[2, 3] = S.NAN
    with pytest.raises(AssertionError, match=r"element \[2, 3\]"):
        S.check(got, ref, 1.0, 1.0, extra=1e9)
    got = ref.clone(); got[1, 0] += 1e-6
    with pytest.raises(AssertionError):
        S.check(got, ref)
    assert abs(S.check(got, ref, 0.0, 0.0, extra=2e-6) - 0.5) < 1e-6
    with pytest.raises(AssertionError, match="shape"):
        S.check(ref[:2], ref)
    # the same inequality as norm_bwd_common.check where extra == 0
    import norm_bwd_common as NB
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(50, 3, generator=g, dtype=torch.float64)
    for eps in (1e-7, 1e-5, 1e-3):
        got = ref + eps * torch.randn(50, 3, generator=g, dtype=torch.float64)
        verdicts = []
        for fn in (S.check, NB.check):
            try:
                fn(got, ref, 1e-5, 1e-5, "x")
                verdicts.append(True)
            except AssertionError:
                verdicts.append(False)
        assert verdicts[0] == verdicts[1]


# ---------------------------------------------------------------------------------------------------------------------------
# argument validation (library in dry-run mode: nothing launches, a dummy non-null pointer stands for every buffer)
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_their_arguments():
    from vid2vid_amd.lib import lib
    t = torch.zeros(1 << 12)
    p = C.c_void_p(t.data_ptr())
    prev = lib.v2v_set_dry_run(1)
    try:
        # channel window past the stride
        assert lib.v2v_pack_channels_nhwc(p, p, 1, 3, 4, 4, 8, 5, 1.0, 0.1, F32, None) == 0, lib.v2v_last_error()
        assert lib.v2v_pack_channels_nhwc(p, p, 1, 3, 4, 4, 8, 6, 1.0, 0.1, F32, None) == EINVAL
        assert lib.v2v_pack_channels_nhwc(p, p, 1, 3, 4, 4, 8, -1, 1.0, 0.1, F32, None) == EINVAL
        assert lib.v2v_unpack_channels_nchw(p, p, 1, 2, 4, 4, 8, 6, BF16, None) == 0
        assert lib.v2v_unpack_channels_nchw(p, p, 1, 2, 4, 4, 8, 7, BF16, None) == EINVAL
        assert lib.v2v_concat_channels_nhwc(p, 8, 3, p, 24, 17, 5, 35, F32, None) == 0
        assert lib.v2v_concat_channels_nhwc(p, 8, 4, p, 24, 17, 5, 35, F32, None) == EINVAL
        assert lib.v2v_concat_channels_nhwc(p, 8, 3, p, 24, 20, 5, 35, F32, None) == EINVAL
        assert lib.v2v_pack_concat_nhwc(p, 3, p, 5, 0.05, p, 1, 4, 4, 8, F32, None) == 0
        assert lib.v2v_pack_concat_nhwc(p, 3, None, 0, 0.05, p, 1, 4, 4, 8, BF16, None) == 0
        assert lib.v2v_pack_concat_nhwc(p, 3, p, 6, 0.05, p, 1, 4, 4, 8, F32, None) == EINVAL
        assert lib.v2v_pack_concat_nhwc(p, 3, None, 5, 0.05, p, 1, 4, 4, 8, F32, None) == EINVAL
        # fg mask
        assert lib.v2v_fg_mask_nhwc(p, p, 99, 16, 5, p, 3, F32, None) == 0
        assert lib.v2v_fg_mask_nhwc(p, p, 99, 16, 5, p, 0, F32, None) == EINVAL
        assert lib.v2v_fg_mask_nhwc(p, p, 99, 16, 5, p, -1, F32, None) == EINVAL
        for a in ((None, p, p), (p, None, p), (p, p, None)):
            assert lib.v2v_fg_mask_nhwc(a[0], a[1], 99, 16, 5, a[2], 3, F32, None) == EINVAL
        # normalize
        assert lib.v2v_flownet_normalize(p, p, p, p, p, 1, 4, 4, 255.0, None) == 0
        assert lib.v2v_flownet_normalize(p, p, p, p, p, 1, 4, 4, 0.0, None) == EINVAL
        assert lib.v2v_flownet_normalize(p, p, p, p, None, 1, 4, 4, 255.0, None) == EINVAL
        # warp: mode, and at least one output
        for mode, want in ((0, 0), (1, 0), (2, EINVAL), (-1, EINVAL)):
            assert lib.v2v_warp_diff_norm(p, 48, p, 48, p, p, p, 1, 3, 4, 4, mode, 0.5, None) == want
        assert lib.v2v_warp_diff_norm(p, 48, p, 48, p, None, p, 1, 3, 4, 4, 0, 0.5, None) == 0
        assert lib.v2v_warp_diff_norm(p, 48, p, 48, p, p, None, 1, 3, 4, 4, 0, 0.5, None) == 0
        assert lib.v2v_warp_diff_norm(p, 48, p, 48, p, None, None, 1, 3, 4, 4, 0, 0.5, None) == EINVAL
        # resize
        assert lib.v2v_resize_planar(p, p, 1, 4, 4, 8, 8, 1, 1.0, None) == 0
        assert lib.v2v_resize_planar(p, p, 0, 4, 4, 8, 8, 1, 1.0, None) == EINVAL
        assert lib.v2v_resize_planar(p, p, 1, 4, 4, 0, 8, 1, 1.0, None) == EINVAL
        # fold
        assert lib.v2v_reflect_pad_fold(p, p, 1, 4, 5, 3, 8, F32, None) == 0
        assert lib.v2v_reflect_pad_fold(p, p, 1, 4, 5, 4, 8, F32, None) == EINVAL
        assert lib.v2v_reflect_pad_fold(p, p, 1, 5, 4, 4, 8, F32, None) == EINVAL
        assert lib.v2v_reflect_pad_fold(p, p, 1, 4, 5, -1, 8, F32, None) == EINVAL
        # avgpool: whole 16-byte vectors; instance mean; copies
        assert lib.v2v_avgpool3s2_nhwc(p, p, 1, 4, 4, 8, BF16, None) == 0
        assert lib.v2v_avgpool3s2_nhwc(p, p, 1, 4, 4, 4, BF16, None) == EINVAL
        assert lib.v2v_instance_mean_planar(p, p, p, p, 2, 16, None) == 0
        assert lib.v2v_instance_mean_planar(p, p, p, p, 0, 16, None) == EINVAL
        assert lib.v2v_instance_mean_planar(p, p, p, C.c_void_p(t.data_ptr() + 2), 2, 16, None) == EINVAL
        assert lib.v2v_instance_mean_workspace(2, 10000) == 4096 * 4 + 4096 * 3 * 4 + 10000 * 4
        assert lib.v2v_memset_zero(p, 16, None) == 0 and lib.v2v_memset_zero(None, 16, None) == EINVAL
        assert lib.v2v_memset_zero(p, -1, None) == EINVAL
        assert lib.v2v_memcpy_d2d(p, p, 16, None) == 0 and lib.v2v_memcpy_d2d(p, None, 16, None) == EINVAL
        assert not t.any(), "a dry-run call wrote to its buffer"
    finally:
        lib.v2v_set_dry_run(prev)
