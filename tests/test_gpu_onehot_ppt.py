"""The label stems' two forms (csrc/onehot_stem.hip): one 8x32 tile per workgroup (PPT = 1) and two vertically stacked tiles
(PPT = 2, each tap's weight blob fetched once for both).  The pair form changes which workgroup computes a pixel, never the
order in which the pixel's sum is formed, and every half writes the statistics row its tile has in the one-tile form.  So the
check is equality BIT FOR BIT, with V2V_ONEHOT_PPT forcing either form on the same inputs, of
  * the raw fp32 NHWC output,
  * the per-tile statistics rows,
  * with the in-launch finalize: scale / shift / mean / invstd and the running statistics, after each of two launches (the
    ticket counter re-arms itself),
and that the words around every output buffer keep their fill pattern.  No tolerance is involved.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NC = 35                       # label2city: 35 label planes (+ 1 edge plane) per frame -> 108 weight rows at T = 3
GUARD = 1024                  # fp32 words in front of and behind every output
FILL = -7.25                  # guard / background pattern (exact in fp32; no stem output of random weights equals it everywhere)


class _Guarded:
    """n fp32 words with GUARD words of FILL on either side."""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.float32, device=DEV)
        if init is not None:
            self.body().copy_(init)

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def bits(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + self.n:] == FILL).all()), "%s: guard band overwritten" % what
        return b[GUARD:GUARD + self.n].view(torch.int32).clone()


def _maps(B, T, H, W, seed):
    """Blocky labels with a few out-of-range values (255), and an instance map whose upper ~70 % of rows are ONE instance
    (tiles without any edge pixel: the edge pass is skipped) and whose lower rows change at every pixel (tiles full of
    edges)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, NC, (B, T, H // 3 + 1, W // 5 + 1), generator=g)
    lab = lab.repeat_interleave(3, 2).repeat_interleave(5, 3)[:, :, :H, :W].contiguous()
    lab[torch.rand(lab.shape, generator=g) < 0.02] = 255
    inst = torch.zeros(B, T, H, W, dtype=torch.int64)
    cut = (H * 7) // 10
    inst[:, :, cut:, :] = torch.randint(1, 1000, (B, T, H - cut, W), generator=g)
    return lab, inst


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _run(form, cfg, lab, inst, w, bias):
    from vid2vid_amd import lib as L
    lib = L.lib
    H, W, cout, prec, T, mode, edges, B, fin, slice_ = cfg
    dtype = L.BF16 if prec == "bf16" else L.F32
    cin = T * (NC + (1 if edges else 0))
    os.environ["V2V_ONEHOT_PPT"] = str(form)
    try:
        got = lib.v2v_onehot_conv_ppt(B, T, H, W, NC, int(edges), cout, dtype, slice_)
        assert got == (form if slice_ != 64 else 1), "V2V_ONEHOT_PPT=%d built form %d" % (form, got)
        n = lib.v2v_onehot_conv_table_bytes(cin, cout, dtype, slice_, T, NC)
        assert n > 0
        table = torch.zeros(n, dtype=torch.uint8, device=DEV)
        wd = w.to(DEV)
        L.check(lib.v2v_onehot_conv_pack_weights(_ptr(wd), _ptr(table), cin, cout, dtype, slice_, T, NC, None), "pack")
        if mode == "float":
            labels, insts, in_u8 = lab.float().to(DEV), inst.float().to(DEV), 0
        else:
            labels, insts, in_u8 = lab.to(torch.uint8).to(DEV), inst.to(torch.int32).to(DEV), 1
            if mode == "codes":
                codes = torch.empty(B * T, H, W, dtype=torch.uint8, device=DEV)
                for b in range(B):          # v2v_label_codes is per sample: edges do not cross samples
                    L.check(lib.v2v_label_codes(_ptr(labels[b]), _ptr(insts[b]) if edges else None, 1, _ptr(codes[b * T:]), T, H, W, NC, None),
                            "label_codes")
                labels, in_u8 = codes, 2
        inst_p = _ptr(insts) if edges else None
        bd = bias.to(DEV)
        rows = lib.v2v_onehot_conv_stats_rows(H, W)
        assert rows == -(-H // 8) * -(-W // 32)
        cstride = (cout + 3) // 4 * 4
        out = _Guarded(B * H * W * cstride)
        stats = _Guarded(B * rows * cout * 2)
        res = {}
        if B > 1:
            L.check(lib.v2v_onehot_conv7x7_batch(_ptr(labels), inst_p, in_u8, _ptr(table), _ptr(bd), out.ptr(), stats.ptr(), B, T, H, W,
                                                 NC, cout, cstride, dtype, slice_, None), "onehot_conv7x7_batch")
        elif fin:
            g = torch.Generator().manual_seed(5)
            counter = torch.zeros(8, dtype=torch.int32, device=DEV)
            gamma, beta = torch.randn(cout, generator=g).to(DEV), torch.randn(cout, generator=g).to(DEV)
            ss = _Guarded(4 * cout)
            rm, rv = _Guarded(cout, torch.zeros(cout)), _Guarded(cout, torch.ones(cout))
            fn = L.OneHotNorm()
            fn.counter, fn.gamma, fn.beta, fn.scale_shift = counter.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ss.ptr()
            fn.running_mean, fn.running_var, fn.eps, fn.momentum, fn.count = rm.ptr(), rv.ptr(), 1e-5, 0.1, H * W
            for launch in (1, 2):           # the second launch finds the ticket counter re-armed by the first
                L.check(lib.v2v_onehot_conv7x7_norm(_ptr(labels), inst_p, in_u8, _ptr(table), _ptr(bd), out.ptr(), stats.ptr(), T, H, W,
                                                    NC, cout, cstride, dtype, slice_, C.byref(fn), None), "onehot_conv7x7_norm")
                torch.cuda.synchronize()
                res["scale_shift_%d" % launch] = ss.bits("scale_shift")
                res["running_mean_%d" % launch] = rm.bits("running_mean")
                res["running_var_%d" % launch] = rv.bits("running_var")
                assert int(counter.abs().sum()) == 0, "ticket counter not re-armed"
        else:
            for _ in range(2):
                L.check(lib.v2v_onehot_conv7x7(_ptr(labels), inst_p, in_u8, _ptr(table), _ptr(bd), out.ptr(), stats.ptr(), T, H, W,
                                               NC, cout, cstride, dtype, slice_, None), "onehot_conv7x7")
        torch.cuda.synchronize()
        res["out"] = out.bits("out")
        res["stats"] = stats.bits("stats")
        # the launch did write: every real channel of every pixel, every statistics row
        o = out.body().view(B, H, W, cstride)[..., :cout].cpu()
        assert bool(torch.isfinite(o).all()) and not bool((o == FILL).any())
        assert not bool((stats.body().cpu() == FILL).any())
        return res
    finally:
        os.environ.pop("V2V_ONEHOT_PPT", None)


# (H, W, cout, precision, T, label input, instance edges, B, in-launch finalize, slice)
#  16x32 one pair | 8x32 a lone half | 24x40 odd tile rows + ragged width | 20x70 ragged both ways, the mirror reaches across the
#  half boundary | 40x33 five tile rows, one ragged column.  cout 128 / 64 / 16 = 32-channel slices x 4 / x 2, one 16-channel
#  slice; slice 64 has the one-tile form only (the switch must leave it alone).
CASES = [
    (16, 32, 128, "bf16", 3, "codes", True, 1, True, 0),
    (16, 32, 64, "fp32", 2, "float", True, 1, False, 0),
    (16, 32, 16, "bf16", 2, "u8", False, 2, False, 0),
    (8, 32, 128, "bf16", 3, "u8", True, 1, True, 0),
    (8, 32, 16, "fp32", 3, "codes", True, 2, False, 0),
    (8, 32, 64, "bf16", 2, "float", False, 1, False, 0),
    (24, 40, 64, "bf16", 3, "codes", True, 2, False, 0),
    (24, 40, 128, "fp32", 3, "u8", True, 1, True, 0),
    (24, 40, 16, "bf16", 2, "float", True, 1, True, 0),
    (20, 70, 128, "bf16", 2, "codes", True, 1, False, 0),
    (20, 70, 64, "fp32", 3, "float", False, 2, False, 0),
    (20, 70, 16, "bf16", 3, "u8", True, 1, True, 0),
    (40, 33, 128, "bf16", 3, "float", True, 2, False, 0),
    (40, 33, 64, "bf16", 3, "u8", False, 1, True, 0),
    (40, 33, 16, "fp32", 2, "codes", True, 1, True, 0),
    (40, 33, 100, "fp32", 3, "codes", False, 1, False, 0),
    (24, 40, 128, "bf16", 3, "codes", True, 1, True, 64),
]


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "%dx%d-c%d-%s-T%d-%s-%s-B%d-%s-s%d" % (
    c[0], c[1], c[2], c[3], c[4], c[5], "edges" if c[6] else "noedges", c[7], "fin" if c[8] else "nofin", c[9]))
def test_pair_form_equals_one_tile_form_bit_for_bit(cfg):
    H, W, cout, prec, T, mode, edges, B, fin, slice_ = cfg
    lab, inst = _maps(B, T, H, W, seed=H * 131 + W)
    g = torch.Generator().manual_seed(cout + T)
    w = torch.randn(cout, T * (NC + (1 if edges else 0)), 7, 7, generator=g) * 0.05
    bias = torch.randn(cout, generator=g)
    one = _run(1, cfg, lab, inst, w, bias)
    two = _run(2, cfg, lab, inst, w, bias)
    assert one.keys() == two.keys()
    for k in one:
        diff = int((one[k] != two[k]).sum())
        assert diff == 0, "%s: %d of %d words differ between the one-tile and the pair form" % (k, diff, one[k].numel())
