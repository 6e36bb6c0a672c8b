"""Multi-stream inference on the GPU: B sequences per frame plan.

The definition under test: stream b of a B-stream call produces what a batch-1 model with the same weights produces on
sequence b alone.  Model level: every stream against the pinned CPU oracle stepped on that stream alone (the 1e-3 per-pixel
bar of the inference-vs-oracle tests), streams that cannot see each other (bit equality), the interface.  Kernel level, all
bit exact: v2v_in_finalize_rows against v2v_bn_finalize on the sample's slice of the conv's statistics rows, and the batched
head / tail launches against the batch-1 launches per sample."""
import os
import tempfile

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from util import sd_from_npz, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = 5


@pytest.fixture(autouse=True)
def _fp32_default():
    from vid2vid_amd import networks as N
    N.set_precision("fp32")
    yield
    N.set_precision("fp32")


# ------------------------------------------------------------------ models and streams
def _model(g, S=1, precision="fp32", **kw):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "g"))
    for s in range(S):
        torch.save(sd_from_npz(g, "sd%d." % s), os.path.join(ck, "g", "latest_net_G%d.pth" % s))
    d = dict(name="g", checkpoints_dir=ck, label_nc=35, use_instance=True, fg=True, use_real_img=True, ngf=8, n_blocks=2,
             n_blocks_local=1, n_scales_spatial=S, n_downsample_G=2, loadSize=64, precision=precision)
    d.update(kw)
    return create_model(make_opt(**d))


def _label_stream(seed, H=32, W=64, n=FRAMES + 2):
    from vid2vid_amd import synthetic
    lab, inst, frames = synthetic.label2city_sequence(n, H, W, seed=seed, cell=8)
    return lab, inst, frames


def _label_inputs(streams, t):
    H, W = streams[0][0].shape[-2:]
    A = torch.stack([s[0][t:t + 3] for s in streams]).view(len(streams), 3, 1, H, W)
    I = torch.stack([s[1][t:t + 3] for s in streams]).view(len(streams), 3, 1, H, W)
    Bf = torch.cat([s[2][:, :2] for s in streams]) if t == 0 else None
    return A, Bf, I


def _run(model, streams, frames, inputs=_label_inputs):
    model.fake_B_prev = None
    outs = []
    for t in range(frames):
        fake, last = model.inference(*inputs(streams, t))
        outs.append((fake, last, [p.clone() for p in model.fake_B_prev]))
    return outs


_ORACLE = {}


def _oracle_frames(key, make, streams, frames, inputs):
    """Per stream: [(fake_B, real_A_last, window per scale)] of the CPU oracle stepped on that stream alone; computed once."""
    if key not in _ORACLE:
        res = []
        for s in streams:
            orc = make()
            per = []
            for t in range(frames):
                fake, last = orc.step(*inputs([s], t))
                per.append((fake.clone(), last.clone(), [p.clone() for p in orc.fake_B_prev]))
            res.append(per)
        _ORACLE[key] = res
    return _ORACLE[key]


def _check_against_oracle(outs, ref, S, what):
    worst = 0.0
    for t, (fake, last, window) in enumerate(outs):
        assert tuple(fake.shape[:2]) == (len(ref), 3)
        for b in range(len(ref)):
            rf, rl, rw = ref[b][t]
            worst = max(worst, assert_close(fake[b:b + 1], rf, 1e-3, "%s stream %d frame %d fake_B" % (what, b, t)))
            assert_close(last[b], rl, 1e-6, "%s stream %d frame %d real_A_last" % (what, b, t))
            for si in range(S):
                assert_close(window[si][b], rw[si], 1e-3, "%s stream %d frame %d fake_B_prev[%d]" % (what, b, t, si))
    print("%s: worst per-pixel relative error of fake_B %.2e" % (what, worst))


# ------------------------------------------------------------------ 1. per stream against the oracle
def test_three_label_streams_match_the_oracle_per_stream(golden):
    """B = 3, one spatial scale, labels + instances + --fg, fp32, 5 frames (first-frame plan -> steady plan): the fused head
    and tail, the batched stems, per-sample norms from the statistics rows."""
    from oracle import vid2vid_oracle as O
    g = golden("inference_label2city_s1_32x64")
    streams = [_label_stream(100 + b) for b in range(3)]
    sd = sd_from_npz(g, "sd0.")
    ref = _oracle_frames("s1", lambda: O.InferenceOracle([sd], 35, True, True, [26], 2, 2, 1), streams, FRAMES, _label_inputs)
    model = _model(g, 1)
    outs = _run(model, streams, FRAMES)
    _check_against_oracle(outs, ref, 1, "S=1 B=3")
    fp = model._active_plan
    assert fp.B == 3 and tuple(fp.labels.shape) == (3, 3, 32, 64) and not fp.use_raw_only


def test_two_streams_two_spatial_scales_match_the_oracle(golden):
    from oracle import vid2vid_oracle as O
    g = golden("inference_label2city_s2_32x64")
    streams = [_label_stream(100 + b) for b in range(2)]
    sds = [sd_from_npz(g, "sd%d." % s) for s in range(2)]
    ref = _oracle_frames("s2", lambda: O.InferenceOracle(sds, 35, True, True, [26], 2, 2, 1), streams, FRAMES, _label_inputs)
    outs = _run(_model(g, 2), streams, FRAMES)
    _check_against_oracle(outs, ref, 2, "S=2 B=2")


def _raw_inputs(streams, t):
    A = torch.cat([s[0][:, t:t + 3] for s in streams])
    return A, (torch.cat([s[1][:, :2] for s in streams]) if t == 0 else None), None


def test_two_raw_input_streams_match_the_oracle(golden):
    from oracle import vid2vid_oracle as O
    from vid2vid_amd import synthetic
    g = golden("inference_edge2face_s1_32x32")
    streams = [synthetic.edge2face_sequence(FRAMES + 2, 32, 32, seed=300 + b) for b in range(2)]
    sd = sd_from_npz(g, "sd0.")
    ref = _oracle_frames("raw", lambda: O.InferenceOracle([sd], 0, False, False, [], 2, 2, 1), streams, FRAMES, _raw_inputs)
    model = _model(g, 1, label_nc=0, input_nc=15, use_instance=False, fg=False)
    outs = _run(model, streams, FRAMES, _raw_inputs)
    _check_against_oracle(outs, ref, 1, "raw B=2")


# ------------------------------------------------------------------ 2. streams do not talk
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_streams_do_not_see_each_other(golden, precision):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1, precision=precision)
    s = [_label_stream(200 + b) for b in range(5)]
    n = 3
    base = [o[0] for o in _run(model, [s[0], s[1], s[2]], n)]
    assert tuple(base[0].shape) == (3, 3, 32, 64)
    other = [o[0] for o in _run(model, [s[0], s[3], s[4]], n)]
    rot1 = [o[0] for o in _run(model, [s[1], s[2], s[0]], n)]
    rot2 = [o[0] for o in _run(model, [s[2], s[0], s[1]], n)]
    for t in range(n):
        assert torch.isfinite(base[t]).all()
        assert torch.equal(base[t][0], other[t][0]), "frame %d: stream 0 changed with the data of streams 1 and 2" % t
        assert not torch.equal(base[t][1], other[t][1])
        for b, (run, pos) in {1: (rot1, 0), 2: (rot2, 0), 0: (rot1, 2)}.items():
            assert torch.equal(base[t][b], run[t][pos]), "frame %d: stream %d depends on its position" % (t, b)
        assert torch.equal(base[t][0], rot2[t][1]) and torch.equal(base[t][2], rot1[t][1])


# ------------------------------------------------------------------ 3. interface
def test_interface_shapes_restart_and_fresh_outputs(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1)
    s = [_label_stream(100 + b) for b in range(3)]
    f1, l1 = model.inference(*_label_inputs(s[:1], 0))
    assert tuple(f1.shape) == (1, 3, 32, 64) and tuple(l1.shape) == (36, 32, 64)
    assert [tuple(p.shape) for p in model.fake_B_prev] == [(2, 3, 32, 64)]
    with pytest.raises(ValueError):
        model.inference(*_label_inputs(s, 1))                    # B changes inside a sequence
    assert [tuple(p.shape) for p in model.fake_B_prev] == [(2, 3, 32, 64)]     # ... and nothing was restarted
    model.fake_B_prev = None
    fa, la = model.inference(*_label_inputs(s, 0))
    assert tuple(fa.shape) == (3, 3, 32, 64) and tuple(la.shape) == (3, 36, 32, 64)
    assert [tuple(p.shape) for p in model.fake_B_prev] == [(3, 2, 3, 32, 64)]
    keep = fa.clone()
    fb, lb = model.inference(*_label_inputs(s, 1))
    assert fa.data_ptr() != fb.data_ptr() and la.data_ptr() != lb.data_ptr()
    assert torch.equal(fa, keep) and not torch.equal(fa, fb)     # the first frame's tensor was not overwritten by the replay
    assert torch.equal(model.fake_B_prev[0][:, -1], fb)          # newest slot of every stream's window
    with pytest.raises(ValueError):
        model.inference(*_label_inputs(s[:2], 2))
    model.fake_B_prev = None                                     # restart: the same first frame again
    fc, _ = model.inference(*_label_inputs(s, 0))
    assert torch.equal(fc, keep)
    # stream 0 of the 3-stream call is the single-stream frame.  Not bit for bit: the B = 1 plan runs the paired fused-norm
    # launches, the B = 3 plan conv + finalize + apply, with other tiles and summation orders.  Both sides meet the oracle at the
    # 1e-3 per-pixel bar (tests 1 above, test_gpu_golden), so they agree with each other within twice that.
    assert_close(fc[:1], f1, 2e-3, "stream 0 of B = 3 against the B = 1 plan")


def test_single_stream_restart_after_multi_stream(golden):
    g = golden("inference_label2city_s1_32x64")
    model = _model(g, 1)
    s = [_label_stream(100 + b) for b in range(2)]
    solo = [o[0] for o in _run(model, s[:1], 2)]
    _run(model, s, 2)
    again = [o[0] for o in _run(model, s[:1], 2)]
    assert all(torch.equal(a, b) for a, b in zip(solo, again))


# ------------------------------------------------------------------ 4. v2v_in_finalize_rows
def _engine(precision="fp32"):
    from vid2vid_amd import networks as N
    N.set_precision(precision)
    return N.get_engine(DEV)


@pytest.mark.parametrize("C_", [6, 64, 72])
@pytest.mark.parametrize("N_", [1, 2, 3])
def test_in_finalize_rows_equals_bn_finalize_on_the_sample_slice(N_, C_):
    """Rows of a real conv launch (implicit-GEMM tile 3: 64-pixel M tiles), OH*OW of exactly one tile per sample and of two,
    with and without gamma / beta: all four output rows bit for bit v2v_bn_finalize on the sample's slice."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    eng = _engine()
    torch.manual_seed(N_ * 100 + C_)
    conv = nn.Conv2d(8, C_, 3, padding=1).to(DEV)
    eng.tile_override[(8, C_, 3, 1, 0)] = 3
    eng.per_stream = True
    try:
        for (H, W) in ((8, 8), (8, 16)):
            x = eng.pack(torch.randn(N_, 8, H, W, device=DEV))
            raw, rows, shp = eng.conv(x, conv, want_stats=True, label="t")
            rps = eng.last_rows_per_sample
            assert shp == (N_, H, W) and rps == H * W // 64 and rows == N_ * rps
            st = eng.scratch("stats", rows * C_ * 2)[:rows * C_ * 2].clone()
            for affine in (False, True):
                gamma = (torch.rand(C_, device=DEV) + 0.5) if affine else None
                beta = torch.randn(C_, device=DEV) if affine else None
                got = torch.full((N_, 4, C_), float("nan"), device=DEV)
                L.check(L.lib.v2v_in_finalize_rows(_ptr(st), rps, N_, C_, H * W, _ptr(gamma), _ptr(beta), 1e-5, _ptr(got), None,
                                                   _stream()), "in_finalize_rows")
                for n in range(N_):
                    want = torch.full((4, C_), float("nan"), device=DEV)
                    sl = st[n * rps * C_ * 2:(n + 1) * rps * C_ * 2].clone()
                    L.check(L.lib.v2v_bn_finalize(_ptr(sl), rps, C_, H * W, _ptr(gamma), _ptr(beta), 1e-5, _ptr(want), None, None,
                                                  0.1, None, _stream()), "bn_finalize")
                    assert torch.equal(got[n], want), (N_, C_, H, W, affine, n)
                # and the statistics are those of the sample's raw output
                r = raw[:N_ * H * W * ((C_ + 3) // 4 * 4)].view(N_, H * W, -1)[..., :C_].double()
                assert torch.allclose(got[:, 2].double(), r.mean(1), rtol=1e-5, atol=1e-6)
    finally:
        eng.per_stream = False
        eng.tile_override.pop((8, C_, 3, 1, 0), None)


def test_in_finalize_rows_two_stage_equals_bn_finalize():
    """More than 512 rows per sample: the row groups of v2v_bn_finalize's first stage, per sample, then its second stage."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import _ptr, _stream
    torch.manual_seed(3)
    N_, C_, rps = 2, 72, 515
    st = torch.randn(N_ * rps, C_, 2, device=DEV).abs_()
    nbytes = L.lib.v2v_in_finalize_rows_workspace(rps, C_, N_)
    assert nbytes == N_ * L.lib.v2v_bn_finalize_groups(rps) * C_ * 16 > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    got = torch.empty(N_, 4, C_, device=DEV)
    L.check(L.lib.v2v_in_finalize_rows(_ptr(st), rps, N_, C_, rps * 64, None, None, 1e-5, _ptr(got), _ptr(ws), _stream()), "rows")
    for n in range(N_):
        want = torch.empty(4, C_, device=DEV)
        ws1 = torch.empty(L.lib.v2v_bn_finalize_groups(rps) * C_ * 2, dtype=torch.float64, device=DEV)
        L.check(L.lib.v2v_bn_finalize(_ptr(st[n * rps:(n + 1) * rps].contiguous()), rps, C_, rps * 64, None, None, 1e-5, _ptr(want),
                                      None, None, 0.1, _ptr(ws1), _stream()), "bn_finalize")
        assert torch.equal(got[n], want)


@pytest.mark.parametrize("norm_cls", [nn.BatchNorm2d, nn.InstanceNorm2d])
def test_ragged_group_takes_in_stats_and_meets_the_bar(norm_cls):
    """OH*OW = 60 is no multiple of the 64-pixel M tile: rows straddle samples, the engine reads raw again (v2v_in_stats);
    one tile per sample (8x8) takes the rows.  Both against torch per sample at the 1e-3 bar."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Plan
    eng = _engine()
    torch.manual_seed(11)
    conv = nn.Conv2d(8, 16, 3, padding=1).to(DEV)
    norm = norm_cls(16, affine=norm_cls is nn.BatchNorm2d).to(DEV)
    if norm.affine:
        with torch.no_grad():
            norm.weight.uniform_(0.5, 1.5); norm.bias.normal_()
    eng.tile_override[(8, 16, 3, 1, 0)] = 3
    eng.per_stream = True
    try:
        for (H, W), want in (((6, 10), "in_stats"), ((8, 8), "in_finalize_rows")):
            xin = torch.randn(2, 8, H, W, device=DEV)
            with torch.no_grad():
                x = eng.pack(xin)
                plan = Plan()
                eng.plan = plan
                try:
                    with plan:
                        y = eng.conv_group(x, conv, L.PAD_ZERO, None, norm, L.ACT_RELU, 0.0, label="g")
                finally:
                    eng.plan = None
                names = [L.lib.v2v_plan_op_name(plan.h, i).decode() for i in range(plan.num_ops)]
                assert names[-2:] == [want, "in_apply"] and "conv" in names[-3], names
                plan.run()
                got = eng.unpack(y)
                ref = torch.cat([F.relu(F.batch_norm(conv(xin[n:n + 1]).double(), None, None,
                                                     None if not norm.affine else norm.weight.double(),
                                                     None if not norm.affine else norm.bias.double(), True, 0.1, norm.eps))
                                 for n in range(2)])
            assert_close(got, ref.float(), 1e-3, "%s %dx%d" % (norm_cls.__name__, H, W))
    finally:
        eng.per_stream = False
        eng.tile_override.pop((8, 16, 3, 1, 0), None)


# ------------------------------------------------------------------ 5. batched head and tail against batch 1, per sample
def _maps(B, T, H, W, u8, with_inst, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 35, (B, T, H, W), generator=g)
    lab[:, :, 1, 2] = 40                                          # out of range: no label plane
    lab[:, -1, 0, 0] = 26
    inst = torch.randint(0, 4, (B, T, H // 2 + 1, W // 2 + 1), generator=g).repeat_interleave(2, 2).repeat_interleave(2, 3)[..., :H, :W]
    inst[:, :, 0, 1] += 7; inst[:, :, H - 1, W - 2] += 7; inst[:, :, 2, 0] += 7; inst[:, :, H - 3, W - 1] += 7     # edges on all four borders
    if u8:
        return lab.to(torch.uint8).to(DEV), (inst.to(torch.int32).to(DEV) if with_inst else None)
    return lab.float().to(DEV), (inst.float().to(DEV) if with_inst else None)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("HW", [(24, 40), (8, 8)])
def test_batched_prologue_equals_batch_one_per_sample(precision, B, HW):
    from vid2vid_amd.engine import LabelSource
    eng = _engine(precision)
    H, W = HW
    T = 3
    for u8 in (False, True):
        for with_inst in (True, False):
            for fg in ((), (26,)):
                lab, inst = _maps(B, T, H, W, u8, with_inst, seed=B * 10 + H)
                win = torch.randn(B, 6, H, W, device=DEV)
                src = LabelSource(lab, inst, T, 35)
                x0, mask, packed, last = eng.frame_prologue(src, H, W, fg, True, window=win, last_C=3)
                assert x0.N == B and tuple(src.codes.shape) == (B, T, H, W) and tuple(mask.shape) == (B, 1, H, W)
                assert tuple(last.shape) == (B, 3, H, W) and packed.N == B
                for b in range(B):
                    s1 = LabelSource(lab[b], None if inst is None else inst[b], T, 35)
                    _, m1, p1, l1 = eng.frame_prologue(s1, H, W, fg, True, window=win[b:b + 1], last_C=3)
                    assert torch.equal(src.codes[b], s1.codes) and torch.equal(mask[b], m1[0])
                    assert torch.equal(packed.t[b], p1.t[0]) and torch.equal(last[b], l1[0])
                if with_inst:
                    assert (src.codes & 128).any() and ((src.codes & 127) == 127).any()
                assert bool(mask.any()) == bool(fg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("HW", [(4, 4), (24, 40)])
def test_batched_gather_sum_stem_equals_batch_one_per_sample(precision, HW):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import LabelSource
    eng = _engine(precision)
    H, W = HW
    T, B = 3, 3
    torch.manual_seed(5)
    for cout, with_inst in ((16, True), (40, True), (16, False)):
        per = 35 + int(with_inst)
        conv = nn.Conv2d(T * per, cout, 7).to(DEV)
        lab, inst = _maps(B, T, H, W, False, with_inst, seed=H + cout)
        src = LabelSource(lab, inst, T, 35)
        x0, _, _, _ = eng.frame_prologue(src, H, W, (), False)
        cs = (cout + 3) // 4 * 4
        raw, rows, shp = eng.onehot_conv(x0, conv, label="stem")
        tiles = L.lib.v2v_onehot_conv_stats_rows(H, W)
        assert shp == (B, H, W) and rows == B * tiles
        raw = raw[:B * H * W * cs].view(B, H, W, cs)[..., :cout].clone()
        st = eng.scratch("stats", rows * cout * 2)[:rows * cout * 2].view(B, tiles, cout, 2).clone()
        for b in range(B):
            s1 = LabelSource(lab[b], None if inst is None else inst[b], T, 35)
            x1, _, _, _ = eng.frame_prologue(s1, H, W, (), False)
            r1, rows1, _ = eng.onehot_conv(x1, conv, label="stem")
            assert rows1 == tiles
            assert torch.equal(raw[b], r1[:H * W * cs].view(H, W, cs)[..., :cout])
            assert torch.equal(st[b], eng.scratch("stats", rows1 * cout * 2)[:rows1 * cout * 2].view(tiles, cout, 2))
        assert torch.isfinite(raw).all() and raw.abs().max() > 0


@pytest.mark.parametrize("B", [2, 3])
def test_batched_rolling_blend_equals_batch_one_per_sample(B):
    eng = _engine()
    H, W, slots = 24, 40, 2
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    raw0, flow, wgt, prev, fg = r(B, 3, H, W), 3.0 * r(B, 2, H, W), torch.sigmoid(r(B, 1, H, W)), r(B, 3, H, W), r(B, 3, H, W)
    mask = (r(B, 1, H, W) > 0.5).float()
    win0 = r(B, slots, 3, H, W)
    for with_fg in (True, False):
        raw, win = raw0.clone(), win0.clone()
        final, _ = eng.warp_blend(raw, flow, wgt, prev, fg if with_fg else None, mask if with_fg else None, roll=win)
        for b in range(B):
            raw1, win1 = raw0[b:b + 1].clone(), win0[b].clone()
            f1, _ = eng.warp_blend(raw1, flow[b:b + 1].contiguous(), wgt[b:b + 1].contiguous(), prev[b:b + 1].contiguous(),
                                   fg[b:b + 1].contiguous() if with_fg else None, mask[b:b + 1].contiguous() if with_fg else None, roll=win1)
            assert torch.equal(final[b], f1[0]) and torch.equal(raw[b], raw1[0])
            assert torch.equal(win[b], win1), "window contents after the launch"
            assert torch.equal(win[b, 0], win0[b, 1]) and torch.equal(win[b, 1], final[b])
    with pytest.raises(RuntimeError, match="overlap"):                     # the gather source inside a rolled window is refused
        w = win0.clone()
        inside = w.view(-1)[3 * H * W:3 * H * W * (B + 1)].view(B, 3, H, W)      # dense (B, 3, H, W) inside the windows
        eng.warp_blend(raw0.clone(), flow, wgt, inside, None, None, roll=w)


@pytest.mark.parametrize("u8", [False, True])
def test_batched_onehot_planar_equals_batch_one_per_sample(u8):
    eng = _engine()
    B, T, H, W = 3, 3, 24, 40
    for with_inst in (True, False):
        lab, inst = _maps(B, T, H, W, u8, with_inst, seed=9)
        out = eng.onehot_planar(lab[:, T - 1], None if inst is None else inst[:, T - 1], H, W, 35)
        assert tuple(out.shape) == (B, 35 + int(with_inst), H, W)
        for b in range(B):
            assert torch.equal(out[b], eng.onehot_planar(lab[b, T - 1], None if inst is None else inst[b, T - 1], H, W, 35))
        assert out[:, :35].sum(1).min() == 0 and out[:, :35].sum(1).max() == 1      # the out-of-range label has no plane
