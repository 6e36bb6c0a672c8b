"""Head and tail of the one-scale inference frame: v2v_frame_prologue (label codes + foreground mask + window pack in one
launch, no one-hot tensor) and v2v_warp_blend_roll (the blend rolls the window of generated frames itself).  Both are checked
bit for bit: the prologue against the three kernels it replaces, the frame plan against the same model on the plan that still
uses them (encode_labels, pack_nchw_to_nhwc, two device copies)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T_G, LABEL_NC = 3, 35


def _engine(prec):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine
    return Engine(DEV, L.BF16 if prec == "bf16" else L.F32)


def _maps(H, W, with_inst, seed):
    """Label maps with an out-of-range label, instance maps whose edges touch all four borders."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, LABEL_NC, (T_G, H, W), generator=g)
    lab[:, ::3, 1::4] = 26                              # foreground label present in every frame
    lab[0, 1, 2] = 200                                  # out of range: no label plane, code 127
    lab[T_G - 1, H - 1, W - 1] = LABEL_NC               # first id outside [0, label_nc)
    inst = None
    if with_inst:
        inst = torch.randint(0, 4, (T_G, H // 4 + 1, W // 4 + 1), generator=g)
        inst = inst.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, 1:H + 1, 2:W + 2].contiguous()
        inst[:, 0, 3] = 1000                            # edges on the top, bottom, left and right borders and in two corners
        inst[:, H - 1, 5] = 1001
        inst[:, 2, 0] = 1002
        inst[:, 4, W - 1] = 1003
        inst[:, 0, 0] = 1004
        inst[:, H - 1, W - 1] = 1005
    return lab, inst


@pytest.mark.parametrize("fg_labels", [(), (26,)])
@pytest.mark.parametrize("with_inst", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("H,W", [(24, 40), (8, 8)])
def test_prologue_equals_the_three_kernels(H, W, prec, u8, with_inst, fg_labels):
    from vid2vid_amd.engine import LabelSource
    eng = _engine(prec)
    lab, inst = _maps(H, W, with_inst, seed=H * W)
    labd = lab.to(DEV, torch.uint8 if u8 else torch.float32)
    instd = None if inst is None else inst.to(DEV, torch.int32 if u8 else torch.float32)
    window = torch.randn(1, (T_G - 1) * 3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    # the three existing launches
    ref_src = LabelSource(labd, instd, T_G, LABEL_NC)
    ref_codes = eng.label_codes(ref_src, H, W)
    _, ref_mask = eng.encode_labels(labd, instd, T_G, H, W, LABEL_NC, fg_labels, True)
    ref_pack = eng.pack(window)
    # the prologue; its outputs come from torch.empty: poison the allocator's recycled blocks first
    for shape, dt in (((T_G, H, W), torch.uint8), ((1, 1, H, W), torch.float32), (tuple(ref_pack.t.shape), ref_pack.t.dtype),
                      ((1, 3, H, W), torch.float32)):
        junk = torch.empty(shape, dtype=dt, device=DEV)
        junk.view(torch.uint8).fill_(0x7f)
        del junk
    src = LabelSource(labd, instd, T_G, LABEL_NC)
    x0, mask, packed, last = eng.frame_prologue(src, H, W, fg_labels, True, window=window, last_C=3)
    torch.cuda.synchronize()
    assert torch.equal(src.codes, ref_codes)
    assert int((src.codes & 127).eq(127).sum()) >= 2, "the out-of-range labels must be in the map"
    if with_inst:
        e = src.codes[0] >> 7
        assert e[0, 3] and e[H - 1, 5] and e[2, 0] and e[4, W - 1] and e[0, 0] and e[H - 1, W - 1]
    assert torch.equal(mask, ref_mask)
    assert bool(mask.any()) == bool(fg_labels)
    assert packed.C == ref_pack.C and packed.Cs == ref_pack.Cs
    assert torch.equal(packed.t.view(torch.uint8), ref_pack.t.view(torch.uint8))
    assert packed.Cs > packed.C and not packed.t[..., packed.C:].any(), "pad channels are zero"
    assert torch.equal(last, window[:, -3:])
    # the Act a gather-sum stem sees: shape and source of the encoding, no storage
    per = LABEL_NC + int(with_inst)
    assert (x0.N, x0.H, x0.W, x0.C) == (1, H, W, T_G * per) and x0.onehot is src and x0.t.device.type == "meta"
    # without a window: codes and mask only
    src2 = LabelSource(labd, instd, T_G, LABEL_NC)
    _, mask2, packed2, last2 = eng.frame_prologue(src2, H, W, fg_labels, False)
    assert mask2 is None and packed2 is None and last2 is None and torch.equal(src2.codes, ref_codes)


@pytest.mark.parametrize("with_fg", [False, True])
@pytest.mark.parametrize("H,W", [(24, 40), (8, 8)])
def test_warp_blend_roll_equals_blend_then_copies(H, W, with_fg):
    eng = _engine("fp32")
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    window = rnd(T_G - 1, 3, H, W)
    raw, flow, weight = rnd(1, 3, H, W), 3.0 * rnd(1, 2, H, W), torch.sigmoid(rnd(1, 1, H, W))
    fg = rnd(1, 3, H, W) if with_fg else None
    mask = (rnd(1, 1, H, W) > 0).float() if with_fg else None
    raw_a, raw_b = raw.clone(), raw.clone()
    ref, _ = eng.warp_blend(raw_a, flow, weight, window[-1:].clone(), fg, mask)
    ref_window = torch.cat([window[1:], ref])
    rolled = window.clone()
    got, _ = eng.warp_blend(raw_b, flow, weight, window[-1:].clone(), fg, mask, roll=rolled)
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and torch.equal(raw_b, raw_a)
    assert torch.equal(rolled, ref_window)
    with pytest.raises(RuntimeError):                   # gathering from the window the launch rolls is refused
        eng.warp_blend(raw_b, flow, weight, rolled[-1:], fg, mask, roll=rolled)


def _plan_ops(model):
    from vid2vid_amd.lib import lib
    p = model._active_plan.plan
    return [lib.v2v_plan_op_name(p.h, i).decode() for i in range(p.num_ops)]


def _model(prec, no_first_img):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    opt = make_opt(label_nc=LABEL_NC, use_instance=True, fg=True, use_real_img=not no_first_img, no_first_img=no_first_img,
                   random_init_ok=True, ngf=8, n_blocks=2, n_downsample_G=2, loadSize=64, precision=prec, gpu_ids=[0])
    return create_model(opt)


def _five_frames(model, lab, inst, frames, check_window):
    H, W = lab.shape[-2:]
    model.fake_B_prev = None
    outs, kept, plans = [], [], []
    for t in range(5):
        fake, real_A = model.inference(lab[t:t + 3].view(1, 3, 1, H, W), frames[:, :2] if t == 0 else None,
                                       inst[t:t + 3].view(1, 3, 1, H, W))
        outs.append((fake, real_A))
        kept.append((fake.clone(), real_A.clone()))
        plans.append(model._active_plan)
        if check_window:
            win = model.fake_B_prev[0]
            assert win.shape == (T_G - 1, 3, H, W)
            assert torch.equal(win[-1], fake[0]), "frame %d: the newest slot holds the frame just generated" % t
            if t >= 1:
                assert torch.equal(win[-2], kept[t - 1][0][0]), "frame %d: the slot before it holds the previous frame" % t
    torch.cuda.synchronize()
    for t in range(5):                                   # returned tensors are fresh: later replays do not change them
        assert torch.equal(outs[t][0], kept[t][0]) and torch.equal(outs[t][1], kept[t][1]), "frame %d aliases a plan buffer" % t
    return kept, plans


@pytest.mark.parametrize("prec,no_first_img", [("bf16", True), ("fp32", True), ("bf16", False)])
def test_five_frames_equal_the_unfused_plan(prec, no_first_img, monkeypatch):
    """label2city 64x32, S = 1, --fg --use_instance.  no_first_img: frame 0 runs the raw-only plan (no warp, the blend with the
    foreground still rolls the window), frame 1 switches to the steady plan."""
    from vid2vid_amd import synthetic
    H, W = 32, 64
    lab, inst, frames = synthetic.label2city_sequence(7, H, W, seed=11)
    torch.manual_seed(0)
    new = _model(prec, no_first_img)
    with torch.no_grad():
        new.netG0.model_final_flow[1].weight.mul_(20.0)          # flows of a few pixels: the gather leaves its own pixel
    new.engine.refresh_weights()
    old = _model(prec, no_first_img)
    old.netG0.load_state_dict(new.netG0.state_dict())
    old.engine.refresh_weights()
    # the second model records its plans with the codes switched off: encode_labels writes the one-hot tensor, the stems read the
    # maps, pack_nchw_to_nhwc packs the window and two device copies roll it
    monkeypatch.setenv("V2V_LABEL_CODES", "0")
    ref, _ = _five_frames(old, lab, inst, frames, check_window=True)
    ops_old = _plan_ops(old)
    monkeypatch.delenv("V2V_LABEL_CODES")
    got, plans = _five_frames(new, lab, inst, frames, check_window=True)
    ops_new = _plan_ops(new)
    assert "encode_labels" in ops_old and "memcpy_d2d" in ops_old and "frame_prologue" not in ops_old
    assert ops_new.count("frame_prologue") == 1
    assert not {"encode_labels", "label_codes", "pack_nchw_to_nhwc", "memcpy_d2d"} & set(ops_new)
    assert (plans[0] is not plans[1]) == no_first_img and plans[1] is plans[4]
    flows = new._active_plan.out["flow0"]
    assert float(flows.abs().max()) > 1.0, "the test needs a flow that displaces the gather"
    for t in range(5):
        assert torch.equal(got[t][0], ref[t][0]), "fake_B of frame %d differs from the unfused plan" % t
        assert torch.equal(got[t][1], ref[t][1]), "real_A_last of frame %d differs from the unfused plan" % t
    assert torch.isfinite(got[4][0]).all() and float(got[4][0].std()) > 0
