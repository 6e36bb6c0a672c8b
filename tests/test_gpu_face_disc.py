"""--add_face_disc on the MI355X: the three face-window kernels (v2v_face_window, v2v_pack_concat_window_nhwc,
v2v_unpack_window_nchw) against torch restatements, and the face discriminator of Vid2VidModelD against the reference's
own CPU run (tests/golden/face_disc_pose_64x128.npz, made by tests/golden/make_golden_pose.py), against the oracle at the
pose2body_512p geometry, without a host synchronisation, and inside one train.py-ordered chunk."""
import os

import numpy as np
import pytest
import torch

from util import assert_close
from face_disc_common import CASES, FINE, ORDER, face_region_torch, fill_weights, make_inputs

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "face_disc_pose_64x128.npz")
FACE_LOSSES = ["G_f_GAN", "G_f_GAN_Feat", "D_f_real", "D_f_fake"]


def _engine(prec="fp32"):
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine
    return Engine(DEV, L.BF16 if prec == "bf16" else L.F32)


def _face_maps(N, H, W, openpose, kind, gen):
    a = (torch.rand(N, 3, H, W, generator=gen) * 1.6 - 0.8)
    if kind == "random":
        m = torch.rand(N, H, W, generator=gen) < 2e-4
    else:
        m = torch.zeros(N, H, W, dtype=torch.bool)
        if kind == "single":
            m[N - 1, H // 3, W // 5] = True
        elif kind == "corner_tl":
            m[0, 0, 0] = True
        elif kind == "corner_br":
            m[N - 1, H - 1, W - 1] = True
        elif kind == "full":
            m[:] = True
        elif kind == "union":
            m[0, 2, W - 3] = True; m[N - 1, H - 2, 1] = True
    if openpose:
        a[:, 0][m], a[:, 1][m], a[:, 2][m] = 0.2, -1.0, -0.6
        if kind == "random":         # near misses of every threshold
            nm = torch.rand(N, H, W, generator=gen) < 1e-3
            a[:, 0][nm], a[:, 1][nm], a[:, 2][nm] = 0.21, -1.0, -0.6
    else:
        a[:, 2][m] = 0.95
        if kind == "random":
            nm = torch.rand(N, H, W, generator=gen) < 1e-3
            a[:, 2][nm] = 0.9
    return torch.cat([a, torch.rand(N, 3, H, W, generator=gen)], 1)       # 6 channels as the pose input


@pytest.mark.gpu
@pytest.mark.parametrize("openpose", [False, True])
def test_face_window_equals_torch_exactly(openpose):
    eng = _engine()
    gen = torch.Generator().manual_seed(3 + openpose)
    checked = 0
    for (H, W, fine) in ((64, 128, 128), (512, 256, 512), (1024, 512, 1024)):
        crop = fine // 32 * 8
        for N in (1, 3, 6):
            for kind in ("random", "empty", "single", "corner_tl", "corner_br", "full", "union"):
                a = _face_maps(N, H, W, openpose, kind, gen)
                want = face_region_torch(a, fine, openpose)
                win = eng.face_window(a.to(DEV), openpose, crop, crop)
                got = [int(v) for v in win.cpu().tolist()]
                if want[0] is None:
                    assert got[0] == 0, (H, W, N, kind)
                    assert 0 <= got[1] and got[2] - got[1] == crop and got[2] <= H and 0 <= got[3] and got[4] - got[3] == crop and got[4] <= W
                else:
                    assert got[0] == 1 and tuple(got[1:5]) == want, (H, W, N, kind, got, want)
                checked += 1
    # repeated calls with other shapes never see an earlier call's accumulators
    a = _face_maps(2, 64, 128, openpose, "empty", gen)
    assert int(eng.face_window(a.to(DEV), openpose, 32, 32)[0].item()) == 0
    assert checked == 63


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_window_pack_and_unpack_equal_slicing(prec):
    from vid2vid_amd import autograd as AG
    from vid2vid_amd import lib as L
    eng = _engine(prec)
    gen = torch.Generator().manual_seed(11)
    N, H, W, crop = 3, 64, 128, 32
    for kind in ("random", "corner_tl", "corner_br", "empty"):
        a = _face_maps(N, H, W, False, kind, gen).to(DEV)
        b = torch.randn(N, 3, H, W, generator=gen).to(DEV)
        win = eng.face_window(a, False, crop, crop)
        _, ys, ye, xs, xe = [int(v) for v in win[:5].tolist()]
        got = AG.pack_concat_window(eng, a, b, win, (crop, crop))
        ref = AG.pack_concat(eng, a[:, :, ys:ye, xs:xe].contiguous(), b[:, :, ys:ye, xs:xe].contiguous())
        assert got.C == ref.C == 9 and got.t.shape == ref.t.shape
        assert torch.equal(got.t, ref.t), kind                            # same values, same padding channels
        if prec == "bf16":
            cat = torch.cat([a, b], 1)[:, :, ys:ye, xs:xe].permute(0, 2, 3, 1)
            assert torch.equal(got.t[..., :9], cat.to(torch.bfloat16))
        # backward of the x1 operand: the window's slice inside, zeros outside
        dy = torch.randn(got.t.shape, generator=gen).to(DEV).to(got.t.dtype)
        dx = torch.full((N, 3, H, W), float("nan"), device=DEV)
        cs = got.t.shape[-1]
        L.check(L.lib.v2v_unpack_window_nchw(dy.data_ptr(), win.data_ptr(), N, 3, H, W, crop, crop, cs, 6, dx.data_ptr(),
                                             eng.dtype, torch.cuda.current_stream().cuda_stream), "unpack_window")
        want = torch.zeros(N, 3, H, W, device=DEV)
        want[:, :, ys:ye, xs:xe] = dy[..., 6:9].permute(0, 3, 1, 2).float()
        assert torch.equal(dx, want), kind
        # through autograd: gradient to b only, and a gradient request for real_A is refused
        bb = b.clone().requires_grad_(True)
        y = AG.pack_concat_window(eng, a, bb, win, (crop, crop))
        y.t.backward(dy)
        assert torch.equal(bb.grad, want)
    with pytest.raises(NotImplementedError):
        AG.pack_concat_window(eng, a.clone().requires_grad_(True), b, win, (crop, crop))


def _golden_model(case):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    opt = make_opt(isTrain=True, label_nc=0, input_nc=6, add_face_disc=True, num_D=3, ndf=8, no_vgg=True, loadSize=FINE,
                   fineSize=FINE, n_scales_temporal=1, precision="fp32", gpu_ids=[0], random_init_ok=True,
                   openpose_only=case == "openpose")
    D = Vid2VidModelD(); D.initialize(opt)
    fill_weights(D.netD, 100)
    fill_weights(D.netD_f, 200)
    D.engine.refresh_weights()
    return D


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_face_disc_vs_reference_golden(case):
    g = np.load(GOLDEN)
    D = _golden_model(case)
    assert D.loss_names == [str(n) for n in g["loss_names"]]
    t = {k: v.to(DEV) for k, v in make_inputs(case).items()}
    t["fake_B"].requires_grad_(True)
    region = D.get_face_region(t["real_A"])
    assert tuple(-1 if v is None else v for v in region) == tuple(int(v) for v in g["%s.region" % case])
    losses = D(0, [t[k] for k in ORDER])
    ld = dict(zip(D.loss_names, [torch.mean(x) for x in losses]))
    loss_G, loss_D, _, _ = D.get_losses(ld, [], 0)
    for k in list(ld) + ["total_G", "total_D"]:
        v = float((ld[k] if k in ld else loss_G if k == "total_G" else loss_D).detach())
        ref = float(g["%s.loss.%s" % (case, k)])
        assert abs(v - ref) <= 1e-3 * max(abs(ref), 1e-3), "%s loss %s: %.6f vs %.6f" % (case, k, v, ref)
    if case == "none":
        assert all(float(ld[k].detach()) == 0.0 for k in FACE_LOSSES)
    # netD_f's gradients of loss_D
    D.optimizer_D.zero_grad()
    loss_D.backward(retain_graph=True)
    if case == "none":                                                    # exact zeros (reference: no D_f term at all)
        for name, p in D.netD_f.named_parameters():
            assert p.grad is None or not p.grad.any(), name
    elif "%s.gradDf.%s" % (case, next(D.netD_f.named_parameters())[0]) in g:
        names = [n for n, _ in D.netD_f.named_parameters()]
        scale = np.sqrt(np.mean(np.concatenate([g["%s.gradDf.%s" % (case, n)].ravel() for n in names]) ** 2))
        checked = 0
        for name, p in D.netD_f.named_parameters():
            rv = torch.as_tensor(g["%s.gradDf.%s" % (case, name)])
            if np.sqrt(np.mean(rv.numpy() ** 2)) < 1e-3 * scale:       # biases in front of a norm: rounding noise only
                assert p.grad.abs().max().item() < 1e-2 * scale, name
                continue
            assert_close(p.grad.contiguous(), rv, 1e-3, "%s grad D_f %s" % (case, name))
            checked += 1
        assert checked >= 4
    # d loss_G / d fake_B, and the face path's share
    (g_all,) = torch.autograd.grad(loss_G, t["fake_B"], retain_graph=True)
    if "%s.dfake_B" % case in g:
        assert_close(g_all, g["%s.dfake_B" % case], 1e-3, "%s d loss_G / d fake_B" % case)
    (g_face,) = torch.autograd.grad(ld["G_f_GAN"] + ld["G_f_GAN_Feat"], t["fake_B"], retain_graph=True)
    if region[0] is None:
        assert not g_face.any()
    else:
        ys, ye, xs, xe = region
        assert_close(g_face[:, :, ys:ye, xs:xe], g["%s.dfake_B_face_win" % case], 1e-3, "%s face d fake_B" % case)
        outside = g_face.clone()
        outside[:, :, ys:ye, xs:xe] = 0
        assert not outside.any()


def _oracle_face(sdf, real_A, real_B, fake_B, win, num_D_opt=3, n_layers=3, lambda_feat=10.0):
    """reference :149-160 + compute_loss_D (:168-179) + GAN_and_FM_loss (:199-213) on torch-sliced crops, netD_f with one scale"""
    from oracle import vid2vid_oracle as O
    ys, ye, xs, xe = win
    A, B, F_ = real_A[:, :, ys:ye, xs:xe], real_B[:, :, ys:ye, xs:xe], fake_B[:, :, ys:ye, xs:xe]
    msd = lambda x: O.multiscale_discriminator(sdf, x, n_layers, 1)
    pred_real = msd(torch.cat([A, B], 1))
    pred_fake = msd(torch.cat([A, F_.detach()], 1))
    D_real, D_fake = O.gan_loss(pred_real, True), O.gan_loss(pred_fake, False)
    pred_fake = msd(torch.cat([A, F_], 1))
    G_gan = O.gan_loss(pred_fake, True)
    fm = 0
    for i in range(min(len(pred_fake), num_D_opt)):
        for j in range(len(pred_fake[i]) - 1):
            fm = fm + (1.0 / num_D_opt) * (4.0 / (n_layers + 1)) * torch.nn.functional.l1_loss(pred_fake[i][j], pred_real[i][j].detach()) * lambda_feat
    return {"G_f_GAN": G_gan * 2, "G_f_GAN_Feat": fm * 2, "D_f_real": D_real, "D_f_fake": D_fake}


@pytest.mark.gpu
def test_face_disc_pose2body_512p_geometry_vs_oracle():
    """512-row frames, fineSize 512 (a 128x128 crop), num_D 3 (netD_f: one scale), ndf 64, a face blob in the input."""
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    torch.manual_seed(0)
    H, W, N = 512, 256, 2
    opt = make_opt(isTrain=True, label_nc=0, input_nc=6, add_face_disc=True, num_D=3, ndf=64, no_vgg=True, loadSize=512,
                   fineSize=512, n_scales_temporal=1, precision="fp32", gpu_ids=[0], random_init_ok=True)
    D = Vid2VidModelD(); D.initialize(opt)
    gen = torch.Generator().manual_seed(21)
    real_A = torch.rand(N, 6, H, W, generator=gen) * 1.6 - 0.8
    real_A[0, 2, 60:90, 200:230] = 0.95                                  # face near the right border: the clamp applies in x
    real_A[1, 2, 70:95, 205:240] = 0.95
    t = {k: torch.tanh(torch.randn(N, 3, H, W, generator=gen)) for k in ("real_B", "fake_B", "fake_B_raw", "real_B_prev", "fake_B_prev")}
    t.update(real_A=real_A, flow=torch.randn(N, 2, H, W, generator=gen), weight=torch.rand(N, 1, H, W, generator=gen),
             flow_ref=torch.randn(N, 2, H, W, generator=gen), conf_ref=(torch.rand(N, 1, H, W, generator=gen) > 0.3).float())
    win = face_region_torch(real_A, 512)
    assert win[3] - win[2] == 128 and win[3] == W - 1 and D.get_face_region(real_A.to(DEV)) == win
    td = {k: v.to(DEV) for k, v in t.items()}
    td["fake_B"].requires_grad_(True)
    losses = dict(zip(D.loss_names, D(0, [td[k] for k in ORDER])))
    sdf = {k: v.detach().cpu().clone() for k, v in D.netD_f.state_dict().items()}
    params = {n for n, _ in D.netD_f.named_parameters()}
    for k in params:
        sdf[k].requires_grad_(True)
    fB = t["fake_B"].clone().requires_grad_(True)
    ref = _oracle_face(sdf, t["real_A"], t["real_B"], fB, win)
    for k in FACE_LOSSES:
        got, want = float(losses[k].detach()), float(ref[k].detach())
        assert abs(got - want) <= 1e-3 * abs(want), (k, got, want)
    D.optimizer_D.zero_grad()
    ((losses["D_f_fake"] + losses["D_f_real"]) * 0.5).backward(retain_graph=True)
    ((ref["D_f_fake"] + ref["D_f_real"]) * 0.5).backward(retain_graph=True)
    # gradients at this size: the gates of the project's other full-size gradient checks (tests/test_gpu_golden.py, training
    # chunk vs oracle): relative norm error <= 2.5e-3 and relative L2 error <= 5e-3 per tensor.  (The per-element metric of
    # tests/util.py is printed: fp32 sums over 8192 output positions per weight put single elements at a few 1e-3.)
    scale = torch.cat([sdf[n].grad.flatten() for n in params]).pow(2).mean().sqrt().item()
    checked = 0
    for n, p in D.netD_f.named_parameters():
        rv = sdf[n].grad
        if rv.pow(2).mean().sqrt().item() < 1e-3 * scale:                # biases in front of a norm: rounding noise only
            continue
        _gate(p.grad.contiguous(), rv, "grad D_f " + n)
        checked += 1
    assert checked >= 5
    (g_face,) = torch.autograd.grad(losses["G_f_GAN"] + losses["G_f_GAN_Feat"], td["fake_B"])
    (r_face,) = torch.autograd.grad(ref["G_f_GAN"] + ref["G_f_GAN_Feat"], fB)
    _gate(g_face, r_face, "face d fake_B")
    ys, ye, xs, xe = win
    outside = g_face.clone()
    outside[:, :, ys:ye, xs:xe] = 0
    assert not outside.any()


def _gate(got, ref, what):
    from util import rel_err
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    rn = ref.norm().item()
    e_norm = abs(got.norm().item() - rn) / rn
    e_l2 = (got - ref).norm().item() / rn
    print("%s: norm %.2e, L2 %.2e, per-element %.2e" % (what, e_norm, e_l2, rel_err(got, ref)))
    assert e_norm <= 2.5e-3 and e_l2 <= 5e-3, (what, e_norm, e_l2)


@pytest.mark.gpu
def test_face_block_makes_no_host_sync():
    D = _golden_model("mid")
    t = {k: v.to(DEV) for k, v in make_inputs("mid").items()}
    t["fake_B"].requires_grad_(True)
    D(0, [t[k] for k in ORDER])                                          # warm-up: tile searches, scratch allocation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        face = D._face_losses(t["real_A"], t["real_B"], t["fake_B"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(face) == 4
    torch.cuda.set_sync_debug_mode("error")                             # the check does see a host read (positive control)
    try:
        with pytest.raises(RuntimeError):
            D.get_face_region(t["real_A"])
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.gpu
def test_pose2body_style_training_chunk_end_to_end(tmp_path):
    """create_model + train.py's order of calls (:55-93, :130-138) for one chunk of a scaled-down pose2body_512p flag set."""
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    from vid2vid_amd.models.models import create_optimizer
    torch.manual_seed(0)
    H, W = 128, 64
    opt = make_opt(isTrain=True, label_nc=0, input_nc=6, n_scales_spatial=2, num_D=3, add_face_disc=True, no_first_img=True,
                   loadSize=128, fineSize=128, ngf=8, ndf=8, n_blocks=2, n_blocks_local=1, n_downsample_G=2, no_vgg=True,
                   n_frames_total=4, max_frames_per_gpu=2, n_scales_temporal=1, niter_fix_global=0, precision="fp32",
                   gpu_ids=[0], random_init_ok=True, checkpoints_dir=str(tmp_path), name="pose2body")
    modelG, modelD, flowNet, optimizer_G, optimizer_D, optimizer_D_T = create_optimizer(opt, create_model(opt))
    mD = modelD.module
    assert len(mD.loss_names) == 13
    n_load = modelG.module.n_frames_load
    T = n_load + opt.n_frames_G - 1
    gen = torch.Generator().manual_seed(5)
    A = torch.rand(1, T, 6, H, W, generator=gen) * 1.6 - 0.8
    A[0, :, 2, 30:50, 20:40] = 0.95
    B = torch.tanh(torch.randn(1, T, 3, H, W, generator=gen))
    A, B = A.to(DEV), B.to(DEV)

    def reshape(ts):
        return [None if t is None else t.contiguous().view(-1, t.size(2), t.size(3), t.size(4)) for t in ts]

    fake_B, fake_B_raw, flow, weight, real_A, real_Bp, fake_B_last = modelG(A, B, None, None)
    real_B_prev, real_B = real_Bp[:, :-1], real_Bp[:, 1:]
    flow_ref, conf_ref = flowNet(real_B, real_B_prev)
    fake_B_prev = modelG.module.compute_fake_B_prev(real_B_prev, None, fake_B)
    losses = modelD(0, reshape([real_B, fake_B, fake_B_raw, real_A, real_B_prev, fake_B_prev, flow, weight, flow_ref, conf_ref]))
    losses = [torch.mean(x) for x in losses]
    loss_dict = dict(zip(mD.loss_names, losses))
    frames_all, skipped = mD.get_all_skipped_frames((None,) * 4, real_B, fake_B, flow_ref, conf_ref, 1, opt.n_frames_D,
                                                    n_load, 0, flowNet)
    loss_dict_T = []
    if skipped[0][0] is not None:
        lt = modelD(1, [f[0] for f in skipped])
        loss_dict_T.append(dict(zip(mD.loss_names_T, [torch.mean(x) for x in lt])))
    loss_G, loss_D, loss_D_T, t_act = mD.get_losses(loss_dict, loss_dict_T, 1)
    vals = [float(v.detach()) for v in losses]
    assert len(vals) == 13 and all(np.isfinite(vals)) and all(float(loss_dict[k].detach()) > 0 for k in FACE_LOSSES)
    assert mD.get_face_region(real_A[0, -1:] if real_A.dim() == 5 else real_A[-1:])[0] is not None     # util.save_all_tensors
    before = [p.detach().clone() for p in mD.netD_f.parameters()]
    optimizer_G.zero_grad(); loss_G.backward(); optimizer_G.step()
    optimizer_D.zero_grad(); loss_D.backward(); optimizer_D.step()
    for s in range(t_act):
        optimizer_D_T[s].zero_grad(); loss_D_T[s].backward(); optimizer_D_T[s].step()
    torch.cuda.synchronize()
    assert any((p.detach() - b).abs().max().item() > 0 for p, b in zip(mD.netD_f.parameters(), before))
    mD.save("latest")
    path = os.path.join(str(tmp_path), "pose2body", "latest_net_D_f.pth")
    saved = torch.load(path)
    for k, v in mD.netD_f.state_dict().items():
        assert torch.equal(saved[k], v.detach().cpu()), k
