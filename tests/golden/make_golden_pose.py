#!/usr/bin/env python3
"""Golden fixture of the face discriminator (--add_face_disc, the pose2body recipes) made by executing the REFERENCE's
Vid2VidModelD on CPU (build container only; the GPU box reads the committed .npz):

    python tests/golden/make_golden_pose.py      # writes tests/golden/face_disc_pose_64x128.npz

Flags --dataset_mode pose --label_nc 0 --input_nc 6 --add_face_disc --num_D 3 --ndf 8 --no_vgg, two frames of 64x128,
fineSize 128 (a 32x32 face crop).  Five cases of the face mask: mid-frame, touching a border (the clamp applies), a box
that is the union of two frames, no face, and --openpose_only.  Each case records get_face_region, the 13 losses of
forward(0, ...), netD_f's parameter gradients of loss_D and d loss_G / d fake_B (and of the two face G terms alone).
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims, save                                      # noqa: E402
from face_disc_common import CASES, FINE, ORDER, fill_weights, make_inputs       # noqa: E402

# netD_f's loss_D gradients are stored for these cases (the no-face case must give exact zeros; the union case is checked
# through its window, losses and fake_B gradient) -- all four would not fit the 1 MiB limit of a committed file
GRAD_CASES = ("mid", "border", "openpose")


def main():
    install_shims()
    from options.train_options import TrainOptions
    from models.vid2vid_model_D import Vid2VidModelD
    arrays = {}
    for case in CASES:
        ck = tempfile.mkdtemp()
        sys.argv = ["train.py", "--name", "pose", "--dataset_mode", "pose", "--label_nc", "0", "--input_nc", "6",
                    "--add_face_disc", "--num_D", "3", "--ndf", "8", "--no_vgg", "--gpu_ids", "-1", "--checkpoints_dir", ck,
                    "--loadSize", str(FINE), "--fineSize", str(FINE)]
        if case == "openpose":
            sys.argv.append("--openpose_only")
        opt = TrainOptions().parse(save=False)
        opt.gpu_ids = [-1]
        opt.n_gpus_gen = 1
        torch.manual_seed(80)
        D = Vid2VidModelD(); D.initialize(opt)
        fill_weights(D.netD, 100)           # closed-form weights (face_disc_common): nothing of them is stored
        fill_weights(D.netD_f, 200)
        assert len(D.loss_names) == 13, D.loss_names
        arrays["loss_names"] = np.array(D.loss_names)
        t = make_inputs(case)
        t["fake_B"].requires_grad_(True)
        region = D.get_face_region(t["real_A"])
        arrays["%s.region" % case] = np.array([-1 if v is None else v for v in region], dtype=np.int64)
        losses = D(0, [t[k] for k in ORDER])
        losses = [torch.mean(x) for x in losses]
        ld = dict(zip(D.loss_names, losses))
        loss_G, loss_D, _, _ = D.get_losses(ld, [], 0)
        for k, v in ld.items():
            arrays["%s.loss.%s" % (case, k)] = np.array(float(v))
        arrays["%s.loss.total_G" % case] = np.array(float(loss_G))
        arrays["%s.loss.total_D" % case] = np.array(float(loss_D))
        # netD_f's parameter gradients of loss_D
        for p in list(D.netD.parameters()) + list(D.netD_f.parameters()):
            p.grad = None
        loss_D.backward(retain_graph=True)
        if case in GRAD_CASES:
            for name, p in D.netD_f.named_parameters():
                arrays["%s.gradDf.%s" % (case, name)] = p.grad.detach().numpy().copy()
        else:
            arrays["%s.gradDf_absmax" % case] = np.array(max(float(p.grad.abs().max()) if p.grad is not None else 0.0
                                                            for p in D.netD_f.parameters()))
        # d loss_G / d fake_B, and the face path's share of it
        (g_all,) = torch.autograd.grad(loss_G, t["fake_B"], retain_graph=True)
        if case == "mid":
            arrays["%s.dfake_B" % case] = g_all.numpy()
        face_G = ld["G_f_GAN"] + ld["G_f_GAN_Feat"]
        if face_G.requires_grad:
            (g_face,) = torch.autograd.grad(face_G, t["fake_B"], allow_unused=True)
            g_face = torch.zeros_like(t["fake_B"]) if g_face is None else g_face
        else:
            g_face = torch.zeros_like(t["fake_B"])
        if region[0] is not None:           # zero outside the window: only the window is stored
            ys, ye, xs, xe = region
            outside = g_face.clone()
            outside[:, :, ys:ye, xs:xe] = 0
            assert not outside.any()
            arrays["%s.dfake_B_face_win" % case] = g_face[:, :, ys:ye, xs:xe].numpy().copy()
        else:
            arrays["%s.dfake_B_face_absmax" % case] = np.array(float(g_face.abs().max()))
        print(case, region, {k: round(float(v), 5) for k, v in ld.items()})
    save("face_disc_pose_64x128", **arrays)


if __name__ == "__main__":
    main()
