"""Training chunks of a pose2body_512p geometry (512x256 frames, input_nc 6, num_D 3, ndf 64, fineSize 512 = a 128x128 face
crop) with or without --add_face_disc, in train.py's order of calls (:55-93, :130-138), for a kernel trace of what the
face discriminator adds:

    rocprofv3 --kernel-trace --stats -d <dir> -o face -- python scripts/face_disc_chunk.py --face
    rocprofv3 --kernel-trace --stats -d <dir> -o base -- python scripts/face_disc_chunk.py

Prints the device time per chunk (events around the last --chunks - 1 chunks; the first one builds the packings)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--face", action="store_true")
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=256)
    args = ap.parse_args()
    import tempfile
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    from vid2vid_amd.models.models import create_optimizer
    torch.manual_seed(0)
    H, W = args.height, args.width
    opt = make_opt(isTrain=True, label_nc=0, input_nc=6, n_scales_spatial=1, num_D=3, ndf=64, ngf=32, n_downsample_G=3,
                   add_face_disc=args.face, no_first_img=True, loadSize=H, fineSize=512, no_vgg=True, n_frames_total=4,
                   max_frames_per_gpu=2, n_scales_temporal=1, precision="bf16", gpu_ids=[0], random_init_ok=True,
                   checkpoints_dir=tempfile.mkdtemp(), name="face_prof")
    modelG, modelD, flowNet, optimizer_G, optimizer_D, optimizer_D_T = create_optimizer(opt, create_model(opt))
    mD = modelD.module
    n_load = modelG.module.n_frames_load
    T = n_load + opt.n_frames_G - 1
    gen = torch.Generator().manual_seed(5)
    A = torch.rand(1, T, 6, H, W, generator=gen) * 1.6 - 0.8
    A[0, :, 2, H // 8:H // 8 + 40, W // 2:W // 2 + 30] = 0.95            # a face blob
    B = torch.tanh(torch.randn(1, T, 3, H, W, generator=gen))
    A, B = A.cuda(), B.cuda()

    def reshape(ts):
        return [None if t is None else t.contiguous().view(-1, t.size(2), t.size(3), t.size(4)) for t in ts]

    def chunk():
        fake_B, fake_B_raw, flow, weight, real_A, real_Bp, _ = modelG(A, B, None, None)
        real_B_prev, real_B = real_Bp[:, :-1], real_Bp[:, 1:]
        flow_ref, conf_ref = flowNet(real_B, real_B_prev)
        fake_B_prev = modelG.module.compute_fake_B_prev(real_B_prev, None, fake_B)
        losses = modelD(0, reshape([real_B, fake_B, fake_B_raw, real_A, real_B_prev, fake_B_prev, flow, weight, flow_ref, conf_ref]))
        loss_dict = dict(zip(mD.loss_names, [torch.mean(x) for x in losses]))
        loss_G, loss_D, _, _ = mD.get_losses(loss_dict, [], 0)
        optimizer_G.zero_grad(); loss_G.backward(); optimizer_G.step()
        optimizer_D.zero_grad(); loss_D.backward(); optimizer_D.step()
        return loss_dict

    chunk()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.chunks - 1):
        ld = chunk()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / max(args.chunks - 1, 1)
    print("face_disc=%d %dx%d: %.2f ms per chunk (%d frames), %d losses, finite=%s" % (
        int(args.face), W, H, ms, n_load, len(ld), all(torch.isfinite(v).item() for v in ld.values())))


if __name__ == "__main__":
    main()
