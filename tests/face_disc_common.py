"""Shared by tests/golden/make_golden_pose.py and the face discriminator tests: the deterministic inputs and weights of the
face-disc fixture (closed-form, no RNG: the fixture stores only results, which keeps it under the size limit), and a torch
restatement of the reference's get_face_region (models/vid2vid_model_D.py:215-230)."""
import math

import torch

H, W, NF, FINE = 64, 128, 2, 128
CASES = ("mid", "border", "union", "none", "openpose")
ORDER = ("real_B", "fake_B", "fake_B_raw", "real_A", "real_B_prev", "fake_B_prev", "flow", "weight", "flow_ref", "conf_ref")
# face pixels per case: (frame, y0, y1, x0, x1)
BLOBS = {
    "mid": [(0, 20, 28, 50, 62), (1, 20, 28, 52, 64)],
    "border": [(0, 0, 4, 120, 128), (1, 1, 3, 124, 128)],
    "union": [(0, 10, 15, 10, 15), (1, 40, 51, 90, 101)],
    "none": [],
    "openpose": [(0, 20, 28, 50, 62), (1, 20, 28, 52, 64)],
}


def wave(shape, k):
    """A smooth-ish deterministic pattern in [-1, 1] (fp64 arithmetic, rounded to fp32)."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float64)
    return torch.sin(i * (0.37 + 0.011 * k) + 1.3 * k).mul(torch.cos(i * 0.0131 + 0.7 * k)).float().reshape(shape)


def set_face(real_A, frame, y0, y1, x0, x1, openpose):
    if openpose:
        real_A[frame, 0, y0:y1, x0:x1] = 0.2
        real_A[frame, 1, y0:y1, x0:x1] = -1.0
        real_A[frame, 2, y0:y1, x0:x1] = -0.6
    else:
        real_A[frame, 2, y0:y1, x0:x1] = 0.95


def make_inputs(case):
    """The ten tensors of Vid2VidModelD.forward(0, ...) for one case (planar fp32, NF frames of H x W)."""
    t = {"real_A": wave((NF, 6, H, W), 1) * 0.85}          # |value| <= 0.85: no face pixel outside the blobs in either mode
    for j, k in enumerate(("real_B", "fake_B", "fake_B_raw", "real_B_prev", "fake_B_prev")):
        t[k] = wave((NF, 3, H, W), 2 + j)
    t["flow"] = wave((NF, 2, H, W), 8) * 2.0
    t["weight"] = wave((NF, 1, H, W), 9) * 0.5 + 0.5
    t["flow_ref"] = wave((NF, 2, H, W), 10) * 2.0
    t["conf_ref"] = (wave((NF, 1, H, W), 11) > -0.4).float()
    for b in BLOBS[case]:
        set_face(t["real_A"], *b, openpose=case == "openpose")
    return t


def fill_weights(net, seed):
    """Closed-form weights of the reference's initialiser's scale (conv N(0, 0.02), norm weight N(1, 0.02), bias 0 plus a
    small pattern); buffers (running statistics) are left as they are."""
    with torch.no_grad():
        for i, (name, p) in enumerate(net.named_parameters()):
            w = wave(tuple(p.shape), seed + i)
            if name.endswith("bias"):
                p.copy_(w * 0.01)
            elif p.dim() == 1:
                p.copy_(1.0 + 0.02 * w)
            else:
                p.copy_(0.02 * math.sqrt(3.0) * w)


def face_region_torch(real_A, fine_size, openpose=False):
    """get_face_region of the reference restated in torch: (ys, ye, xs, xe) or four None."""
    _, _, h, w = real_A.shape
    a = real_A.float()
    if not openpose:
        mask = a[:, 2] > 0.9
    else:
        mask = (a[:, 0] > 0.19) & (a[:, 0] < 0.21) & (a[:, 1] < -0.99) & (a[:, 2] > -0.61) & (a[:, 2] < -0.59)
    face = mask.nonzero()
    if not face.size(0):
        return None, None, None, None
    y, x = face[:, 1], face[:, 2]
    return window_from_box(int(y.min()), int(y.max()), int(x.min()), int(x.max()), h, w, fine_size)


def window_from_box(ys, ye, xs, xe, h, w, fine_size):
    """reference :223-229, from the inclusive box of the face pixels"""
    yc, ylen = (ys + ye) // 2, fine_size // 32 * 8
    xc, xlen = (xs + xe) // 2, fine_size // 32 * 8
    yc = max(ylen // 2, min(h - 1 - ylen // 2, yc))
    xc = max(xlen // 2, min(w - 1 - xlen // 2, xc))
    return yc - ylen // 2, yc + ylen // 2, xc - xlen // 2, xc + xlen // 2
