"""Inputs and CPU references shared by tests/test_cpu_flow_bwd_oracles.py and tests/test_gpu_flow_bwd.py."""
import torch

from oracle import vid2vid_oracle as O

FLOWNETC = (20, 1, 20, 1, 2)          # pad_size, kernel_size, max_displacement, stride1, stride2 (FlowNetC.py:31)

# (N, C, H, W, pad, k, max_disp, stride1, stride2)
CORR_CASES = [
    (1, 256, 12, 20) + FLOWNETC,      # FlowNetC's parameter set and channel count: the LDS tile kernel, 4 channel groups
    (1, 256, 13, 23) + FLOWNETC,      # ragged
    (1, 256, 32, 64) + FLOWNETC,      # the maps of a 512x256 frame: every displacement row in range somewhere, two pixel tiles
    (2, 70, 9, 40, 4, 1, 4, 1, 2),    # the same geometry class with 5 x 5 displacements, two pixel tiles, a ragged channel group
    (2, 5, 17, 23, 4, 3, 4, 2, 1),    # kernel_size 3, stride1 2
    (1, 3, 11, 14, 3, 1, 4, 1, 2),    # pad != max_displacement (smaller output)
    (2, 4, 10, 13, 6, 3, 4, 1, 2),    # pad > max_displacement: in1 is sampled in the padding too
]


def away_from_integers(n, h, w, seed, spread=3):
    """Flow whose sample positions x + fx, y + fy keep a fractional part in [0.05, 0.95] (>= 1e-3 from every integer, where the
    reference's d/dflow jumps), with integer parts that also leave the image on every side (the clamps bind)."""
    g = torch.Generator().manual_seed(seed)
    whole = torch.randint(-spread, spread + 1, (n, 2, h, w), generator=g).float()
    frac = 0.05 + 0.9 * torch.rand(n, 2, h, w, generator=g)
    flow = whole + frac
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    for pos in (xs[None] + flow[:, 0], ys[None] + flow[:, 1]):
        assert float((pos - pos.round()).abs().min()) >= 1e-3
    return flow


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def autograd_correlation(a, b, go, params):
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = O.correlation(a, b, *params)
    assert out.shape == go.shape, (out.shape, go.shape)
    return torch.autograd.grad((out * go).sum(), [a, b])


def autograd_resample2d(img, flow, go, kernel_size=1):
    img, flow = img.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    return torch.autograd.grad((O.resample2d(img, flow, kernel_size) * go).sum(), [img, flow])


def autograd_channelnorm(x, go):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad((O.channelnorm(x) * go).sum(), [x])[0]
