#!/usr/bin/env python3
"""Workload for one kernel trace of the FlowNet2 native-op backward passes (csrc/flow_ops_bwd.hip): FlowNetC's correlation
(pad 20, kernel 1, max_disp 20, stride1 1, stride2 2, C = 256, N = 1) forward and backward on the feature maps of a 512x256
and a 1024x512 frame (32x64 and 64x128), then Resample2d / ChannelNorm backward on 3-channel images of those sizes; each
warm, `reps` launches.  Prints the algorithmic operations / bytes and the HBM-bound estimates next to event timings.

    rocprofv3 --kernel-trace --stats -d <dir> -o flow_bwd -- python scripts/flow_bwd_profile.py [--reps 20]
    python scripts/rocprof_by_grid.py <dir>/flow_bwd_results.db correlation resample2d channelnorm zero_f32
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vid2vid_amd.lib import lib, check

HBM_TBS = 6.3        # achievable HBM bandwidth of the MI355X, TB/s (8.0 spec)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
dev = "cuda:0"
P = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch, back to back


torch.manual_seed(0)
for (fh, fw) in ((256, 512), (512, 1024)):
    h, w, c = fh // 8, fw // 8, 256
    f1, f2 = torch.randn(1, c, h, w, device=dev), torch.randn(1, c, h, w, device=dev)
    out = torch.empty(1, 441, h, w, device=dev)
    go = torch.randn(1, 441, h, w, device=dev)
    g1, g2 = torch.empty_like(f1), torch.empty_like(f2)
    fwd = lambda: check(lib.v2v_correlation_forward(P(f1), P(f2), P(out), 1, c, h, w, 20, 1, 20, 1, 2, 1, stream()), "fwd")
    bwd = lambda: check(lib.v2v_correlation_backward(P(f1), P(f2), P(go), P(g1), P(g2), 1, c, h, w, 441, h, w, 20, 1, 20, 1, 2, 1,
                                                     stream()), "bwd")
    tf, tb = timed(fwd, a.reps), timed(bwd, a.reps)
    gflop = 2.0 * h * w * 441 * c / 1e9
    print("correlation %4dx%-4d (maps %dx%d, C %d): forward %.3f GFLOP %8.1f us | backward (both gradients) %.3f GFLOP %8.1f us | "
          "backward / forward = %.2f   [events, back to back]" % (fw, fh, h, w, c, gflop, tf, 2 * gflop, tb, tb / tf))
    # a smooth flow of a few pixels, as an optical flow is (white-noise flows scatter the 64 lanes of a wave over 64 rows: the slow
    # case of global float atomics, not the one a warp sees)
    yy, xx = torch.meshgrid(torch.arange(fh, device=dev, dtype=torch.float32), torch.arange(fw, device=dev, dtype=torch.float32), indexing="ij")
    flow = torch.stack([4.3 * torch.sin(xx / 97.0 + yy / 61.0), 3.1 * torch.cos(xx / 83.0 - yy / 45.0)])[None].contiguous()
    img = torch.randn(1, 3, fh, fw, device=dev)
    gout = torch.randn(1, 3, fh, fw, device=dev)
    gi, gf = torch.empty_like(img), torch.empty_like(flow)
    rs = lambda: check(lib.v2v_resample2d_backward(P(img), P(flow), P(gout), P(gi), P(gf), 1, 3, fh, fw, fh, fw, 1, stream()), "rs")
    x, nrm, gn = torch.randn(1, 3, fh, fw, device=dev), torch.rand(1, 1, fh, fw, device=dev) + 1, torch.randn(1, 1, fh, fw, device=dev)
    gx = torch.empty_like(x)
    cn = lambda: check(lib.v2v_channelnorm_backward(P(x), P(nrm), P(gn), P(gx), 1, 3, fh, fw, 2, stream()), "cn")
    trs, tcn = timed(rs, a.reps), timed(cn, a.reps)
    px = fh * fw
    # resample2d backward: flow (2) + grad_out (3) read, 4 image taps per channel (12, mostly cache hits: counted once = 3), grad_img
    # zeroed (3) and updated by 12 atomics (read-modify-write in L2: counted once = 3 written), grad_flow (2) written
    b_rs = px * 4 * (2 + 3 + 3 + 3 + 3 + 2)
    b_cn = px * 4 * (3 + 1 + 1 + 3)                      # x, out, grad_out read; grad_in written
    print("resample2d_backward  %4dx%-4d C 3: %6.2f MB -> HBM bound %5.1f us, measured %7.1f us (zero + scatter/gather launches)"
          % (fw, fh, b_rs / 1e6, b_rs / (HBM_TBS * 1e6), trs))
    print("channelnorm_backward %4dx%-4d C 3: %6.2f MB -> HBM bound %5.1f us, measured %7.1f us" % (fw, fh, b_cn / 1e6, b_cn / (HBM_TBS * 1e6), tcn))
