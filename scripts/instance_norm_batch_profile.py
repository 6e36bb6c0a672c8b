#!/usr/bin/env python3
"""Workload for one kernel trace of the InstanceNorm2d path at batch > 1 (csrc/instance_norm.hip) next to the BatchNorm2d
group of the same shape: a ResnetBlock-shaped group, ReflectionPad2d(1) + Conv2d(512, 512, 3) + norm + ReLU + residual at
32x64, N = 4, bf16, inference (no_grad), `reps` times each, warm.  The BatchNorm group is the existing code (statistics in the
conv epilogue, finalize in the conv launch, bn_apply); the InstanceNorm group runs the conv without statistics, then
in_stats and in_apply.  Prints event timings per group and the bytes each norm kernel moves.

    rocprofv3 --kernel-trace --stats -d <dir> -o in_batch -- python scripts/instance_norm_batch_profile.py [--reps 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from vid2vid_amd import lib as L
from vid2vid_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("--height", type=int, default=32)
ap.add_argument("--width", type=int, default=64)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
dev = "cuda:0"
N, Cc, H, W = a.batch, a.channels, a.height, a.width

torch.manual_seed(0)
eng = Engine(dev, L.BF16)
conv = nn.Conv2d(Cc, Cc, 3).to(dev)
with torch.no_grad():
    conv.weight.normal_(0, 0.02)
norms = {"BatchNorm2d": nn.BatchNorm2d(Cc, affine=True).to(dev), "InstanceNorm2d": nn.InstanceNorm2d(Cc, affine=False).to(dev)}
x = torch.randn(N, Cc, H, W, device=dev)


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
    return e0.elapsed_time(e1) / reps * 1e3          # us per group, back to back


with torch.no_grad():
    xa = eng.pack(x)
    elems = N * H * W * Cc
    for name, norm in norms.items():
        n0 = len(eng.conv_log)
        run = lambda: eng.conv_group(xa, conv, L.PAD_REFLECT, 1, norm, L.ACT_RELU, 0.0, add0=xa, label=name)
        us = timed(run, a.reps)
        c = eng.conv_log[n0]
        print("%-15s N %d  %d -> %d 3x3 @ %dx%d bf16: %8.1f us per group [events, back to back]  conv tile %s split-K %d"
              % (name, N, Cc, Cc, H, W, us, c["tile"], c["splitk"]))
    print("raw tensor: %.2f MB fp32;  in_stats reads it once (%.2f MB);  bn_apply / in_apply read raw + residual and write y "
          "(%.2f MB)" % (elems * 4 / 1e6, elems * 4 / 1e6, elems * (4 + 2 + 2) / 1e6))
