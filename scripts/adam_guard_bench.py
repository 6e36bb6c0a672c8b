"""Cost of the gradient guard in front of the Adam step.

Six arms over flat fp32 buffers of the 512x256 generator's parameter count (scripts/adam_ema_bench.py's), alternating inside
every round of one process:

    a  adam_dev         v2v_adam_step_dev                                      (4 words read + 3 written per element)
    b  guard_skip       v2v_adam_step_dev_guard, skip_nonfinite only           (1 read, then 4 + 3)
    c  guard_clip_skip  v2v_adam_step_dev_guard, max_norm and skip_nonfinite   (1 read, then 4 + 3)
    d  guard_ema        v2v_adam_step_dev_guard_ema, max_norm and skip         (1 read, then 5 + 4)
    e  torch_clip       torch.nn.utils.clip_grad_norm_ on the parameter list (views of the flat buffers, the generator's own
                        tensor sizes), then (a)
    f  sumsq            v2v_grad_sumsq alone                                   (1 read)

Each sample is `--iters` back-to-back calls between two device events; per arm the median and min-max over `--rounds` samples
are reported in microseconds per call.  The gradient's norm is far above max_norm, so (c), (d) and (e) do clip.  Writes one
JSON document (default profiles/adam_guard_bench.json) and prints it.

    python scripts/adam_guard_bench.py [--rounds 9] [--iters 30] [--out profiles/adam_guard_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def generator_sizes():
    """(numel, 64-float aligned length) of every trainable tensor of optimizer_G for bench.py's training geometry (label2city
    512x256, ngf 128, one scale, --fg --use_instance), in FlatBuffers' order.  Built on the CPU."""
    from vid2vid_amd import networks as N
    from vid2vid_amd.options import make_opt
    opt = make_opt(isTrain=True, label_nc=35, use_instance=True, fg=True, loadSize=512, n_scales_spatial=1)
    in_nc = opt.label_nc * opt.n_frames_G + opt.n_frames_G
    net = N.define_G(in_nc, opt.output_nc, (opt.n_frames_G - 1) * opt.output_nc, opt.ngf, opt.netG, opt.n_downsample_G,
                     opt.norm, 0, [], opt)
    return [(p.numel(), (p.numel() + 63) // 64 * 64) for p in net.parameters() if p.requires_grad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_guard_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_guard_bench: needs the MI355X (a CPU run measures nothing)")
    from vid2vid_amd.lib import lib, check
    sizes = generator_sizes()
    n = sum(a for _, a in sizes)
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, m, v = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
    m.mul_(0.1); v.mul_(v).mul_(0.01)
    ema = p.clone()
    params, o = [], 0
    for numel, aligned in sizes:                           # what a user hands to clip_grad_norm_: one tensor per parameter
        q = torch.nn.Parameter(p[o:o + numel], requires_grad=True)
        q.grad = g[o:o + numel]
        params.append(q)
        o += aligned
    ptr = lambda t: C.c_void_p(t.data_ptr())
    hyper = (0.5, 0.999, 1e-8, 0.0, 1.0)
    decay, max_norm = 0.999, 1.0
    state = torch.zeros(2, dtype=torch.int32)
    state[1:2].view(torch.float32)[0] = 2e-4
    state = state.to(dev)
    guard = torch.zeros(int(lib.v2v_adam_guard_workspace_bytes()) // 4, dtype=torch.int32, device=dev)
    g0 = g.clone()

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def adam_dev():
        check(lib.v2v_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), n, *hyper, ptr(state), stream()), "adam_step_dev")

    def guarded(max_norm_):
        check(lib.v2v_adam_step_dev_guard(ptr(p), ptr(g), ptr(m), ptr(v), n, *hyper, ptr(state), ptr(guard), max_norm_, 1,
                                          stream()), "adam_step_dev_guard")

    def guard_ema():
        check(lib.v2v_adam_step_dev_guard_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, *hyper, ptr(state), decay, ptr(guard),
                                              max_norm, 1, stream()), "adam_step_dev_guard_ema")

    def torch_clip():
        g.copy_(g0)                                        # clip_grad_norm_ rescales in place: every call sees the same gradient
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        adam_dev()

    def torch_clip_overhead():                             # the copy alone, subtracted from (e) below
        g.copy_(g0)

    def sumsq():
        check(lib.v2v_grad_sumsq(ptr(g), n, ptr(guard), stream()), "grad_sumsq")

    arms = {"adam_dev": adam_dev, "guard_skip": lambda: guarded(0.0), "guard_clip_skip": lambda: guarded(max_norm),
            "guard_ema": guard_ema, "torch_clip": torch_clip, "restore_copy": torch_clip_overhead, "sumsq": sumsq}
    samples = {k: [] for k in arms}
    for fn in arms.values():                               # warm-up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    assert torch.isfinite(p).all() and torch.isfinite(ema).all()
    out = {"numel": n, "tensors": len(params), "rounds": args.rounds, "iters_per_sample": args.iters, "max_norm": max_norm,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call (device events around iters calls)", "arms": {}}
    for name in arms:
        s = sorted(samples[name])
        out["arms"][name] = {"median_us": round(statistics.median(s), 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2)}
    a = {k: x["median_us"] for k, x in out["arms"].items()}
    out["torch_clip_minus_restore_copy_us"] = round(a["torch_clip"] - a["restore_copy"], 2)
    out["guard_skip_minus_adam_dev_us"] = round(a["guard_skip"] - a["adam_dev"], 2)
    out["guard_clip_skip_minus_adam_dev_us"] = round(a["guard_clip_skip"] - a["adam_dev"], 2)
    out["adam_dev_spread_us"] = round(out["arms"]["adam_dev"]["max_us"] - out["arms"]["adam_dev"]["min_us"], 2)
    out["sumsq_over_adam_dev"] = round(a["sumsq"] / a["adam_dev"], 4)
    out["sumsq_GBps_at_median"] = round(4 * n / (a["sumsq"] * 1e-6) / 1e9, 1)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
