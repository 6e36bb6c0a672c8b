"""Cost of keeping the generator's weight average inside the Adam step.

Three arms over flat fp32 buffers of the 512x256 generator's parameter count, alternating inside every round of one process:

    adam        v2v_adam_step                                     (4 words read + 3 written per element)
    adam_ema    v2v_adam_step_ema                                 (5 read + 4 written)
    adam_lerp   v2v_adam_step, then torch.lerp_ on a flat shadow  (4 + 3, then 2 read + 1 written)

Each sample is `--iters` back-to-back calls between two device events; per arm the median and min-max over `--rounds` samples
are reported in microseconds per call, with the bytes the arm has to move and the bandwidth that implies.  Writes one JSON
document (default profiles/adam_ema_bench.json) and prints it.

    python scripts/adam_ema_bench.py [--rounds 9] [--iters 50] [--out profiles/adam_ema_bench.json]
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


def generator_numel():
    """Flat length of optimizer_G for bench.py's training geometry (label2city 512x256, ngf 128, one scale, --fg
    --use_instance): every trainable tensor rounded up to FlatBuffers' 64-float alignment.  Built on the CPU."""
    from vid2vid_amd import networks as N
    from vid2vid_amd.options import make_opt
    opt = make_opt(isTrain=True, label_nc=35, use_instance=True, fg=True, loadSize=512, n_scales_spatial=1)
    in_nc = opt.label_nc * opt.n_frames_G + opt.n_frames_G
    net = N.define_G(in_nc, opt.output_nc, (opt.n_frames_G - 1) * opt.output_nc, opt.ngf, opt.netG, opt.n_downsample_G,
                     opt.norm, 0, [], opt)
    return sum((p.numel() + 63) // 64 * 64 for p in net.parameters() if p.requires_grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--numel", type=int, default=0, help="0: the 512x256 generator's parameter count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_ema_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_ema_bench: needs the MI355X (a CPU run measures nothing)")
    from vid2vid_amd.lib import lib, check
    n = args.numel or generator_numel()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, m, v = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
    m.mul_(0.1); v.mul_(v).mul_(0.01)
    ema = p.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    hyper = (2e-4, 0.5, 0.999, 1e-8, 0.0, 1.0)
    decay = 0.999
    step = [0]

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def adam():
        step[0] += 1
        check(lib.v2v_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, *hyper, step[0], stream()), "adam_step")

    def adam_ema():
        step[0] += 1
        check(lib.v2v_adam_step_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, *hyper, step[0], decay, stream()), "adam_step_ema")

    def adam_lerp():
        adam()
        ema.lerp_(p, 1.0 - decay)

    arms = {"adam": (adam, 7), "adam_ema": (adam_ema, 9), "adam_lerp": (adam_lerp, 10)}
    samples = {k: [] for k in arms}
    for fn, _ in arms.values():                          # warm-up: code objects, allocator
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, _) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    assert torch.isfinite(p).all() and torch.isfinite(ema).all()
    out = {"numel": n, "rounds": args.rounds, "iters_per_sample": args.iters, "ema_decay": decay,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call (device events around iters calls)", "arms": {}}
    for name, (_, words) in arms.items():
        s = sorted(samples[name])
        med = statistics.median(s)
        out["arms"][name] = {"median_us": round(med, 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2),
                             "words_per_element": words, "bytes": 4 * words * n,
                             "GBps_at_median": round(4 * words * n / (med * 1e-6) / 1e9, 1)}
    a = out["arms"]
    out["ema_over_adam"] = round(a["adam_ema"]["median_us"] / a["adam"]["median_us"], 4)
    out["ema_over_lerp"] = round(a["adam_ema"]["median_us"] / a["adam_lerp"]["median_us"], 4)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
