#!/usr/bin/env python3
"""uint8 image inputs in the stream pool (opt.inputs_u8_slots) against the fp32 window path of the same tree, end to
end from pinned host memory.

One pose2body-shaped model (label_nc = 0, input_nc = 6, DensePose part-index table on channel 2) at 512x256, random-init weights
(seeded; flow head scaled to a few pixels), one spatial scale, under opt.compact_streams with S = 4 pooled slots.  Per active
count K in {1, 4} two arms, timed as wall-clock milliseconds per `inference()` call of running sequences, a device
synchronisation closing each window of `calls` calls (after `warmup` calls):

    fp32   input_A fp32 planes (S, tG, C, H, W) in pinned host memory: the call uploads tG C H W 4 bytes per active stream
    u8     opt.inputs_u8 + opt.inputs_u8_slots, input_A uint8 (S, 1, H, W, C) in pinned host memory: C H W bytes per active stream

The arms alternate window by window (the order flips every round), both run the same convolution tiles (opt.frame_tune = 0), and
the record holds every window, the median and the spread per arm, the bytes staged per call and the launch count of each plan.
The parent commit cannot run the u8 arm; its fp32 path is compared through bench.py.

    python scripts/inputs_u8_slots_bench.py [--rounds 6] [--calls 40] [--warmup 5] [--json profiles/inputs_u8_slots_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C_, PART, S = 256, 512, 6, 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--active", default="1,4")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five windows per arm")
    import torch
    from vid2vid_amd import visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model

    dev = torch.device("cuda", 0)
    opt = make_opt(label_nc=0, input_nc=C_, use_instance=False, fg=False, use_real_img=True, random_init_ok=True, loadSize=W,
                   precision=args.precision, gpu_ids=[0], n_scales_spatial=1, ngf=args.ngf, dataroot="datasets/pose/",
                   compact_streams=True)
    opt.frame_tune = 0
    torch.manual_seed(0)
    model = create_model(opt)
    with torch.no_grad():
        model.netG0.model_final_flow[1].weight.mul_(0.1)
    model.engine.refresh_weights()
    tG = opt.n_frames_G
    g = torch.Generator().manual_seed(1234)
    n_frames = tG + 7
    clip = torch.randint(0, 256, (S, n_frames, H, W, C_), generator=g, dtype=torch.uint8)
    first = torch.tanh(torch.randn(S, tG - 1, 3, H, W, generator=g))
    lut = visual.input_lut(C_, densepose_part_channel=PART)
    opt.input_lut = lut.to(dev)
    planes = visual.decode_inputs(clip, lut)
    steps = n_frames - tG + 1
    feeds = {"fp32": [planes[:, t:t + tG].contiguous().pin_memory() for t in range(steps)],
             "u8": [clip[:, t + tG - 1:t + tG].contiguous().pin_memory() for t in range(steps)]}
    result = dict(precision=args.precision, calls=args.calls, warmup=args.warmup, rounds=args.rounds, H=H, W=W, channels=C_, tG=tG,
                  slots=S, active={})

    def start(arm, active):
        model.fake_B_prev = None
        opt.inputs_u8 = opt.inputs_u8_slots = arm == "u8"
        A0 = clip[:, :tG].contiguous() if arm == "u8" else feeds["fp32"][0]
        model.inference(A0, first, None, active=active)

    def window(arm, active, n):
        feed = feeds[arm]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n):
            model.inference(feed[(i + 1) % len(feed)], None, None, active=active)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n

    arms = ["fp32", "u8"]
    for K in [int(k) for k in args.active.split(",") if k]:
        active = list(range(K))
        samples, launches = {a: [] for a in arms}, {}
        for r in range(args.rounds):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                start(arm, active)
                fp = model._active_plan
                assert fp.pool is not None and fp.B == K and (fp.win_u8 is not None) == (arm == "u8")
                launches[arm] = fp.plan.num_ops
                window(arm, active, args.warmup)
                samples[arm].append(window(arm, active, args.calls))
        case = dict(bytes_per_call=dict(fp32=K * tG * C_ * H * W * 4, u8=K * C_ * H * W), plan_ops=launches, ms_per_call={})
        for arm in arms:
            s = sorted(samples[arm])
            case["ms_per_call"][arm] = dict(median=s[len(s) // 2], min=s[0], max=s[-1], windows=samples[arm])
            print("K=%d of %d  %-5s %.3f ms/call [%.3f ... %.3f]  (%d plan ops, %.2f MB staged per call)"
                  % (K, S, arm, s[len(s) // 2], s[0], s[-1], launches[arm], case["bytes_per_call"][arm] / 1e6))
        result["active"][str(K)] = case
    opt.inputs_u8 = opt.inputs_u8_slots = False
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: {a: round(v["ms_per_call"][a]["median"], 4) for a in arms} for k, v in result["active"].items()}))


if __name__ == "__main__":
    main()
