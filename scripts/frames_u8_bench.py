#!/usr/bin/env python3
"""uint8 frames from the frame plan (opt.frames_u8) against converting after the call.

bench.py's flagship configuration (label2city 512x256, one spatial scale, --fg, ngf 128, bf16, random-init weights seeded as
there, flow head scaled to a few pixels) on its seeded synthetic inputs, stream b drawn with seed 1234 + b.  Three cases:
`b1` (one stream), `b4` (four streams, plain plan) and `pool_2of4` (opt.compact_streams, slots 0 and 1 of 4 live).  Per case two
arms, timed as milliseconds per `inference()` call of a running sequence until uint8 HWC images exist on the device:

    u8        opt.frames_u8 on: the call returns the images, written by the last launch of the frame plan
    baseline  opt.frames_u8 off, then visual.tensor2im on every live stream's row of the returned fake_B (the code path that
              existed before the option; for `pool_2of4` the two idle slots are NOT converted, which favours the baseline)

`rounds` rounds, the arms (and the cases) alternating inside a round so that clock drift hits them alike; `calls` calls per
sample between two device events; per arm the median over the rounds with min and max, and all samples.  The whole-frame tile
search is off (opt.frame_tune = 0) so that both arms of a case replay the same convolution tiles.

    python scripts/frames_u8_bench.py [--rounds 9] [--calls 40] [--json profiles/frames_u8_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o frames_u8 -- python scripts/frames_u8_bench.py --trace
    python scripts/rocprof_by_grid.py <dir>/.../frames_u8_results.db frames_u8 tensor2im

--trace: a short run (1 round, 10 calls per sample) for a kernel tracer: the in-graph duration of the image launch per grid
(grid y = images of the launch), to set against its traffic of 15 H W bytes per image.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"b1": (1, False, [0]), "b4": (4, False, [0, 1, 2, 3]), "pool_2of4": (4, True, [0, 1])}    # streams, compact, live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--cases", default="b1,b4,pool_2of4")
    ap.add_argument("--json", default="")
    ap.add_argument("--trace", action="store_true", help="1 round of 10 calls per sample: for a run under a kernel tracer")
    args = ap.parse_args()
    if args.trace:
        args.rounds, args.calls = 1, 10
    import torch
    from vid2vid_amd import synthetic, visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model

    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    cases = [c for c in args.cases.split(",") if c]
    opt = make_opt(label_nc=35, use_instance=True, fg=True, use_real_img=True, random_init_ok=True, loadSize=W,
                   precision=args.precision, gpu_ids=[0], n_scales_spatial=1, ngf=args.ngf)
    opt.frame_tune = 0
    torch.manual_seed(0)
    model = create_model(opt)
    with torch.no_grad():
        model.netG0.model_final_flow[1].weight.mul_(0.1)
    tG = opt.n_frames_G
    seqs = [synthetic.label2city_sequence(tG + 2, H, W, seed=1234 + b, device=dev) for b in range(4)]

    def inputs(B, t):
        A = torch.stack([s[0][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W)
        I = torch.stack([s[1][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W)
        return A, (torch.cat([s[2][:, :tG - 1] for s in seqs[:B]]) if t == 0 else None), I

    def call(arm, live, A, F0, I, kw):
        """One inference() call of the arm; returns the images of the live streams as the arm delivers them."""
        if arm == "u8":
            return model.inference(A, F0, I, **kw)[0]
        fake = model.inference(A, F0, I, **kw)[0]
        return [visual.tensor2im(fake[b]) for b in live]

    def time_calls(case, arm, n, check=False):
        B, compact, live = CASES[case]
        kw = dict(active=live) if compact else {}
        opt.compact_streams, opt.frames_u8 = compact, arm == "u8"
        try:
            model.fake_B_prev = None
            call(arm, live, *inputs(B, 0), kw)
            A1, _, I1 = inputs(B, 1)
            for _ in range(3):
                images = call(arm, live, A1, None, I1, kw)
            fp = model._active_plan
            assert fp.frames_u8 == (arm == "u8") and (fp.pool is not None) == compact and fp.B == len(live)
            if check:           # the two arms deliver the same bytes (same windows, same inputs: 5th call of the sequence)
                return images if arm == "baseline" else [images[b] for b in live], (None if arm == "baseline" else images)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                call(arm, live, A1, None, I1, kw)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        finally:
            opt.compact_streams = opt.frames_u8 = False

    arms = ["u8", "baseline"]
    for case in cases:                                  # build every plan outside the timed rounds, and compare the arms' bytes
        got, whole = time_calls(case, "u8", 0, check=True)
        want, _ = time_calls(case, "baseline", 0, check=True)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), case
        idle = [b for b in range(CASES[case][0]) if b not in CASES[case][2]]
        assert whole.dtype == torch.uint8 and tuple(whole.shape) == (CASES[case][0], H, W, 3) and not whole[idle].any()
    torch.cuda.synchronize(dev)
    samples = {c: {a: [] for a in arms} for c in cases}
    for r in range(args.rounds):
        for case in (cases if r % 2 == 0 else cases[::-1]):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                samples[case][arm].append(time_calls(case, arm, args.calls))
    table = {}
    print("%10s %10s %12s %10s %10s" % ("case", "arm", "ms (median)", "min", "max"))
    for case in cases:
        table[case] = {}
        for arm in arms:
            v = sorted(samples[case][arm])
            table[case][arm] = dict(ms=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                                    samples=[round(x, 4) for x in samples[case][arm]])
            print("%10s %10s %12.3f %10.3f %10.3f" % (case, arm, v[len(v) // 2], v[0], v[-1]))
        u, b = table[case]["u8"], table[case]["baseline"]
        table[case]["u8_minus_baseline_ms"] = round(u["ms"] - b["ms"], 4)
        table[case]["ranges_overlap"] = bool(u["ms_max"] >= b["ms_min"] and b["ms_max"] >= u["ms_min"])
        table[case]["image_launch_bytes"] = 15 * H * W * len(CASES[case][2]) + 3 * H * W * (CASES[case][0] - len(CASES[case][2]))
    out = dict(config="label2city %dx%d S=1 --fg ngf %d %s, frame_tune off" % (W, H, args.ngf, args.precision), rounds=args.rounds,
               calls_per_sample=args.calls, device=torch.cuda.get_device_name(0),
               unit="ms per inference() call until uint8 images of the live streams exist on the device", table=table)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
