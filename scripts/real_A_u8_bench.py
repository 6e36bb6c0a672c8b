#!/usr/bin/env python3
"""real_A as a uint8 picture from the frame plan (opt.real_A_u8) against the fp32 real_A_last.

bench.py's flagship configuration (label2city 512x256, one spatial scale, --fg, ngf 128, bf16, random-init weights seeded as
there, flow head scaled to a few pixels) on its seeded synthetic inputs as uint8 label maps + int32 instance ids, stream b drawn
with seed 1234 + b, opt.frames_u8 on in every arm.  Two cases: `b1` (one stream) and `pool_b4` (opt.compact_streams, four slots,
all live).  Per case three arms, timed as wall-clock milliseconds per `inference()` call of a running sequence, every sample
(`calls` calls) closed by a device synchronisation:

    off        opt.real_A_u8 off: the call returns the fp32 one-hot planes (label_nc + 1, H, W) per stream
    off_label  the same, then visual.tensor2label on every stream's planes: the picture the way a caller made it before
    on         opt.real_A_u8 on: the call returns the pictures, written by one launch of the frame plan from the label maps

`rounds` rounds, the arms (and the cases) alternating inside a round so that clock drift hits them alike; per arm the median over
the rounds with min and max, and all samples.  The whole-frame tile search is off (opt.frame_tune = 0) so that the arms of a case
replay the same convolution tiles.

    python scripts/real_A_u8_bench.py [--rounds 9] [--calls 40] [--json profiles/real_A_u8_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"b1": (1, False), "pool_b4": (4, True)}      # streams, compact
ARMS = ["off", "off_label", "on"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--cases", default="b1,pool_b4")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("at least 3 rounds")
    import torch
    from vid2vid_amd import synthetic, visual
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model

    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    cases = [c for c in args.cases.split(",") if c]
    opt = make_opt(label_nc=35, use_instance=True, fg=True, use_real_img=True, random_init_ok=True, loadSize=W,
                   precision=args.precision, gpu_ids=[0], n_scales_spatial=1, ngf=args.ngf, frames_u8=True)
    opt.frame_tune = 0
    torch.manual_seed(0)
    model = create_model(opt)
    with torch.no_grad():
        model.netG0.model_final_flow[1].weight.mul_(0.1)
    tG = opt.n_frames_G
    seqs = [synthetic.label2city_sequence(tG + 2, H, W, seed=1234 + b, device=dev) for b in range(4)]

    def inputs(B, t):
        A = torch.stack([s[0][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W).to(torch.uint8)
        I = torch.stack([s[1][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W).to(torch.int32)
        return A, (torch.cat([s[2][:, :tG - 1] for s in seqs[:B]]) if t == 0 else None), I

    def call(arm, B, A, F0, I):
        """One inference() call of the arm; returns (images, pictures or planes)."""
        image, second = model.inference(A, F0, I)
        if arm == "off_label":
            second = torch.stack([visual.tensor2label(p, opt.label_nc) for p in second.view(B, -1, H, W)])
        return image, second

    def time_calls(case, arm, n, check=False):
        B, compact = CASES[case]
        opt.compact_streams, opt.real_A_u8 = compact, arm == "on"
        try:
            model.fake_B_prev = None
            call(arm, B, *inputs(B, 0))
            A1, _, I1 = inputs(B, 1)
            for _ in range(3):
                out = call(arm, B, A1, None, I1)
            fp = model._active_plan
            assert fp.real_A_u8 == (arm == "on") and fp.frames_u8 and (fp.pool is not None) == compact and fp.B == B
            if check:           # the arms deliver the same bytes (same windows, same inputs: 5th call of the sequence)
                return out
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                call(arm, B, A1, None, I1)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / n
        finally:
            opt.compact_streams = opt.real_A_u8 = False

    for case in cases:                                  # build every plan outside the timed rounds, and compare the arms' bytes
        image_on, pic_on = time_calls(case, "on", 0, check=True)
        image_off, pic_off = time_calls(case, "off_label", 0, check=True)
        B = CASES[case][0]
        assert pic_on.dtype == torch.uint8 and tuple(pic_on.shape) == (B, H, W, 3) and pic_on.any()
        assert torch.equal(pic_on, pic_off) and torch.equal(image_on, image_off), case
        time_calls(case, "off", 0, check=True)
    torch.cuda.synchronize(dev)
    samples = {c: {a: [] for a in ARMS} for c in cases}
    for r in range(args.rounds):
        for case in (cases if r % 2 == 0 else cases[::-1]):
            for arm in (ARMS if r % 2 == 0 else ARMS[::-1]):
                samples[case][arm].append(time_calls(case, arm, args.calls))
    table = {}
    print("%10s %10s %12s %10s %10s" % ("case", "arm", "ms (median)", "min", "max"))
    for case in cases:
        table[case] = {}
        for arm in ARMS:
            v = sorted(samples[case][arm])
            table[case][arm] = dict(ms=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                                    samples=[round(x, 4) for x in samples[case][arm]])
            print("%10s %10s %12.3f %10.3f %10.3f" % (case, arm, v[len(v) // 2], v[0], v[-1]))
        on = table[case]["on"]
        for base in ("off", "off_label"):
            b = table[case][base]
            table[case]["on_minus_%s_ms" % base] = round(on["ms"] - b["ms"], 4)
            table[case]["ranges_overlap_%s" % base] = bool(on["ms_max"] >= b["ms_min"] and b["ms_max"] >= on["ms_min"])
        B = CASES[case][0]
        table[case]["bytes_written_for_the_second_result"] = dict(off=4 * (opt.label_nc + 1) * H * W * B, on=3 * H * W * B)
    out = dict(config="label2city %dx%d S=1 --fg ngf %d %s, uint8 labels, frames_u8 on, frame_tune off"
               % (W, H, args.ngf, args.precision), rounds=args.rounds, calls_per_sample=args.calls,
               device=torch.cuda.get_device_name(0),
               unit="wall-clock ms per inference() call, each sample of calls_per_sample calls closed by a device synchronisation",
               table=table)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
