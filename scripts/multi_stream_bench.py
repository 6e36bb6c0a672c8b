#!/usr/bin/env python3
"""Multi-stream inference: ms per frame-plan replay and aggregate frames/s for B sequences per plan.

bench.py's flagship configuration (label2city 512x256, one spatial scale, --fg, ngf 128, bf16, random-init weights seeded as
there, flow head scaled to a few pixels) and its seeded synthetic inputs, stream b drawn with seed 1234 + b.  For every B the
plan is built once (tile search included), the sequence is started, and the steady plan's graph is replayed: `rounds` rounds,
alternating over the B values inside a round so that clock and thermal drift hits all of them alike; per B the median over the
rounds of (ms per replay) is reported, with min and max.  aggregate frames/s = B / (ms per replay).

    python scripts/multi_stream_bench.py [--streams 1,2,4,8] [--rounds 7] [--replays 40] [--json profiles/multi_stream_bench.json]
    python scripts/multi_stream_bench.py --streams 4 --rounds 1 --trace     # a short run to put under a kernel tracer
    python scripts/multi_stream_bench.py --streams 4 --slots 8 [--json profiles/stream_slots_bench.json]

--slots K measures, per B > 1 and inside the same alternating rounds, four arms: the plain plan's graph replay
(`plain`), the slot plan's graph replay with every stream steady (`slots_steady`), and whole `inference()` calls -- input staging,
mode copy, replay, output clones -- on the plain plan (`plain_calls`) and on the slot plan under a rolling schedule that restarts
one slot every K frames, slot after slot (`slots_rolling`; the restart's first-frame work is inside the timed region).

    python scripts/multi_stream_bench.py --streams 1 --pool 4 [--json profiles/stream_pool_bench.json]

--pool S times whole `inference()` calls of a running server with S slots of which K = 1..S are active (slots
0..K-1; the others idle), inside the same alternating rounds: `pool` (opt.compact_streams: the K-row pool plan), `slots_idle`
(the S-row slot plan with the same S - K slots idle) and `dense` (a plain call with K streams: the K-row plan without a pool).
The pool plans are built ahead with prepare_streams.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--json", default="")
    ap.add_argument("--slots", type=int, default=0, help="K > 0: also time the slot plan; rolling schedule restarts one slot every K frames")
    ap.add_argument("--pool", type=int, default=0, help="S > 1: time inference() calls with K = 1..S of S slots active, compact vs slot plan vs dense")
    ap.add_argument("--trace", action="store_true", help="no per-op table, few replays: for a run under a kernel tracer")
    args = ap.parse_args()
    import torch
    from vid2vid_amd import synthetic
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model

    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    Bs = [int(v) for v in args.streams.split(",")]
    opt = make_opt(label_nc=35, use_instance=True, fg=True, use_real_img=True, random_init_ok=True, loadSize=W,
                   precision=args.precision, gpu_ids=[0], n_scales_spatial=1, ngf=args.ngf)
    torch.manual_seed(0)
    model = create_model(opt)
    with torch.no_grad():
        model.netG0.model_final_flow[1].weight.mul_(0.1)
    tG = opt.n_frames_G
    seqs = [synthetic.label2city_sequence(tG + 2, H, W, seed=1234 + b, device=dev) for b in range(max(Bs))]

    def inputs(B, t):
        A = torch.stack([s[0][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W)
        I = torch.stack([s[1][t:t + tG] for s in seqs[:B]]).view(B, tG, 1, H, W)
        F0 = torch.cat([s[2][:, :tG - 1] for s in seqs[:B]]) if t == 0 else None
        return A, F0, I

    plans = {}
    for B in Bs:                                   # build: first-frame plan is the steady plan here (use_real_img)
        model.fake_B_prev = None
        for t in range(2):
            fake, _ = model.inference(*inputs(B, t))
        assert tuple(fake.shape) == (B, 3, H, W) and bool(torch.isfinite(fake).all())
        plans[B] = model._active_plan
    torch.cuda.synchronize(dev)

    def time_plan(fp, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):
            fp.plan.launch()
        e0.record()
        for _ in range(n):
            fp.plan.launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    samples = {B: [] for B in Bs}
    for r in range(args.rounds):
        for B in (Bs if r % 2 == 0 else Bs[::-1]):
            samples[B].append(time_plan(plans[B], args.replays))
    rows = []
    for B in Bs:
        v = sorted(samples[B])
        med = v[len(v) // 2]
        fp = plans[B]
        names = [n for n, _, _ in fp.plan.profile()] if not args.trace else []
        rows.append(dict(streams=B, ms_per_replay=round(med, 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                         aggregate_frames_per_s=round(B / med * 1e3, 2), launches=fp.plan.num_ops,
                         in_finalize_rows=names.count("in_finalize_rows"), in_stats=names.count("in_stats"),
                         paired_convs=sum(1 for c in fp.conv_log if c.get("pair"))))
    base = next((r for r in rows if r["streams"] == 1), None)
    for r in rows:
        r["vs_single_stream"] = round(r["aggregate_frames_per_s"] / base["aggregate_frames_per_s"], 4) if base else None
    per_op = {}
    if not args.trace:
        for B in Bs:                               # where the time goes: per op kind, one eager timed pass of the plan
            acc = {}
            for name, label, ms in plans[B].plan.profile():
                acc[name] = acc.get(name, 0.0) + ms
            per_op[str(B)] = {k: round(v, 4) for k, v in sorted(acc.items(), key=lambda kv: -kv[1])}
    out = dict(config="label2city %dx%d S=1 --fg ngf %d %s" % (W, H, args.ngf, args.precision), rounds=args.rounds,
               replays_per_sample=args.replays, device=torch.cuda.get_device_name(0), table=rows, per_op_ms=per_op)
    print("%8s %14s %22s %10s" % ("streams", "ms / replay", "aggregate frames/s", "vs B=1"))
    for r in rows:
        print("%8d %14.3f %22.1f %10s" % (r["streams"], r["ms_per_replay"], r["aggregate_frames_per_s"], r["vs_single_stream"]))
    if args.slots > 0:
        out["slots"] = slots_arms(args, model, inputs, [B for B in Bs if B > 1], plans, time_plan, dev)
    if args.pool > 1:
        out["pool"] = pool_arms(args, model, args.pool, H, W, dev)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def slots_arms(args, model, inputs, Bs, plans, time_plan, dev):
    """The four arms of --slots for every B in Bs; returns {B: {arm: dict(ms, ms_min, ms_max, samples)}}."""
    import torch
    K = args.slots
    slot_plans = {}
    for B in Bs:
        model.fake_B_prev = None
        for t in range(2):
            fake, _ = model.inference(*inputs(B, t), active=list(range(B)))
        assert model._active_plan.slots and bool(torch.isfinite(fake).all())
        slot_plans[B] = model._active_plan
        names = [n for n, _, _ in slot_plans[B].plan.profile()]
        assert "warp_blend_slots" in names and "memcpy_d2d" not in names
    torch.cuda.synchronize(dev)
    first = {B: inputs(B, 0) for B in Bs}
    steady = {B: inputs(B, 1)[0::2] for B in Bs}

    def time_calls(B, rolling, n):
        """ms per inference() call over n calls of a running sequence; rolling: restart slot (i // K) % B every K-th call."""
        A0, F0, I0 = first[B]
        A1, I1 = steady[B]
        model.fake_B_prev = None
        kw = dict(active=list(range(B))) if rolling else {}
        model.inference(A0, F0, I0, **kw)
        for _ in range(3):
            model.inference(A1, None, I1, **kw)
        assert model._active_plan is (slot_plans[B] if rolling else plans[B])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            if rolling and i % K == 0:
                model.inference(A0, F0, I0, restart=[(i // K) % B])
            else:
                model.inference(A1, None, I1)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    arms = {"plain": lambda B: time_plan(plans[B], args.replays), "slots_steady": lambda B: time_plan(slot_plans[B], args.replays),
            "plain_calls": lambda B: time_calls(B, False, args.replays), "slots_rolling": lambda B: time_calls(B, True, args.replays)}
    samples = {B: {a: [] for a in arms} for B in Bs}
    order = list(arms)
    for r in range(args.rounds):
        for B in Bs:
            for a in (order if r % 2 == 0 else order[::-1]):
                samples[B][a].append(arms[a](B))
    res = {}
    print("%8s %16s %12s %10s %10s" % ("streams", "arm", "ms (median)", "min", "max"))
    for B in Bs:
        res[str(B)] = {}
        for a in order:
            v = sorted(samples[B][a])
            res[str(B)][a] = dict(ms=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                                  samples=[round(x, 4) for x in samples[B][a]])
            print("%8d %16s %12.3f %10.3f %10.3f" % (B, a, v[len(v) // 2], v[0], v[-1]))
        res[str(B)]["restart_every"] = K
    return res


def pool_arms(args, model, S, H, W, dev):
    """The three arms of --pool for K = 1..S active of S slots; returns {K: {arm: dict(ms, ms_min, ms_max, samples)}}."""
    import torch
    from vid2vid_amd import synthetic
    opt = model.opt
    tG = opt.n_frames_G
    seqs = [synthetic.label2city_sequence(tG + 2, H, W, seed=1234 + b, device=dev) for b in range(S)]

    def inputs(B, t):
        A = torch.stack([q[0][t:t + tG] for q in seqs[:B]]).view(B, tG, 1, H, W)
        I = torch.stack([q[1][t:t + tG] for q in seqs[:B]]).view(B, tG, 1, H, W)
        return A, (torch.cat([q[2][:, :tG - 1] for q in seqs[:B]]) if t == 0 else None), I

    opt.compact_streams = True
    model.prepare_streams(S, H, W, 1, True)
    opt.compact_streams = False

    def time_calls(arm, K, n):
        B = K if arm == "dense" else S
        kw = {} if arm == "dense" else dict(active=list(range(K)))
        opt.compact_streams = arm == "pool"
        try:
            model.fake_B_prev = None
            model.inference(*inputs(B, 0), **kw)
            A1, _, I1 = inputs(B, 1)
            for _ in range(3):
                fake, _ = model.inference(A1, None, I1, **kw)
            fp = model._active_plan
            assert (fp.pool is not None) == (arm == "pool") and fp.B == (S if arm == "slots_idle" else K)
            assert bool(torch.isfinite(fake).all()) and (arm == "dense" or K == S or not fake[K:].any())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                model.inference(A1, None, I1, **kw)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        finally:
            opt.compact_streams = False

    order = ["pool", "slots_idle", "dense"]
    Ks = list(range(1, S + 1))
    for K in Ks:                                    # build every plan (tile search included) outside the timed rounds
        for a in order:
            time_calls(a, K, 2)
    samples = {K: {a: [] for a in order} for K in Ks}
    for r in range(args.rounds):
        for K in (Ks if r % 2 == 0 else Ks[::-1]):
            for a in (order if r % 2 == 0 else order[::-1]):
                samples[K][a].append(time_calls(a, K, args.replays))
    res = {}
    print("%8s %12s %12s %10s %10s" % ("active", "arm", "ms (median)", "min", "max"))
    for K in Ks:
        res[str(K)] = {}
        for a in order:
            v = sorted(samples[K][a])
            res[str(K)][a] = dict(ms=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                                  samples=[round(x, 4) for x in samples[K][a]])
            print("%8d %12s %12.3f %10.3f %10.3f" % (K, a, v[len(v) // 2], v[0], v[-1]))
    res["slots"] = S
    return res


if __name__ == "__main__":
    main()
