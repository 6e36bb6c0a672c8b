#!/usr/bin/env python
"""The conv tile search's choices, frozen: which (tile, split-K, prefetch) configurations the tuner times for a fixed matrix of layers,
in its order, and which runners-up it keeps for a fixed hand-written set of "elapsed" times.  No GPU needed.

Two modes give the same lists:

  --mode engine   drives Engine._autotune / Engine._autotune_pair of a record-only engine in the dry-run library with the timing
                  primitives stubbed (a fake event class, a one-element _thrash, elapsed times from MS below) and a recording proxy
                  around engine.lib: the first descriptor-carrying library call of each timing attempt gives the configuration, and
                  the first-pass sequence of those IS the candidate list.  Needs nothing of tile_search.py: it also runs on a tree
                  from before that module existed, which is how tests/data/tile_search_candidates.json was first recorded.
  --mode direct   asks tile_search.conv_candidates / pair_candidates (candidate lists only).

tests/test_cpu_tile_search.py compares the direct lists (and tile_search.runners_up on the recorded times) with the committed file.
Regenerate it only for a change that MEANS to alter what the search tries or keeps:

    python scripts/tile_search_record.py --write tests/data/tile_search_candidates.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# environment of each pass (the tile-table views are built at import: every pass but the first runs in a child process)
PASSES = {"default": {}, "exp_tiles": {"V2V_EXP_TILES": "1"}, "s2_patch_0": {"V2V_S2_PATCH": "0"}}

# "elapsed" milliseconds of the i-th timing attempt of a search (hand-written: no order, no ties), and the factor the 11-repetition
# second pass finds the j-th front-runner off by
MS = [0.0310, 0.0240, 0.0405, 0.0262, 0.0198, 0.0570, 0.0221, 0.0349, 0.0287, 0.0455, 0.0203, 0.0330, 0.0251, 0.0612, 0.0236, 0.0299]
SECOND_PASS = [1.30, 0.90, 1.10, 0.80, 1.20, 1.00]


def fake_ms(i):
    return MS[i % len(MS)] + 1e-4 * (i // len(MS))


# ---------------- the layer matrix ----------------
# Forward rows: fields that differ from BASE (a bf16 3x3 / stride 1 Conv2d behind ReflectionPad2d(1), 64 -> 64 channels at 32 x 64, raw
# fp32 output with statistics rows, no in-kernel finalize).  dtype 0 fp32 / 1 bf16; pad_mode 0 zero / 1 reflect; out_mode 0 raw fp32
# NHWC / 1 activation NHWC / 2 planar fp32.  OH / OW follow from the geometry.
BASE = dict(dtype=1, N=1, H=32, W=64, cin=64, cs=64, cout=64, K=3, stride=1, pad=1, pad_mode=1, transposed=0, out_mode=0,
            stats=True, fin=False, role="fwd")
SMALL, LARGE = dict(H=32, W=64), dict(H=64, W=128)
C128, C1024 = dict(cin=128, cs=128, cout=128), dict(cin=1024, cs=1024, cout=1024)
PAIRX = dict(cin=32, cs=32, cout=32, H=64, W=128)
S2 = dict(stride=2, pad_mode=0)
T2 = dict(transposed=1, stride=2, pad_mode=0)
C7 = dict(K=7, pad=3)
HEAD = dict(C7, out_mode=2, stats=False)
FIN = dict(fin=True)


def _row(*parts, **fields):
    row = {}
    for part in parts:
        row.update(part)
    return dict(row, **fields)


FWD = [
    ("c3_64_small", _row(SMALL)), ("c3_64_large", _row(LARGE)), ("c3_64_large_f32", _row(LARGE, dtype=0)),
    ("c3_64to128_large", _row(LARGE, cout=128)), ("c3_64to128_large_fin", _row(LARGE, FIN, cout=128)),
    ("c3_128_small", _row(SMALL, **C128)), ("c3_128_large", _row(LARGE, **C128)), ("c3_128_large_f32", _row(LARGE, dtype=0, **C128)),
    ("c3_128_large_fin", _row(LARGE, FIN, **C128)), ("c3_128_large_act", _row(LARGE, out_mode=1, stats=False, **C128)),
    ("c3_128_large_n2", _row(LARGE, N=2, **C128)),
    ("c3_1024_small", _row(SMALL, **C1024)), ("c3_1024_large", _row(LARGE, **C1024)), ("c3_1024_small_f32", _row(SMALL, dtype=0, **C1024)),
    ("c3_1024_16x32", _row(C1024, H=16, W=32)),
    ("c3_pairx", _row(PAIRX)), ("c3_pairx_fin", _row(PAIRX, **FIN)), ("c3_pairx_f32", _row(PAIRX, dtype=0)),
    ("c3_pairx_256x512", _row(PAIRX, H=256, W=512)), ("c3_cs32_odd", _row(PAIRX, W=72)),
    ("c3_s2_small", _row(SMALL, cout=128, **S2)), ("c3_s2_large", _row(S2, cout=128, H=128, W=256)),
    ("c3_s2_large_f32", _row(S2, dtype=0, cout=128, H=128, W=256)), ("c3_s2_large_fin", _row(S2, FIN, cout=128, H=128, W=256)),
    ("c3_s2_128to256", _row(S2, cin=128, cs=128, cout=256, H=128, W=256)), ("c3_s2_reflect", _row(SMALL, cout=128, stride=2)),
    ("t3_small", _row(SMALL, cout=32, **T2)), ("t3_large", _row(LARGE, cin=128, cs=128, cout=64, **T2)),
    ("t3_large_f32", _row(LARGE, dtype=0, cin=128, cs=128, cout=64, **T2)), ("t3_256to128", _row(LARGE, cin=256, cs=256, cout=128, **T2)),
    ("t3_32to16_small", _row(SMALL, cin=32, cs=32, cout=16, **T2)), ("t3_32to16", _row(T2, cin=32, cs=32, cout=16, H=64, W=128)),
    ("t3_32to16_256x512", _row(T2, cin=32, cs=32, cout=16, H=256, W=512)),
    ("c7_cs8_cout32", _row(C7, LARGE, cin=6, cs=8, cout=32)), ("c7_cs8_cout64", _row(C7, LARGE, cin=6, cs=8, cout=64)),
    ("c7_cs8_cout64_fin", _row(C7, LARGE, FIN, cin=6, cs=8, cout=64)), ("c7_cs8_cout32_f32", _row(C7, LARGE, dtype=0, cin=3, cs=4, cout=32)),
    ("c7_cs32_cout3_head", _row(HEAD, LARGE, cin=32, cs=32, cout=3)), ("c7_cs32_cout3_head_f32", _row(HEAD, LARGE, dtype=0, cin=32, cs=32, cout=3)),
    ("c7_cs32_cout3_raw", _row(C7, LARGE, cin=32, cs=32, cout=3)), ("c7_cs32_cout32", _row(C7, LARGE, cin=32, cs=32, cout=32)),
    ("c7_cs32_cout32_fin", _row(C7, LARGE, FIN, cin=32, cs=32, cout=32)),
    ("c7_cs64_cout3_head", _row(HEAD, LARGE, cin=64, cs=64, cout=3)), ("c7_cs64_cout32", _row(C7, LARGE, cout=32)),
    ("c7_cs64_cout64_small", _row(C7, SMALL)), ("c7_cs64_cout64", _row(C7, LARGE)), ("c7_cs64_cout64_act", _row(C7, LARGE, out_mode=1, stats=False)),
    ("c7_cs128_cout64", _row(C7, LARGE, cin=108, cs=128)), ("c7_cs128_cout128", _row(C7, H=128, W=256, cin=108, cs=128, cout=128)),
    ("c7_cs128_cout32_head", _row(HEAD, LARGE, cin=128, cs=128, cout=32)), ("c7_cs128_cout3_head", _row(HEAD, LARGE, cin=128, cs=128, cout=3)),
]
# Backward-data rows: the forward layer (kind, cin, cout, K, stride, pad; reflect: behind a ReflectionPad2d(pad)) and its forward input
# size -- the descriptor is autograd._conv_backward_data's (pad 2 - p for a 3x3 behind reflect padding, on the padded grid)
BWD = [
    ("bwd_c3_zero_small", _row(SMALL, kind="conv", cin=128, cout=128, K=3, stride=1, pad=1, reflect=False)),
    ("bwd_c3_zero_large", _row(LARGE, kind="conv", cin=128, cout=128, K=3, stride=1, pad=1, reflect=False)),
    ("bwd_c3_zero_large_f32", _row(LARGE, dtype=0, kind="conv", cin=128, cout=128, K=3, stride=1, pad=1, reflect=False)),
    ("bwd_c3_reflect_small", _row(SMALL, kind="conv", cin=128, cout=128, K=3, stride=1, pad=1, reflect=True)),
    ("bwd_c3_reflect_large", _row(LARGE, kind="conv", cin=128, cout=128, K=3, stride=1, pad=1, reflect=True)),
    ("bwd_c3_reflect_1024", _row(SMALL, kind="conv", cin=1024, cout=1024, K=3, stride=1, pad=1, reflect=True)),
    ("bwd_c7_head", _row(LARGE, kind="conv", cin=64, cout=3, K=7, stride=1, pad=3, reflect=True)),
    ("bwd_c7_head_f32", _row(LARGE, dtype=0, kind="conv", cin=64, cout=3, K=7, stride=1, pad=3, reflect=True)),
    ("bwd_s2_small", _row(SMALL, kind="conv", cin=64, cout=128, K=3, stride=2, pad=1, reflect=False)),
    ("bwd_s2_large", _row(kind="conv", cin=64, cout=128, K=3, stride=2, pad=1, reflect=False, H=128, W=256)),
    ("bwd_t2_small", _row(SMALL, kind="convT", cin=128, cout=64, K=3, stride=2, pad=1, reflect=False)),
    ("bwd_t2_large", _row(LARGE, kind="convT", cin=128, cout=64, K=3, stride=2, pad=1, reflect=False)),
]
# Paired 3x3 launches: rows of whole and of ragged 64-pixel tiles, 1 / 2 / 4 (/ 16) 128-byte chunks per pixel
PAIRS = [
    ("pair_64_w64", dict(dtype=1, N=1, H=32, W=64, c=64)), ("pair_128_w64", dict(dtype=1, N=1, H=32, W=64, c=128)),
    ("pair_256_w64", dict(dtype=1, N=1, H=32, W=64, c=256)), ("pair_256_w96", dict(dtype=1, N=1, H=32, W=96, c=256)),
    ("pair_1024_w64", dict(dtype=1, N=1, H=32, W=64, c=1024)), ("pair_1024_w32", dict(dtype=1, N=1, H=16, W=32, c=1024)),
    ("pair_128_w256", dict(dtype=1, N=1, H=128, W=256, c=128)), ("pair_128_f32", dict(dtype=0, N=1, H=32, W=64, c=128)),
]


def _vec(dtype):
    return 8 if dtype == 1 else 4


def fwd_fields(delta):
    """(descriptor fields, want_stats, in-kernel finalize, module spec) of a forward row."""
    f = dict(BASE, **delta)
    K, s, p = f["K"], f["stride"], f["pad"]
    if f["transposed"]:
        OH, OW = (f["H"] - 1) * s - 2 * p + K + 1, (f["W"] - 1) * s - 2 * p + K + 1          # output_padding 1
    else:
        OH, OW = (f["H"] + 2 * p - K) // s + 1, (f["W"] + 2 * p - K) // s + 1
    cout, v = f["cout"], _vec(f["dtype"])
    cstride = {0: (cout + 3) // 4 * 4, 1: (cout + v - 1) // v * v, 2: cout}[f["out_mode"]]
    d = dict(N=f["N"], H=f["H"], W=f["W"], cin=f["cin"], cin_stride=f["cs"], cout=cout, cout_stride=cstride, KH=K, KW=K, stride=s, pad=p,
             pad_mode=f["pad_mode"], transposed=f["transposed"], OH=OH, OW=OW, dtype=f["dtype"], out_mode=f["out_mode"])
    mod = dict(kind="convT" if f["transposed"] else "conv", cin=f["cin"], cout=cout, K=K, stride=s, pad=0 if f["pad_mode"] == 1 else p)
    return d, f["stats"], f["fin"], mod


def bwd_fields(delta):
    """The backward-data descriptor autograd._conv_backward_data builds for the layer of a BWD row."""
    f = _row(dict(dtype=1, N=1), delta)
    K, s, p, reflect, v = f["K"], f["stride"], f["pad"], f["reflect"], _vec(f["dtype"])
    H, W = f["H"], f["W"]                                         # of the forward INPUT
    if f["kind"] == "convT":
        OH, OW = (H - 1) * s - 2 * p + K + 1, (W - 1) * s - 2 * p + K + 1
    else:
        OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    HO, WO = (H + 2 * p, W + 2 * p) if reflect else (H, W)
    pad4 = lambda c: (c + v - 1) // v * v
    d = dict(N=f["N"], H=OH, W=OW, cin=f["cout"], cin_stride=pad4(f["cout"]), cout=f["cin"], cout_stride=pad4(f["cin"]), KH=K, KW=K,
             stride=s, pad=0 if reflect else p, pad_mode=0, transposed=int(f["kind"] != "convT"), OH=HO, OW=WO, dtype=f["dtype"], out_mode=1)
    mod = dict(kind=f["kind"], cin=f["cin"], cout=f["cout"], K=K, stride=s, pad=0 if reflect else p)
    return d, reflect, mod


def make_module(spec, device=None):
    import torch.nn as nn
    if spec["kind"] == "convT":
        return nn.ConvTranspose2d(spec["cin"], spec["cout"], spec["K"], spec["stride"], spec["pad"], output_padding=1, device=device)
    return nn.Conv2d(spec["cin"], spec["cout"], spec["K"], spec["stride"], spec["pad"], device=device)


class HostMemory:
    """256-byte aligned host addresses for the operands a dry-run descriptor only has to name."""

    def __init__(self):
        self.buf = (C.c_char * (1 << 14))()
        self.base = (C.addressof(self.buf) + 255) & ~255

    def __call__(self, i):
        return self.base + 256 * i


def make_desc(fields, stats, fin, mem):
    from vid2vid_amd.lib import ConvDesc
    d = ConvDesc()
    d.in_, d.w, d.zero_page, d.out = mem(0), mem(1), mem(2), mem(3)
    for name, v in fields.items():
        setattr(d, name, v)
    d.act_param, d.out_scale, d.splitk = 0.0, 1.0, 1
    if stats:
        d.stats = mem(4)
    if fin:
        d.fin_counter, d.fin_scale_shift, d.fin_count = mem(5), mem(6), fields["N"] * fields["OH"] * fields["OW"]
    return d


# ---------------- --mode direct ----------------
def compute_direct():
    from vid2vid_amd import tile_search as TS
    mem, out = HostMemory(), {}
    for name, delta in FWD:
        fields, stats, fin, spec = fwd_fields(delta)
        d = make_desc(fields, stats, fin, mem)
        out[name] = {"cands": [list(c) for c in TS.conv_candidates(d, fields["dtype"], fields["cout"], make_module(spec, "meta"), "fwd")]}
    for name, delta in BWD:
        fields, reflect, spec = bwd_fields(delta)
        d = make_desc(fields, False, False, mem)
        out[name] = {"cands": [list(c) for c in TS.conv_candidates(d, fields["dtype"], fields["cout"], make_module(spec, "meta"), "bwd")]}
    for name, p in PAIRS:
        v = _vec(p["dtype"])
        out[name] = {"cands": [list(c) for c in TS.pair_candidates(p["N"], p["H"], p["W"], (p["c"] + v - 1) // v * v, p["c"], p["dtype"])],
                     "default": TS.default_pair_tile(p["W"])}
    return out


# ---------------- --mode engine ----------------
class _Recorder:
    """engine.lib with a log of timing attempts: {cfg: (tile, splitk, prefetch) of the descriptor at the attempt's first library call
    that carries one (split-K 0 = 1), launched: the launch call accepted it, reps: timed repetitions, ms: the stub's elapsed time}.
    An attempt ends when the library refuses it or when the stubbed last event is waited for."""
    LAUNCHES = ("v2v_conv2d", "v2v_conv2d_pair")
    SIZED = ("v2v_conv_stats_rows", "v2v_conv_splitk_workspace")

    def __init__(self, real):
        self._real, self.attempts, self._open = real, [], None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self.LAUNCHES + self.SIZED:
            return fn

        def call(*args):
            from vid2vid_amd.lib import ConvDesc
            d = next(a._obj for a in args if isinstance(getattr(a, "_obj", None), ConvDesc))
            if self._open is None:
                self._open = dict(cfg=(int(d.tile), max(int(d.splitk), 1), int(d.prefetch)), launched=False, events=0)
                self.attempts.append(self._open)
            rc = fn(*args)
            if name in self.LAUNCHES and rc == 0:
                self._open["launched"] = True
            elif rc <= 0 or name in self.LAUNCHES:
                self._open = None
            return rc
        return call

    def new_search(self):
        self.attempts, self._open, self._first_ms = [], None, {}

    def event(self):
        self._open["events"] += 1

    def close(self):
        a, self._open = self._open, None
        a["reps"] = a.pop("events") // 2
        if a["reps"] == 11:                 # second pass of _autotune: the j-th front-runner again
            j = sum(1 for b in self.attempts if b.get("reps") == 11) - 1
            a["ms"] = self._first_ms[a["cfg"]] * SECOND_PASS[j]
        else:
            a["ms"] = self._first_ms[a["cfg"]] = fake_ms(len(self.attempts) - 1)
        self.last_ms = a["ms"]


def compute_engine():
    import torch
    from vid2vid_amd import engine as E
    from vid2vid_amd.lib import lib
    rec = _Recorder(E.lib)

    class FakeEvent:
        def __init__(self, enable_timing=False):
            rec.event()

        def record(self):
            pass

        def synchronize(self):
            rec.close()

        def elapsed_time(self, other):
            return rec.last_ms

    def first_pass():
        return [a for a in rec.attempts if a.get("reps") != 11]

    mem, out = HostMemory(), {}
    prev_dry, prev_event, prev_lib = lib.v2v_get_dry_run(), torch.cuda.Event, E.lib
    torch.cuda.Event, E.lib = FakeEvent, rec
    try:
        engines = {}
        for dt in (0, 1):
            engines[dt] = E.Engine(torch.device("cpu"), dt, record_only=True)
            engines[dt]._thrash = torch.empty(1)

        def conv_row(name, d, fields, stats, spec, role, reflect):
            eng = engines[fields["dtype"]]
            rec.new_search()
            before = set(vars(eng))
            res = eng._autotune(d, stats, fields["cout"], mod=make_module(spec), cin_stride=fields["cin_stride"], role=role, reflect=reflect)
            if not isinstance(res[0], tuple):       # a tree from before _autotune returned (best, alts, wide): it returned best and left the
                left = sorted(set(vars(eng)) - before)      # two lists on the engine, as two attributes __init__ never declared (alts, wide)
                res = (res,) + (tuple(vars(eng).pop(k) for k in left) if left else ([], []))
            out[name] = dict(summary(first_pass()), best=list(res[0]), alts=[list(c) for c in res[1]], wide=[list(c) for c in res[2]],
                             second_pass=[list(a["cfg"]) for a in rec.attempts if a.get("reps") == 11])

        for name, delta in FWD:
            fields, stats, fin, spec = fwd_fields(delta)
            conv_row(name, make_desc(fields, stats, fin, mem), fields, stats, spec, "fwd", False)
        for name, delta in BWD:
            fields, reflect, spec = bwd_fields(delta)
            conv_row(name, make_desc(fields, False, False, mem), fields, False, spec, "bwd", reflect)
        for name, p in PAIRS:
            eng = engines[p["dtype"]]
            v = _vec(p["dtype"])
            cs = (p["c"] + v - 1) // v * v
            xa, xb = (E.Act(torch.zeros((p["N"], p["H"], p["W"], cs), dtype=eng.tdtype), p["c"]) for _ in range(2))
            ma, mb = (make_module(dict(kind="conv", cin=p["c"], cout=p["c"], K=3, stride=1, pad=0)) for _ in range(2))
            key = ("pair", name)
            rec.new_search()
            best = eng._autotune_pair(xa, ma, xb, mb, 1, 1, (None, None), key, fuse=None)
            out[name] = dict(summary(rec.attempts), best=list(best), alts=[list(c) for c in eng._tune_alts[key]],
                             log=[list(r) for r in eng.pair_tune_log[key]])
        return out
    finally:
        torch.cuda.Event, E.lib = prev_event, prev_lib
        lib.v2v_set_dry_run(prev_dry)


def summary(attempts):
    """cands: the configurations in the order tried; ran: which of them the library launched (the i-th attempt then "took"
    fake_ms(i)); reps: timed repetitions of those."""
    return dict(cands=[list(a["cfg"]) for a in attempts], ran=[int(a["launched"]) for a in attempts],
                reps=sorted({a["reps"] for a in attempts if "reps" in a}))


def timed_of(row):
    """The sorted [(ms, cfg)] list _autotune held after the first pass of a recorded conv row."""
    return sorted((fake_ms(i), tuple(cfg)) for i, (cfg, ok) in enumerate(zip(row["cands"], row["ran"])) if ok)


def compute(mode, which):
    if which == "default" or all(os.environ.get(k) == v for k, v in PASSES[which].items()):
        return compute_engine() if mode == "engine" else compute_direct()
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--pass", which, "--print"], check=True,
                         stdout=subprocess.PIPE, env=dict(os.environ, **PASSES[which]))
    return json.loads(res.stdout)


def dump(m):
    """One line per row."""
    return "{\n" + ",\n".join(' "%s": {\n' % p + ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in rows.items())
                              + "\n }" for p, rows in m.items()) + "\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("engine", "direct"), default="engine")
    ap.add_argument("--pass", dest="which", choices=tuple(PASSES), help="one pass only (default: all, each in its environment)")
    ap.add_argument("--write", metavar="FILE", help="write {pass: {row: lists}} as JSON")
    ap.add_argument("--print", action="store_true", help="print the JSON instead of a summary")
    args = ap.parse_args()
    if args.which:
        m = compute(args.mode, args.which)
    else:
        m = {which: compute(args.mode, which) for which in PASSES}
    if args.write:
        with open(args.write, "w") as f:
            f.write(dump(m) if not args.which else json.dumps(m))
    if args.print:
        print(json.dumps(m))
    elif not args.which:
        for name, row in m["default"].items():
            print("%-28s %3d candidates, tiles %s" % (name, len(row["cands"]), sorted({c[0] for c in row["cands"]})))


if __name__ == "__main__":
    main()
