#!/usr/bin/env python
"""Acceptance matrix of the conv entry points: which (tile id, descriptor) combinations the library takes and what it answers.

Sweeps every tile id 0 ... 150 over a fixed list of descriptors in dry-run mode (nothing is launched, no GPU needed) and records, per
combination, [v2v_conv_tile_config, v2v_conv_stats_rows, v2v_conv_splitk_workspace, its ticket count, v2v_conv2d, v2v_conv2d_pair with
a twin].  tests/test_cpu_tile_table.py compares the matrix of the current build with the committed one
(tests/data/conv_tile_acceptance.json): a change of the tile table or of build_conv that accepts, refuses or sizes anything
differently shows up as a diff.  Regenerate the file only for a change that MEANS to alter what is accepted:

    python scripts/conv_tile_acceptance.py --write tests/data/conv_tile_acceptance.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE_IDS = range(0, 151)

# name -> descriptor fields that differ from BASE (a bf16 3x3 / stride 1 / reflect pad 1 Conv2d, 64 -> 64 channels at 32 x 64, raw
# fp32 output with statistics, channel-chunk-major weights).  The boolean fields are optional operands: a scratch address or NULL.
BASE = dict(N=1, H=32, W=64, cin=64, cin_stride=64, cout=64, cout_stride=64, KH=3, KW=3, stride=1, pad=1, pad_mode=1, transposed=0,
            OH=32, OW=64, dtype=1, out_mode=0, act=0, act_param=0.0, out_scale=1.0, splitk=1, prefetch=0, w_korder=1, ablate=0,
            act_split=0, fin_count=0, stats=True, fin_counter=False, fin_workspace=False, slabs=False)
C128 = dict(cin=128, cin_stride=128, cout=128, cout_stride=128)
S2 = dict(stride=2, pad_mode=0, OH=16, OW=32, cout=128, cout_stride=128)
T2 = dict(transposed=1, stride=2, pad_mode=0, OH=64, OW=128, cout=32, cout_stride=32)
C7 = dict(KH=7, KW=7, pad=3)
FIN = dict(fin_counter=True, fin_count=32 * 64)
DESCRIPTORS = [
    ("c3_bf16_k1", {}),
    ("c3_bf16_k0", dict(w_korder=0)),
    ("c3_bf16_k2", dict(w_korder=2)),
    ("c3_f32_k1", dict(dtype=0)),
    ("c3_f32_k0", dict(dtype=0, w_korder=0)),
    ("c3_bf16_k1_fin", dict(FIN)),
    ("c3_bf16_k1_raw_act", dict(out_mode=4)),
    ("c3_bf16_k1_act", dict(out_mode=1, act=1, stats=False)),
    ("c3_128_k1_splitk2", dict(C128, splitk=2, slabs=True)),
    ("c3_128_k0_splitk2", dict(C128, splitk=2, slabs=True, w_korder=0)),
    ("c3_128_k1_norm_act", dict(C128, out_mode=3, **FIN)),
    ("c3_128_k1_norm_act_no_counter", dict(C128, out_mode=3, fin_count=32 * 64)),
    ("c3_128_k1_pad2_zero", dict(C128, pad=2, pad_mode=0, OH=34, OW=66)),
    ("c3_big_k1_fin_workspace", dict(FIN, H=256, W=512, OH=256, OW=512, fin_count=256 * 512, fin_workspace=True)),
    ("c3_pairx_k3", dict(cin=32, cin_stride=32, cout=32, cout_stride=32, w_korder=3)),
    ("c3_s2_k1", dict(S2)),
    ("c3_s2_k0", dict(S2, w_korder=0)),
    ("t3_s2_cs64_k2", dict(T2, w_korder=2)),
    ("t3_s2_cs64_k0", dict(T2, w_korder=0)),
    ("t3_s2_pairx_k3", dict(T2, cin=32, cin_stride=32, cout=16, cout_stride=16, w_korder=3)),
    ("c7_cs8_cout32_k0", dict(C7, cin=6, cin_stride=8, cout=32, cout_stride=32, w_korder=0)),
    ("c7_cs32_cout3_nchw_k0", dict(C7, cin=32, cin_stride=32, cout=3, cout_stride=3, out_mode=2, act=3, stats=False, w_korder=0)),
    ("c7_cs32_cout3_act_split_k0", dict(C7, cin=32, cin_stride=32, cout=3, cout_stride=3, out_mode=2, act_split=2, stats=False, w_korder=0)),
    ("c7_cs32_cout32_f32_k0", dict(C7, dtype=0, cin=32, cin_stride=32, cout=32, cout_stride=32, w_korder=0)),
    ("c7_cs64_cout64_k1", dict(C7)),
    ("c7_cs128_cout64_k0", dict(C7, cin=128, cin_stride=128, w_korder=0)),
    ("c7_cs128_cout32_nchw_k0", dict(C7, cin=128, cin_stride=128, cout=32, cout_stride=32, out_mode=2, stats=False, w_korder=0)),
]


def compute():
    """{descriptor name: [[tile_config, stats_rows, splitk_workspace, tickets, conv2d, conv2d_pair] for tile id 0 ... 150]}"""
    from vid2vid_amd.lib import lib, ConvDesc
    scratch = (C.c_char * (1 << 16))()
    base = (C.addressof(scratch) + 255) & ~255                  # member `slot` of a pair gets its own 256-byte aligned addresses
    at = lambda slot, i: base + 4096 * slot + 256 * i

    def desc(fields, tile, slot):
        d = ConvDesc()
        d.in_, d.w, d.zero_page = at(slot, 0), at(slot, 1), at(0, 2)
        d.out, d.fin_scale_shift = at(slot, 3), at(slot, 4)
        for name, i in (("stats", 5), ("fin_counter", 6), ("fin_workspace", 7), ("slabs", 8)):
            setattr(d, name, at(slot, i) if fields[name] else None)
        d.sk_counter = at(slot, 9) if fields["slabs"] else None
        for name, v in fields.items():
            if not isinstance(v, bool):
                setattr(d, name, v)
        d.tile = tile
        return d

    prev = lib.v2v_set_dry_run(1)
    try:
        out = {}
        for name, delta in DESCRIPTORS:
            fields = dict(BASE, **delta)
            rows = []
            for tile in TILE_IDS:
                a, b = desc(fields, tile, 0), desc(fields, tile, 1)
                tickets = C.c_int32(-7)
                rows.append([lib.v2v_conv_tile_config(C.byref(a)), lib.v2v_conv_stats_rows(C.byref(a)),
                             lib.v2v_conv_splitk_workspace(C.byref(a), C.byref(tickets)), tickets.value,
                             lib.v2v_conv2d(C.byref(a), None), lib.v2v_conv2d_pair(C.byref(a), C.byref(b), None)])
            out[name] = rows
        return out
    finally:
        lib.v2v_set_dry_run(prev)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="FILE", help="write the matrix as JSON (default: print a summary)")
    args = ap.parse_args()
    m = compute()
    if args.write:
        with open(args.write, "w") as f:
            f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in m.items()) + "\n}\n")
    for name, rows in m.items():
        ok = [t for t, r in zip(TILE_IDS, rows) if r[4] == 0]
        pair = [t for t, r in zip(TILE_IDS, rows) if r[5] == 0]
        print("%-32s launches: %s\n%-32s pairs:    %s" % (name, ok, "", pair))


if __name__ == "__main__":
    main()
