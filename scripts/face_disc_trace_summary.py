"""Summary of two rocprofv3 --kernel-trace databases of scripts/face_disc_chunk.py (without / with --add_face_disc):
device kernel time per chunk, the difference, and the face-window kernels one by one.

    python scripts/face_disc_trace_summary.py <base_results.db> <face_results.db> [--chunks 4]
"""
import argparse
import sqlite3
from collections import defaultdict

NEW = ("face_window_reset", "face_window_reduce", "face_window_finalize", "pack_concat_window", "unpack_window")


def load(path, steps_per_chunk=2):
    """Per-kernel (calls, ms) of the steady-state chunks: every dispatch that starts after the first chunk's last optimizer
    step (each chunk ends with `steps_per_chunk` Adam launches: optimizer_G, optimizer_D) -- the first chunk also packs the
    weights and builds the plans."""
    c = sqlite3.connect(path)
    rows = c.execute("select name, start, end, duration from kernels order by start").fetchall()
    adam = [r for r in rows if "adam_step" in r[0]]
    t0 = adam[steps_per_chunk - 1][2]
    per = defaultdict(lambda: [0, 0.0])
    for name, start, _, dur in rows:
        if start > t0:
            per[name][0] += 1
            per[name][1] += dur / 1e6                # ns -> ms
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("face")
    ap.add_argument("--chunks", type=int, default=4)
    a = ap.parse_args()
    base, face = load(a.base), load(a.face)
    tb = sum(v[1] for v in base.values())
    tf = sum(v[1] for v in face.values())
    nb = sum(v[0] for v in base.values())
    nf = sum(v[0] for v in face.values())
    k = a.chunks - 1
    print("chunks per run: %d; the %d after the first are summed (kernel durations; launches on the side stream overlap)" % (a.chunks, k))
    print("without --add_face_disc: %8.2f ms kernel time, %6d launches  -> %7.2f ms / chunk" % (tb, nb, tb / k))
    print("with    --add_face_disc: %8.2f ms kernel time, %6d launches  -> %7.2f ms / chunk" % (tf, nf, tf / k))
    print("added by the face discriminator: %.2f ms / chunk, %d launches / chunk" % ((tf - tb) / k, (nf - nb) // k))
    print("\nface-window kernels (with --add_face_disc):")
    print("%-60s %6s %10s %10s" % ("kernel", "calls", "total ms", "us / call"))
    for name, (n, t) in sorted(face.items()):
        if any(s in name for s in NEW):
            print("%-60s %6d %10.4f %10.2f" % (name[:60], n, t, t / n * 1e3))
    print("\nlargest additions (kernel time with - without, ms over the run):")
    diff = sorted(((face.get(n, [0, 0])[1] - base.get(n, [0, 0])[1], n) for n in set(face) | set(base)), reverse=True)
    for d, n in diff[:12]:
        print("  %9.3f  %s" % (d, n[:100]))


if __name__ == "__main__":
    main()
