#!/usr/bin/env python3
"""gmx_squares on RMAT-<scale>, in one process and on one graph:

  * the library's log line (the classes, the wedges, the batches, the squares) and the device time by phase -- plan additions,
    each class, finish; GMX_SQUARES_PHASES -- from the first call, which builds the plan and its additions, and from one
    warm call; then --reps calls without the phase clock: median and min-max of kernel_ms;
  * the total-only query (per_vertex=False) next to the per-vertex one;
  * next to gmx_clustering on the same plan and to one sweep of the rows (gmx_avg_teen_cnt) on the same graph;
  * next to GMX_SQUARES_PLAIN=1 (every credit a global atomic per wedge);
  * --sweep: the same call with GMX_SQUARES_WAVE_MAX, GMX_SQUARES_LDS_SLOTS, GMX_SQUARES_SPLIT and GMX_SQUARES_BATCH_BYTES
    varied one at a time (the value that is the default is measured again in its place), then the best value of each
    together.

  squares_prof.py --scale 20 [--permute] [--symmetrize] [--reps 5] [--sweep] [--skip-plain]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx squares: (plan .* squares \d+)")
PHASES = ("plan", "wave", "block", "global", "finish")
PHASE = re.compile(r"gmx squares phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES))
KNOBS = ("GMX_SQUARES_WAVE_MAX", "GMX_SQUARES_LDS_SLOTS", "GMX_SQUARES_SPLIT", "GMX_SQUARES_BATCH_BYTES", "GMX_SQUARES_PLAIN", "GMX_SQUARES_LOG",
         "GMX_SQUARES_PHASES")
SWEEP = ([{"wave_max": v} for v in (0, 32, 64, 128)] + [{"lds_slots": v} for v in (1024, 2048, 4096, 8192, 16384, 18432)] +
         [{"split": v} for v in (1024, 4096, 16384, 65536, 262144, 1 << 30)] + [{"batch_bytes": v} for v in (64 << 20, 256 << 20, 1 << 30, 4 << 30)])


def call(g, per_vertex=True, phases=False, **knobs):
    """(count, squares, stats, the log line, ms by phase or None) of one call; the lines come from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, v in knobs.items():
        os.environ["GMX_SQUARES_" + name.upper()] = str(v)
    os.environ["GMX_SQUARES_LOG"] = "1"
    if phases:
        os.environ["GMX_SQUARES_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            cnt, n, st = g.squares(per_vertex=per_vertex)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or (phases and not p):
        sys.exit("squares_prof: no log line in %r" % text)
    return cnt, n, st, m.group(1), dict(zip(PHASES, map(float, p.groups()))) if phases else None


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, reps, want=None, per_vertex=True, show=False, **knobs):
    cnt, n, st, line, ph = call(g, per_vertex, phases=show, **knobs)   # warm-up
    if want is not None and (n != want[1] or (per_vertex and not np.array_equal(cnt, want[0]))):
        sys.exit("squares_prof: %s gives another result" % tag)
    if show:
        print("%s %s" % (tag, line))
        print("%s phases (one warm call under GMX_SQUARES_PHASES): %s" % (tag, ", ".join("%s %.3f ms" % (p, ph[p]) for p in PHASES)))
    kms = [call(g, per_vertex, **knobs)[2]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms), (cnt, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="WAVE_MAX, LDS_SLOTS, SPLIT and BATCH_BYTES, one at a time")
    ap.add_argument("--skip-plain", action="store_true", help="leave out the GMX_SQUARES_PLAIN=1 runs (three global atomics per wedge)")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    lcc = g.clustering()   # builds the plan: the first squares call below adds the adjacency and its own additions
    _, _, st, line, ph = call(g, phases=True)
    print("%s first call %s" % (tag, line))
    print("%s first call: the adjacency and the additions %.3f ms (graph preprocessing, outside kernel_ms); kernel_ms %.3f, d2h_ms %.3f" %
          (tag, ph["plan"], st["kernel_ms"], st["d2h_ms"]), flush=True)
    base, want = runs(g, tag, a.reps, show=True)
    total, _ = runs(g, tag + " total only", a.reps, want, per_vertex=False, show=True)
    print("%s total only = %.2f x per vertex" % (tag, total / base))
    lms = [g.clustering()[5]["kernel_ms"] for _ in range(a.reps)]
    print("%s gmx_clustering kernel_ms %s (%d triangles)" % (tag, spread(lms), lcc[3]))
    print("%s squares = %.2f x gmx_clustering" % (tag, base / statistics.median(lms)))
    age = (np.arange(V) % 60).astype(np.int32)
    g.avg_teen_cnt(age, 5)
    sms = [g.avg_teen_cnt(age, 5)[2]["kernel_ms"] for _ in range(a.reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(sms)))
    print("%s squares = %.1f x one sweep of the rows" % (tag, base / statistics.median(sms)), flush=True)
    if not a.skip_plain:
        plain, _ = runs(g, tag + " GMX_SQUARES_PLAIN=1", a.reps, want, plain=1)
        print("%s plain = %.2f x the default" % (tag, plain / base), flush=True)
    if a.sweep:
        named = lambda knobs: " ".join("GMX_SQUARES_%s=%s" % (n.upper(), v) for n, v in knobs.items())
        best = {}
        for knobs in SWEEP:
            ms, _ = runs(g, "%s %s" % (tag, named(knobs)), a.reps, want, show=True, **knobs)
            print("%s %s = %.2f x the default" % (tag, named(knobs), ms / base), flush=True)
            (name, v), = knobs.items()
            if name not in best or ms < best[name][0]:
                best[name] = (ms, v)
        together = {name: v for name, (ms, v) in best.items()}
        ms, _ = runs(g, "%s together %s" % (tag, named(together)), a.reps, want, show=True, **together)
        print("%s together %s = %.2f x the default" % (tag, named(together), ms / base), flush=True)
        ms, _ = runs(g, "%s together, total only" % tag, a.reps, want, per_vertex=False, **together)
        print("%s together, total only = %.2f x the default's total only" % (tag, ms / total), flush=True)
    g.free()


if __name__ == "__main__":
    main()
