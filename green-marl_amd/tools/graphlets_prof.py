#!/usr/bin/env python3
"""gmx_graphlets on RMAT-<scale>, in one process and on one graph:

  * the library's log line (the plan parts built, the items of the walk, the long rows, the triangles, the nine totals) and the
    device time by phase -- plan additions, support, pass A, pass B, walk, squares, 4-cliques, finish; GMX_GRAPHLETS_PHASES --
    from the first call, which builds the plan's additions, and from one warm call; then --reps calls without the phase
    clock: median and min-max of kernel_ms;
  * the whole call next to clustering() + ktruss(truss=False) + squares() + kclique(4) on the same handle, and the
    graphlet-specific phases (pass A + pass B + walk) next to clustering() + ktruss(truss=False);
  * the walk next to its GMX_GRAPHLETS_PLAIN=1 form (one work item per edge, one global atomic per match);
  * the totals-only query (per_vertex=False) next to the per-vertex one;
  * --sweep: the same call with GMX_GRAPHLETS_CAP and GMX_GRAPHLETS_LONG varied one at a time.

  graphlets_prof.py --scale 20 [--permute] [--symmetrize] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx graphlets: (plan .* totals [0-9 ]+)")
PHASES = ("plan", "support", "pass_a", "pass_b", "walk", "squares", "kclique", "finish")
PHASE = re.compile(r"gmx graphlets phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES))
KNOBS = ("GMX_GRAPHLETS_CAP", "GMX_GRAPHLETS_LONG", "GMX_GRAPHLETS_PLAIN", "GMX_GRAPHLETS_LOG", "GMX_GRAPHLETS_PHASES", "GMX_GRAPHLETS_NO_ORDER")
SWEEP = [{"cap": v} for v in (128, 256, 512, 1024)] + [{"long": v} for v in (256, 1024, 2048, 8192, 1 << 30)]


def call(g, per_vertex=True, phases=False, **knobs):
    """(gdv, totals, stats, the log line, ms by phase or None) of one call; the lines come from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, v in knobs.items():
        os.environ["GMX_GRAPHLETS_" + name.upper()] = str(v)
    os.environ["GMX_GRAPHLETS_LOG"] = "1"
    if phases:
        os.environ["GMX_GRAPHLETS_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            gdv, totals, st = g.graphlets(per_vertex=per_vertex)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or (phases and not p):
        sys.exit("graphlets_prof: no log line in %r" % text)
    return gdv, totals, st, m.group(1), dict(zip(PHASES, map(float, p.groups()))) if phases else None


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, reps, want=None, per_vertex=True, show=False, **knobs):
    gdv, totals, st, line, ph = call(g, per_vertex, phases=show, **knobs)   # warm-up
    if want is not None and (not np.array_equal(totals, want[1]) or (per_vertex and not np.array_equal(gdv, want[0]))):
        sys.exit("graphlets_prof: %s gives another result" % tag)
    if show:
        print("%s %s" % (tag, line))
        print("%s phases (one warm call under GMX_GRAPHLETS_PHASES): %s" % (tag, ", ".join("%s %.3f ms" % (p, ph[p]) for p in PHASES)))
    kms = [call(g, per_vertex, **knobs)[2]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms), (gdv, totals), ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_GRAPHLETS_CAP and GMX_GRAPHLETS_LONG, one at a time")
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
    g.triangle_counting_directed()   # builds the plan: the first graphlets call below adds the adjacency, the groups and the class lists
    _, _, st, line, ph = call(g, phases=True)
    print("%s first call %s" % (tag, line))
    print("%s first call: the adjacency and the groups %.3f ms (graph preprocessing, outside kernel_ms); kernel_ms %.3f (with the class lists of squares and kclique), d2h_ms %.3f" %
          (tag, ph["plan"], st["kernel_ms"], st["d2h_ms"]), flush=True)
    base, want, ph = runs(g, tag, a.reps, show=True)
    total, _, _ = runs(g, tag + " totals only", a.reps, want, per_vertex=False, show=True)
    print("%s totals only = %.2f x per vertex" % (tag, total / base))
    family = {"clustering": lambda: g.clustering()[5], "ktruss(truss=False)": lambda: g.ktruss(truss=False)[4], "squares": lambda: g.squares()[2],
              "kclique(4)": lambda: g.kclique(4)[2]}
    med = {}
    for name, f in family.items():
        f()
        ms = [f()["kernel_ms"] for _ in range(a.reps)]
        med[name] = statistics.median(ms)
        print("%s %s kernel_ms %s" % (tag, name, spread(ms)))
    four = sum(med.values())
    print("%s graphlets = %.2f x clustering + ktruss(truss=False) + squares + kclique(4) (%.3f ms)" % (tag, base / four, four))
    own, two = ph["pass_a"] + ph["pass_b"] + ph["walk"], med["clustering"] + med["ktruss(truss=False)"]
    print("%s pass A + pass B + walk (%.3f ms) = %.2f x clustering + ktruss(truss=False) (%.3f ms)" % (tag, own, own / two, two), flush=True)
    plain, _, pp = runs(g, tag + " GMX_GRAPHLETS_PLAIN=1", a.reps, want, show=True, plain=1)
    print("%s plain walk %.3f ms = %.2f x the staged walk (%.3f ms); the whole call %.2f x" % (tag, pp["walk"], pp["walk"] / ph["walk"], ph["walk"], plain / base), flush=True)
    if a.sweep:
        named = lambda knobs: " ".join("GMX_GRAPHLETS_%s=%s" % (n.upper(), v) for n, v in knobs.items())
        for knobs in SWEEP:
            ms, _, p = runs(g, "%s %s" % (tag, named(knobs)), a.reps, want, show=True, **knobs)
            print("%s %s = %.2f x the default; walk %.3f ms, pass A %.3f ms, pass B %.3f ms" % (tag, named(knobs), ms / base, p["walk"], p["pass_a"], p["pass_b"]), flush=True)
    g.free()


if __name__ == "__main__":
    main()
