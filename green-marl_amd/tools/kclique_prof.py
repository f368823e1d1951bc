#!/usr/bin/env python3
"""gmx_kclique on RMAT-<scale>, in one process and on one graph:

  * the library's log line (the size classes, the batches, the cliques) and the device time by phase -- plan additions,
    matrices, each class's count kernel, finish; GMX_KCLIQUE_PHASES, which launches every class once more to time its matrix
    -- from one call; then a warm-up and --reps calls without the phase clock: median and min-max of kernel_ms;
  * the total-only query (per_vertex=False) next to the per-vertex one;
  * k = 3 next to gmx_clustering on the same plan: the same triangles and the same tri[];
  * the LDS counters next to GMX_KCLIQUE_PLAIN=1 (every credit a global atomic);
  * --sweep: the same call with GMX_KCLIQUE_WAVE=0 and with GMX_KCLIQUE_CAP = 64, 128, 256, 512.

  kclique_prof.py --scale 20 [--permute] [--symmetrize] [--k 4] [--reps 5] [--sweep] [--skip-plain]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx kclique: (plan .* cliques \d+)")
PHASES = ("plan", "matrices", "wave", "small", "large", "global", "finish")
PHASE = re.compile(r"gmx kclique phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES))
KNOBS = ("GMX_KCLIQUE_CAP", "GMX_KCLIQUE_WAVE", "GMX_KCLIQUE_PLAIN", "GMX_KCLIQUE_LOG", "GMX_KCLIQUE_PHASES")


def call(g, k, per_vertex=True, phases=False, **knobs):
    """(count, cliques, stats, the log line, ms by phase or None) of one call; the lines come from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, v in knobs.items():
        os.environ["GMX_KCLIQUE_" + name.upper()] = str(v)
    os.environ["GMX_KCLIQUE_LOG"] = "1"
    if phases:
        os.environ["GMX_KCLIQUE_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            cnt, n, st = g.kclique(k, per_vertex=per_vertex)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or (phases and not p):
        sys.exit("kclique_prof: no log line in %r" % text)
    return cnt, n, st, m.group(1), dict(zip(PHASES, map(float, p.groups()))) if phases else None


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, k, reps, want=None, per_vertex=True, show=False, **knobs):
    cnt, n, st, line, ph = call(g, k, per_vertex, phases=show, **knobs)   # warm-up (the first call on the graph also builds the plan's additions)
    if want is not None and (n != want[1] or (per_vertex and not np.array_equal(cnt, want[0]))):
        sys.exit("kclique_prof: %s gives another result" % tag)
    if show:
        print("%s %s" % (tag, line))
        print("%s phases (one call under GMX_KCLIQUE_PHASES): %s" % (tag, ", ".join("%s %.3f ms" % (p, ph[p]) for p in PHASES)))
    kms = [call(g, k, per_vertex, **knobs)[2]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms), (cnt, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_KCLIQUE_WAVE=0 and GMX_KCLIQUE_CAP over 64 .. 512")
    ap.add_argument("--skip-plain", action="store_true", help="leave out the GMX_KCLIQUE_PLAIN=1 runs (a global atomic per clique and member)")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s k=%d" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "", a.k)
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    base, want = runs(g, tag, a.k, a.reps, show=True)
    total, _ = runs(g, tag + " total only", a.k, a.reps, want, per_vertex=False)
    print("%s total only = %.2f x per vertex" % (tag, total / base))
    if a.k == 3:
        tri, _, _, T, _, _ = g.clustering()
        if T != want[1] or not np.array_equal(tri, want[0]):
            sys.exit("kclique_prof: k = 3 is not gmx_clustering's tri[]")
        lcc = [g.clustering()[5]["kernel_ms"] for _ in range(a.reps)]
        print("%s gmx_clustering kernel_ms %s" % (tag, spread(lcc)))
        print("%s k = 3 = %.2f x gmx_clustering (the same tri[], %d triangles)" % (tag, base / statistics.median(lcc), T))
    if not a.skip_plain:
        plain, _ = runs(g, tag + " GMX_KCLIQUE_PLAIN=1", a.k, a.reps, want, plain=1)
        print("%s plain = %.2f x the LDS counters" % (tag, plain / base), flush=True)
    if a.sweep:
        for knobs in ({"wave": 0}, {"cap": 64}, {"cap": 128}, {"cap": 256}, {"cap": 512}):
            name = " ".join("GMX_KCLIQUE_%s=%s" % (n.upper(), v) for n, v in knobs.items())
            ms, _ = runs(g, "%s %s" % (tag, name), a.k, a.reps, want, show=True, **knobs)
            print("%s %s = %.2f x the default" % (tag, name, ms / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
