#!/usr/bin/env python3
"""gmx_ktruss on RMAT-<scale> or on the triangulated N x N grid, in one process and on one graph:

  * the library's log line (levels, rounds, the entries the level scans read, grid and tail rounds, the largest truss
    number) and the device time by phase -- plan additions, support, level scans, grid rounds, tail launches, finish;
    hipEvents around steps that end in a read-back, GMX_KTRUSS_PHASES -- with the largest number of decrements one edge
    received: a warm-up, then --reps calls; median and min-max of kernel_ms;
  * kernel_ms of the support phase alone (truss=False) next to gmx_clustering's on the same plan: the same triangles, found
    per edge instead of per vertex;
  * the whole call next to gmx_kcore (mode both) and next to one sweep of the rows (gmx_avg_teen_cnt);
  * --sweep: the same call with GMX_KTRUSS_TAIL = 0, 256, 1024, 4096, 16384, 65536, 262144.

  ktruss_prof.py --scale 20 [--permute] [--symmetrize] [--reps 5] [--sweep]
  ktruss_prof.py --grid 1024 [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx ktruss: (plan V \d+ E \d+ up (\d+) order \w+ built \d adj_built \d; support \w+ triangles (\d+); levels (\d+) rounds (\d+) "
                  r"scanned (\d+) grid_rounds (\d+) tail_rounds (\d+) slots (\d+) max_truss (\d+) top (\d+))")
PHASES = ("plan", "support", "scans", "grid", "tail", "finish")
PHASE = re.compile(r"gmx ktruss phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES) + r", max_decrements (\d+)")
SWEEP = (0, 256, 1024, 4096, 16384, 65536, 262144)
KNOBS = ("GMX_KTRUSS_TAIL", "GMX_KTRUSS_LOG", "GMX_KTRUSS_PHASES")


def call(g, tail=None, truss=True):
    """(truss, support, stats, the log line, ms by phase, the largest decrement count) of one call; the lines come from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    if tail is not None:
        os.environ["GMX_KTRUSS_TAIL"] = str(tail)
    os.environ["GMX_KTRUSS_LOG"] = os.environ["GMX_KTRUSS_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            tr, su, k, n, st = g.ktruss(truss=truss)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or not p:
        sys.exit("ktruss_prof: no log line in %r" % text)
    return tr, su, st, m, dict(zip(PHASES, map(float, p.groups()[:len(PHASES)]))), int(p.group(len(PHASES) + 1))


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, reps, want=None, tail=None, phases=True, truss=True):
    tr, su, st, m, first, maxdec = call(g, tail, truss)   # warm-up (the first call on the graph also builds the plan's additions)
    if want is not None and not (np.array_equal(tr, want[0]) and np.array_equal(su, want[1])):
        sys.exit("ktruss_prof: %s gives another result" % tag)
    if phases:
        print("%s %s" % (tag, m.group(1)))
        print("%s edges %s triangles %s levels %s rounds %s scanned / edges %.2f grid_rounds %s tail_rounds %s slots / edges %.2f "
              "largest decrement count %d; plan additions %.3f ms" % (tag, m.group(2), m.group(3), m.group(4), m.group(5), int(m.group(6)) / max(int(m.group(2)), 1),
                                                                     m.group(7), m.group(8), int(m.group(9)) / max(int(m.group(2)), 1), maxdec, first["plan"]))
    kms, ph = [], []
    for _ in range(reps):
        _, _, st, _, p, _ = call(g, tail, truss)
        kms.append(st["kernel_ms"])
        ph.append(p)
    if phases:
        for p in PHASES[1:]:
            print("%s   %-8s %s" % (tag, p, spread([x[p] for x in ph])))
    print("%s kernel_ms %s%s" % (tag, spread(kms), "" if phases else "  grid_rounds %s tail_rounds %s" % (m.group(7), m.group(8))), flush=True)
    return statistics.median(kms), (tr, su)


def yardsticks(g, tag, reps):
    """kernel_ms of gmx_clustering (the same triangles per vertex), gmx_kcore mode both (the same peeling on vertices) and
    gmx_avg_teen_cnt (every slot read once)."""
    out = {}
    g.clustering()
    out["clustering"] = [g.clustering()[5]["kernel_ms"] for _ in range(reps)]
    g.kcore("both")
    out["kcore both"] = [g.kcore("both")[2]["kernel_ms"] for _ in range(reps)]
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    out["one sweep of the rows"] = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    for name, ms in out.items():
        print("%s %s kernel_ms %s" % (tag, name, spread(ms)), flush=True)
    return {k: statistics.median(v) for k, v in out.items()}


def triangulated_grid(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = i * n + j
    s = np.concatenate([v[:-1, :].ravel(), v[:, :-1].ravel(), v[:-1, :-1].ravel()])
    d = np.concatenate([v[1:, :].ravel(), v[:, 1:].ravel(), v[1:, 1:].ravel()])
    return n * n, s, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--grid", type=int, default=0, help="the triangulated N x N grid instead of RMAT")
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_KTRUSS_TAIL over %s" % (SWEEP,))
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    if a.grid:
        tag = "grid-%d" % a.grid
        g = gmx.Graph.from_edges(*triangulated_grid(a.grid))
    else:
        V = 1 << a.scale
        tag = "RMAT-%d%s%s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "")
        g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
        if a.symmetrize:
            s = g.symmetrize()
            g.free()
            g = s
    base, want = runs(g, tag, a.reps)
    sup_ms, _ = runs(g, tag + " support only", a.reps, phases=False, truss=False)
    y = yardsticks(g, tag, a.reps)
    print("%s support only = %.2f x gmx_clustering; ktruss = %.1f x gmx_kcore both = %.1f x one sweep of the rows" % (
        tag, sup_ms / y["clustering"], base / y["kcore both"], base / y["one sweep of the rows"]))
    if a.sweep:
        best = None
        for t in SWEEP:
            ms, _ = runs(g, "%s GMX_KTRUSS_TAIL=%d" % (tag, t), a.reps, want, t, phases=False)
            if best is None or ms < best[0]:
                best = (ms, t)
        print("%s the sweep's best: GMX_KTRUSS_TAIL=%d, %.3f ms = %.2f x the default" % (tag, best[1], best[0], best[0] / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
