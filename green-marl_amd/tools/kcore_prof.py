#!/usr/bin/env python3
"""gmx_kcore on RMAT-<scale>, in one process and on one graph:

  * the library's log line (levels, rounds, the entries the level scans read, grid and tail rounds, the largest core) and
    the device time by phase -- degrees, level scans, grid rounds, tail launches; hipEvents around steps that end in a
    read-back, GMX_KCORE_PHASES -- with the largest number of decrements one vertex received: a warm-up, then --reps
    calls; median and min-max of kernel_ms;
  * the yardstick "one sweep of the rows": kernel_ms of gmx_avg_teen_cnt on the same graph;
  * --sweep: the same call with GMX_KCORE_TAIL = 0, 256, 1024, 4096, 16384, 65536, 262144.

  kcore_prof.py --scale 24 [--permute] [--symmetrize] [--mode in|out|both] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx kcore: (V \d+ E \d+ mode \d reverse [01] levels (\d+) rounds (\d+) scanned (\d+) grid_rounds (\d+) tail_rounds (\d+) "
                  r"slots (\d+) max_core (\d+) top (\d+))")
PHASES = ("degrees", "scans", "grid", "tail")
PHASE = re.compile(r"gmx kcore phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES) + r", max_decrements (\d+)")
SWEEP = (0, 256, 1024, 4096, 16384, 65536, 262144)


def call(g, mode, tail=None):
    """(core, max_core, stats, the log line, ms by phase, the largest decrement count) of one call; the lines come from stderr."""
    os.environ.pop("GMX_KCORE_TAIL", None)
    if tail is not None:
        os.environ["GMX_KCORE_TAIL"] = str(tail)
    os.environ["GMX_KCORE_LOG"] = os.environ["GMX_KCORE_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            core, k, st = g.kcore(mode)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in ("GMX_KCORE_TAIL", "GMX_KCORE_LOG", "GMX_KCORE_PHASES"):
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or not p:
        sys.exit("kcore_prof: no log line in %r" % text)
    return core, k, st, m, dict(zip(PHASES, map(float, p.groups()[:4]))), int(p.group(5))


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, mode, reps, want=None, tail=None, phases=True):
    core, k, st, m, _, maxdec = call(g, mode, tail)   # warm-up
    if want is not None and not np.array_equal(core, want):
        sys.exit("kcore_prof: %s gives another result" % tag)
    if phases:
        print("%s %s" % (tag, m.group(1)))
        print("%s levels %s rounds %s scanned / V %.2f grid_rounds %s tail_rounds %s largest decrement count %d" % (
            tag, m.group(2), m.group(3), int(m.group(4)) / max(g.V, 1), m.group(5), m.group(6), maxdec))
    kms, ph = [], []
    for _ in range(reps):
        _, _, st, _, p, _ = call(g, mode, tail)
        kms.append(st["kernel_ms"])
        ph.append(p)
    if phases:
        for p in PHASES:
            print("%s   %-8s %s" % (tag, p, spread([x[p] for x in ph])))
    print("%s kernel_ms %s%s" % (tag, spread(kms), "" if phases else "  grid_rounds %s tail_rounds %s" % (m.group(5), m.group(6))), flush=True)
    return statistics.median(kms), core


def one_sweep(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one probe per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--mode", choices=("in", "out", "both"), default="in")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_KCORE_TAIL over %s" % (SWEEP,))
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s %s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "", a.mode)
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    base, want = runs(g, tag, a.mode, a.reps)
    sweep = one_sweep(g, tag, a.reps)
    print("%s kcore = %.1f x one sweep of the rows" % (tag, base / sweep))
    if a.sweep:
        best = None
        for t in SWEEP:
            ms, _ = runs(g, "%s GMX_KCORE_TAIL=%d" % (tag, t), a.mode, a.reps, want, t, phases=False)
            if best is None or ms < best[0]:
                best = (ms, t)
        print("%s the sweep's best: GMX_KCORE_TAIL=%d, %.3f ms = %.2f x the default" % (tag, best[1], best[0], best[0] / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
