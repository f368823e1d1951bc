#!/usr/bin/env python3
"""gmx_msf on RMAT-<scale> with weights 1 .. 100, in one process and on one graph:

  * the library's log line (rounds, grid and tail rounds, slots, the forest) and kernel_ms of the call as it runs by
    default: a warm-up, then --reps calls; median and min-max; the same with the component array;
  * one call with GMX_MSF_PHASES: per round the list, its slots / E, the slots selected, the device time of find, hook and
    next and the largest number of atomics one tree's word received; the tail launch; the finish (this mode synchronises
    at every step: its times add up to more than an unprofiled call);
  * next to it, on the same graph: kernel_ms of gmx_wcc, and of gmx_avg_teen_cnt as "one sweep of the rows";
  * --sweep: the call with GMX_MSF_TAIL = 0, 256, 1024, 4096, 16384, 65536, 262144, 1048576.

  msf_prof.py --scale 24 [--permute] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx msf: (V \d+ E \d+ reverse [01] rounds (\d+) grid_rounds (\d+) tail_rounds (\d+) slots (\d+) forest_edges (\d+) weight (-?\d+) comps (\d+))")
ROUND = re.compile(r"gmx msf round (\d+): list (\d+) slots (\d+) selected (\d+) find ([0-9.]+) ms hook ([0-9.]+) ms next ([0-9.]+) ms max_atomics (\d+)")
TAIL = re.compile(r"gmx msf tail: list (\d+) slots (\d+) rounds (\d+) read (\d+) tail ([0-9.]+) ms")
FINISH = re.compile(r"gmx msf finish: components ([0-9.]+) ms")
SWEEP = (0, 256, 1024, 4096, 16384, 65536, 262144, 1048576)


def call(g, w, components=False, tail=None, phases=False):
    """(the outputs of one call, what it wrote to stderr)."""
    os.environ.pop("GMX_MSF_TAIL", None)
    os.environ.pop("GMX_MSF_PHASES", None)
    if tail is not None:
        os.environ["GMX_MSF_TAIL"] = str(tail)
    if phases:
        os.environ["GMX_MSF_PHASES"] = "1"
    os.environ["GMX_MSF_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = g.msf(w, components=components)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in ("GMX_MSF_TAIL", "GMX_MSF_LOG", "GMX_MSF_PHASES"):
        os.environ.pop(name, None)
    if not LINE.search(text):
        sys.exit("msf_prof: no log line in %r" % text)
    return out, text


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, w, tag, reps, want=None, components=False, tail=None):
    out, text = call(g, w, components, tail)   # warm-up
    if want is not None and out[0].tobytes() != want.tobytes():
        sys.exit("msf_prof: %s gives another forest" % tag)
    m = LINE.search(text)
    kms = [call(g, w, components, tail)[0][-1]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s  grid_rounds %s tail_rounds %s" % (tag, spread(kms), m.group(3), m.group(4)), flush=True)
    return statistics.median(kms), out[0], m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_MSF_TAIL over %s" % (SWEEP,))
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    w = np.random.default_rng(1997).integers(1, 101, g.E).astype(np.int32)
    base, want, m = runs(g, w, tag, a.reps)
    print("%s %s" % (tag, m.group(1)))
    runs(g, w, tag + " with comp", a.reps, want, components=True)
    _, text = call(g, w, components=True, phases=True)
    for r in ROUND.finditer(text):
        print("%s   round %s: list %9s slots / E %6.3f selected %9s find %8.3f ms hook %7.3f ms next %7.3f ms largest atomic count %s" % (
            tag, r.group(1), r.group(2), int(r.group(3)) / max(g.E, 1), r.group(4), float(r.group(5)), float(r.group(6)), float(r.group(7)), r.group(8)))
    t = TAIL.search(text)
    if t:
        print("%s   tail: list %s slots %s rounds %s (the last, empty one included) slots read %s, %.3f ms" % (tag, t.group(1), t.group(2), t.group(3), t.group(4),
                                                                                                        float(t.group(5))))
    f = FINISH.search(text)
    if f:
        print("%s   finish (components) %.3f ms" % (tag, float(f.group(1))))
    g.wcc()
    wms = [g.wcc()[2]["kernel_ms"] for _ in range(a.reps)]
    print("%s gmx_wcc kernel_ms %s" % (tag, spread(wms)))
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    sms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(a.reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(sms)))
    print("%s msf = %.1f x gmx_wcc = %.1f x one sweep of the rows" % (tag, base / statistics.median(wms), base / statistics.median(sms)), flush=True)
    if a.sweep:
        best = None
        for t in SWEEP:
            ms, _, _ = runs(g, w, "%s GMX_MSF_TAIL=%d" % (tag, t), a.reps, want, tail=t)
            if best is None or ms < best[0]:
                best = (ms, t)
        print("%s the sweep's best: GMX_MSF_TAIL=%d, %.3f ms = %.2f x the default" % (tag, best[1], best[0], best[0] / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
