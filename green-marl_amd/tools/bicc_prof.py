#!/usr/bin/env python3
"""gmx_biconnected on RMAT-<scale> or on an N x N grid, in one process:

  * the library's GMX_BICC_LOG line and its GMX_BICC_PHASES line (device time of forest, walks and finish; that mode
    synchronises at every phase) of one call;
  * kernel_ms of gmx_biconnected next to gmx_wcc (whose forest it starts from) and next to gmx_conduct (one sweep of the
    rows) on the same graph: a warm-up of each, then --reps rounds that alternate them; median and min-max;
  * the same with GMX_BICC_SKIP=0 (no jumps), where the cursor moves are a number of the graph alone;
  * --sweep: kernel_ms, cursor moves and jumps over GMX_BICC_WALKS, and kernel_ms over GMX_BICC_TAIL.

  bicc_prof.py --scale 20 [--permute] [--symmetrize] [--reps 5] [--sweep]
  bicc_prof.py --grid 1024 [--reps 3] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_BICC_TAIL", "GMX_BICC_SKIP", "GMX_BICC_WALKS", "GMX_BICC_PHASES")
FIELDS = ("V", "E", "levels", "roots", "tree", "walks", "steps", "jumps", "links", "grid_levels", "tail_levels", "blocks", "bridges", "artic", "tecc")
LINE = re.compile("gmx bicc: " + " ".join(r"%s (?P<%s>-?\d+)" % (f, f) for f in FIELDS))
PHASES = re.compile(r"gmx bicc phases: .*")


def call(g, **env):
    """(the four counts, kernel_ms, the log line, its fields, the phases line or None) of one gmx_biconnected call with the
    given knobs; no array is downloaded.  The lines are read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_BICC_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = g.biconnected(bridges=False, artic=False, blocks=False, tecc=False)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS:
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("bicc_prof: no log line in %r" % text)
    ph = PHASES.search(text)
    return res[4:8], res[8]["kernel_ms"], m.group(0), {k: int(v) for k, v in m.groupdict().items()}, ph.group(0) if ph else None


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f  (%d runs)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def grid_graph(gmx, n):
    v = np.arange(n * n, dtype=np.int32).reshape(n, n)
    s = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    d = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return gmx.Graph.from_edges(n * n, s, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--grid", type=int, default=0, help="an N x N grid instead of RMAT")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="GMX_BICC_WALKS and GMX_BICC_TAIL, one at a time")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    if a.grid:
        tag = "grid-%d" % a.grid
        g = grid_graph(gmx, a.grid)
    else:
        N = 1 << a.scale
        tag = "RMAT-%d%s%s" % (a.scale, "p" if a.permute else "", " symmetrised" if a.symmetrize else "")
        g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
        if a.symmetrize:
            s = g.symmetrize()
            g.free()
            g = s
    counts, _, line, f, _ = call(g)   # warm-up
    print(line)
    print("%s %s" % (tag, call(g, GMX_BICC_PHASES="1")[4]))
    print("%s blocks %d bridges %d articulation points %d 2-edge-connected components %d; %.2f moves per walk, %.1f %% of them jumps" % (
        (tag,) + tuple(counts) + (f["steps"] / max(f["walks"], 1), 100.0 * f["jumps"] / max(f["steps"], 1))), flush=True)
    member = np.zeros(g.V, np.int32)
    g.wcc()
    g.conduct(member, 0)
    c0, _, _, f0, ph0 = call(g, GMX_BICC_SKIP="0", GMX_BICC_PHASES="1")
    assert c0 == counts, (c0, counts)
    print("%s without jumps: %d moves (%.2f per walk); %s" % (tag, f0["steps"], f0["steps"] / max(f0["walks"], 1), ph0))
    ms = {"biconnected": [], "biconnected, no jumps": [], "wcc": [], "conduct (one sweep of the rows)": []}
    for _ in range(a.reps):
        ms["biconnected"].append(call(g)[1])
        ms["biconnected, no jumps"].append(call(g, GMX_BICC_SKIP="0")[1])
        ms["wcc"].append(g.wcc()[2]["kernel_ms"])
        ms["conduct (one sweep of the rows)"].append(g.conduct(member, 0)[1]["kernel_ms"])
    for k, v in ms.items():
        print("%s %-32s kernel %s" % (tag, k, spread(v)))
    print("%s biconnected / wcc = %.2f" % (tag, statistics.median(ms["biconnected"]) / max(statistics.median(ms["wcc"]), 1e-9)), flush=True)
    if a.sweep:
        for v in (0, 1 << 20, 1 << 18, 1 << 16, 1 << 14, 1 << 12, 1 << 10):
            if v and g.E // v > 20000:
                continue   # (tens of thousands of launches: not a candidate)
            r = [call(g, GMX_BICC_WALKS=str(v)) for _ in range(max(3, a.reps))]
            assert all(x[0] == counts for x in r)
            print("%s GMX_BICC_WALKS=%-8d kernel %s  moves %d jumps %d" % (tag, v, spread([x[1] for x in r]), r[-1][3]["steps"], r[-1][3]["jumps"]), flush=True)
        for v in (0, 256, 1024, 4096, 16384):
            r = [call(g, GMX_BICC_TAIL=str(v)) for _ in range(max(3, a.reps))]
            print("%s GMX_BICC_TAIL=%-8d  kernel %s  grid_levels %d tail_levels %d" % (tag, v, spread([x[1] for x in r]), r[-1][3]["grid_levels"],
                                                                                   r[-1][3]["tail_levels"]), flush=True)
    g.free()


if __name__ == "__main__":
    main()
