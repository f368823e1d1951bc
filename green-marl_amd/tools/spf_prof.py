#!/usr/bin/env python3
"""gmx_sssp_path_f64 (sssp_path_adj.gm) on RMAT-<scale> x 16 from its top hub, or on a chain, in one process:

  * costs equal to integer lengths 1 .. 100, double(len): the call without a target next to gmx_sssp_path (round schedule) on
    the same graph and lengths -- kernel_ms (a warm-up, then --reps calls; median and min-max), rounds of both, the ratio, and
    a check that the distances agree;
  * the same call with `end` at the median finite distance: kernel_ms, iterations and edges_examined against the call
    without a target;
  * the host-clock split of a call into grid rounds and tail launches (the library's GMX_SSSP_F64_LOG line), and the cost
    of a grid round;
  * --sweep: the same over GMX_SSSP_F64_TAIL = 0, 1024, 4096, 16384;
  * --chain N: a chain of N vertices with unit costs and `end` at 3 N / 4 instead of RMAT (thousands of nearly empty rounds).

  spf_prof.py --scale 20 [--permute] [--reps 5] [--sweep]
  spf_prof.py --chain 4096 [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_SSSP_F64_TAIL",)
LINE = re.compile(r"gmx sssp_path_f64: V (\d+) E (\d+) root (-?\d+) end (-?\d+); tail (\d+); rounds (\d+): (\d+) grid \+ (\d+) tail in (\d+) launches; "
                  r"queued (\d+); slots (\d+) grid \+ (\d+) tail; ms ([0-9.]+) grid \+ ([0-9.]+) tail")
FIELDS = ("V", "E", "root", "end", "tail_from", "rounds", "grid_rounds", "tail_rounds", "tail_launches", "queued", "grid_slots", "tail_slots",
          "grid_ms", "tail_ms")
DBL_MAX = float(np.finfo(np.float64).max)


def call(g, cost, root, end, **env):
    """(dist, prev_node, prev_edge, stats, fields of the library's line) of one call; the line is read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_SSSP_F64_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = g.sssp_path_f64(cost, root, end)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS + ("GMX_SSSP_F64_LOG",):
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("spf_prof: no log line in %r" % text)
    return out + ({k: (float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, m.groups())},)


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, cost, root, end, tag, reps, **env):
    call(g, cost, root, end, **env)                          # warm-up
    res = [call(g, cost, root, end, **env) for _ in range(reps)]
    st, f = res[0][3], res[0][4]
    kms = [r[3]["kernel_ms"] for r in res]
    grid = statistics.median([r[4]["grid_ms"] for r in res])
    tail = statistics.median([r[4]["tail_ms"] for r in res])
    print("%s end %d: rounds %d = %d grid + %d tail in %d launches (tail from %d slots), queue entries %d, slots %d (%.2f x E)"
          % (tag, end, f["rounds"], f["grid_rounds"], f["tail_rounds"], f["tail_launches"], f["tail_from"], st["vertices_reached"],
             st["edges_examined"], st["edges_examined"] / max(f["E"], 1)))
    print("%s   kernel_ms %s; host clock %.3f ms grid (%.1f us per grid round) + %.3f ms tail (%.1f us per tail round)"
          % (tag, spread(kms), grid, 1e3 * grid / max(f["grid_rounds"], 1), tail, 1e3 * tail / max(f["tail_rounds"], 1)), flush=True)
    return statistics.median(kms), st, res[0][0]


def median_end(dist):
    fin = np.flatnonzero(dist < DBL_MAX)
    order = fin[np.argsort(dist[fin], kind="stable")]
    return int(order[len(order) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the same over GMX_SSSP_F64_TAIL")
    ap.add_argument("--chain", type=int, default=0, help="a chain of N vertices with unit costs instead of RMAT")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = gmx.GMX_GRAPH_NO_REVERSE
    sweep = [{}] + ([{"GMX_SSSP_F64_TAIL": str(v)} for v in (0, 1024, 4096, 16384)] if a.sweep else [])
    if a.chain:
        V = a.chain
        g = gmx.Graph.upload(np.concatenate([np.arange(V), [V - 1]]).astype(np.int32), np.arange(1, V, dtype=np.int32), flags=N)
        cost = np.ones(V - 1)
        for env in sweep:
            tag = "chain-%d%s" % (V, "".join(" %s=%s" % kv for kv in env.items()))
            runs(g, cost, 0, 3 * V // 4, tag, a.reps, **env)
        return
    V = 1 << a.scale
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute, flags=N)
    begin = g.download(reverse=False)[0]
    root = int(np.argmax(np.diff(begin)))
    length = np.random.default_rng(1).integers(1, 101, g.E).astype(np.int32)
    cost = length.astype(np.float64)
    os.environ["GMX_SSSP_PATH_SCHEDULE"] = "round"
    g.sssp_path(length, root)
    ref = [g.sssp_path(length, root) for _ in range(a.reps)]
    ims = [r[3]["kernel_ms"] for r in ref]
    base = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    print("%s gmx_sssp_path (int32, round schedule): rounds %d, slots %d, kernel_ms %s"
          % (base, ref[0][3]["iterations"], ref[0][3]["edges_examined"], spread(ims)), flush=True)
    for env in sweep:
        tag = base + "".join(" %s=%s" % kv for kv in env.items())
        ms, st, dist = runs(g, cost, root, -1, tag, a.reps, **env)
        want = np.where(ref[0][0] == gmx.INT_MAX, DBL_MAX, ref[0][0].astype(np.float64))
        print("%s   %.2f x gmx_sssp_path; distances %s" % (tag, ms / statistics.median(ims), "agree" if np.array_equal(dist, want) else "DIFFER"))
        end = median_end(dist)
        pms, pst, _ = runs(g, cost, root, end, tag, a.reps, **env)
        print("%s   end at the median distance: %.2f x the time, %d of %d rounds, %.2f x the slots of the call without a target"
              % (tag, pms / ms, pst["iterations"], st["iterations"], pst["edges_examined"] / max(st["edges_examined"], 1)), flush=True)
    g.free()


if __name__ == "__main__":
    main()
