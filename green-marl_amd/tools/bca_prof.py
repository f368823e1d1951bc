#!/usr/bin/env python3
"""The multi-source traversal (GMX_BCB_MSBFS=1) against the staged per-seed traversals (GMX_BCB_MSBFS=0) behind the same
entries, on RMAT-<scale>, in one process: a warm-up of each method with GMX_BCB_TRACE=1 (its trace lines are summed: batches
by path, levels, rows, slots, saturated visits), the bytes of the two compared, then --reps rounds that alternate the
methods; device time by events (stats.kernel_ms: from the first launch to the last, the host round trips of the
traversals included) and host wall time; median and min-max per method and the ratio of the medians.  A difference counts
only if it exceeds the larger min-max spread of the two methods.

  bca_prof.py --scale 16 --all            [--width 0] [--reps 3] [--permute]     gmx_bc_all, every vertex a source
  bca_prof.py --scale 24 --seeds 256      [--width 0] [--reps 3] [--permute]     gmx_bc_batch, K seeds (fixed rng, the top hub first)

Split of a run into kernels: a run of its own under `rocprofv3 --kernel-trace --stats -- bca_prof.py ... --only 1 --reps 1`
(no counters in that run); --only takes one method (0 or 1) and skips the comparison.  In a job script every such step
runs under its own `timeout` and the steps are chained with `&&`."""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

BATCH = re.compile(r"gmx bc_batch batch \d+: seeds \d+ width (\d+) depth (\d+) path (batched|per-seed) rows (\d+) short \+ (\d+) long, slots (\d+)")
MSBFS = re.compile(r"gmx bc_batch msbfs batch \d+: levels (\d+) rows (\d+) short \+ (\d+) long slots (\d+) saturated (\d+)")


def traced(call):
    """call() with the library's stderr lines caught: (result, text)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        os.environ["GMX_BCB_TRACE"] = "1"
        try:
            out = call()
        finally:
            os.environ.pop("GMX_BCB_TRACE")
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return out, f.read()


def summary(text):
    b = [m.groups() for m in BATCH.finditer(text)]
    m = [tuple(int(x) for x in g.groups()) for g in MSBFS.finditer(text)]
    s = "batches %d (%d batched, width %s), sweep rows %d short + %d long, sweep slots %d" % (
        len(b), sum(x[2] == "batched" for x in b), "/".join(sorted({x[0] for x in b})) or "-", sum(int(x[3]) for x in b), sum(int(x[4]) for x in b),
        sum(int(x[5]) for x in b))
    if m:
        s += "; traversal levels %d, rows %d short + %d long, slots %d, saturated visits %d" % tuple(sum(x[i] for x in m) for i in range(5))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--all", action="store_true", help="gmx_bc_all: every vertex a source")
    ap.add_argument("--seeds", type=int, default=256, help="gmx_bc_batch with this many seeds (without --all)")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="one method only (GMX_BCB_MSBFS value), for a run under the profiler")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = 1 << a.scale
    g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.all:
        tag = "RMAT-%d%s all sources width %d" % (a.scale, "p" if a.permute else "", a.width)
        seeds = None
    else:
        deg = np.diff(g.download(reverse=False)[0])
        seeds = np.random.default_rng(a.scale).integers(0, N, a.seeds).astype(np.int32)
        seeds[0] = int(np.argmax(deg))
        tag = "RMAT-%d%s K=%d width %d" % (a.scale, "p" if a.permute else "", a.seeds, a.width)

    def run(method):
        os.environ["GMX_BCB_MSBFS"] = str(method)
        t0 = time.perf_counter()
        out, st = g.bc_all(True, a.width) if a.all else g.bc_batch(seeds, True, a.width)
        return out, st, (time.perf_counter() - t0) * 1e3

    methods = (0, 1) if a.only is None else (a.only,)
    names = {0: "staged", 1: "msbfs"}
    outs = {}
    for m in methods:                                   # warm-up of each, traced
        (out, st, _), text = traced(lambda: run(m))
        outs[m] = out
        print("%s %-6s: reached %d, %s" % (tag, names[m], st["vertices_reached"], summary(text)), flush=True)
    if len(outs) == 2:
        same = outs[0].tobytes() == outs[1].tobytes()
        print("%s: bytes of the two methods %s" % (tag, "EQUAL" if same else "DIFFER"), flush=True)
        if not same:
            sys.exit("bca_prof: the two methods differ")
    dev = {m: [] for m in methods}
    wall = {m: [] for m in methods}
    for _ in range(a.reps):
        for m in methods:                               # alternating
            _, st, w = run(m)
            dev[m].append(st["kernel_ms"])
            wall[m].append(w)
    for what, ms in (("device", dev), ("wall", wall)):
        for m in methods:
            print("%s %-6s %-6s median %10.2f ms  min %10.2f  max %10.2f" % (tag, names[m], what, statistics.median(ms[m]), min(ms[m]), max(ms[m])), flush=True)
        if len(methods) == 2:
            spread = max(max(ms[m]) - min(ms[m]) for m in methods)
            d = statistics.median(ms[0]) - statistics.median(ms[1])
            print("%s %s: staged / msbfs = %.3f; difference %.2f ms, larger min-max spread %.2f ms: %s" % (
                tag, what, statistics.median(ms[0]) / statistics.median(ms[1]), d, spread,
                "no difference that counts" if abs(d) <= spread else ("msbfs faster" if d > 0 else "staged faster")), flush=True)
    g.free()


if __name__ == "__main__":
    main()
