#!/usr/bin/env python3
"""gmx_random_bipartite_matching on the bipartite double cover of RMAT-<scale> (2 V vertices, vertex v < V left with the
graph's row v shifted by + V), or on a fan-in graph next to a chain of equal E, in one process:

  * per grid round: live lefts, slots of their rows, proposals, touched rights and host-clock ms (the library's GMX_RBM_LOG=2
    lines, one call);
  * rounds (grid + tail), matched, proposals, slots, and the host-clock ms of a call split into grid rounds and the tail
    launch, next to kernel_ms: a warm-up, then --reps calls; median and min-max;
  * the yardstick "one pass over the edges": kernel_ms of gmx_avg_teen_cnt on the same graph (same E, forward CSR only), and
    round 1's ms as a multiple of it;
  * --sweep: the same over GMX_RBM_TAIL;
  * --fanin K: K lefts with one edge each to ONE right (every proposal of round 1 hits one address) next to a chain cover of
    K edges (K lefts, K distinct rights): the difference of their first rounds is the price of the contended address.

  match_prof.py --scale 20 [--permute] [--reps 5] [--sweep]
  match_prof.py --fanin 1048576"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_RBM_TAIL",)
LINE = re.compile(r"gmx random_bipartite_matching: V (\d+) E (\d+) lefts (\d+); tail (\d+); rounds (\d+) grid \+ (\d+) tail; matched (\d+); "
                  r"proposals (\d+) slots (\d+); ms ([0-9.]+) grid \+ ([0-9.]+) tail")
FIELDS = ("V", "E", "lefts", "tail_from", "grid_rounds", "tail_rounds", "matched", "proposals", "slots", "grid_ms", "tail_ms")
ROUND = re.compile(r"gmx random_bipartite_matching round (\d+): live (\d+) slots (\d+) proposals (\d+) touched (\d+) ms ([0-9.]+)")


def call(g, left, level="1", **env):
    """(match, count, stats, fields of the library's line, its per-round lines) of one call; the lines are read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_RBM_LOG"] = level
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            match, cnt, st = g.random_bipartite_matching(left)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS + ("GMX_RBM_LOG",):
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("match_prof: no log line in %r" % text)
    f = {k: (float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, m.groups())}
    return match, cnt, st, f, [tuple(float(x) if "." in x else int(x) for x in r) for r in ROUND.findall(text)]


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, left, tag, reps, **env):
    fs, kms = [], []
    for _ in range(reps):
        _, _, st, f, _ = call(g, left, **env)
        fs.append(f)
        kms.append(st["kernel_ms"])
    f = fs[0]
    print("%s rounds %d grid + %d tail (tail from %d slots)" % (tag, f["grid_rounds"], f["tail_rounds"], f["tail_from"]))
    for k in ("grid_ms", "tail_ms"):
        print("%s %-9s %s" % (tag, k, spread([x[k] for x in fs])))
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms)


def one_pass(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one gather and one add per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one pass over E (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)
    return statistics.median(ms)


def profile(g, left, tag, reps, sweep):
    call(g, left)                                            # warm-up
    match, cnt, st, f, rounds = call(g, left, level="2")
    print("%s V %d E %d lefts %d: matched %d, rounds %d grid + %d tail, proposals %d (%.2f x E), slots %d (%.2f x E)"
          % (tag, f["V"], f["E"], f["lefts"], cnt, f["grid_rounds"], f["tail_rounds"], f["proposals"], f["proposals"] / max(f["E"], 1),
             f["slots"], f["slots"] / max(f["E"], 1)))
    for r, live, slots, props, touched, ms in rounds:
        print("%s   round %2d: live %10d slots %11d proposals %11d touched %10d  %9.3f ms" % (tag, r, live, slots, props, touched, ms))
    total = runs(g, left, tag, reps)
    first = []
    for _ in range(reps):
        rr = call(g, left, level="2")[4]
        if rr:
            first.append(rr[0][5])
    base = one_pass(g, tag, reps)
    if first:
        print("%s round 1 %s = %.2f x one pass; whole call %.2f x one pass" % (tag, spread(first), statistics.median(first) / base, total / base),
              flush=True)
    if sweep:
        for v in (0, 256, 4096, 65536, 1048576):
            runs(g, left, "%s GMX_RBM_TAIL=%d" % (tag, v), max(3, reps), GMX_RBM_TAIL=str(v))
    return total, (statistics.median(first) if first else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the split over GMX_RBM_TAIL")
    ap.add_argument("--fanin", type=int, default=0, help="K lefts, one right, next to a chain of K edges, instead of RMAT")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = gmx.GMX_GRAPH_NO_REVERSE
    if a.fanin:
        K = a.fanin
        left = np.zeros(2 * K, np.uint8)
        left[:K] = 1
        begin = np.concatenate([np.arange(K + 1), np.full(K, K)]).astype(np.int32)
        totals = {}
        for name, idx in (("fan-in", np.full(K, 2 * K - 1, np.int32)), ("chain", (K + np.arange(K)).astype(np.int32))):
            g = gmx.Graph.upload(begin, idx, flags=N)
            totals[name] = profile(g, left, "%s-%d" % (name, K), a.reps, False)
            g.free()
        (fa, f1), (ca, c1) = totals["fan-in"], totals["chain"]
        print("round 1: fan-in %.3f ms - chain %.3f ms = %.3f ms for one contended address (%d proposals); whole call: %.3f ms - %.3f ms "
              "(the fan-in graph runs a second, silent round)" % (f1, c1, f1 - c1, K, fa, ca))
        return
    V = 1 << a.scale
    tag = "RMAT-%d%s cover" % (a.scale, "p" if a.permute else "")
    r = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute, flags=N)
    begin, idx, _, _ = r.download(reverse=False)
    r.free()
    idx += V
    begin = np.concatenate([begin, np.full(V, begin[V], np.int32)]).astype(np.int32)
    g = gmx.Graph.upload(begin, idx, flags=N)
    del begin, idx
    left = np.zeros(2 * V, np.uint8)
    left[:V] = 1
    profile(g, left, tag, a.reps, a.sweep)
    g.free()


if __name__ == "__main__":
    main()
