#!/usr/bin/env python3
"""Route queries (gmx_route_*, bidir_dijkstra.gm) on RMAT-<scale> x 16 with weights 1 .. 100, or on a chain, in one process:

  * gmx_route_create: wall ms and the library's h2d_ms (upload, check, reverse-slot pairing and gathers of the weights);
  * --pairs N (default 64) queries on ONE route object, half of them from the top hub to random targets it reaches, half
    between random vertices: per query the wall clock and kernel_ms (a warm-up pass over all pairs, then --reps passes;
    median over the passes per pair, then median and worst over the pairs), rounds and slots per side from the library's
    GMX_ROUTE_LOG line;
  * the same queries with GMX_ROUTE_SIDES=forward (one-sided search with early exit), with a check that flag and cost agree;
  * gmx_sssp_path from the same sources (each distinct source once per pass): what a caller has without route queries --
    wall clock (the upload of the lengths included), kernel_ms and h2d_ms -- with a check that the costs agree;
  * --sweep: the default pass over GMX_ROUTE_TAIL = 0, 1024, 4096, 16384;
  * --chain N: a chain of N vertices with unit weights, 0 -> 3 N / 4, instead of RMAT (thousands of nearly empty rounds).

  route_prof.py --scale 22 [--permute] [--pairs 64] [--reps 3] [--sweep]
  route_prof.py --chain 4096 [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_ROUTE_SIDES", "GMX_ROUTE_TAIL")
LINE = re.compile(r"gmx route: V (\d+) E (\d+) src (-?\d+) dst (-?\d+) sides (both|forward); tail (\d+); rounds F (\d+) grid \+ (\d+) tail, "
                  r"R (\d+) grid \+ (\d+) tail in (\d+) launches; slots F (\d+) R (\d+); queued (\d+); found ([01]) cost (-?\d+) meet (-?\d+) "
                  r"hops (\d+); ms ([0-9.]+)")
FIELDS = ("V", "E", "src", "dst", "sides", "tail_from", "f_grid", "f_tail", "r_grid", "r_tail", "tail_launches", "f_slots", "r_slots", "queued",
          "found", "cost", "meet", "hops", "ms")


def pick_pairs(reach_from_hub, hub, V, n, seed=7):
    """n pairs: the first half hub -> a random vertex the hub reaches, the rest random -> random (src != dst)."""
    rng = np.random.default_rng(seed)
    reach = np.flatnonzero(reach_from_hub)
    reach = reach[reach != hub]
    pairs = [(hub, int(t)) for t in rng.choice(reach, n // 2)]
    while len(pairs) < n:
        s, t = (int(x) for x in rng.integers(0, V, 2))
        if s != t:
            pairs.append((s, t))
    return pairs


def query(r, src, dst, **env):
    """(found, cost, hops, stats, wall ms, fields of the library's line) of one query; the line is read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_ROUTE_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            found, cost, _, _, hops, st = r.query(src, dst, cap=64)
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS + ("GMX_ROUTE_LOG",):
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("route_prof: no log line in %r" % text)
    f = {k: (v if k == "sides" else float(v) if k == "ms" else int(v)) for k, v in zip(FIELDS, m.groups())}
    return found, cost, hops, st, wall, f


def passes(r, pairs, tag, reps, **env):
    """A warm-up pass, then reps passes over all pairs; prints the figures and returns [(found, cost)] per pair."""
    for s, t in pairs:
        query(r, s, t, **env)
    res = [[query(r, s, t, **env) for s, t in pairs] for _ in range(reps)]
    wall = [statistics.median(p[k][4] for p in res) for k in range(len(pairs))]
    kms = [statistics.median(p[k][3]["kernel_ms"] for p in res) for k in range(len(pairs))]
    spread = [max(p[k][4] for p in res) - min(p[k][4] for p in res) for k in range(len(pairs))]
    f = [x[5] for x in res[0]]
    med = lambda key: statistics.median(x[key] for x in f)
    print("%s: %d pairs x %d passes, %d found, tail from %d slots" % (tag, len(pairs), reps, sum(x["found"] for x in f), f[0]["tail_from"]))
    print("%s   wall ms per query: median %.3f  worst %.3f  (spread between passes: median %.3f, worst %.3f); kernel_ms: median %.3f  worst %.3f"
          % (tag, statistics.median(wall), max(wall), statistics.median(spread), max(spread), statistics.median(kms), max(kms)))
    print("%s   per query, median (worst): rounds F %d (%d) R %d (%d); slots F %d (%d) R %d (%d); tail launches %d (%d); hops %d (%d)"
          % (tag, med("f_grid") + med("f_tail"), max(x["f_grid"] + x["f_tail"] for x in f), med("r_grid") + med("r_tail"),
             max(x["r_grid"] + x["r_tail"] for x in f), med("f_slots"), max(x["f_slots"] for x in f), med("r_slots"), max(x["r_slots"] for x in f),
             med("tail_launches"), max(x["tail_launches"] for x in f), med("hops"), max(x["hops"] for x in f)), flush=True)
    half = len(pairs) // 2
    for name, sl in (("hub -> reachable", slice(0, half)), ("random -> random", slice(half, None))):
        if wall[sl]:
            print("%s   %s: wall ms median %.3f worst %.3f; slots F+R median %d" % (tag, name, statistics.median(wall[sl]), max(wall[sl]),
                  statistics.median(x["f_slots"] + x["r_slots"] for x in f[sl])), flush=True)
    return [(x[0], x[1]) for x in res[0]], statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="the default pass over GMX_ROUTE_TAIL")
    ap.add_argument("--chain", type=int, default=0, help="a chain of N vertices with unit weights instead of RMAT")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    sweep = [{"GMX_ROUTE_TAIL": str(v)} for v in (0, 1024, 4096, 16384)] if a.sweep else []
    if a.chain:
        V = a.chain
        g = gmx.Graph.upload(np.concatenate([np.arange(V), [V - 1]]).astype(np.int32), np.arange(1, V, dtype=np.int32))
        r = g.route(np.ones(V - 1, np.int32))
        for env in [{}] + sweep:
            for sides in ({}, {"GMX_ROUTE_SIDES": "forward"}):
                e = dict(env, **sides)
                passes(r, [(0, 3 * V // 4)], "chain-%d%s" % (V, "".join(" %s=%s" % kv for kv in e.items())), a.reps, **e)
        r.free()
        return
    V = 1 << a.scale
    base = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    begin = g.download(reverse=False)[0]
    hub = int(np.argmax(np.diff(begin)))
    weight = np.random.default_rng(1).integers(1, 101, g.E).astype(np.int32)
    pairs = pick_pairs(g.hop_dist(hub)[0] != gmx.INT_MAX, hub, V, a.pairs)
    t0 = time.perf_counter()
    r = g.route(weight)
    create = (time.perf_counter() - t0) * 1e3
    _, _, _, st = g.bidir_dijkstra(weight, *pairs[0])          # create + query + free: its h2d_ms is the create's device side
    print("%s V %d E %d hub %d: gmx_route_create %.1f ms wall, %.1f ms on the device (upload, check, pairing of the reverse slots, gathers)"
          % (base, V, g.E, hub, create, st["h2d_ms"]), flush=True)
    both, both_ms = passes(r, pairs, base + " both", a.reps)
    fwd, fwd_ms = passes(r, pairs, base + " forward", a.reps, GMX_ROUTE_SIDES="forward")
    print("%s   both / forward: %.2f x the wall clock; flags and costs %s" % (base, both_ms / fwd_ms, "agree" if both == fwd else "DIFFER"), flush=True)
    for env in sweep:
        passes(r, pairs, base + " both" + "".join(" %s=%s" % kv for kv in env.items()), a.reps, **env)
    r.free()
    # what a caller has today: the whole tree from every distinct source
    want = dict(zip(pairs, both))
    srcs = sorted({s for s, _ in pairs})
    os.environ["GMX_SSSP_PATH_SCHEDULE"] = "round"
    g.sssp_path(weight, hub)
    wall, kms, hms, ok = [], [], [], True
    for s in srcs:
        t0 = time.perf_counter()
        dist, _, _, st = g.sssp_path(weight, s)
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(st["kernel_ms"])
        hms.append(st["h2d_ms"])
        for (ps, pt), (found, cost) in want.items():
            if ps == s:
                ok = ok and (found, cost) == ((True, int(dist[pt])) if dist[pt] != gmx.INT_MAX else (False, None))
    print("%s gmx_sssp_path from the %d distinct sources: wall ms median %.3f worst %.3f; kernel_ms median %.3f worst %.3f; h2d_ms median %.3f; "
          "flags and costs %s" % (base, len(srcs), statistics.median(wall), max(wall), statistics.median(kms), max(kms), statistics.median(hms),
                                   "agree" if ok else "DIFFER"))
    print("%s   route query (both) / gmx_sssp_path: %.3f x the wall clock" % (base, both_ms / statistics.median(wall)), flush=True)
    g.free()


if __name__ == "__main__":
    main()
