#!/usr/bin/env python3
"""gmx_louvain on RMAT-<scale>, in one process and on one graph:

  * the library's log line (levels, rounds, rollbacks, the size of every level) and, from one call under GMX_LOUVAIN_PHASES,
    the device time of every level's contraction and of every round's evaluate and commit-measure-judge-undo launches, with
    their sums and shares; then a warm-up and --reps calls without the phase clock: median and min-max of kernel_ms;
  * ms per level and per half-round of level 0;
  * gmx_communities (ms per round), gmx_wcc and one sweep of the rows (gmx_avg_teen_cnt) on the same graph, and the ratios;
  * --sweep: the same call with GMX_LOUVAIN_WAVE_MIN, GMX_LOUVAIN_BLOCK_MIN and GMX_LOUVAIN_LDS_SLOTS at other values.

  louvain_prof.py --scale 20 [--permute] [--symmetrize] [--reps 5] [--sweep] [--weighted]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx louvain: (V .* overflowed \d+)")
LEVEL = re.compile(r"gmx louvain level (\d+): n (\d+) nnz (\d+) contract ([0-9.]+) ms")
ROUND = re.compile(r"gmx louvain level (\d+) round (\d+): kept (\d+) rollbacks (\d+) overflowed (\d+) evaluate ([0-9.]+) ms judge ([0-9.]+) ms")
KNOBS = ("GMX_LOUVAIN_WAVE_MIN", "GMX_LOUVAIN_BLOCK_MIN", "GMX_LOUVAIN_LDS_SLOTS", "GMX_LOUVAIN_LOG", "GMX_LOUVAIN_PHASES")


def call(g, weight, phases=False, **knobs):
    """(result, the log line, the stderr text) of one call."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, v in knobs.items():
        os.environ["GMX_LOUVAIN_" + name.upper()] = str(v)
    os.environ["GMX_LOUVAIN_LOG"] = "1"
    if phases:
        os.environ["GMX_LOUVAIN_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = g.louvain(weight)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m = LINE.search(text)
    if not m:
        sys.exit("louvain_prof: no log line in %r" % text)
    return out, m.group(1), text


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1:5] == b[1:5] and all(a[5][k] == b[5][k] for k in ("iterations", "vertices_reached", "edges_examined"))


def runs(g, weight, tag, reps, want=None, show=False, **knobs):
    out, line, text = call(g, weight, phases=show, **knobs)
    if want is not None and not same(out, want):
        sys.exit("louvain_prof: %s gives another result" % tag)
    if show:
        print("%s %s" % (tag, line))
        print("%s Q %.6f comms %d levels %d" % (tag, out[3], out[1], out[2]))
        levels = [(int(a), int(b), int(c), float(d)) for a, b, c, d in LEVEL.findall(text)]
        rounds = [(int(a), int(b), int(c), int(d), int(e), float(f), float(h)) for a, b, c, d, e, f, h in ROUND.findall(text)]
        ev, ju, co = sum(r[5] for r in rounds), sum(r[6] for r in rounds), sum(l[3] for l in levels)
        for lv, n, nnz, cms in levels:
            mine = [r for r in rounds if r[0] == lv]
            e, j = sum(r[5] for r in mine), sum(r[6] for r in mine)
            print("%s level %d: n %d nnz %d contract %.3f ms rounds %d evaluate %.3f ms judge %.3f ms = %.3f ms per half-round; overflowed %d rollbacks %d"
                  % (tag, lv, n, nnz, cms, len(mine), e, j, (e + j) / max(1, 2 * len(mine)), sum(r[4] for r in mine), sum(r[3] for r in mine)))
        for r in rounds:
            if r[0] == 0:
                print("%s level 0 round %d: kept %d rollbacks %d overflowed %d evaluate %.3f ms judge %.3f ms" % ((tag,) + r[1:]))
        tot = max(ev + ju + co, 1e-9)
        print("%s phases (one call under GMX_LOUVAIN_PHASES): evaluate %.3f ms (%.1f %%) judge %.3f ms (%.1f %%) contract %.3f ms (%.1f %%)"
              % (tag, ev, 100 * ev / tot, ju, 100 * ju / tot, co, 100 * co / tot))
    kms = [call(g, weight, **knobs)[0][5]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms), out, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--weighted", action="store_true", help="weights 1 .. 100 instead of none")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the thresholds and the table size at other values")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s%s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "", "w" if a.weighted else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    weight = np.random.default_rng(a.scale).integers(1, 101, g.E).astype(np.int32) if a.weighted else None
    base, want, text = runs(g, weight, tag, a.reps, show=True)
    rounds_run = len(ROUND.findall(text))
    print("%s gmx_louvain = %.3f ms per round run over all levels (%d rounds)" % (tag, base / max(1, rounds_run), rounds_run))
    g.communities(1000)
    lp = [g.communities(1000) for _ in range(a.reps)]
    lp_ms, lp_rounds = statistics.median([x[3]["kernel_ms"] for x in lp]), max(1, lp[0][1])
    print("%s gmx_communities kernel_ms %s, %d rounds = %.3f ms per round" % (tag, spread([x[3]["kernel_ms"] for x in lp]), lp[0][1], lp_ms / lp_rounds))
    lv0 = [(float(e), float(j)) for lv, r, k, rb, o, e, j in ROUND.findall(text) if int(lv) == 0]
    lv0_round = sum(e + j for e, j in lv0) / max(1, len(lv0))
    print("%s a level-0 round of gmx_louvain (%.3f ms under the phase clock) = %.2f x a round of gmx_communities" % (tag, lv0_round, lv0_round / (lp_ms / lp_rounds)))
    g.wcc()
    wcc = statistics.median([g.wcc()[2]["kernel_ms"] for _ in range(a.reps)])
    age = np.random.default_rng(1).integers(10, 60, g.V).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    sweep = statistics.median([g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(a.reps)])
    print("%s gmx_wcc %.3f ms, one sweep of the rows (gmx_avg_teen_cnt) %.3f ms" % (tag, wcc, sweep))
    print("%s gmx_louvain = %.1f x gmx_communities = %.1f x gmx_wcc = %.0f x one sweep of the rows; a level-0 half-round = %.1f x one sweep"
          % (tag, base / lp_ms, base / wcc, base / sweep, lv0_round / 2 / sweep), flush=True)
    if a.sweep:
        for knobs in ({"wave_min": 1}, {"wave_min": 17}, {"block_min": 64}, {"block_min": 1024}, {"lds_slots": 512}, {"lds_slots": 8192}):
            name = " ".join("GMX_LOUVAIN_%s=%s" % (n.upper(), v) for n, v in knobs.items())
            ms, _, _ = runs(g, weight, "%s %s" % (tag, name), a.reps, want, **knobs)
            print("%s %s = %.2f x the default" % (tag, name, ms / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
