#!/usr/bin/env python3
"""gmx_wcc on RMAT-<scale>, in one process and on one graph:

  * the library's log line (sampled slots, the skipped tree, the live list, the slots of the final pass) and kernel_ms by
    phase -- sampling, compress, live list, final, finish -- from the hipEvents of GMX_WCC_PHASES: a warm-up, then --reps
    calls; median and min-max;
  * the detour it replaces: symmetrize() (host clock, once) + scc() on the symmetric graph (kernel_ms);
  * the yardstick "one sweep of the rows": kernel_ms of gmx_avg_teen_cnt on the same graph;
  * the same with GMX_WCC_SKIP=0 and with K = GMX_WCC_SAMPLE_ROUNDS = 0, 1, 2, 4.

  wcc_prof.py --scale 24 [--permute] [--reps 5] [--no-scc]"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_WCC_SAMPLE_ROUNDS", "GMX_WCC_SKIP", "GMX_WCC_GIANT")
LINE = re.compile(r"gmx wcc: (V \d+ E \d+ sample_rounds \d+ sampled (\d+) giant \d+ skipped (\d+) live (\d+) reverse [01] final_slots (\d+) "
                  r"comps (\d+) largest (\d+))")
PHASES = ("sampling", "compress", "live", "final", "finish")
PHASE = re.compile(r"gmx wcc phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES))


def call(g, **env):
    """(comp, count, stats, the log line, ms by phase) of one call; the lines are read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_WCC_LOG"] = os.environ["GMX_WCC_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            comp, n, st = g.wcc()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS + ("GMX_WCC_LOG", "GMX_WCC_PHASES"):
        os.environ.pop(k, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or not p:
        sys.exit("wcc_prof: no log line in %r" % text)
    return comp, n, st, m, dict(zip(PHASES, map(float, p.groups())))


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, reps, want=None, **env):
    comp, n, st, m, _ = call(g, **env)   # warm-up
    if want is not None and (n != want[1] or not np.array_equal(comp, want[0])):
        sys.exit("wcc_prof: %s gives another result" % tag)
    print("%s %s; edges_examined %d = %.3f x E" % (tag, m.group(1), st["edges_examined"], st["edges_examined"] / max(g.E, 1)))
    kms, phases = [], []
    for _ in range(reps):
        _, _, st, _, ph = call(g, **env)
        kms.append(st["kernel_ms"])
        phases.append(ph)
    for p in PHASES:
        print("%s   %-9s %s" % (tag, p, spread([x[p] for x in phases])))
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return statistics.median(kms), (comp, n)


def one_sweep(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one probe per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)
    return statistics.median(ms)


def detour(g, tag, reps, want):
    import gmx
    t0 = time.perf_counter()
    try:
        s = g.symmetrize()
    except gmx.GmxError as e:
        print("%s symmetrize() + scc(): not measured (%s)" % (tag, e), flush=True)
        return None
    sym_ms = (time.perf_counter() - t0) * 1e3
    comp, n, _ = s.scc()   # warm-up
    if n != want[1] or not np.array_equal(comp, want[0]):
        sys.exit("wcc_prof: symmetrize() + scc() gives another result")
    ms = [s.scc()[2]["kernel_ms"] for _ in range(reps)]
    print("%s symmetrize() %9.3f ms (host clock, E %d -> %d) + scc() kernel_ms %s" % (tag, sym_ms, g.E, s.E, spread(ms)), flush=True)
    s.free()
    return sym_ms + statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scc", action="store_true", help="leave out symmetrize() + scc()")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    base, want = runs(g, tag, a.reps)
    sweep = one_sweep(g, tag, a.reps)
    print("%s wcc = %.2f x one sweep of the rows" % (tag, base / sweep))
    if not a.no_scc:
        d = detour(g, tag, a.reps, want)
        if d is not None:
            print("%s symmetrize() + scc() = %.1f x wcc" % (tag, d / base))
    ms0, _ = runs(g, "%s GMX_WCC_SKIP=0" % tag, a.reps, want, GMX_WCC_SKIP="0")
    print("%s the skip: %.3f ms against %.3f ms without = %.2f x" % (tag, base, ms0, ms0 / base))
    for K in (0, 1, 2, 4):
        ms, _ = runs(g, "%s K=%d" % (tag, K), a.reps, want, GMX_WCC_SAMPLE_ROUNDS=str(K))
        print("%s K=%d = %.2f x the default, %.2f x one sweep" % (tag, K, ms / base, ms / sweep), flush=True)
    g.free()


if __name__ == "__main__":
    main()
