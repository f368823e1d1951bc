#!/usr/bin/env python3
"""gmx_coloring on RMAT-<scale>, in one process and on one graph:

  * the library's log line (rounds, grid and tail rounds, vertices by regime, extra window passes, colours, class 0);
  * the device time by phase -- count, colour per regime, release, tail launches; hipEvents around every step, which
    synchronises (GMX_COLOR_PHASES) -- in calls of their own: a warm-up, then --reps calls;
  * kernel_ms of the call as it runs by default (no phase events): a warm-up, then --reps calls; median and min-max;
  * the yardsticks on the same graph: "one sweep of the rows" (kernel_ms of gmx_avg_teen_cnt) and gmx_kcore in mode both,
    whose release step has the same shape;
  * --sweep: the same call with GMX_COLOR_TAIL, GMX_COLOR_WAVE_MIN and GMX_COLOR_BLOCK_MIN varied one at a time, the
    result compared with the default's.

  color_prof.py --scale 24 [--permute] [--symmetrize] [--order degree|id|random] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINE = re.compile(r"gmx color: (V \d+ E \d+ user_prio [01] rounds (\d+) grid_rounds (\d+) tail_rounds (\d+) group (\d+) wave (\d+) block (\d+) "
                  r"passes (\d+) colors (\d+) class0 (\d+))")
PHASES = ("count", "group", "wave", "block", "release", "tail")
PHASE = re.compile(r"gmx color phases: " + ", ".join(r"%s ([0-9.]+) ms" % p for p in PHASES))
KNOBS = ("GMX_COLOR_TAIL", "GMX_COLOR_WAVE_MIN", "GMX_COLOR_BLOCK_MIN", "GMX_COLOR_WINDOW", "GMX_COLOR_LOG", "GMX_COLOR_PHASES")
SWEEPS = (("GMX_COLOR_TAIL", (0, 256, 1024, 4096, 16384, 65536, 262144)),
          ("GMX_COLOR_WAVE_MIN", (1, 17, 33, 65)),
          ("GMX_COLOR_BLOCK_MIN", (65, 128, 256, 512, 1024, 4096, 8192)))


def call(g, prio, env=None, phases=False):
    """(color, num_colors, stats, the log line, ms by phase or None) of one call; the lines come from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for k, v in (env or {}).items():
        os.environ[k] = str(v)
    os.environ["GMX_COLOR_LOG"] = "1"
    if phases:
        os.environ["GMX_COLOR_PHASES"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            color, n, st = g.coloring(prio)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m, p = LINE.search(text), PHASE.search(text)
    if not m or (phases and not p):
        sys.exit("color_prof: no log line in %r" % text)
    return color, n, st, m, dict(zip(PHASES, map(float, p.groups()))) if phases else None


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, prio, reps, want=None, env=None, full=True):
    color, n, st, m, _ = call(g, prio, env)   # warm-up
    if want is not None and not np.array_equal(color, want):
        sys.exit("color_prof: %s gives another result" % tag)
    if full:
        print("%s %s" % (tag, m.group(1)))
        call(g, prio, env, phases=True)
        ph = [call(g, prio, env, phases=True)[4] for _ in range(reps)]
        for p in PHASES:
            print("%s   %-8s %s" % (tag, p, spread([x[p] for x in ph])))
    kms = [call(g, prio, env)[2]["kernel_ms"] for _ in range(reps)]
    print("%s kernel_ms %s%s" % (tag, spread(kms), "" if full else "  grid_rounds %s tail_rounds %s group %s wave %s block %s" % m.groups()[2:7]), flush=True)
    return statistics.median(kms), color, int(m.group(2))


def one_sweep(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one probe per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)
    return statistics.median(ms)


def kcore_both(g, tag, reps):
    g.kcore("both")
    st = [g.kcore("both")[2] for _ in range(reps)]
    print("%s gmx_kcore both: rounds %d kernel_ms %s" % (tag, st[0]["iterations"], spread([s["kernel_ms"] for s in st])), flush=True)
    return statistics.median([s["kernel_ms"] for s in st]), st[0]["iterations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--order", choices=("degree", "id", "random"), default="degree")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="one knob at a time: %s" % (SWEEPS,))
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s %s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "", a.order)
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    prio = {"degree": None, "id": np.zeros(V, np.int32), "random": np.random.default_rng(1).integers(0, 1 << 30, V).astype(np.int32)}[a.order]
    base, want, rounds = runs(g, tag, prio, a.reps)
    print("%s %.1f us a round" % (tag, 1000 * base / max(rounds, 1)))
    sweep = one_sweep(g, tag, a.reps)
    kc, kc_rounds = kcore_both(g, tag, a.reps)
    print("%s coloring = %.1f x one sweep of the rows = %.2f x gmx_kcore both (%.1f us a round there)" % (tag, base / sweep, base / kc, 1000 * kc / max(kc_rounds, 1)))
    if a.sweep:
        for knob, values in SWEEPS:
            best = None
            for t in values:
                ms, _, _ = runs(g, "%s %s=%d" % (tag, knob, t), prio, a.reps, want, {knob: t}, full=False)
                if best is None or ms < best[0]:
                    best = (ms, t)
            print("%s the sweep's best: %s=%d, %.3f ms = %.2f x the default" % (tag, knob, best[1], best[0], best[0] / base), flush=True)
    g.free()


if __name__ == "__main__":
    main()
