#!/usr/bin/env python3
"""gmx_triangle_counting_directed on RMAT-<scale>, in one process:

  * plan build time (the library's own figure, from its GMX_TCD_LOG line) with the degree order and with GMX_TCD_NO_ORDER=1;
  * kernel_ms (device events around the count kernel) with the default settings and with GMX_TCD_NO_ORDER=1: a warm-up of
    each, then --reps rounds that alternate the two; median and min-max;
  * the regime shares of the log line: work items staged in LDS / searched in memory, slots walked by a lane alone, by
    list-streaming, by tail-streaming, and slots with an empty side;
  * on the symmetrised graph the same entry next to gmx_triangle_counting (which has the hub bit matrix), with the
    assertion T_directed = 3 T;
  * --sweep: kernel_ms over GMX_TCD_ALONE, GMX_TCD_RATIO and GMX_TCD_CAP, one knob at a time.

  tcd_prof.py --scale 22 [--permute] [--reps 5] [--sweep] [--no-sym]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_TCD_NO_ORDER", "GMX_TCD_CAP", "GMX_TCD_ALONE", "GMX_TCD_RATIO")
LINE = re.compile(r"gmx triangle_counting_directed: plan V (\d+) out (\d+) up (\d+) order (degree|identity) built (\d) build_ms ([0-9.]+); "
                  r"part (\d+)/(\d+) cap (\d+) alone (\d+) ratio (\d+); items (\d+) staged \+ (\d+) memory; "
                  r"slots (\d+) alone \+ (\d+) list \+ (\d+) tail \+ (\d+) empty")
FIELDS = ("V", "out", "up", "order", "built", "build_ms", "part", "nparts", "cap", "alone_max", "ratio", "staged", "memory", "alone", "list",
          "tail", "empty")


def call(g, **env):
    """(T, kernel_ms, fields of the library's line) of one call with the given knobs; the line is read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_TCD_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            T, st = g.triangle_counting_directed()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS:
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("tcd_prof: no log line in %r" % text)
    f = {k: (v if k == "order" else float(v) if k == "build_ms" else int(v)) for k, v in zip(FIELDS, m.groups())}
    return T, st["kernel_ms"], f


def shares(f):
    items = f["staged"] + f["memory"] or 1
    slots = f["alone"] + f["list"] + f["tail"] + f["empty"] or 1
    return ("items %d: %.2f %% staged, %.2f %% in memory; slots %d: %.1f %% alone, %.1f %% list-streamed, %.1f %% tail-streamed, %.1f %% empty" % (
        items, 100.0 * f["staged"] / items, 100.0 * f["memory"] / items, slots, 100.0 * f["alone"] / slots, 100.0 * f["list"] / slots,
        100.0 * f["tail"] / slots, 100.0 * f["empty"] / slots))


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def order_runs(g, tag, reps):
    """Warm-up (and plan build) of each order, then alternating rounds; every switch rebuilds the plan outside kernel_ms."""
    T = None
    ms = {"degree": [], "identity": []}
    for order, env in (("degree", {}), ("identity", {"GMX_TCD_NO_ORDER": "1"})):
        t, _, f = call(g, **env)
        T = t if T is None else T
        if t != T:
            sys.exit("tcd_prof: the two orders disagree: %d != %d" % (t, T))
        print("%s order %-8s plan build %9.2f ms  OUT' %d  UP' %d" % (tag, order, f["build_ms"], f["out"], f["up"]))
        print("%s order %-8s %s" % (tag, order, shares(f)), flush=True)
        ms[order].append(call(g, **env)[1])               # the plan is there: a run without the build before it
    for _ in range(reps - 1):
        for order, env in (("degree", {}), ("identity", {"GMX_TCD_NO_ORDER": "1"})):
            call(g, **env)                                # rebuilds the plan for this order
            ms[order].append(call(g, **env)[1])
    for order in ms:
        print("%s order %-8s kernel %s" % (tag, order, spread(ms[order])))
    print("%s T = %d; identity / degree order = %.2f" % (tag, T, statistics.median(ms["identity"]) / statistics.median(ms["degree"])), flush=True)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="kernel_ms over GMX_TCD_ALONE / RATIO / CAP on the directed graph")
    ap.add_argument("--no-sym", action="store_true", help="skip the symmetrised graph")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = 1 << a.scale
    tag = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
    order_runs(g, tag, a.reps)
    if a.sweep:
        call(g)                                           # the degree-ordered plan
        for knob, values in (("GMX_TCD_ALONE", (0, 2, 4, 8, 16, 48)), ("GMX_TCD_RATIO", (1, 2, 4, 8, 16, 64)), ("GMX_TCD_CAP", (256, 512, 1024))):
            for v in values:
                ms = [call(g, **{knob: str(v)})[1] for _ in range(max(3, a.reps))]
                print("%s %s=%-5d kernel %s" % (tag, knob, v, spread(ms)), flush=True)
    if not a.no_sym:
        s = g.symmetrize()
        g.free()
        stag = tag + " symmetrised"
        Td = order_runs(s, stag, a.reps)
        call(s)
        Tu, _ = s.triangle_counting()                     # warm-up: builds the oriented copy and the hub bit matrix
        und = [s.triangle_counting()[1]["kernel_ms"] for _ in range(a.reps)]
        dire = [call(s)[1] for _ in range(a.reps)]
        print("%s gmx_triangle_counting          kernel %s" % (stag, spread(und)))
        print("%s gmx_triangle_counting_directed kernel %s" % (stag, spread(dire)))
        print("%s directed / undirected = %.2f" % (stag, statistics.median(dire) / statistics.median(und)))
        assert Td == 3 * Tu, (Td, Tu)
        print("%s T_directed = %d = 3 x %d: OK" % (stag, Td, Tu), flush=True)
        s.free()
    else:
        g.free()


if __name__ == "__main__":
    main()
