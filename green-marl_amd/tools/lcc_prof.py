#!/usr/bin/env python3
"""gmx_clustering on RMAT-<scale>, in one process:

  * the library's GMX_LCC_LOG line of the first call (the plan's build time and the hub matrix's are in it) and the
    regime and credit shares it reports;
  * kernel_ms (device events around the count kernel and the finishing kernel) of gmx_clustering next to
    gmx_triangle_counting_directed on the same graph: the same plan and the same kind of walk without any credit, so the
    baseline for what the credits cost.  A warm-up of each, then --reps rounds that alternate them; median and min-max;
  * the same with GMX_LCC_PLAIN=1: one global atomic per match for the third corner instead of the packed LDS counters;
  * with --symmetrize, on the symmetrised graph, gmx_triangle_counting as well, and the identities between the three counts;
  * --sweep: kernel_ms over GMX_LCC_ALONE, GMX_LCC_RATIO, GMX_LCC_HUB_TAIL, GMX_LCC_CAP and GMX_LCC_HUBS, one knob at a time.

  lcc_prof.py --scale 22 [--permute] [--symmetrize] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_LCC_NO_ORDER", "GMX_LCC_CAP", "GMX_LCC_ALONE", "GMX_LCC_RATIO", "GMX_LCC_HUB_TAIL", "GMX_LCC_HUBS", "GMX_LCC_PLAIN")
LINE = re.compile(r"gmx clustering: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) build_ms (?P<build_ms>[\d.]+) "
                  r"hubs (?P<hubs>\d+) hub_ms (?P<hub_ms>[\d.]+); cap (?P<cap>\d+) alone (?P<alone_max>\d+) ratio (?P<ratio>\d+) "
                  r"hub_tail (?P<hub_tail>\d+) w (?P<w>\w+); items (?P<staged>\d+) staged \+ (?P<memory>\d+) memory; slots (?P<alone>\d+) alone \+ "
                  r"(?P<list>\d+) list \+ (?P<tail>\d+) tail \+ (?P<hub>\d+) hub \+ (?P<empty>\d+) empty; credits (?P<lds>\d+) lds \+ (?P<glob>\d+) global")


def call(g, **env):
    """(triangles, wedges, kernel_ms, the log line, its fields) of one gmx_clustering call with the given knobs; no array is
    downloaded.  The line is read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_LCC_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            _, _, _, T, W, st = g.clustering(tri=False, deg=False, lcc=False)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS:
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("lcc_prof: no log line in %r" % text)
    f = {k: (v if k in ("order", "w") else float(v) if k.endswith("_ms") else int(v)) for k, v in m.groupdict().items()}
    return T, W, st["kernel_ms"], m.group(0), f


def shares(f):
    items = f["staged"] + f["memory"] or 1
    slots = f["alone"] + f["list"] + f["tail"] + f["hub"] + f["empty"] or 1
    credits = f["lds"] + f["glob"] or 1
    return ("items %d: %.2f %% staged, %.2f %% in memory; slots %d: %.1f %% alone, %.1f %% list, %.1f %% tail, %.1f %% hub, %.1f %% empty; "
            "third-corner credits %d: %.2f %% lds, %.2f %% global" % (
                items, 100.0 * f["staged"] / items, 100.0 * f["memory"] / items, slots, 100.0 * f["alone"] / slots, 100.0 * f["list"] / slots,
                100.0 * f["tail"] / slots, 100.0 * f["hub"] / slots, 100.0 * f["empty"] / slots, credits, 100.0 * f["lds"] / credits,
                100.0 * f["glob"] / credits))


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f  (%d runs)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true", help="run on the symmetrised graph, with gmx_triangle_counting next to it")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="kernel_ms over the GMX_LCC_* knobs, one at a time")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = 1 << a.scale
    tag = "RMAT-%d%s%s" % (a.scale, "p" if a.permute else "", " symmetrised" if a.symmetrize else "")
    g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    T, W, _, line, f = call(g)                            # builds the plan, the work items and the hub matrix
    print(line)
    print("%s plan build %.2f ms, hub matrix (%d hubs) %.2f ms" % (tag, f["build_ms"], f["hubs"], f["hub_ms"]))
    print("%s %s" % (tag, shares(f)))
    print("%s triangles %d wedges %d transitivity %.6f" % (tag, T, W, 3.0 * T / W if W else 0.0), flush=True)
    Tp, Wp, _, _, fp = call(g, GMX_LCC_PLAIN="1")
    Td = g.triangle_counting_directed()[0]                # warm-up (the plan is shared)
    assert (Tp, Wp) == (T, W) and fp["w"] == "global" and fp["lds"] == 0
    ms = {"clustering": [], "clustering, plain w credits": [], "triangle_counting_directed": []}
    if a.symmetrize:
        Tu = g.triangle_counting()[0]                     # warm-up: builds the oriented copy and its hub matrix
        assert Tu == T and Td == 3 * T, (Tu, Td, T)
        print("%s triangles = gmx_triangle_counting = gmx_triangle_counting_directed / 3: OK" % tag)
        ms["triangle_counting"] = []
    for _ in range(a.reps):
        ms["clustering"].append(call(g)[2])
        ms["clustering, plain w credits"].append(call(g, GMX_LCC_PLAIN="1")[2])
        ms["triangle_counting_directed"].append(g.triangle_counting_directed()[1]["kernel_ms"])
        if a.symmetrize:
            ms["triangle_counting"].append(g.triangle_counting()[1]["kernel_ms"])
    for k, v in ms.items():
        print("%s %-28s kernel %s" % (tag, k, spread(v)))
    base = statistics.median(ms["triangle_counting_directed"])
    print("%s clustering / triangle_counting_directed = %.2f; plain / packed w credits = %.2f" % (
        tag, statistics.median(ms["clustering"]) / base, statistics.median(ms["clustering, plain w credits"]) / statistics.median(ms["clustering"])),
        flush=True)
    if a.sweep:
        for knob, values in (("GMX_LCC_ALONE", (0, 2, 4, 8, 16, 48)), ("GMX_LCC_RATIO", (1, 2, 4, 8, 16, 64)), ("GMX_LCC_HUB_TAIL", (1, 2, 4, 16, 64)),
                             ("GMX_LCC_CAP", (256, 512, 1024)), ("GMX_LCC_HUBS", (0, 4096, 16384, 65536))):
            for v in values:
                call(g, **{knob: str(v)})                 # (a new number of hubs rebuilds the matrix, outside kernel_ms)
                r = [call(g, **{knob: str(v)})[2] for _ in range(max(3, a.reps))]
                print("%s %s=%-6d kernel %s" % (tag, knob, v, spread(r)), flush=True)
    g.free()


if __name__ == "__main__":
    main()
