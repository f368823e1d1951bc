#!/usr/bin/env python3
"""gmx_v_cover on RMAT-<scale>, in one process:

  * plan build time and list entries (the library's own figures, from its GMX_VC_LOG line);
  * rounds (grid + tail), picks, kept, covered / selected;
  * host-clock ms of the call split into grid rounds, the tail launch and the finish, next to kernel_ms: a warm-up that
    builds the plan, then --reps calls; median and min-max;
  * the work counters skips (cursor steps over covered ends), evals (vertex evaluations) and walks (list entries of newly
    covered vertices), and their sum per edge;
  * --sweep: the same over GMX_VC_TAIL and GMX_VC_WAVE, one knob at a time.

  vc_prof.py --scale 20 [--permute] [--reps 5] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_VC_TAIL", "GMX_VC_WAVE")
LINE = re.compile(r"gmx v_cover: plan (built|reused) build_ms ([0-9.]+) V (\d+) E (\d+) L (\d+); tail (\d+) wave (\d+); rounds (\d+) grid \+ (\d+) tail; "
                  r"picks (\d+) kept (\d+) covered (\d+); skips (\d+) evals (\d+) walks (\d+); ms ([0-9.]+) grid \+ ([0-9.]+) tail \+ ([0-9.]+) finish")
FIELDS = ("plan", "build_ms", "V", "E", "L", "tail_from", "wave_min", "grid_rounds", "tail_rounds", "picks", "kept", "covered", "skips", "evals",
          "walks", "grid_ms", "tail_ms", "finish_ms")


def call(g, **env):
    """(select, covered, stats, fields of the library's line) of one call with the given knobs; the line is read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_VC_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            sel, cov, st = g.v_cover()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS:
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("vc_prof: no log line in %r" % text)
    f = {k: (v if k == "plan" else float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, m.groups())}
    return sel, cov, st, f


def spread(ms):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (statistics.median(ms), min(ms), max(ms))


def runs(g, tag, reps, **env):
    fs, kms = [], []
    for _ in range(reps):
        _, _, st, f = call(g, **env)
        fs.append(f)
        kms.append(st["kernel_ms"])
    f = fs[0]
    print("%s rounds %d grid + %d tail (tail from %d active, wave from %d entries)" % (tag, f["grid_rounds"], f["tail_rounds"], f["tail_from"], f["wave_min"]))
    for k in ("grid_ms", "tail_ms", "finish_ms"):
        print("%s %-9s %s" % (tag, k, spread([x[k] for x in fs])))
    print("%s kernel_ms %s" % (tag, spread(kms)), flush=True)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the split over GMX_VC_TAIL and GMX_VC_WAVE")
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    N = 1 << a.scale
    tag = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
    sel, cov, st, f = call(g)                             # warm-up: builds the plan
    print("%s V %d E %d: plan %s in %.2f ms, %d list entries" % (tag, f["V"], f["E"], f["plan"], f["build_ms"], f["L"]))
    print("%s covered %d selected %d picks %d kept %d" % (tag, cov, int(sel.sum()), f["picks"], f["kept"]))
    work = f["skips"] + f["evals"] + f["walks"]
    print("%s skips %d evals %d walks %d: %.2f x E" % (tag, f["skips"], f["evals"], f["walks"], work / max(f["E"], 1)), flush=True)
    runs(g, tag, a.reps)
    if a.sweep:
        for knob, values in (("GMX_VC_TAIL", (0, 256, 1024, 2048, 8192, 65536)), ("GMX_VC_WAVE", (0, 32, 128, 512, 2000000000))):
            for v in values:
                runs(g, "%s %s=%d" % (tag, knob, v), max(3, a.reps), **{knob: str(v)})
    g.free()


if __name__ == "__main__":
    main()
