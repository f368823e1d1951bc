#!/usr/bin/env python3
"""gmx_closeness on RMAT-<scale>, in one process and on one graph:

  * for GMX_CLOSE_WORDS = 1, 2 and 4: the library's log line (sweeps, levels, vertices by regime, slots, pairs) and
    kernel_ms -- device events around the call's launches -- per call, per sweep and per level: a warm-up, then --reps
    calls; median [min - max]; the four arrays compared with the first width's;
  * the yardstick on the same graph: "one sweep of the rows" (kernel_ms of gmx_avg_teen_cnt);
  * what the library offered before for the same answer: gmx_hop_dist from 256 sampled roots, its median kernel_ms per call
    scaled to the source count -- an EXTRAPOLATION, labelled as such (it leaves out the V distances each call downloads);
  * --sweep: GMX_CLOSE_BATCH (levels launched per host read) at every width, interleaved, and GMX_CLOSE_LONG_MIN at the
    default width.

  close_prof.py --scale 16 [--permute] [--symmetrize] [--mode out|in|both] [--pivots K] [--reps 5] [--batch B] [--sweep]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FIELDS = ("V", "E", "mode", "sources", "words", "sweeps", "levels", "lane", "wave", "saturated", "slots", "pairs")
LINE = re.compile(r"gmx close: (" + " ".join(r"%s (\d+)" % f for f in FIELDS) + ")")
KNOBS = ("GMX_CLOSE_WORDS", "GMX_CLOSE_LONG_MIN", "GMX_CLOSE_BATCH", "GMX_CLOSE_LOG")
LONG_MINS = (1, 64, 128, 256, 512, 1024, 1 << 30)
BATCHES = (1, 2, 3, 4)


def call(g, mode, sources, env=None):
    """((far, reach, ecc, harm), stats, the log line's fields, the line) of one call; the line comes from stderr."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for k, v in (env or {}).items():
        os.environ[k] = str(v)
    os.environ["GMX_CLOSE_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            far, reach, ecc, harm, st = g.closeness(mode, sources)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for name in KNOBS:
        os.environ.pop(name, None)
    m = LINE.search(text)
    if not m:
        sys.exit("close_prof: no log line in %r" % text)
    return (far, reach, ecc, harm), st, dict(zip(FIELDS, map(int, m.groups()[1:]))), m.group(1)


def spread(ms, unit="ms", scale=1.0):
    return "median %10.3f %s [%10.3f - %10.3f]" % (statistics.median(ms) * scale, unit, min(ms) * scale, max(ms) * scale)


def runs(g, tag, mode, sources, reps, env, want=None):
    got, st, f, line = call(g, mode, sources, env)   # warm-up
    if want is not None and any(a.tobytes() != b.tobytes() for a, b in zip(got, want)):
        sys.exit("close_prof: %s gives other bytes" % tag)
    ms = [call(g, mode, sources, env)[1]["kernel_ms"] for _ in range(reps)]
    print("%s %s" % (tag, line))
    print("%s   per call   %s" % (tag, spread(ms)))
    print("%s   per sweep  %s" % (tag, spread(ms, "us", 1000.0 / max(f["sweeps"], 1))))
    print("%s   per level  %s" % (tag, spread(ms, "us", 1000.0 / max(f["levels"], 1))))
    print("%s   per source %s" % (tag, spread(ms, "us", 1000.0 / max(f["sources"], 1))), flush=True)
    return ms, got, f


def one_sweep(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one probe per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)


def hop_dist_extrapolated(g, tag, nsources):
    """gmx_hop_dist from 256 sampled roots; its median per call times the source count."""
    roots = np.random.default_rng(2).integers(0, g.V, 256)
    g.hop_dist(int(roots[0]))
    ms = [g.hop_dist(int(r))[1]["kernel_ms"] for r in roots]
    print("%s gmx_hop_dist, 256 sampled roots: kernel_ms per call %s" % (tag, spread(ms)))
    print("%s EXTRAPOLATION: %d calls of gmx_hop_dist at the median = %.1f ms (kernel time only; each call also downloads V distances)"
          % (tag, nsources, statistics.median(ms) * nsources), flush=True)
    return statistics.median(ms) * nsources


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--mode", choices=("out", "in", "both"), default="in")
    ap.add_argument("--pivots", type=int, default=0, help="K sampled sources instead of every vertex")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="GMX_CLOSE_BATCH of the width comparison (0: the library's default)")
    ap.add_argument("--sweep", action="store_true", help="GMX_CLOSE_LONG_MIN in %s" % (LONG_MINS,))
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    tag = "RMAT-%d%s%s %s %s" % (a.scale, "p" if a.permute else "", "s" if a.symmetrize else "", a.mode, "pivots %d" % a.pivots if a.pivots else "all")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute)
    if a.symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    sources = np.random.default_rng(1).integers(0, V, a.pivots).astype(np.int32) if a.pivots else None
    n = a.pivots or V
    want, med = None, {}
    for words in (1, 2, 4):
        ms, got, f = runs(g, "%s words %d" % (tag, words), a.mode, sources, a.reps, dict({"GMX_CLOSE_WORDS": words}, **({"GMX_CLOSE_BATCH": a.batch} if a.batch else {})), want)
        want = want or got
        med[words] = (statistics.median(ms), min(ms), max(ms))
    noise = max(hi - lo for _, lo, hi in med.values())
    for words in (2, 4):
        d = med[1][0] - med[words][0]
        print("%s words %d against 1: %.2f x, %+.3f ms; the larger min-max spread is %.3f ms: %s" % (
            tag, words, med[1][0] / med[words][0], -d, noise, "counts" if abs(d) > noise else "does not count"))
    one_sweep(g, tag, a.reps)
    if a.mode != "both":
        old = hop_dist_extrapolated(g, tag, n)
        print("%s the extrapolation / gmx_closeness at 1 word = %.1f" % (tag, old / med[1][0]))
    if a.sweep:
        for words in (1, 2, 4):
            for b in BATCHES:
                runs(g, "%s words %d GMX_CLOSE_BATCH=%d" % (tag, words, b), a.mode, sources, a.reps, {"GMX_CLOSE_WORDS": words, "GMX_CLOSE_BATCH": b}, want)
        for t in LONG_MINS:
            runs(g, "%s GMX_CLOSE_LONG_MIN=%d" % (tag, t), a.mode, sources, a.reps, {"GMX_CLOSE_LONG_MIN": t}, want)
    g.free()


if __name__ == "__main__":
    main()
