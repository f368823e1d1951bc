#!/usr/bin/env python3
"""gmx_bc (per seed) against gmx_bc_batch at widths 16 / 32 / 64 on RMAT-<scale>, the same K seeds (fixed rng, the top
hub first), in one process: a warm-up of each (with GMX_BCB_TRACE=1, so the per-batch lines are printed), then --reps
rounds that alternate the four; device time by events (stats.kernel_ms); median and min-max per method, the ratio to the
per-seed median, and the batched bytes compared with gmx_bc's.

  bcb_prof.py --scale 24 --seeds 64 [--permute] [--reps 5] [--literal]

Split of a batch into traversals, level transposition, row finding, forward / reverse short and long rows and the BC
accumulate: a run of its own under `rocprofv3 --kernel-trace --stats -- bcb_prof.py ... --only 64 --reps 1` (no counters in
that run); --only takes one width (1 = gmx_bc) and skips the comparison.  KERNEL_GROUPS maps kernel names to those parts;
`bcb_prof.py --groups <kernel_stats.csv>` sums a stats file by them."""
import argparse
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

WIDTHS = (16, 32, 64)
KERNEL_GROUPS = (          # first match wins; bcb_short / bcb_long: template argument true = forward (sigma), false = reverse (delta)
    ("level transposition", ("bcb_stage_kernel", "bcb_transpose_kernel", "bcb_seed_kernel")),
    ("row finding", ("bcb_find_kernel",)),
    ("forward short", ("bcb_short_kernel<16, true>", "bcb_short_kernel<32, true>", "bcb_short_kernel<64, true>")),
    ("forward long", ("bcb_long_kernel<16, true>", "bcb_long_kernel<32, true>", "bcb_long_kernel<64, true>")),
    ("reverse short", ("bcb_short_kernel<16, false>", "bcb_short_kernel<32, false>", "bcb_short_kernel<64, false>")),
    ("reverse long", ("bcb_long_kernel<16, false>", "bcb_long_kernel<32, false>", "bcb_long_kernel<64, false>")),
    ("BC accumulate", ("bcb_accumulate_kernel",)),
    ("per-seed sweeps", ("bfs_visit_kernel", "bfs_visit_big_kernel", "bfs_level_bitmap_kernel", "bfs_order_", "fill_sigma_kernel", "fill_f32_kernel")),
    ("graph construction", ("rmat_", "keys_from_", "csr_extract", "apply_perm", "bfs_hint_kernel", "bfs_degkey", "rocprim")),
    ("traversals", ("bfs_",)),
)


def group_of(kernel):
    for name, pats in KERNEL_GROUPS:
        if any(p in kernel for p in pats):
            return name
    return "other (copies, fills)"


def groups(path):
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            g = group_of(row["Name"])
            tot[g] = tot.get(g, 0.0) + ns
    whole = sum(tot.values()) or 1.0
    for g, ns in sorted(tot.items(), key=lambda kv: -kv[1]):
        print("%-22s %10.3f ms  %5.1f %%" % (g, ns / 1e6, 100 * ns / whole))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--literal", action="store_true", help="skip_root = 0 (this fork's form: 0 / NaN); default is the (v != s) form")
    ap.add_argument("--only", type=int, default=None, help="one width only (1 = gmx_bc), for a run under the profiler")
    ap.add_argument("--groups", default=None, help="sum a rocprofv3 kernel_stats.csv by KERNEL_GROUPS and exit")
    a = ap.parse_args()
    if a.groups:
        return groups(a.groups)
    import gmx
    gmx.require_device()
    skip = not a.literal
    N = 1 << a.scale
    g = gmx.Graph.rmat(N, 16 * N, 1997, 0.57, 0.19, 0.19, a.permute)
    deg = np.diff(g.download(reverse=False)[0])
    seeds = np.random.default_rng(a.scale).integers(0, N, a.seeds).astype(np.int32)
    seeds[0] = int(np.argmax(deg))
    tag = "RMAT-%d%s K=%d skip_root=%d" % (a.scale, "p" if a.permute else "", a.seeds, skip)

    def run(width):
        if width == 1:
            return g.bc(seeds, skip)
        return g.bc_batch(seeds, skip, width)

    methods = (1,) + WIDTHS if a.only is None else (a.only,)
    os.environ["GMX_BCB_TRACE"] = "1"
    sys.stderr.flush()
    ref = None
    for w in methods:                                   # warm-up of each, traced; bytes against gmx_bc
        out, st = run(w)
        if w == 1:
            ref = out
        elif ref is not None:
            same = out.tobytes() == ref.tobytes()
            print("%s width %2d: bytes %s gmx_bc's; slots walked %d" % (tag, w, "EQUAL" if same else "DIFFER FROM", st["edges_examined"]), flush=True)
            if not same:
                sys.exit("bcb_prof: width %d differs from gmx_bc" % w)
    os.environ.pop("GMX_BCB_TRACE")
    ms = {w: [] for w in methods}
    for _ in range(a.reps):
        for w in methods:                               # alternating
            ms[w].append(run(w)[1]["kernel_ms"])
    base = statistics.median(ms[1]) if 1 in ms else None
    for w in methods:
        med = statistics.median(ms[w])
        print("%s %-9s median %9.2f ms  min %9.2f  max %9.2f  per seed %7.3f ms%s" % (
            tag, "per-seed" if w == 1 else "width %d" % w, med, min(ms[w]), max(ms[w]), med / a.seeds,
            "" if base is None or w == 1 else "  batched/per-seed %.3f" % (med / base)), flush=True)
    g.free()


if __name__ == "__main__":
    main()
