"""Adamic-Adar edge scores (gmx_adamic_adar) on RMAT graphs: first-call and warm device time, the download, the whole
call, and the traffic lower bound next to what the device's copy rate would need for it.

    python green-marl_amd/tools/aa_prof.py --scale 22 [--permute 0|1] [--reps 5] [--baseline]

--baseline also sends all E (from, to) slots through gmx_common_nbr_counts: the same intersections unstaged, one wave per
pair, without weights or sums.  Its wall time includes the upload of the pairs; the duration of its kernel
(common_nbr_count_kernel) next to aa_rows_kernel's comes from running this script under
`rocprofv3 --kernel-trace --stats`.  The count it returns must equal the call's edges_examined."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import gmx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--permute", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    gmx.require_device()
    V = 1 << a.scale
    t0 = time.time()
    g = gmx.Graph.rmat(V, a.ef << a.scale, 1997, 0.57, 0.19, 0.19, bool(a.permute))
    gen_s = time.time() - t0
    E = g.E
    t0 = time.time()
    aa = g.adamic_adar()
    first_wall = time.time() - t0
    first = dict(g.last_stats)
    warm, d2h, wall = [], [], []
    for _ in range(a.reps):
        t0 = time.time()
        b = g.adamic_adar()
        wall.append((time.time() - t0) * 1e3)
        assert b.tobytes() == aa.tobytes()
        del b
        warm.append(g.last_stats["kernel_ms"])
        d2h.append(g.last_stats["d2h_ms"])
    med = float(np.median(warm)) if warm else first["kernel_ms"]
    # what any form of the computation moves: aa written, the forward CSR read, the weights written
    bound = 8 * E + 4 * (V + E) + 8 * V
    copy_gbs = gmx.copy_bandwidth()
    out = {"scale": a.scale, "ef": a.ef, "permute": a.permute, "V": V, "E": E, "gen_s": round(gen_s, 2),
           "common_nbr_hits": first["edges_examined"], "nonzero": int(np.count_nonzero(aa)), "inf": int(np.isinf(aa).sum()),
           "nan": int(np.isnan(aa).sum()), "first_kernel_ms": round(first["kernel_ms"], 3), "first_wall_ms": round(first_wall * 1e3, 3),
           "warm_kernel_ms": [round(x, 3) for x in warm], "warm_median_ms": round(med, 3),
           "d2h_ms": round(float(np.median(d2h)) if d2h else first["d2h_ms"], 3),
           "whole_call_ms": round(float(np.median(wall)) if wall else first_wall * 1e3, 3),
           "bound_bytes": bound, "bound_gbs_at_kernel_time": round(bound / (med * 1e-3) / 1e9, 2), "copy_gbs": round(copy_gbs, 1),
           "fraction_of_bound": round(bound / (copy_gbs * 1e9) / (med * 1e-3), 5)}
    if a.baseline:
        begin, idx, _, _ = g.download(reverse=False)
        src = np.repeat(np.arange(V, dtype=np.int32), np.diff(begin))
        t0 = time.time()
        counts = g.common_nbr_counts(src, idx)
        out["baseline_wall_ms"] = round((time.time() - t0) * 1e3, 3)
        out["baseline_hits"] = int(counts.sum())
        assert out["baseline_hits"] == first["edges_examined"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
