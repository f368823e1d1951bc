"""gmx_sssp next to gmx_sssp_path (both schedules) on an RMAT graph with the bench.py apps configuration: permuted RMAT,
lengths 1..100 from default_rng(1), root = the vertex with most out-edges.

    python green-marl_amd/tools/sssp_prof.py [--scale 24] [--permute 1] [--reps 5] [--delta D]

Per entry: the device times (kernel_ms) of --reps calls after one warm-up, their median and spread (max - min) / median,
relaxation rounds, queue entries and edges examined.  gmx_sssp is the yardstick: its code does not depend on the schedule
switch, so the ratio of the medians is a comparison inside one process.  dist must agree between all three and the two
schedules must return identical prev arrays.  The kernels behind the times: run the script under
`rocprofv3 --kernel-trace --stats` (no counters)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import gmx  # noqa: E402


def measure(call, reps):
    call()                                                   # warm-up: code object, allocations
    times, st, out = [], None, None
    for _ in range(reps):
        *out, st = call()
        times.append(st["kernel_ms"])
    med = float(np.median(times))
    return out, {"kernel_ms": [round(t, 3) for t in times], "median_ms": round(med, 3),
                 "spread": round((max(times) - min(times)) / med, 4), "rounds": st["iterations"],
                 "queue_entries": st["vertices_reached"], "edges_examined": st["edges_examined"],
                 "h2d_ms": round(st["h2d_ms"], 3), "d2h_ms": round(st["d2h_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--permute", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--delta", type=str, default=None, help="GMX_SSSP_DELTA for the near / far schedule")
    a = ap.parse_args()
    gmx.require_device()
    V = 1 << a.scale
    g = gmx.Graph.rmat(V, a.ef << a.scale, 1997, 0.57, 0.19, 0.19, bool(a.permute))
    begin = g.download(reverse=False)[0]
    root = int(np.argmax(np.diff(begin)))
    length = np.random.default_rng(1).integers(1, 101, g.E).astype(np.int32)
    out = {"scale": a.scale, "ef": a.ef, "permute": a.permute, "V": V, "E": g.E, "root": root, "delta": a.delta or "from the mean length"}
    (dist,), out["gmx_sssp"] = measure(lambda: g.sssp(length, root), a.reps)
    if a.delta:
        os.environ["GMX_SSSP_DELTA"] = a.delta
    prev = {}
    for schedule in ("round", "nearfar"):
        os.environ["GMX_SSSP_PATH_SCHEDULE"] = schedule
        (d, pn, pe), res = measure(lambda: g.sssp_path(length, root), a.reps)
        assert np.array_equal(d, dist), schedule
        prev[schedule] = (pn, pe)
        res["vs_gmx_sssp"] = round(res["median_ms"] / out["gmx_sssp"]["median_ms"], 4)
        out["gmx_sssp_path " + schedule] = res
    assert all(np.array_equal(x, y) for x, y in zip(prev["round"], prev["nearfar"]))
    out["reached"] = int((dist != gmx.INT_MAX).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
