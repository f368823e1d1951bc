"""Strongly connected components (gmx_scc) on RMAT graphs: first-call and warm device time, and where the time goes.

    python green-marl_amd/tools/scc_prof.py --scale 24 [--permute 0|1] [--reps 5]

The first call on a graph also builds the traversal hints of the transposed view (per graph, as for hop_dist).  The
per-phase line comes from the library (GMX_SCC_PHASES=1: an event at every phase boundary, so the phase times split the
call's kernel_ms): time and vertices removed by trim, by the FW-BW of the pivot, by colouring and by the single-workgroup
tail, the relabel, and the outer rounds."""
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
    a = ap.parse_args()
    gmx.require_device()
    V = 1 << a.scale
    t0 = time.time()
    g = gmx.Graph.rmat(V, a.ef << a.scale, 1997, 0.57, 0.19, 0.19, bool(a.permute))
    gen_s = time.time() - t0
    t0 = time.time()
    comp, n, first = g.scc()
    first_wall = time.time() - t0
    warm = []
    for _ in range(a.reps):
        c2, n2, st = g.scc()
        assert n2 == n and np.array_equal(c2, comp)
        warm.append(st["kernel_ms"])
    os.environ["GMX_SCC_PHASES"] = "1"
    sys.stderr.flush()
    g.scc()
    sys.stderr.flush()
    del os.environ["GMX_SCC_PHASES"]
    print(json.dumps({"scale": a.scale, "ef": a.ef, "permute": a.permute, "V": V, "E": g.E, "gen_s": round(gen_s, 2),
                      "components": n, "largest": first["vertices_reached"], "rounds": first["iterations"],
                      "edges_examined": first["edges_examined"], "first_kernel_ms": round(first["kernel_ms"], 3),
                      "first_wall_ms": round(first_wall * 1e3, 3), "warm_kernel_ms": [round(x, 3) for x in warm],
                      "warm_median_ms": round(float(np.median(warm)), 3), "d2h_ms": round(st["d2h_ms"], 3)}))


if __name__ == "__main__":
    main()
