"""Label-propagation communities (gmx_communities) on RMAT graphs: per round the evaluations, slots, changes, device time
and the share of the three evaluation kernels, and round 0 -- one pass over every vertex with out-edges in the worst table
state, every neighbour still carrying its own id -- as slots per second next to gmx_avg_teen_cnt's on the same graph in
the same process (one flat slot array, one gathered property per slot: what such a pass must at least do).

    python green-marl_amd/tools/comm_prof.py --scale 22 [--permute 0|1] [--sym 1] [--reps 3]

The per-round lines come from the library (GMX_COMM_ROUNDS=1: an event around every round)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import gmx  # noqa: E402

ROUND = re.compile(r"gmx communities round (\d+): evals (\d+) short \+ (\d+) wave \+ (\d+) block \((\d+) overflowed\), slots (\d+), "
                   r"changes (\d+), ([0-9.]+) ms")


def logged_run(g, max_rounds):
    """One call with the library's per-round lines (written to the C stderr) caught in a file."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["GMX_COMM_ROUNDS"] = "1"
        try:
            out = g.communities(max_rounds)
        finally:
            del os.environ["GMX_COMM_ROUNDS"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    rows = []
    for m in ROUND.finditer(text):
        r, s, w, b, o, slots, ch = (int(x) for x in m.groups()[:7])
        rows.append({"round": r, "short": s, "wave": w, "block": b, "overflowed": o, "slots": slots, "changes": ch, "ms": float(m.group(8))})
    return out, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--permute", type=int, default=0)
    ap.add_argument("--sym", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=1000)
    a = ap.parse_args()
    gmx.require_device()
    V = 1 << a.scale
    t0 = time.time()
    g = gmx.Graph.rmat(V, a.ef << a.scale, 1997, 0.57, 0.19, 0.19, bool(a.permute))
    if a.sym:
        g = g.symmetrize()
    gen_s = time.time() - t0
    comm, rounds, conv, first = g.communities(a.max_rounds)
    warm = []
    for _ in range(a.reps):
        c2, r2, v2, st = g.communities(a.max_rounds)
        assert (r2, v2) == (rounds, conv) and np.array_equal(c2, comm)
        warm.append(st["kernel_ms"])
    (_, _, _, _), rows = logged_run(g, a.max_rounds)
    os.environ["GMX_COMM_WORKLIST"] = "0"
    c0, r0, v0, full = g.communities(a.max_rounds)
    del os.environ["GMX_COMM_WORKLIST"]
    assert (r0, v0) == (rounds, conv) and np.array_equal(c0, comm)
    age = np.random.default_rng(1).integers(0, 40, V).astype(np.int32)
    teen = [g.avg_teen_cnt(age, 20)[2]["kernel_ms"] for _ in range(a.reps + 1)][1:]
    teen_ms = float(np.median(teen))
    print("communities rmat%d ef%d permute %d sym %d: V %d, E %d, generated in %.2f s" % (a.scale, a.ef, a.permute, a.sym, V, g.E, gen_s))
    print("  round     evals      short%  wave%  block%  overflowed         slots     changes        ms")
    for r in rows:
        n = max(1, r["short"] + r["wave"] + r["block"])
        print("  %5d %9d      %6.2f %6.2f  %6.2f  %10d  %12d  %10d  %8.3f" % (r["round"], n, 100.0 * r["short"] / n, 100.0 * r["wave"] / n,
                                                                             100.0 * r["block"] / n, r["overflowed"], r["slots"], r["changes"], r["ms"]))
    teen_rate = g.E / (teen_ms * 1e-3)
    line = {"scale": a.scale, "ef": a.ef, "permute": a.permute, "sym": a.sym, "V": V, "E": g.E, "rounds": rounds, "converged": conv,
            "labels": int(len(np.unique(comm))), "largest": int(np.bincount(comm).max()),
            "evaluations": first["vertices_reached"], "slots": first["edges_examined"],
            "first_kernel_ms": round(first["kernel_ms"], 3), "warm_kernel_ms": [round(x, 3) for x in warm],
            "warm_median_ms": round(float(np.median(warm)), 3), "d2h_ms": round(st["d2h_ms"], 3),
            "no_worklist_kernel_ms": round(full["kernel_ms"], 3), "no_worklist_evaluations": full["vertices_reached"],
            "avg_teen_cnt_ms": round(teen_ms, 3), "avg_teen_cnt_gslots_s": round(teen_rate * 1e-9, 2)}
    if rows:
        r0_rate = rows[0]["slots"] / (rows[0]["ms"] * 1e-3)
        line.update({"round0_ms": rows[0]["ms"], "round0_gslots_s": round(r0_rate * 1e-9, 2), "round0_vs_avg_teen_cnt": round(teen_rate / r0_rate, 2)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
