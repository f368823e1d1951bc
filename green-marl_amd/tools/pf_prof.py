"""Potential-friend sets (gmx_potential_friends) on RMAT graphs: device time of the sizing call and of the filling call,
two-hop items per second, rows and items per regime, overflowed rows and batches -- next to gmx_adamic_adar's items per
second on the same graph in the same process (the nearest kernel: one gather and one membership decision per item).

    python green-marl_amd/tools/pf_prof.py --scale 20 [--rows lo:hi] [--permute 0|1] [--reps 3] [--max-items N] [--sweep]

The sizing call covers the rows asked for (default: all).  The filling call covers the same rows if their sets hold at most
--max-items entries (default 2^29: 2 GiB of host memory); otherwise the longest prefix of the rows that does, and the
output says which.  The per-evaluation lines come from the library (GMX_PF_LOG=1).  --sweep instead times the sizing call
under a list of threshold settings (GMX_PF_WAVE_MAX, GMX_PF_BLOCK_MAX, GMX_PF_LDS_SLOTS, GMX_PF_LDS_BITS)."""
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

LINE = re.compile(r"gmx potential_friends (count|fill) rows \[(\d+), (\d+)\): rows (\d+) wave \+ (\d+) block \+ (\d+) bitmap \((\d+) overflowed\), "
                  r"items (\d+) wave \+ (\d+) block \+ (\d+) bitmap")


def logged(fn):
    """fn() with the library's lines (written to the C stderr) caught in a file."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["GMX_PF_LOG"] = "1"
        try:
            out = fn()
        finally:
            del os.environ["GMX_PF_LOG"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    rows = []
    for m in LINE.finditer(text):
        w, b, k, o, iw, ib, ik = (int(x) for x in m.groups()[3:])
        rows.append({"mode": m.group(1), "lo": int(m.group(2)), "hi": int(m.group(3)), "rows": [w, b, k], "overflowed": o, "items": [iw, ib, ik]})
    return out, rows


SWEEP = [{}, {"GMX_PF_WAVE_MAX": "32"}, {"GMX_PF_WAVE_MAX": "512", "GMX_PF_LDS_SLOTS": "16384"}, {"GMX_PF_WAVE_MAX": "0"},
         {"GMX_PF_BLOCK_MAX": "512"}, {"GMX_PF_BLOCK_MAX": "8192"}, {"GMX_PF_BLOCK_MAX": "8192", "GMX_PF_LDS_SLOTS": "16384"},
         {"GMX_PF_BLOCK_MAX": "32768", "GMX_PF_LDS_SLOTS": "16384"}, {"GMX_PF_WAVE_MAX": "0", "GMX_PF_BLOCK_MAX": "0"},
         {"GMX_PF_LDS_BITS": "1"}, {"GMX_PF_WAVE_MAX": "0", "GMX_PF_BLOCK_MAX": "0", "GMX_PF_LDS_BITS": "1"}]


def sweep(g, lo, hi, reps):
    """The sizing call's device time under every setting of SWEEP; the counts must not move."""
    want = g.potential_friend_counts(lo, hi)
    for env in SWEEP:
        os.environ.update(env)
        try:
            (counts, rows), ms = logged(lambda: g.potential_friend_counts(lo, hi)), []
            assert np.array_equal(counts, want)
            for _ in range(reps):
                g.potential_friend_counts(lo, hi)
                ms.append(g.last_stats["kernel_ms"])
        finally:
            for k in env:
                del os.environ[k]
        print(json.dumps({"knobs": env, "sizing_kernel_ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3),
                          "rows": rows[0]["rows"], "overflowed": rows[0]["overflowed"], "items": rows[0]["items"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--permute", type=int, default=0)
    ap.add_argument("--rows", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-items", type=int, default=1 << 29)
    ap.add_argument("--aa", type=int, default=1)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    gmx.require_device()
    V = 1 << a.scale
    t0 = time.time()
    g = gmx.Graph.rmat(V, a.ef << a.scale, 1997, 0.57, 0.19, 0.19, bool(a.permute))
    gen_s = time.time() - t0
    lo, hi = (int(x) for x in a.rows.split(":")) if a.rows else (0, V)
    if a.sweep:
        print("potential_friends sweep rmat%d ef%d permute %d: V %d, E %d, rows [%d, %d)" % (a.scale, a.ef, a.permute, V, g.E, lo, hi))
        return sweep(g, lo, hi, max(a.reps, 1))
    counts, log = logged(lambda: g.potential_friend_counts(lo, hi))
    first = dict(g.last_stats)
    size_ms = []
    for _ in range(a.reps):
        c2 = g.potential_friend_counts(lo, hi)
        assert np.array_equal(c2, counts)
        size_ms.append(g.last_stats["kernel_ms"])
    items = first["edges_examined"]
    size_med = float(np.median(size_ms)) if size_ms else first["kernel_ms"]
    run = np.cumsum(counts)
    fill_hi = hi if (len(run) == 0 or run[-1] <= a.max_items) else lo + int(np.searchsorted(run, a.max_items, side="right"))
    fill_ms, fill_d2h, fill_wall, st = [], [], [], None
    (pb, pi, st), fill_log = logged(lambda: g.potential_friends(lo, fill_hi))
    for _ in range(a.reps):
        t0 = time.time()
        pb2, pi2, st = g.potential_friends(lo, fill_hi)
        fill_wall.append((time.time() - t0) * 1e3)
        assert pb2.tobytes() == pb.tobytes() and pi2.tobytes() == pi.tobytes()
        del pi2
        fill_ms.append(st["kernel_ms"])
        fill_d2h.append(st["d2h_ms"])
    fill_items = st["edges_examined"]
    fill_med = float(np.median(fill_ms))
    # the filling call's device time holds its own counting pass; what the fill adds is the difference to a sizing call
    # over the same rows
    g.potential_friend_counts(lo, fill_hi)
    count_again = [0.0]
    for _ in range(a.reps):
        g.potential_friend_counts(lo, fill_hi)
        count_again.append(g.last_stats["kernel_ms"])
    count_same = float(np.median(count_again[1:])) if a.reps else g.last_stats["kernel_ms"]
    print("potential_friends rmat%d ef%d permute %d: V %d, E %d, generated in %.2f s; rows [%d, %d), filled [%d, %d)"
          % (a.scale, a.ef, a.permute, V, g.E, gen_s, lo, hi, lo, fill_hi))
    print("  pass   rows [lo, hi)            wave-rows  block-rows bitmap-rows  overflowed       wave-items      block-items     bitmap-items")
    for r in log + fill_log[1:]:
        print("  %-5s  [%9d, %9d)  %10d  %10d  %10d  %10d  %15d  %15d  %15d" % ((r["mode"], r["lo"], r["hi"]) + tuple(r["rows"]) + (r["overflowed"],)
                                                                                 + tuple(r["items"])))
    out = {"scale": a.scale, "ef": a.ef, "permute": a.permute, "V": V, "E": g.E, "rows": [lo, hi], "two_hop_items": items,
           "total": int(run[-1]) if len(run) else 0, "largest_set": int(counts.max()) if len(counts) else 0,
           "nonempty": first["vertices_reached"],
           "sizing_first_kernel_ms": round(first["kernel_ms"], 3), "sizing_kernel_ms": [round(x, 3) for x in size_ms],
           "sizing_median_ms": round(size_med, 3), "sizing_gitems_s": round(items / (size_med * 1e-3) * 1e-9, 3),
           "filled_rows": [lo, fill_hi], "filled_two_hop_items": fill_items, "filled_total": int(pb[-1]),
           "fill_call_kernel_ms": [round(x, 3) for x in fill_ms], "fill_call_median_ms": round(fill_med, 3),
           "count_pass_same_rows_ms": round(count_same, 3), "fill_pass_ms": round(fill_med - count_same, 3),
           "fill_call_gitems_s": round(2 * fill_items / (fill_med * 1e-3) * 1e-9, 3),
           "fill_d2h_ms": round(float(np.median(fill_d2h)), 3), "fill_call_wall_ms": round(float(np.median(fill_wall)), 3),
           "batches": st["iterations"]}
    if a.aa:
        g.adamic_adar()
        aa_ms = []
        for _ in range(max(a.reps, 1)):
            g.adamic_adar()
            aa_ms.append(g.last_stats["kernel_ms"])
        aa_items = g.last_stats["edges_examined"]
        aa_med = float(np.median(aa_ms))
        out.update({"adamic_adar_items": aa_items, "adamic_adar_ms": round(aa_med, 3),
                    "adamic_adar_gitems_s": round(aa_items / (aa_med * 1e-3) * 1e-9, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
