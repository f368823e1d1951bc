#!/usr/bin/env python3
"""gmx_random_walk_sampling on RMAT-<scale> (p_size 0.1, p_jump 0.15 unless given), for 1024 tokens and V / 16 tokens, in one process:

  * the call's line: rounds grid + tail, tail launches, sort rounds, dense rounds, draws, count, host-clock ms, next to kernel_ms:
    a warm-up, then --reps calls; median and min-max;
  * per grid round (the library's GMX_RW_LOG=2 lines, one call): live vertices, tokens, draws, vertices touched, how they were
    put in order, ms -- the first rounds and the mean; per tail launch: rounds, ms, ms per round;
  * for each token count the regimes: the default, GMX_RW_TAIL=0 (grid rounds; the ordering chosen per round), and GMX_RW_TAIL=0
    with GMX_RW_ORDER=dense and =sort forced: what the sparse ordering and the tail are worth;
  * the yardstick "one sweep of the rows": kernel_ms of gmx_avg_teen_cnt on the same graph.

  rw_prof.py --scale 22 [--permute] [--reps 3] [--p-size 0.1] [--p-jump 0.15]"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KNOBS = ("GMX_RW_TAIL", "GMX_RW_ORDER")
X0 = 0x0AA849495101
LINE = re.compile(r"gmx random_walk_sampling: V (\d+) tokens (\d+); tail (\d+); batches (\d+); rounds (\d+) grid \+ (\d+) tail; tail launches (\d+); "
                  r"sort rounds (\d+) dense rounds (\d+); draws (\d+); count (\d+); ms ([0-9.]+)")
FIELDS = ("V", "tokens", "tail_from", "batches", "grid_rounds", "tail_rounds", "tail_launches", "sort_rounds", "dense_rounds", "draws", "count", "ms")
ROUND = re.compile(r"gmx random_walk_sampling round (\d+): live (\d+) tokens (\d+) draws (\d+) next (\d+) (sort|dense|none) count (\d+) ms ([0-9.]+)")
TAIL = re.compile(r"gmx random_walk_sampling tail launch (\d+): rounds (\d+) live (\d+) count (\d+) ms ([0-9.]+)")


def call(g, p_size, p_jump, tokens, level="1", **env):
    """(stats, fields of the library's line, per-round lines, per-tail-launch lines) of one call; the lines are read from stderr."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["GMX_RW_LOG"] = level
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = g.random_walk_sampling(p_size, p_jump, tokens, X0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    for k in KNOBS + ("GMX_RW_LOG",):
        os.environ.pop(k, None)
    m = LINE.search(text)
    if not m:
        sys.exit("rw_prof: no log line in %r" % text[-500:])
    f = {k: (float(v) if k == "ms" else int(v)) for k, v in zip(FIELDS, m.groups())}
    rounds = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), r[5], int(r[6]), float(r[7])) for r in ROUND.findall(text)]
    tails = [(int(t[0]), int(t[1]), int(t[2]), int(t[3]), float(t[4])) for t in TAIL.findall(text)]
    return out[5], f, rounds, tails, out


def spread(ms):
    return "median %10.3f ms  min %10.3f  max %10.3f" % (statistics.median(ms), min(ms), max(ms))


def one_pass(g, tag, reps):
    """kernel_ms of gmx_avg_teen_cnt: every slot read once, one gather and one add per slot."""
    age = (np.arange(g.V, dtype=np.int64) * 2654435761 % 60).astype(np.int32)
    g.avg_teen_cnt(age, 25)
    ms = [g.avg_teen_cnt(age, 25)[2]["kernel_ms"] for _ in range(reps)]
    print("%s one sweep of the rows (gmx_avg_teen_cnt) kernel_ms %s" % (tag, spread(ms)), flush=True)
    return statistics.median(ms)


def regime(g, tag, a, tokens, base, want, **env):
    call(g, a.p_size, a.p_jump, tokens, **env)               # warm-up
    st, f, rounds, tails, out = call(g, a.p_size, a.p_jump, tokens, level="2", **env)
    key = (out[0].tobytes(), out[1].tobytes(), out[2:5])
    if want and want[0] != key:
        sys.exit("rw_prof: %s differs from the first regime's result" % tag)
    want[:] = [key]
    print("%s V %d tokens %d: count %d, rounds %d grid + %d tail in %d launches, sort rounds %d dense rounds %d, draws %d, batches %d"
          % (tag, f["V"], f["tokens"], f["count"], f["grid_rounds"], f["tail_rounds"], f["tail_launches"], f["sort_rounds"], f["dense_rounds"],
             f["draws"], f["batches"]))
    for r, live, tok, draws, nxt, how, cnt, ms in (rounds if len(rounds) <= 6 else rounds[:4] + rounds[-2:]):
        print("%s   round %5d: live %9d tokens %9d draws %10d touched %9d %-5s count %9d  %8.3f ms" % (tag, r, live, tok, draws, nxt, how, cnt, ms))
    if rounds:
        for how in ("sort", "dense"):
            ms = [r[7] for r in rounds if r[5] == how]
            if ms:
                print("%s   %d %s rounds (logged, synchronised): mean %.3f ms, mean live %.0f" % (tag, len(ms), how, statistics.mean(ms),
                                                                                             statistics.mean([r[1] for r in rounds if r[5] == how])))
    for k, r, live, cnt, ms in tails[:3]:
        print("%s   tail launch %d: rounds %d live %d count %d  %8.3f ms = %.4f ms per round" % (tag, k, r, live, cnt, ms, ms / max(r, 1)))
    fs, kms = [], []
    for _ in range(a.reps):
        st, f, _, _, _ = call(g, a.p_size, a.p_jump, tokens, **env)
        fs.append(f["ms"])
        kms.append(st["kernel_ms"])
    nr = max(f["grid_rounds"] + f["tail_rounds"], 1)
    print("%s host ms   %s" % (tag, spread(fs)))
    print("%s kernel_ms %s = %.4f ms per round = %.2f x one sweep for the call" % (tag, spread(kms), statistics.median(kms) / nr,
                                                                              statistics.median(kms) / base), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--permute", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--p-size", type=float, default=0.1)
    ap.add_argument("--p-jump", type=float, default=0.15)
    a = ap.parse_args()
    import gmx
    gmx.require_device()
    V = 1 << a.scale
    name = "RMAT-%d%s" % (a.scale, "p" if a.permute else "")
    g = gmx.Graph.rmat(V, 16 * V, 1997, 0.57, 0.19, 0.19, a.permute, flags=gmx.GMX_GRAPH_NO_REVERSE)
    base = one_pass(g, name, a.reps)
    for tokens in (1024, V // 16):
        want = []
        regime(g, "%s %d tokens default" % (name, tokens), a, tokens, base, want)
        regime(g, "%s %d tokens GMX_RW_TAIL=0" % (name, tokens), a, tokens, base, want, GMX_RW_TAIL="0")
        regime(g, "%s %d tokens GMX_RW_TAIL=0 GMX_RW_ORDER=dense" % (name, tokens), a, tokens, base, want, GMX_RW_TAIL="0", GMX_RW_ORDER="dense")
        regime(g, "%s %d tokens GMX_RW_TAIL=0 GMX_RW_ORDER=sort" % (name, tokens), a, tokens, base, want, GMX_RW_TAIL="0", GMX_RW_ORDER="sort")
    g.free()


if __name__ == "__main__":
    main()
