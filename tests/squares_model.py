"""Two independent one-thread forms of gmx_squares (gmx.h): the 4-cycles of the stored slots read as an undirected simple
graph, N(v) = { u != v : v -> u or u -> v is stored }, in total and through every vertex; what the log line's classes and
batches must be for a call's knobs; the named shapes with their closed forms.

  squares_definition   A = the simple symmetric adjacency, P = A A off the diagonal: count[v] = sum over w != v of C(P[v, w], 2),
                       squares = sum(count) / 4.  A dense float64 product, exact here (entries below 2^53): keep V <= 4096.
  squares_schedule     the device's walk.  The vertices are renumbered by ascending (|N|, id) (kclique_model.orientation;
                       ordered=False: the ids are kept).  Every square has one highest vertex u; for v in DOWN'(u) and w in
                       N'(v), w < u, the wedge u - v - w is counted into c(w); the squares with top u and opposite w number
                       C(c(w), 2); per wedge x = c(w) - 1 goes to v, and to u and w in a doubled accumulator."""
from math import comb

import numpy as np

WAVE_MAX, LDS_SLOTS, SPLIT, BATCH_BYTES = 128, 4096, 4096, 1 << 30   # the defaults of gmx_squares.hip
WAVE_MAX_TOP, LDS_SLOTS_MIN, LDS_SLOTS_TOP, MAX_PARTS = 128, 64, 18432, 1024


def _simple_pairs(V, begin, idx):
    """(a, b) of every ordered pair of distinct neighbours, each once, sorted by (a, b)."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin))
    keep = rows != idx
    s, d = rows[keep], idx[keep]
    keys = np.unique(np.concatenate([s * V + d, d * V + s])) if V else np.zeros(0, np.int64)
    return (keys // V, keys % V) if V else (keys, keys)


def squares_definition(V, begin, idx):
    """dict(count[int64, V] by the caller's id, squares)."""
    a, b = _simple_pairs(V, begin, idx)
    A = np.zeros((V, V), np.float64)
    A[a, b] = 1.0
    P = A @ A
    np.fill_diagonal(P, 0.0)
    count = (P * (P - 1.0) / 2.0).sum(axis=1)
    assert V == 0 or (P.max() < 2.0 ** 26 and count.max() < 2.0 ** 53)
    count = count.astype(np.int64)
    total = int(count.sum())
    assert total % 4 == 0
    return {"count": count, "squares": total // 4}


def plan_ids(V, a, ordered=True):
    """perm[caller's id -> plan id] for the first ends `a` of the simple pairs: kclique_model.orientation's."""
    order = np.argsort(np.bincount(a, minlength=V), kind="stable") if ordered else np.arange(V)
    perm = np.empty(V, np.int64)
    perm[order] = np.arange(V)
    return perm


def squares_schedule(V, begin, idx, ordered=True):
    """dict(count[int64, V] by the caller's id, squares, D[int64, V] and W[int64, V] by plan id, wedges = the sum of W over
    the vertices with D >= 2, up = |UP'|)."""
    a, b = _simple_pairs(V, begin, idx)
    perm = plan_ids(V, a, ordered)
    pa, pb = perm[a], perm[b]
    keys = np.sort(pa * V + pb)
    ra, rb = (keys // V, keys % V) if V else (keys, keys)
    nb = np.concatenate([[0], np.cumsum(np.bincount(ra, minlength=V))]).astype(np.int64)
    # the slot (u, v), v < u: |{ w in N'(v) : w < u }| = the position of u in v's sorted row = that of the mirrored slot
    down = rb < ra
    mirror = np.searchsorted(keys, rb * V + ra)
    pre = (mirror - nb[rb])[down]
    du, dv = ra[down], rb[down]
    D = np.bincount(du, minlength=V).astype(np.int64)
    W = np.bincount(du, weights=pre, minlength=V).astype(np.int64)
    db = np.concatenate([[0], np.cumsum(D)])
    mid, end2 = np.zeros(V, np.int64), np.zeros(V, np.int64)
    squares = 0
    for u in np.nonzero((D >= 2) & (W > 0))[0].tolist():
        vs, ln = dv[db[u]:db[u + 1]], pre[db[u]:db[u + 1]]
        off = np.cumsum(ln) - ln
        at = np.repeat(nb[vs] - off, ln) + np.arange(int(W[u]))
        ws, wv = rb[at], np.repeat(vs, ln)
        assert np.all(ws < u)
        c = np.bincount(ws, minlength=u)
        squares += int((c * (c - 1) // 2).sum())
        x = c[ws] - 1
        np.add.at(mid, wv, x)
        np.add.at(end2, ws, x)
        end2[u] += int(x.sum())
    assert not (end2 & 1).any()
    cnt = mid + end2 // 2
    live = D >= 2
    return {"count": cnt[perm] if V else np.zeros(0, np.int64), "squares": squares, "D": D, "W": W, "wedges": int(W[live].sum()), "up": int(D.sum())}


def brute_force(V, begin, idx):
    """(count, squares) over every 4-subset: each of its three cyclic orders that is a cycle is a square."""
    from itertools import combinations
    a, b = _simple_pairs(V, begin, idx)
    A = np.zeros((V, V), bool)
    A[a, b] = True
    count, squares = np.zeros(V, np.int64), 0
    for p, q, r, s in combinations(range(V), 4):
        n = int(A[p, q] and A[q, r] and A[r, s] and A[s, p]) + int(A[p, q] and A[q, s] and A[s, r] and A[r, p]) + int(A[p, r] and A[r, q] and A[q, s] and A[s, p])
        if n:
            squares += n
            count[[p, q, r, s]] += n
    return count, squares


# ---- what the log line must show
def knobs_in_force(wave_max=WAVE_MAX, lds_slots=LDS_SLOTS, split=SPLIT, batch_bytes=BATCH_BYTES, **others):
    return {"wave_max": min(max(int(wave_max), 0), WAVE_MAX_TOP), "lds_slots": min(max(int(lds_slots), LDS_SLOTS_MIN), LDS_SLOTS_TOP),
            "split": max(int(split), 1), "batch_bytes": max(int(batch_bytes), 1)}


def classes_of(D, W, **knobs):
    """The items fields and the batches of the log line for the schedule's D and W (by plan id) under these knobs."""
    k = knobs_in_force(**knobs)
    D, W = np.asarray(D, np.int64), np.asarray(W, np.int64)
    live = D >= 2
    wave = live & (W <= k["wave_max"]) & (k["wave_max"] > 0)
    block = live & ~wave & (W <= k["lds_slots"] // 2)
    glob = live & ~wave & ~block
    key = np.where(live, W + 1, 0)
    order = np.argsort(key, kind="stable")
    ug = order[glob[order]]            # the global class in list order: ascending W, ties by id
    words = lambda u: (max(int(u), 1) + 63) // 64 * 64
    budget, batches, a = k["batch_bytes"] // 4, 0, 0
    while a < len(ug):
        b, stride = a + 1, words(ug[a])
        while b < len(ug) and (b + 1 - a) * max(stride, words(ug[b])) <= budget:
            stride = max(stride, words(ug[b]))
            b += 1
        batches += 1
        a = b
    return {"wave": int(wave.sum()), "block": int(block.sum()), "glob": int(glob.sum()), "split": int((glob & (W > k["split"])).sum()),
            "skipped": int((~live).sum()), "batches": batches}


# ---- named shapes (also uploaded by the GPU tests): (V, src, dst), and their closed forms: (count[int64, V], squares)
def cycle(n):
    return n, np.arange(n), (np.arange(n) + 1) % n


def path(n):
    return n, np.arange(n - 1), np.arange(1, n)


def star(n):
    """Vertex 0 joined to n leaves."""
    return n + 1, np.zeros(n, np.int64), np.arange(1, n + 1)


def binary_tree(n):
    return n, (np.arange(1, n) - 1) // 2, np.arange(1, n)


def clique(n):
    a, b = np.nonzero(np.triu(np.ones((n, n), bool), 1))
    return n, a, b


def clique_counts(n):
    return np.full(n, 3 * comb(n - 1, 3), np.int64), 3 * comb(n, 4)


def bipartite(a, b):
    """K_{a,b}: the a side holds the ids 0 .. a - 1."""
    s, d = np.nonzero(np.ones((a, b), bool))
    return a + b, s, d + a


def bipartite_counts(a, b):
    return np.concatenate([np.full(a, (a - 1) * comb(b, 2)), np.full(b, (b - 1) * comb(a, 2))]).astype(np.int64), comb(a, 2) * comb(b, 2)


def hypercube(d):
    v = np.arange(1 << d)
    s = np.concatenate([v[(v >> i) & 1 == 0] for i in range(d)])
    t = np.concatenate([v[(v >> i) & 1 == 0] | (1 << i) for i in range(d)])
    return 1 << d, s, t


def hypercube_counts(d):
    return np.full(1 << d, comb(d, 2), np.int64), (1 << d) // 4 * comb(d, 2) if d >= 2 else 0


def grid(m, n):
    """m rows of n vertices, row-major."""
    v = np.arange(m * n).reshape(m, n)
    return m * n, np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])


def grid_counts(m, n):
    cells = np.zeros((m + 1, n + 1), np.int64)
    cells[1:m, 1:n] = 1                 # cell (i, j) has its corners at rows i - 1, i and columns j - 1, j
    count = cells[:-1, :-1] + cells[:-1, 1:] + cells[1:, :-1] + cells[1:, 1:]
    return count.ravel(), (m - 1) * (n - 1)
