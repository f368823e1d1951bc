"""A one-thread model of gmx_ktruss (gmx.h): per-edge triangle support and truss numbers of the stored slots read as an
undirected simple graph, N(v) = { u != v : v -> u or u -> v is stored }.

support(e) = |N(a) & N(b)| for e = {a, b}; truss(e) = the largest k such that e lies in a subgraph in which every edge is in at
least k - 2 triangles of that subgraph.  The model runs the device's synchronous schedule, which fixes the statistics:
  level   s = the smallest support among the live edges; round 0 of the level queues every live edge with support <= s;
  round   every queued edge e gets truss s + 2.  For every triangle {e, e1, e2} none of whose edges was removed in an earlier
          round: both others queued in this round -> nothing; only e1 queued -> e2 is decremented iff id(e) < id(e1) (and the
          mirror image); neither -> both are decremented.  The decrement that reaches s queues the edge for the next round.
Edge ids are positions in UP' (the edges (x, y), x < y, in the ascending-degree numbering of test_clustering_host's model,
row-major and sorted); only the tie-break between two queued edges of a triangle reads them, and no result depends on it."""
import numpy as np

LIVE = 1 << 62


def ktruss_model(V, begin, idx, peel=True):
    """dict(edges[(a, b) by the caller's ids, a < b, sorted], support[int32, E] and truss[int32, E] by forward slot,
    edge_support, edge_truss [by the position in edges], max_truss, num_edges, triangles, levels, rounds, scanned, slots
    (the sum over the edges of the smaller end degree), top (edges of the largest truss number), rounds_per_level)."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    E = len(idx)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin))
    keep = rows != idx
    lo, hi = np.minimum(rows, idx)[keep], np.maximum(rows, idx)[keep]
    keys = np.unique(lo * V + hi) if V else np.zeros(0, np.int64)
    U = len(keys)
    ea, eb = ((keys // V).tolist(), (keys % V).tolist()) if V else ([], [])
    # the device's edge ids: positions in UP' of the degree-ordered plan
    deg = np.bincount(np.concatenate([keys // V, keys % V]).astype(np.int64), minlength=V) if V else np.zeros(0, np.int64)
    order = np.argsort(deg, kind="stable")
    perm = np.empty(V, np.int64)
    perm[order] = np.arange(V)
    if U:
        pa, pb = perm[keys // V], perm[keys % V]
        dev_id = np.empty(U, np.int64)
        dev_id[np.argsort(np.minimum(pa, pb) * V + np.maximum(pa, pb))] = np.arange(U)
        dev_id = dev_id.tolist()
    else:
        dev_id = []
    nbr = [dict() for _ in range(V)]   # x -> edge (position in keys), live edges only
    for e in range(U):
        nbr[ea[e]][eb[e]] = e
        nbr[eb[e]][ea[e]] = e
    sup0 = [0] * U
    for e in range(U):
        a, b = nbr[ea[e]], nbr[eb[e]]
        if len(a) > len(b):
            a, b = b, a
        sup0[e] = sum(1 for x in a if x in b)
    slots = int(np.minimum(deg[keys // V], deg[keys % V]).sum()) if U else 0
    truss = [0] * U
    levels = rounds = scanned = top = 0
    per_level = []
    s = -2
    if peel and U:
        sup = list(sup0)
        rem = [LIVE] * U
        live = list(range(U))
        rnd = 0
        while True:
            cand = [e for e in live if rem[e] == LIVE]
            if not cand:
                break
            scanned += len(live)
            s = min(sup[e] for e in cand)
            levels += 1
            queue = [e for e in cand if sup[e] <= s]
            live = [e for e in cand if sup[e] > s]
            for e in queue:
                rem[e] = rnd
            top = 0
            r0 = rnd
            while queue:
                nxt = []
                for e in queue:
                    truss[e] = s + 2
                    a, b = ea[e], eb[e]
                    na, nb = nbr[a], nbr[b]
                    if len(na) > len(nb):
                        na, nb = nb, na
                    for x, e1 in na.items():
                        e2 = nb.get(x)
                        if e2 is None:
                            continue
                        in1, in2 = rem[e1] == rnd, rem[e2] == rnd
                        if in1 and in2:
                            continue
                        if in1:
                            hit = (e2,) if dev_id[e] < dev_id[e1] else ()
                        elif in2:
                            hit = (e1,) if dev_id[e] < dev_id[e2] else ()
                        else:
                            hit = (e1, e2)
                        for t in hit:
                            sup[t] -= 1
                            if sup[t] == s:
                                rem[t] = rnd + 1
                                nxt.append(t)
                for e in queue:   # gone before the next round: "removed in an earlier round"
                    del nbr[ea[e]][eb[e]]
                    del nbr[eb[e]][ea[e]]
                top += len(queue)
                rnd += 1
                queue = nxt
            per_level.append(rnd - r0)
        rounds = rnd
    edge_support, edge_truss = np.array(sup0, np.int32), np.array(truss, np.int32)
    support, tr = np.zeros(E, np.int32), np.zeros(E, np.int32)
    if U:
        at = np.searchsorted(keys, (np.minimum(rows, idx) * V + np.maximum(rows, idx))[keep])
        support[keep] = edge_support[at]
        tr[keep] = edge_truss[at]
    return {"edges": list(zip(ea, eb)), "support": support, "truss": tr, "edge_support": edge_support, "edge_truss": edge_truss,
            "max_truss": s + 2 if rounds else 0, "num_edges": U, "triangles": int(edge_support.sum(dtype=np.int64)) // 3, "levels": levels,
            "rounds": rounds, "scanned": scanned, "slots": slots if peel else 0, "top": top if rounds else 0, "rounds_per_level": per_level}


# ---- named shapes (also uploaded by the GPU tests): (V, src, dst)
def two_cliques_and_a_path():
    """K_5 on 0 .. 4 and K_9 on 4 .. 12 sharing vertex 4, and the path 12 - 13 - 14 - 15."""
    s, d = [], []
    for lo, hi in ((0, 5), (4, 13)):
        for a in range(lo, hi):
            for b in range(a + 1, hi):
                s.append(a)
                d.append(b)
    for a in (12, 13, 14):
        s.append(a)
        d.append(a + 1)
    return 16, np.array(s), np.array(d)


def book(m):
    """The spine {0, 1} and the pages {0, p}, {1, p} for p = 2 .. m + 1."""
    p = np.arange(2, m + 2)
    return m + 2, np.concatenate([[0], np.zeros(m, np.int64), np.ones(m, np.int64)]), np.concatenate([[1], p, p])


def star_with_a_triangle(n):
    """Leaves 1 .. n of the centre 0, and the edge {1, 2}."""
    return n + 1, np.concatenate([np.zeros(n, np.int64), [2]]), np.concatenate([np.arange(1, n + 1), [1]])


def triangulated_grid(n):
    """(i, j) - (i + 1, j), (i, j) - (i, j + 1) and (i, j) - (i + 1, j + 1) on n x n vertices."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = (i * n + j)
    s = np.concatenate([v[:-1, :].ravel(), v[:, :-1].ravel(), v[:-1, :-1].ravel()])
    d = np.concatenate([v[1:, :].ravel(), v[:, 1:].ravel(), v[1:, 1:].ravel()])
    return n * n, s, d
