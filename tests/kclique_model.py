"""A one-thread model of gmx_kclique (gmx.h): the k-cliques of the stored slots read as an undirected simple graph,
N(v) = { u != v : v -> u or u -> v is stored }, in total and through every vertex.

The model runs the device's recursion on Python-int bit sets.  The vertices are renumbered by ascending (|N|, id), as
test_clustering_host's model does it (ordered=False: the ids are kept), UP'(v) is the set of neighbours above v, and a k-clique
is found once, at its lowest vertex v:  P_1 = UP'(v);  choose i_1 in P_1, P_2 = P_1 & UP'(i_1);  choose i_2 in P_2, ... after
k - 2 choices the last set is only popcounted.  A chosen vertex gets its subtree's total when the recursion returns, the
members of the last set +1 each, v the vertex total.  (The device numbers UP'(v) locally; the sets are the same.  The +1
credits are summed in bit planes, one carry-save addition per last set, so that the model does not walk them bit by bit.)"""
from math import comb

import numpy as np

_popcount = int.bit_count if hasattr(int, "bit_count") else (lambda x: bin(x).count("1"))


def _bits(x):
    while x:
        b = x & -x
        yield b.bit_length() - 1
        x ^= b


def orientation(V, begin, idx, ordered=True):
    """(perm[caller's id -> plan id], up[plan id -> bit set of the plan ids of UP'], deg) of the forward CSR."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin))
    keep = rows != idx
    s, d = rows[keep], idx[keep]
    keys = np.unique(np.concatenate([s * V + d, d * V + s])) if V else np.zeros(0, np.int64)
    a, b = (keys // V, keys % V) if V else (keys, keys)
    deg = np.bincount(a, minlength=V).astype(np.int64)
    order = np.argsort(deg, kind="stable") if ordered else np.arange(V)
    perm = np.empty(V, np.int64)
    perm[order] = np.arange(V)
    pa, pb = perm[a], perm[b]
    up = [0] * V
    for x, y in zip(pa[pa < pb].tolist(), pb[pa < pb].tolist()):
        up[x] |= 1 << y
    return perm, up, deg


def kclique_model(V, begin, idx, k, ordered=True):
    """dict(count[int64, V] by the caller's id, cliques, up = |UP'|, up_len[int64, V] = |UP'(v)| by plan id)."""
    assert 3 <= k <= 8
    perm, up, _ = orientation(V, begin, idx, ordered)
    cnt = [0] * V          # the chosen vertices' and v's credits, by plan id
    planes = []            # the last sets' +1 credits: bit plane p holds bit p of every vertex's sum

    def add(q):
        for i in range(len(planes)):
            planes[i], q = planes[i] ^ q, planes[i] & q
            if not q:
                return
        planes.append(q)

    def walk(P, left):
        if left == 0:
            if P:
                add(P)
            return _popcount(P)
        total = 0
        for j in _bits(P):
            Q = P & up[j]
            if Q:
                sub = walk(Q, left - 1)
                cnt[j] += sub
                total += sub
        return total

    cliques = 0
    for v in range(V):
        if up[v]:
            t = walk(up[v], k - 2)
            cnt[v] += t
            cliques += t
    for p, plane in enumerate(planes):
        for j in _bits(plane):
            cnt[j] += 1 << p
    count = np.array([cnt[x] for x in perm.tolist()], np.int64) if V else np.zeros(0, np.int64)
    up_len = np.array([_popcount(x) for x in up], np.int64)
    return {"count": count, "cliques": cliques, "up": int(up_len.sum()), "up_len": up_len}


# ---- named shapes (also uploaded by the GPU tests): (V, src, dst), and their closed forms: (count[int64, V], cliques)
def clique(n):
    a, b = np.nonzero(np.triu(np.ones((n, n), bool), 1))
    return n, a, b


def clique_counts(n, k):
    return np.full(n, comb(n - 1, k - 1), np.int64), comb(n, k)


def multipartite(sizes):
    """The complete multipartite graph: part p holds the next sizes[p] ids, two vertices are joined iff their parts differ."""
    part = np.repeat(np.arange(len(sizes)), sizes)
    a, b = np.nonzero(np.triu(part[:, None] != part[None, :], 1))
    return len(part), a, b


def esym(sizes, j):
    """e_j(sizes), the elementary symmetric polynomial: the ways to take one vertex from each of j different parts."""
    e = [1] + [0] * j
    for s in sizes:
        for i in range(j, 0, -1):
            e[i] += e[i - 1] * s
    return e[j]


def multipartite_counts(sizes, k):
    sizes = list(sizes)
    per = [esym(sizes[:p] + sizes[p + 1:], k - 1) for p in range(len(sizes))]
    return np.repeat(np.array(per, np.int64), sizes), esym(sizes, k)


def hub_over(shape):
    """One extra vertex with id 0 joined to all the others, which keep their order behind it."""
    V, s, d = shape
    return V + 1, np.concatenate([np.zeros(V, np.int64), np.asarray(s) + 1]), np.concatenate([np.arange(1, V + 1), np.asarray(d) + 1])


def hub_over_counts(counts_of, k):
    """counts_of(j) -> (count, total) of the shape's j-cliques, j >= 2: a k-clique of the hubbed graph is one of the shape's,
    or the hub with one of its (k-1)-cliques."""
    ck, tk = counts_of(k)
    cl, tl = counts_of(k - 1)
    return np.concatenate([[tl], ck + cl]).astype(np.int64), tk + tl
