"""Two independent one-thread forms of gmx_graphlets (gmx.h): the census of the connected subgraphs on 2, 3 and 4 vertices of
the stored slots read as an undirected simple graph, N(v) = { u != v : v -> u or u -> v is stored }, per vertex by orbit
(ORCA's numbering, the 15-entry graphlet degree vector) and in total (G0 .. G8); the named shapes with their closed forms.

  graphlets_definition  every 3- and 4-subset of the vertices, classified by the degree sequence of the subgraph it induces,
                        credits its vertices' orbits.  Dense and cubic in memory: keep V <= 256.  Induced counts only.
  graphlets_formulas    the equations of gmx_graphlets.hip on d, t(e) and T, with squares_model and kclique_model supplying n8
                        and n14, and the transform to induced counts.

Orbits: 0 degree | 1 end, 2 middle of the path on 3 | 3 triangle | 4 end, 5 inner of the path on 4 | 6 leaf, 7 centre of the claw
| 8 4-cycle | 9 tail's end, 10 far corners, 11 carrying corner of the paw | 12 degree-2, 13 degree-3 corners of the diamond | 14 K4.
Totals: edges, paths on 3, triangles, paths on 4, claws, 4-cycles, paws, diamonds, 4-cliques."""
from math import comb

import numpy as np
import scipy.sparse as sp

from kclique_model import kclique_model
from squares_model import _simple_pairs, bipartite, clique, cycle, grid, grid_counts, path, squares_schedule, star

ORBITS, GRAPHLETS = 15, 9
NAMES = ("edges", "paths3", "triangles", "paths4", "claws", "cycles4", "paws", "diamonds", "cliques4")
# totals[j] = sum(gdv[:, TOTAL_OF[j][0]]) / TOTAL_OF[j][1], in either convention
TOTAL_OF = ((0, 2), (2, 1), (3, 3), (4, 2), (7, 1), (8, 4), (11, 1), (13, 2), (14, 4))


def totals_of(gdv):
    col = gdv.sum(axis=0) if len(gdv) else np.zeros(ORBITS, np.int64)
    out = []
    for k, div in TOTAL_OF:
        assert int(col[k]) % div == 0, (k, div, int(col[k]))
        out.append(int(col[k]) // div)
    return np.array(out, np.int64)


def identities_hold(gdv):
    """The sum identities every graphlet gives, which gmx_graphlets verifies before it returns (either convention)."""
    c = [int(x) for x in (gdv.sum(axis=0) if len(gdv) else np.zeros(ORBITS, np.int64))]
    return c[4] == c[5] and c[6] == 3 * c[7] and c[9] == c[11] and c[10] == 2 * c[11] and c[12] == c[13] and c[1] == 2 * c[2]


def nonzero_of(gdv):
    """stats.vertices_reached: the vertices with a non-zero 4-node orbit."""
    return int((gdv[:, 4:] != 0).any(axis=1).sum()) if len(gdv) else 0


def _dense(V, begin, idx):
    a, b = _simple_pairs(V, begin, idx)
    A = np.zeros((V, V), np.uint8)
    A[a, b] = 1
    return A


# ---- the definition
# orbit of a vertex of degree 1, 2, 3 in the induced subgraph, by graphlet
_P4, _CLAW, _C4, _PAW, _DIAMOND, _K4 = range(6)
_ORBIT = np.full((6, 4), -1, np.int64)
_ORBIT[_P4, 1], _ORBIT[_P4, 2] = 4, 5
_ORBIT[_CLAW, 1], _ORBIT[_CLAW, 3] = 6, 7
_ORBIT[_C4, 2] = 8
_ORBIT[_PAW, 1], _ORBIT[_PAW, 2], _ORBIT[_PAW, 3] = 9, 10, 11
_ORBIT[_DIAMOND, 2], _ORBIT[_DIAMOND, 3] = 12, 13
_ORBIT[_K4, 3] = 14


def graphlets_definition(V, begin, idx):
    """dict(gdv[int64, V x 15] by the caller's id, totals[int64, 9]): induced counts, by enumeration of the subsets."""
    A = _dense(V, begin, idx)
    gdv = np.zeros((V, ORBITS), np.int64)
    gdv[:, 0] = A.sum(axis=1)
    # 3-subsets a < b < c: two edges a path (the vertex of degree 2 its middle), three a triangle
    b2, c2 = np.triu_indices(V, 1)
    ebc = A[b2, c2]
    first = np.searchsorted(b2, np.arange(V) + 1)   # the pairs with b > a are a suffix
    for a in range(V):
        b, c, bc = b2[first[a]:], c2[first[a]:], ebc[first[a]:]
        ab, ac = A[a, b], A[a, c]
        m = ab + ac + bc
        keep = m >= 2
        b, c, bc, ab, ac, m = b[keep], c[keep], bc[keep], ab[keep], ac[keep], m[keep]
        tri = m == 3
        for vtx, deg in ((np.full(len(b), a), ab + ac), (b, ab + bc), (c, ac + bc)):
            np.add.at(gdv[:, 3], vtx[tri], 1)
            np.add.at(gdv[:, 2], vtx[~tri & (deg == 2)], 1)
            np.add.at(gdv[:, 1], vtx[~tri & (deg == 1)], 1)
    # 4-subsets a < b < c < d: the triples b < c < d and their three edges once, then every a below them
    if V >= 4:
        n = V
        bi = np.repeat(np.arange(n), [comb(n - 1 - x, 2) for x in range(n)]).astype(np.int32)
        ci = np.concatenate([np.repeat(np.arange(x + 1, n), np.arange(n - x - 2, -1, -1)) for x in range(n)]).astype(np.int32) if n >= 3 else np.zeros(0, np.int32)
        di = np.concatenate([np.arange(y + 1, n) for x in range(n) for y in range(x + 1, n)]).astype(np.int32) if n >= 3 else np.zeros(0, np.int32)
        assert len(bi) == len(ci) == len(di) == comb(n, 3)
        ebc, ebd, ecd = A[bi, ci], A[bi, di], A[ci, di]
        inner = ebc + ebd + ecd
        first = np.searchsorted(bi, np.arange(V) + 1)
        for a in range(V):
            s = slice(first[a], None)
            b, c, d = bi[s], ci[s], di[s]
            ab, ac, ad = A[a, b], A[a, c], A[a, d]
            da = ab + ac + ad
            keep = (da > 0) & (da + inner[s] >= 3)
            if not keep.any():
                continue
            b, c, d, ab, ac, ad, da = b[keep], c[keep], d[keep], ab[keep], ac[keep], ad[keep], da[keep]
            bc, bd, cd = ebc[s][keep], ebd[s][keep], ecd[s][keep]
            db, dc, dd = ab + bc + bd, ac + bc + cd, ad + bd + cd
            conn = (db > 0) & (dc > 0) & (dd > 0)   # three edges or more and no isolated vertex: connected
            m = (da + db + dc + dd) // 2
            top = np.maximum(np.maximum(da, db), np.maximum(dc, dd))
            kind = np.select([m == 6, m == 5, (m == 4) & (top == 3), m == 4, top == 3], [_K4, _DIAMOND, _PAW, _C4, _CLAW], _P4)
            for vtx, deg in ((np.full(len(b), a), da), (b, db), (c, dc), (d, dd)):
                orbit = _ORBIT[kind[conn], deg[conn]]
                assert (orbit >= 4).all()
                np.add.at(gdv, (vtx[conn], orbit), 1)
    return {"gdv": gdv, "totals": totals_of(gdv)}


# ---- the formulas
def _c2(x):
    return x * (x - 1) // 2


def induced_from(n):
    """The non-induced counts n[V x 15] -> the induced ones, solved from the bottom up."""
    o = n.copy()
    o14 = n[:, 14]
    o13 = n[:, 13] - 3 * o14
    o12 = n[:, 12] - 3 * o14
    o11 = n[:, 11] - 2 * o13 - 3 * o14
    o10 = n[:, 10] - 2 * o12 - 2 * o13 - 6 * o14
    o9 = n[:, 9] - 2 * o12 - 3 * o14
    o8 = n[:, 8] - o12 - o13 - 3 * o14
    o7 = n[:, 7] - o11 - o13 - o14
    o6 = n[:, 6] - o9 - o10 - 2 * o12 - o13 - 3 * o14
    o5 = n[:, 5] - 2 * o8 - o10 - 2 * o11 - 2 * o12 - 4 * o13 - 6 * o14
    o4 = n[:, 4] - 2 * o8 - 2 * o9 - o10 - 4 * o12 - 2 * o13 - 6 * o14
    for k, col in ((4, o4), (5, o5), (6, o6), (7, o7), (8, o8), (9, o9), (10, o10), (11, o11), (12, o12), (13, o13)):
        o[:, k] = col
    o[:, 2] = n[:, 2] - n[:, 3]
    o[:, 1] = n[:, 1] - 2 * n[:, 3]
    return o


def graphlets_formulas(V, begin, idx, induced=True):
    """dict(gdv[int64, V x 15] by the caller's id, totals[int64, 9], triangles, nonzero, up = the undirected edges)."""
    a, b = _simple_pairs(V, begin, idx)
    if V == 0:
        return {"gdv": np.zeros((0, ORBITS), np.int64), "totals": np.zeros(GRAPHLETS, np.int64), "triangles": 0, "nonzero": 0, "up": 0}
    A = sp.csr_matrix((np.ones(len(a), np.int64), (a, b)), shape=(V, V))
    d = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    Tm = (A @ A).multiply(A).tocsr()             # t(e) on every edge, both directions
    st = np.asarray(Tm.sum(axis=1)).ravel().astype(np.int64)
    T = st // 2
    t = np.asarray(Tm[a, b]).ravel().astype(np.int64) if len(a) else np.zeros(0, np.int64)   # by ordered pair (a, b): a is v, b is u
    du = d[b]
    def row(x):   # the sum over u in N(v), exact in int64
        out = np.zeros(V, np.int64)
        np.add.at(out, a, x)
        return out
    S = row(du - 1)
    n = np.zeros((V, ORBITS), np.int64)
    n[:, 0] = d
    n[:, 1] = S
    n[:, 2] = _c2(d)
    n[:, 3] = T
    n[:, 4] = row(S[b] - (d[a] - 1)) - 2 * T
    n[:, 5] = row((d[a] - 1) * (du - 1) - t)
    n[:, 6] = row(_c2(du - 1))
    n[:, 7] = d * (d - 1) * (d - 2) // 6
    n[:, 8] = squares_schedule(V, begin, idx)["count"]
    n[:, 9] = row(T[b] - t)
    n[:, 10] = row(t * (du - 2))
    n[:, 11] = T * (d - 2)
    M = (Tm - A).tocsr()                          # t(e) - 1 on every edge
    n[:, 12] = np.asarray((A @ M).multiply(A).sum(axis=1)).ravel().astype(np.int64) // 2
    n[:, 13] = row(_c2(t))
    n[:, 14] = kclique_model(V, begin, idx, 4)["count"]
    gdv = induced_from(n) if induced else n
    return {"gdv": gdv, "totals": totals_of(gdv), "triangles": int(T.sum()) // 3, "nonzero": nonzero_of(gdv), "up": len(a) // 2}


# ---- named shapes (squares_model's: (V, src, dst)) and their closed forms: (gdv[int64, V x 15], totals[int64, 9]), induced
def paw():
    """The triangle 0 1 2 with the tail 3 on vertex 2."""
    return 4, np.array([0, 0, 1, 2]), np.array([1, 2, 2, 3])


def diamond():
    """K4 without the edge 2 3."""
    return 4, np.array([0, 0, 0, 1, 1]), np.array([1, 2, 3, 2, 3])


def _closed(V, rows):
    gdv = np.zeros((V, ORBITS), np.int64)
    for vs, orbits in rows:
        for k, x in orbits.items():
            gdv[vs, k] = x
    return gdv, totals_of(gdv)


def clique_gdv(n):
    return _closed(n, [(slice(None), {0: n - 1, 3: comb(n - 1, 2), 14: comb(n - 1, 3)})])


def clique_subgraph_gdv(n):
    """The subgraph (non-induced) counts of K_n: a vertex of a K4 is the end of 6 and the inner vertex of 6 of its 12 paths, a
    leaf of 3 and the centre of 1 of its 4 claws, on all 3 cycles, the tail's end of 3, a far corner of 6 and the carrying corner of
    3 of its 12 paws, a degree-2 and a degree-3 corner of 3 each of its 6 diamonds."""
    q, w = comb(n - 1, 3), comb(n - 1, 2)
    return _closed(n, [(slice(None), {0: n - 1, 1: 2 * w, 2: w, 3: w, 4: 6 * q, 5: 6 * q, 6: 3 * q, 7: q, 8: 3 * q, 9: 3 * q, 10: 6 * q, 11: 3 * q, 12: 3 * q,
                                      13: 3 * q, 14: q})])


def star_gdv(n):
    return _closed(n + 1, [(0, {0: n, 2: comb(n, 2), 7: comb(n, 3)}), (slice(1, None), {0: 1, 1: n - 1, 6: comb(n - 1, 2)})])


def cycle_gdv(n):
    assert n >= 4
    return _closed(n, [(slice(None), {0: 2, 1: 2, 2: 1, 8: 1} if n == 4 else {0: 2, 1: 2, 2: 1, 4: 2, 5: 2})])


def path_gdv(n):
    i = np.arange(n)
    gdv = np.zeros((n, ORBITS), np.int64)
    gdv[:, 0] = (i >= 1).astype(int) + (i <= n - 2)
    gdv[:, 1] = (i >= 2).astype(int) + (i <= n - 3)
    gdv[:, 2] = (i >= 1) & (i <= n - 2)
    gdv[:, 4] = (i >= 3).astype(int) + (i <= n - 4)
    gdv[:, 5] = ((i >= 1) & (i <= n - 3)).astype(int) + ((i >= 2) & (i <= n - 2))
    return gdv, totals_of(gdv)


def bipartite_gdv(a, b):
    side = lambda p, q: {0: q, 1: q * (p - 1), 2: comb(q, 2), 6: q * comb(p - 1, 2), 7: comb(q, 3), 8: (p - 1) * comb(q, 2)}   # a vertex of the side of p, the other side has q
    return _closed(a + b, [(slice(0, a), side(a, b)), (slice(a, None), side(b, a))])


def paw_gdv():
    return _closed(4, [(slice(0, 2), {0: 2, 1: 1, 3: 1, 10: 1}), (2, {0: 3, 2: 2, 3: 1, 11: 1}), (3, {0: 1, 1: 2, 9: 1})])


def diamond_gdv():
    return _closed(4, [(slice(0, 2), {0: 3, 2: 1, 3: 2, 13: 1}), (slice(2, 4), {0: 2, 1: 2, 3: 1, 12: 1})])


def grid_closed(m, n):
    """What has a closed form on the m x n grid (m, n >= 2), which has no triangle: {orbit: column} for the orbits 0, 2, 7, 8
    (the degree by position, C(d, 2), C(d, 3), the cells at the vertex) and the nine totals (the paths on 4: the sum of
    (d_u - 1)(d_v - 1) over the edges, less the four in every cell)."""
    r, c = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    d = ((r > 0).astype(np.int64) + (r < m - 1) + (c > 0) + (c < n - 1))
    p4 = int(((d[:, :-1] - 1) * (d[:, 1:] - 1)).sum() + ((d[:-1, :] - 1) * (d[1:, :] - 1)).sum())
    cells = (m - 1) * (n - 1)
    dv = d.ravel()
    cols = {0: dv, 2: dv * (dv - 1) // 2, 7: dv * (dv - 1) * (dv - 2) // 6, 8: grid_counts(m, n)[0]}
    totals = np.array([m * (n - 1) + n * (m - 1), int(cols[2].sum()), 0, p4 - 4 * cells, int(cols[7].sum()), cells, 0, 0, 0], np.int64)
    return cols, totals


SHAPES = {"K4": (clique(4), clique_gdv(4)), "K5": (clique(5), clique_gdv(5)), "K65": (clique(65), clique_gdv(65)), "paw": (paw(), paw_gdv()),
          "diamond": (diamond(), diamond_gdv()), "C4": (cycle(4), cycle_gdv(4)), "C5": (cycle(5), cycle_gdv(5)), "path9": (path(9), path_gdv(9)),
          "star70": (star(70), star_gdv(70)), "K3,40": (bipartite(3, 40), bipartite_gdv(3, 40)), "grid5x7": (grid(5, 7), None)}
