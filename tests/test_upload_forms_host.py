"""Uploaded CSRs with rows out of order, host side (no GPU): the graphs test_gpu_upload_forms.py uploads, the properties
each is there for, and the premise of its oracle -- the reference's results on a CSR as stored (rows shuffled, repeats
apart from each other) are its results on the same graph with sorted rows, so the oracle run on the caller's arrays is
the right yardstick for every upload form."""
import collections

import numpy as np
import pytest

import pyoracle as po
from test_scc_host import canonical, csr_of, kosaraju_check

INT_MAX = 2147483647

UGraph = collections.namedtuple("UGraph", "name V begin idx rb ri hub loop_root")


def multigraph_edges(V, hub_edges, seed):
    """A random strongly connected core (cycle + chords), a DAG tail, and a hub (vertex 5) whose out-row holds
    hub_edges entries with repeats; the edge list in shuffled order."""
    rng = np.random.default_rng(seed)
    core = V // 2
    c = np.arange(core)
    s = [c, rng.integers(0, core, 2 * core), np.full(hub_edges, 5), rng.integers(0, V, V)]
    d = [(c + 1) % core, rng.integers(0, core, 2 * core), rng.integers(0, V, hub_edges), None]
    d[3] = np.minimum(V - 1, s[3] + 1 + rng.integers(0, 4, V))   # forward-only edges
    s, d = np.concatenate(s), np.concatenate(d)
    sh = rng.permutation(len(s))
    return s[sh], d[sh]


def unsorted_multigraph(V, hub_edges, seed):
    """multigraph_edges as forward and reverse CSR, every row in the shuffled order, as uploaded verbatim."""
    return csr_of(V, *multigraph_edges(V, hub_edges, seed))


def rows_of(begin):
    return np.repeat(np.arange(len(begin) - 1), np.diff(begin))


def rows_unsorted(begin, idx):
    """True if some row is not non-decreasing."""
    rows = rows_of(begin)
    return bool(np.any((np.diff(idx) < 0) & (np.diff(rows) == 0)))


def sort_rows(begin, idx):
    """Slot order that sorts every row (stable: equal values keep their order) -- do_semi_sort's e_idx2idx."""
    return np.lexsort((idx, rows_of(begin)))


def adjacent_distinct(row):
    """Entries of a row that differ from the slot before: what a repeat filter that compares neighbours keeps."""
    row = np.asarray(row)
    return int(len(row) and 1 + np.count_nonzero(row[1:] != row[:-1]))


def _i32(*a):
    return [np.ascontiguousarray(x, np.int32) for x in a]


def _insert(s, d, extra):
    """Insert the edges `extra` into the edge list at evenly spaced positions, in the given order."""
    s, d = list(s), list(d)
    n = len(s)
    for k, (a, b) in reversed(list(enumerate(extra))):
        at = (n * k) // (len(extra) - 1) if len(extra) > 1 else 0
        s.insert(at, a)
        d.insert(at, b)
    return np.array(s, np.int64), np.array(d, np.int64)


def _loop_root_edges(r, x, symmetric=False):
    """Root r gets a self loop twice and r -> x three times, the copies of each apart from each other in r's row."""
    e = [(r, x), (r, r), (r, x), (r, r), (r, x)]
    if symmetric:
        e = [(r, x), (x, r), (r, r), (r, x), (x, r), (r, r), (r, x), (x, r)]
    return e


def _check_loop_root(begin, idx, r):
    row = idx[begin[r]:begin[r + 1]]
    assert np.count_nonzero(row == r) >= 1                          # a self loop
    assert adjacent_distinct(row) > len(np.unique(row))             # repeats that are not next to each other


def _finish(name, V, s, d, hub, loop_root, x):
    s, d = _insert(s, d, _loop_root_edges(loop_root, x))
    begin, idx, rb, ri = _i32(*csr_of(V, s, d))
    assert rows_unsorted(begin, idx) and rows_unsorted(rb, ri)
    _check_loop_root(begin, idx, loop_root)
    return UGraph(name, V, begin, idx, rb, ri, hub, loop_root)


def multi(V, hub_edges, seed):
    """The SCC tests' unsorted multigraph (hub 5 with hub_edges > V entries) plus a self-loop root."""
    s, d = multigraph_edges(V, hub_edges, seed)
    x = int(V // 2 + 1)                                              # a tail vertex: not a neighbour of the core vertex 7
    g = _finish("multi%d" % V, V, s, d, 5, 7, x)
    hub_row = g.idx[g.begin[5]:g.begin[6]]
    assert len(hub_row) > V                                          # longer than the traversal's queue
    # a filter that only compares neighbouring slots keeps more entries than the row has distinct values: more than V of
    # them on multi150k, i.e. more than any queue of V entries holds
    assert adjacent_distinct(hub_row) > len(np.unique(hub_row))
    if V > 4096:
        assert adjacent_distinct(hub_row) > V
    return g


def rmat16_shuffled():
    """Directed RMAT-16 (permuted), every forward and reverse row shuffled, plus a self-loop root."""
    og = po.rmat_graph(16, permute=True)
    rng = np.random.default_rng(16)
    s, d = rows_of(og.begin), og.node_idx.astype(np.int64)
    sh = rng.permutation(len(s))
    deg = np.diff(og.begin)
    hub = int(np.argmax(deg))
    r = int(np.flatnonzero(deg >= 2)[0])
    x = int(np.setdiff1d(np.arange(og.N), og.node_idx[og.begin[r]:og.begin[r + 1]])[-1])
    return _finish("rmat16_shuffled", og.N, s[sh], d[sh], hub, r, x)


def sym14_shuffled():
    """po.symmetrize(RMAT-14) with rows shuffled and forward = reverse arrays (a symmetric graph: the TC symmetry check's
    case), plus a self loop and a repeated edge pair r <-> x whose copies sit apart."""
    sym = po.symmetrize(po.rmat_graph(14))
    rng = np.random.default_rng(14)
    V = sym.N
    deg = np.diff(sym.begin)
    r = int(np.flatnonzero(deg >= 2)[0])
    cand = np.setdiff1d(np.flatnonzero(deg >= 8), sym.node_idx[sym.begin[r]:sym.begin[r + 1]])
    x = int(cand[cand != r][0])
    s, d = rows_of(sym.begin), sym.node_idx.astype(np.int64)
    sh = rng.permutation(len(s))
    s, d = _insert(s[sh], d[sh], _loop_root_edges(r, x, symmetric=True))
    begin, idx, _, _ = _i32(*csr_of(V, s, d))
    # symmetric: the multiset of (u, v) is that of (v, u), so the forward arrays serve as the reverse CSR
    fwd = np.sort(rows_of(begin).astype(np.int64) * V + idx)
    bwd = np.sort(idx.astype(np.int64) * V + rows_of(begin))
    assert np.array_equal(fwd, bwd)
    assert rows_unsorted(begin, idx)
    _check_loop_root(begin, idx, r)
    row_x = idx[begin[x]:begin[x + 1]]
    assert adjacent_distinct(row_x) > len(np.unique(row_x))         # the mirrored copies of x -> r sit apart too
    return UGraph("sym14_shuffled", V, begin, idx, begin.copy(), idx.copy(), int(np.argmax(deg)), r)


BUILDERS = {
    "multi64": lambda: multi(64, 200, 64),
    "multi150k": lambda: multi(150000, 400000, 150000),
    "rmat16_shuffled": rmat16_shuffled,
    "sym14_shuffled": sym14_shuffled,
}
_CACHE = {}


def ugraph(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


def stored(g):
    """The oracle's graph: the caller's CSR as stored (no semi-sort)."""
    return po.Graph(g.V, g.begin, g.idx, g.rb, g.ri)


def sorted_graph(g):
    """The same graph with every forward and reverse row sorted, and the forward slot order that did it."""
    o, ro = sort_rows(g.begin, g.idx), sort_rows(g.rb, g.ri)
    return po.Graph(g.V, g.begin.copy(), g.idx[o], g.rb.copy(), np.ascontiguousarray(g.ri[ro])), o


def roots(g):
    return sorted({g.hub, 0, g.V - 1, g.loop_root})


def tc_reference(V, begin, idx, cn=False):
    """The emitted triangle count, by formula: T = sum over distinct edges w -> u with w > u (cn: u -> w, the
    common-neighbour form) of sum over v < u of c_v(u) c_v(w), c_v(x) = multiplicity of x in row v.  Exact, any row
    order, and O(E * in-degree) where the oracle walks a hub row once per slot of it (O(degree^2))."""
    from scipy.sparse import csr_matrix
    rows = rows_of(begin).astype(np.int64)
    idx = np.asarray(idx, np.int64)
    up = idx > rows
    C = csr_matrix((np.ones(int(up.sum()), np.int64), (idx[up], rows[up])), shape=(V, V))   # C[x, v] = c_v(x), x > v
    C.sum_duplicates()
    key = np.unique(rows * V + idx)
    a, b = key // V, key % V
    u, w = (a, b) if cn else (b, a)
    keep = w > u
    u, w = u[keep], w[keep]
    return int(C[u].multiply(C[w]).sum()) if len(u) else 0


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("name", list(BUILDERS))
def test_builders_have_their_properties(name):
    g = ugraph(name)      # (each builder asserts what its graph is there for)
    assert len(g.begin) == len(g.rb) == g.V + 1 and len(g.idx) == len(g.ri) == g.begin[-1] == g.rb[-1]
    assert g.idx.min() >= 0 and g.idx.max() < g.V and g.ri.min() >= 0 and g.ri.max() < g.V
    # the reverse CSR is the transpose: the same edge multiset
    fwd = np.sort(rows_of(g.begin).astype(np.int64) * g.V + g.idx)
    bwd = np.sort(g.ri.astype(np.int64) * g.V + rows_of(g.rb))
    assert np.array_equal(fwd, bwd)


@pytest.mark.parametrize("name", ["multi64", "multi150k", "rmat16_shuffled"])
def test_oracle_on_stored_rows_equals_oracle_on_sorted_rows(name):
    g = ugraph(name)
    og, (sg, order) = stored(g), sorted_graph(g)
    for r in roots(g):
        assert np.array_equal(po.hop_dist(og, r)[0], po.hop_dist(sg, r)[0]), r
        assert np.array_equal(po.bfs_queue(og, r), po.bfs_queue(sg, r)), r
        assert np.array_equal(po.bfs_queue(og, r), po.hop_dist(sg, r)[0]), r
    rng = np.random.default_rng(3)
    length = rng.integers(1, 101, og.M).astype(np.int32)
    for r in (g.hub, g.loop_root):
        assert np.array_equal(po.sssp(og, length, r)[0], po.sssp(sg, length[order], r)[0])
        ones = np.ones(og.M, np.int32)
        assert np.array_equal(po.sssp(og, ones, r)[0], po.bfs_queue(og, r))
    age = rng.integers(0, 40, g.V).astype(np.int32)
    for K in (5, 30):
        a1, c1 = po.avg_teen_cnt(og, age, K)
        a2, c2 = po.avg_teen_cnt(sg, age, K)
        assert np.array_equal(c1, c2) and a1.tobytes() == a2.tobytes()
    member = rng.integers(0, 4, g.V).astype(np.int32)
    for num in (0, 1, 3):
        assert po.conduct(og, member, num).tobytes() == po.conduct(sg, member, num).tobytes()
    n1, m1 = kosaraju_check(g.V, og.begin, og.node_idx, og.r_begin, og.r_node_idx)
    n2, m2 = kosaraju_check(g.V, sg.begin, sg.node_idx, sg.r_begin, sg.r_node_idx)
    assert n1 == n2 and np.array_equal(canonical(m1), canonical(m2))
    r1, it1, _ = po.pagerank(og, 0.001, 0.85, 100)
    r2, it2, _ = po.pagerank(sg, 0.001, 0.85, 100)
    assert it1 == it2
    assert float(np.max(np.abs(r1 - r2) / np.abs(r2))) < 1e-12


@pytest.mark.parametrize("name", ["multi64", "rmat16_shuffled", "sym14_shuffled"])
def test_tc_reference_equals_oracle(name):
    """The formula the GPU tests count against (the oracle is quadratic in multi150k's hub row) is the oracle's count
    on sorted rows, and does not depend on the row order."""
    g = ugraph(name)
    sg, _ = sorted_graph(g)
    want, want_cn = po.triangle_counting(sg), po.triangle_counting_cn(sg)
    assert tc_reference(g.V, sg.begin, sg.node_idx) == want
    assert tc_reference(g.V, g.begin, g.idx) == want
    assert tc_reference(g.V, sg.begin, sg.node_idx, cn=True) == want_cn
    assert tc_reference(g.V, g.begin, g.idx, cn=True) == want_cn
    assert want > 0 and want_cn > 0
