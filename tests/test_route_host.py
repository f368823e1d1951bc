"""Route queries with Int edge weights (bidir_dijkstra.gm, sssp_dijkstra.gm) restated on the host, no GPU: a plain heapq
Dijkstra (dijkstra_cost, the arbiter of flag and cost), bidir_dijkstra.gm as written and run by one thread with the map's
ties going to the smallest vertex id (bidir_literal), their agreement on hand shapes and random multigraphs with zero
weights, repeats and self loops, the checker of a returned route that the device tests share (valid_route), the hand shapes
with their pinned flag and cost -- each the smallest graph on which one mistake of a bidirectional search shows -- and the
plumbing: the four entries are exported, the driver is built, and the headers of all four shortest-path programs go into
one program whose two Int get_path overloads are run.  The device tests are test_gpu_route.py."""
import heapq
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "green-marl_amd")
INT_MAX = 2147483647


def csr_of(V, src, dst):
    """Forward CSR with the edges in the order given (src non-decreasing): slot i is edge i."""
    src = np.asarray(src, np.int64)
    assert np.all(np.diff(src) >= 0)
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), np.asarray(dst, np.int32)


def sources(begin):
    begin = np.asarray(begin, np.int64)
    return np.repeat(np.arange(len(begin) - 1, dtype=np.int64), np.diff(begin))


# ------------------------------------------------------------------ the arbiter
def dijkstra_cost(begin, idx, w, src, dst):
    """The shortest distance src -> dst over out-edges, None when dst is not reachable; src == dst: 0."""
    begin, idx, w = [int(x) for x in begin], [int(x) for x in idx], [int(x) for x in w]
    dist = {src: 0}
    heap = [(0, src)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        if u == dst:
            return d
        for e in range(begin[u], begin[u + 1]):
            v, c = idx[e], d + w[e]
            if c < dist.get(v, INT_MAX):
                dist[v] = c
                heapq.heappush(heap, (c, v))
    return None


def dijkstra_all(begin, idx, w, src):
    """dist[V] from src over out-edges (INT_MAX: unreachable), vectorised Bellman-Ford rounds: for the named graphs."""
    begin = np.asarray(begin, np.int64)
    s, d, w = sources(begin), np.asarray(idx, np.int64), np.asarray(w, np.int64)
    dist = np.full(len(begin) - 1, INT_MAX, np.int64)
    dist[src] = 0
    while True:
        live = dist[s] != INT_MAX
        nd = dist.copy()
        np.minimum.at(nd, d[live], dist[s[live]] + w[live])
        if np.array_equal(nd, dist):
            return dist
        dist = nd


# ------------------------------------------------------------------ the program as written
def bidir_literal(begin, idx, w, src, dst):
    """bidir_dijkstra.gm:1-123 with one thread; GetMinKey's ties go to the smallest vertex id.  Returns (found, minCost)."""
    begin, idx, w = [int(x) for x in begin], [int(x) for x in idx], [int(x) for x in w]
    V = len(begin) - 1
    ins = [[] for _ in range(V)]                                     # InNbrs with ToEdge: (source, forward slot)
    for u in range(V):
        for e in range(begin[u], begin[u + 1]):
            ins[idx[e]].append((u, e))
    outs = [[(idx[e], e) for e in range(begin[u], begin[u + 1])] for u in range(V)]
    cost = [[INT_MAX] * V, [INT_MAX] * V]
    fin = [[False] * V, [False] * V]
    reach = [{src: 0}, {dst: 0}]
    cost[0][src] = cost[1][dst] = 0
    cur_min = [0, 0]
    min_cost, mid, terminate = INT_MAX, -1, False
    while not terminate and (reach[0] or reach[1]):
        if reach[0] and (len(reach[0]) <= len(reach[1]) or not reach[1]):
            s = 0
        elif reach[1] and (len(reach[1]) <= len(reach[0]) or not reach[0]):
            s = 1
        else:
            continue
        nxt = min(reach[s], key=lambda v: (reach[s][v], v))
        del reach[s][nxt]
        fin[s][nxt] = True
        cur_min[s] = cost[s][nxt]
        if cur_min[0] + cur_min[1] > min_cost:
            terminate = True
        d = cost[s][nxt]
        for v, e in (outs if s == 0 else ins)[nxt]:
            if fin[s][v]:
                continue
            if d + w[e] + cur_min[1 - s] <= min_cost and cost[s][v] > d + w[e]:
                cost[s][v] = d + w[e]
                reach[s][v] = cost[s][v]
                if cost[1 - s][v] != INT_MAX and cost[0][v] + cost[1][v] < min_cost:
                    min_cost, mid = cost[0][v] + cost[1][v], v
    return (True, min_cost) if mid >= 0 else (False, None)


# ------------------------------------------------------------------ the checker of a returned route
def valid_route(begin, idx, w, src, dst, nodes, edges, cost):
    """None when nodes / edges (the vertices after src and the forward slot into each) are a route src -> dst of weight `cost`
    in the CSR given, else what is wrong: consecutive edges join up, each edge lies in the row of its source and points at
    its node, the weights sum to cost, no vertex repeats (so it has fewer than V edges)."""
    V = len(begin) - 1
    nodes, edges = [int(x) for x in nodes], [int(x) for x in edges]
    if len(nodes) != len(edges):
        return "%d nodes, %d edges" % (len(nodes), len(edges))
    if len(nodes) >= V:
        return "%d edges in a graph of %d vertices" % (len(nodes), V)
    at, total, seen = src, 0, {src}
    for k, (v, e) in enumerate(zip(nodes, edges)):
        if not (int(begin[at]) <= e < int(begin[at + 1])):
            return "edge %d (slot %d) is not in the row of %d" % (k, e, at)
        if int(idx[e]) != v:
            return "edge %d (slot %d) points at %d, not at %d" % (k, e, int(idx[e]), v)
        if v in seen:
            return "vertex %d repeats" % v
        seen.add(v)
        total += int(w[e])
        at = v
    if at != dst:
        return "ends at %d, not at %d" % (at, dst)
    if total != cost:
        return "weights sum to %d, not to %d" % (total, cost)
    return None


def route_of_parents(parent, parent_edge, src, dst):
    """get_path of bidir_dijkstra.gm: the vertices after src up to dst along parent, and the slots into them; ([], []) when
    dst has no predecessor."""
    nodes, edges, n = [], [], dst
    if parent[dst] != -1:
        while n != src:
            nodes.insert(0, int(n))
            edges.insert(0, int(parent_edge[n]))
            n = int(parent[n])
            assert len(nodes) <= len(parent)
    return nodes, edges


# ------------------------------------------------------------------ shapes (shared with the device tests)
def tree4(depth, cut_last=False):
    """Complete 4-ary out-tree, vertex v's children 4v+1 .. 4v+4, (4^(depth+1) - 1) / 3 vertices; cut_last: without the edge
    into the last leaf, which then has no in-edges."""
    V = (4 ** (depth + 1) - 1) // 3
    inner = (4 ** depth - 1) // 3
    s = np.repeat(np.arange(inner), 4)
    d = 4 * s + 1 + np.tile(np.arange(4), inner)
    if cut_last:
        s, d = s[:-1], d[:-1]
    return (V,) + csr_of(V, s, d)


def _tiny_reverse():
    V, b, i = tree4(2, cut_last=True)
    return V, sources(b).tolist(), i.tolist(), [1] * len(i), 0, V - 1, False, None


# name: (V, src, dst, weight, s, t, found, cost), slots as listed (src ascending)
SHAPES = {
    # 0 -> 1 -> 5 (3 + 3) is where the two searches meet first; 0 -> 2 -> 3 -> 4 -> 5 (1 each) is shorter
    "meet_not_best": (6, [0, 0, 1, 2, 3, 4], [1, 2, 5, 3, 4, 5], [3, 1, 3, 1, 1, 1], 0, 5, True, 4),
    # 0 -> 1 -> 2 -> 3 (1 each): F settles 1, R settles 2, they first meet at 4 (0 -> 4 -> 3, 2 + 2); the edge 1 -> 2 joins
    # two vertices that neither side needs to expand again.  _f: the forward side goes first (ties); _r: src has two more
    # out-edges into dead ends, so the reverse side does
    "middle_edge_f": (5, [0, 0, 1, 2, 4], [1, 4, 2, 3, 3], [1, 2, 1, 1, 2], 0, 3, True, 3),
    "middle_edge_r": (7, [0, 0, 0, 0, 1, 2, 4], [1, 4, 5, 6, 2, 3, 3], [1, 2, 9, 9, 1, 1, 2], 0, 3, True, 3),
    "zero_cycle": (5, [0, 1, 2, 2, 3, 3], [1, 2, 1, 3, 2, 4], [1, 0, 0, 0, 0, 1], 0, 4, True, 2),
    "parallel_eq": (3, [0, 0, 0, 1, 1, 1], [1, 1, 1, 2, 2, 2], [2, 1, 1, 3, 3, 4], 0, 2, True, 4),
    "self_loops": (3, [0, 0, 1, 1, 2], [0, 1, 1, 2, 2], [0, 2, 1, 0, 5], 0, 2, True, 2),
    "one_way": (4, [0, 1, 2], [3, 0, 1], [1, 1, 1], 0, 2, False, None),
    "tiny_reverse": _tiny_reverse(),
    "src_is_dst": (2, [0, 1], [1, 0], [2, 3], 0, 0, True, 0),
}


def shape(name):
    """(begin, node_idx, weight[int32], src, dst, found, cost) of a hand shape."""
    V, s, d, w, src, dst, found, cost = SHAPES[name]
    b, i = csr_of(V, s, d)
    return b, i, np.asarray(w, np.int32), src, dst, found, cost


def random_case(seed):
    """V in 2 .. 40, E up to 160, repeats and self loops, weights from {0 .. 3}, src != dst."""
    rng = np.random.default_rng(1000 + seed)
    V = int(rng.integers(2, 41))
    E = int(rng.integers(0, 161))
    s = np.sort(rng.integers(0, V, E))
    d = rng.integers(0, V, E)
    w = rng.integers(0, 4, E).astype(np.int32)
    b, i = csr_of(V, s, d)
    src = int(rng.integers(0, V))
    dst = int((src + 1 + rng.integers(0, V - 1)) % V)
    return b, i, w, src, dst


# ------------------------------------------------------------------ the definition on hand-made cases
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pinned_flag_and_cost(name):
    b, i, w, src, dst, found, cost = shape(name)
    assert dijkstra_cost(b, i, w, src, dst) == cost and (cost is not None) == found
    if src != dst:
        assert bidir_literal(b, i, w, src, dst) == (found, cost)


def test_the_first_meeting_is_not_the_best():
    """meet_not_best after one round of each side: the only vertex both have reached is 1, at 3 + 3."""
    b, i, w, src, dst, _, cost = shape("meet_not_best")
    f1 = {int(i[e]): int(w[e]) for e in range(b[src], b[src + 1])}
    r1 = {int(u): int(w[e]) for e, u in enumerate(sources(b)) if i[e] == dst}
    assert set(f1) & set(r1) == {1} and f1[1] + r1[1] == 6 > cost


def test_the_middle_edge_joins_two_settled_vertices():
    for name in ("middle_edge_f", "middle_edge_r"):
        b, i, w, src, dst, _, cost = shape(name)
        fwd, rev = dijkstra_all(b, i, w, src), [dijkstra_cost(b, i, w, v, dst) for v in range(len(b) - 1)]
        assert fwd[1] == 1 and rev[2] == 1 and fwd[1] + 1 + rev[2] == cost == 3          # ... through 1 -> 2
        assert fwd[4] + rev[4] == 4                                                      # the vertex both sides reach first
    assert np.diff(shape("middle_edge_f")[0])[0] == 2 and np.diff(shape("middle_edge_r")[0])[0] == 4   # out-slots of src; dst has 2 in-slots


def test_src_is_dst_departs_from_the_program():
    """bidir_dijkstra.gm reports a cycle through src, or False when there is none; the entry reports the empty route."""
    b, i, w, src, dst, found, cost = shape("src_is_dst")
    assert (found, cost) == (True, 0)
    assert bidir_literal(b, i, w, 0, 0) == (True, 5)
    b, i = csr_of(2, [0], [1])
    assert bidir_literal(b, i, [2], 0, 0) == (False, None) and dijkstra_cost(b, i, [2], 0, 0) == 0


def test_tree_shapes():
    V, b, i = tree4(6)
    assert V == 5461 and len(i) == 5460 and b[1365] == 5460 and (np.diff(b)[1365:] == 0).all()
    assert dijkstra_cost(b, i, np.ones(len(i), np.int32), 0, V - 1) == 6
    V, b, i = tree4(6, cut_last=True)
    assert V == 5461 and len(i) == 5459 and not (i == V - 1).any()
    assert dijkstra_cost(b, i, np.ones(len(i), np.int32), 0, V - 1) is None


@pytest.mark.parametrize("block", range(4))
def test_literal_agrees_with_dijkstra_on_random_multigraphs(block):
    found = 0
    for seed in range(block * 100, block * 100 + 100):               # 400 graphs
        b, i, w, src, dst = random_case(seed)
        want = dijkstra_cost(b, i, w, src, dst)
        assert bidir_literal(b, i, w, src, dst) == (want is not None, want), seed
        assert dijkstra_all(b, i, w, src)[dst] == (INT_MAX if want is None else want), seed
        found += want is not None
    assert 10 < found < 100                                          # both answers occur


# ------------------------------------------------------------------ the checker checks
def test_valid_route_accepts_and_refuses():
    b, i, w, src, dst, _, cost = shape("parallel_eq")
    assert valid_route(b, i, w, src, dst, [1, 2], [1, 3], cost) is None
    assert valid_route(b, i, w, src, dst, [1, 2], [2, 4], cost) is None              # the other equally short slots
    assert "sum" in valid_route(b, i, w, src, dst, [1, 2], [0, 3], cost)
    assert "row" in valid_route(b, i, w, src, dst, [1, 2], [3, 3], cost)
    assert "ends" in valid_route(b, i, w, src, dst, [1], [1], 1)
    assert "nodes" in valid_route(b, i, w, src, dst, [1, 2], [1], cost)
    b, i, w, src, dst, _, cost = shape("zero_cycle")
    assert valid_route(b, i, w, src, dst, [1, 2, 3, 4], [0, 1, 3, 5], cost) is None
    assert "repeats" in valid_route(b, i, w, src, dst, [1, 2, 1, 2], [0, 1, 2, 1], cost)
    assert "points" in valid_route(b, i, w, src, dst, [1, 3, 3, 4], [0, 1, 3, 5], cost)
    b, i, w, src, dst, _, _ = shape("src_is_dst")
    assert valid_route(b, i, w, src, dst, [], [], 0) is None
    assert "edges in a graph" in valid_route(b, i, w, 0, 0, [1, 0], [0, 1], 5)
    assert route_of_parents([-1, 0, 1], [-1, 1, 3], 0, 2) == ([1, 2], [1, 3]) and route_of_parents([-1, -1], [-1, -1], 0, 1) == ([], [])


# ------------------------------------------------------------------ plumbing
ENTRIES = ("gmx_route_create", "gmx_route_free", "gmx_route_query", "gmx_bidir_dijkstra")
HEADERS_CC = r"""
#include "bidir_dijkstra.h"
#include "sssp_dijkstra.h"
#include "sssp_path.h"
#include "sssp_path_adj.h"
#include <stdio.h>
// every entry of the four shortest-path programs, in one program
bool (*bidir_entry)(gm_graph&, int32_t*, node_t&, node_t&, node_t*, edge_t*) = &bidir_dijkstra;
bool (*dijkstra_entry)(gm_graph&, int32_t*, node_t&, node_t&, node_t*, edge_t*) = &dijkstra;
void (*int_entry)(gm_graph&, int32_t*, int32_t*, node_t&, node_t*) = &sssp_path;
void (*f64_entry)(gm_graph&, double*, double*, node_t&, node_t&, node_t*, edge_t*) = &sssp_path;
void (*tree_path)(gm_graph&, node_t&, node_t&, node_t*, gm_node_seq&) = &get_path;
int32_t (*int_path)(gm_graph&, node_t&, node_t&, node_t*, edge_t*, int32_t*, gm_node_seq&) = &get_path;
double (*f64_path)(gm_graph&, node_t&, node_t&, node_t*, edge_t*, double*, gm_node_seq&) = &get_path;
static void show(const char* what, int end, long total, gm_node_seq& Q) {
    printf("%s %d: %ld %d:", what, end, total, Q.get_size());
    gm_node_seq::seq_iter it = Q.prepare_seq_iteration();
    while (it.has_next()) printf(" %d", (int) it.get_next());
    printf("\n");
}
int main() {
    gm_graph G;
    node_t parent[5] = {-1, 0, 1, -1, 2};            // the route 0 -> 1 -> 2 -> 4, -1 off it
    edge_t parent_edge[5] = {-1, 1, 3, -1, 5};
    int32_t weight[6] = {9, 2, 9, 0, 9, 7};
    for (node_t end = 0; end < 5; end++) {
        node_t begin = 0;
        gm_node_seq Q, T;
        const int32_t total = int_path(G, begin, end, parent, parent_edge, weight, Q);
        show("route", (int) end, (long) total, Q);
        tree_path(G, begin, end, parent, T);
        show("tree", (int) end, 0, T);
    }
    return bidir_entry && dijkstra_entry && int_entry && f64_entry && f64_path ? 0 : 1;
}
"""


def test_entries_are_exported_built_and_all_headers_go_into_one_program(tmp_path):
    """Fails without the feature, on any box: the bindings, the driver, and the four headers in one program."""
    import gmx
    from test_host_cpp import CXX_FLAGS, LINK
    assert all(s in gmx.EXPORTS for s in ENTRIES)
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    assert all(hasattr(gmx.lib(), s) for s in ENTRIES)
    assert hasattr(gmx.Graph, "route") and hasattr(gmx.Graph, "bidir_dijkstra") and hasattr(gmx.Route, "query") and hasattr(gmx.Route, "free")
    exe = os.path.join(PKG, "bin", "bidir_dijkstra")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath> <src> <dst> [<pairs_file> <num_pairs>]" in r.stdout
    src, prog = str(tmp_path / "headers.cc"), str(tmp_path / "headers")
    open(src, "w").write(HEADERS_CC)
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-Wall", "-Werror", src, "-o", prog] + LINK)
    out = subprocess.run([prog], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    # the Int get_path does not push begin and sums from end backwards; sssp_path's pushes begin too; nothing without a predecessor
    assert out == ["route 0: 0 0:", "tree 0: 0 0:", "route 1: 2 1: 1", "tree 1: 0 2: 0 1", "route 2: 2 2: 1 2", "tree 2: 0 3: 0 1 2",
                   "route 3: 0 0:", "tree 3: 0 0:", "route 4: 9 3: 1 2 4", "tree 4: 0 4: 0 1 2 4"]
