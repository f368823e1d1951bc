"""sssp_path_adj.gm (a route query root -> end with double costs, a predecessor node and edge per vertex, pruned against the
best distance to end found so far) restated on the host, no GPU: the loop as written, run by one thread (spf_literal, the
arbiter), the parallel statement the device implements (spf_model: per round a vertex that dropped takes the minimum of the
round's offers and, among the offers equal to it, the smallest slot), their agreement on hand shapes and random multigraphs
with ties and zero costs, the pinned results, and the plumbing: the entry is exported, the driver is built, and both
`sssp_path` overloads link into one program whose `get_path` is checked.  The device tests (test_gpu_sssp_path_adj.py) compare
gmx_sssp_path_f64 with these byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "green-marl_amd")
DBL_MAX = float(np.finfo(np.float64).max)
MAX = DBL_MAX


def sources(begin):
    begin = np.asarray(begin, np.int64)
    return np.repeat(np.arange(len(begin) - 1, dtype=np.int64), np.diff(begin))


def csr_of(V, src, dst):
    """Forward CSR with the edges in the order given (src non-decreasing): slot i is edge i."""
    src = np.asarray(src, np.int64)
    assert np.all(np.diff(src) >= 0)
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), np.asarray(dst, np.int32)


# ------------------------------------------------------------------ the program as written
def spf_literal(begin, node_idx, cost, root, end):
    """sssp_path_adj.gm:1-33 with one thread: vertices ascending, a row in slot order.  Returns (dist[float64], prev_node,
    prev_edge, rounds): rounds = iterations of the loop in which some vertex was updated.  updated_nxt starts as a copy of
    updated, so the root is updated in round 2 again (where it offers what it offered in round 1: nothing changes): with a
    root in range the loop runs two rounds at least."""
    begin = [int(x) for x in begin]
    node_idx = [int(x) for x in node_idx]
    cost = [float(x) for x in cost]
    V = len(begin) - 1
    dist = [DBL_MAX] * V
    updated = [False] * V
    if 0 <= root < V:
        dist[root] = 0.0
        updated[root] = True
    dist_nxt, updated_nxt = list(dist), list(updated)
    prev_node, prev_edge = [-1] * V, [-1] * V
    rounds = 0
    fin = False
    while not fin:
        fin = True
        B = dist[end] if end >= 0 else DBL_MAX
        ups = [n for n in range(V) if updated[n]]
        rounds += 1 if ups else 0
        for n in ups:
            if dist[n] < B:
                for e in range(begin[n], begin[n + 1]):
                    s = node_idx[e]
                    c = dist[n] + cost[e]
                    if c < B and dist_nxt[s] > c:
                        dist_nxt[s] = c
                        updated_nxt[s] = True
                        prev_node[s] = n
                        prev_edge[s] = e
        dist = list(dist_nxt)
        updated = updated_nxt
        updated_nxt = [False] * V
        fin = not any(updated)
    return np.array(dist, np.float64), np.array(prev_node, np.int32), np.array(prev_edge, np.int32), rounds


# ------------------------------------------------------------------ the parallel statement
def spf_model(begin, node_idx, cost, root, end):
    """The same results, a round at a time over arrays: the device's formulation.  Returns (dist, prev_node, prev_edge, rounds,
    slots, updated) with the device's counters: rounds in which some vertex was updated, row slots walked (the rows of the
    updated vertices below the bound), updated vertices summed over the rounds -- the root's second visit not counted."""
    begin = np.asarray(begin, np.int64)
    V = len(begin) - 1
    src, dst = sources(begin), np.asarray(node_idx, np.int64)
    cost = np.asarray(cost, np.float64)
    dist = np.full(V, DBL_MAX)
    upd = np.zeros(V, bool)
    if 0 <= root < V:
        dist[root] = 0.0
        upd[root] = True
    prev_node, prev_edge = np.full(V, -1, np.int32), np.full(V, -1, np.int32)
    deg = np.diff(begin)
    rounds = slots = queued = 0
    while upd.any():
        rounds += 1
        queued += int(upd.sum())
        B = dist[end] if end >= 0 else DBL_MAX
        active = upd & (dist < B)
        slots += int(deg[active].sum())
        e = np.flatnonzero(active[src])
        with np.errstate(over="ignore"):
            c = dist[src[e]] + cost[e]
        ok = c < B
        e, c = e[ok], c[ok]
        dn = dist.copy()
        np.minimum.at(dn, dst[e], c)
        dropped = dn < dist
        win = e[(c == dn[dst[e]]) & dropped[dst[e]]]                 # ascending slots: the first per target is its smallest
        heads, first = np.unique(dst[win], return_index=True)
        prev_edge[heads] = win[first]
        prev_node[heads] = src[win[first]]
        dist, upd = dn, dropped
    return dist, prev_node, prev_edge, rounds, slots, queued


def same(lit, model):
    """The three arrays byte for byte; the literal loop's rounds are the model's, two at least (the root's second visit)."""
    return (lit[0].view(np.uint64).tobytes() == model[0].view(np.uint64).tobytes() and np.array_equal(lit[1], model[1])
            and np.array_equal(lit[2], model[2]) and lit[3] == (max(model[3], 2) if model[3] else 0))


# ------------------------------------------------------------------ shapes (shared with the device tests)
# name: (V, src, dst, cost, root, end), slots as listed (src ascending)
SHAPES = {
    "late_small": (5, [0, 0, 1, 2, 4], [2, 4, 3, 3, 1], [2, 1, 1, 1, 1], 0, -1),
    "pruned": (6, [0, 0, 1, 2, 3], [1, 2, 3, 4, 5], [1, 5, 1, 1, 1], 0, 3),
    "round_dep": (6, [0, 0, 0, 2, 3, 4], [1, 2, 5, 3, 4, 5], [10, 1, 30, 1, 1, 20], 0, 1),
    "end_improves": (5, [0, 0, 2, 3, 3], [1, 2, 3, 1, 4], [10, 1, 1, 1, 8], 0, 1),
    "ulp": (5, [0, 0, 1, 2, 3], [1, 3, 2, 4, 4], [.25, .4, .25, .1, .2], 0, -1),
    "parallel_eq": (2, [0, 0, 0], [1, 1, 1], [2, 1, 1], 0, -1),
    "zero_cycle": (4, [0, 1, 2, 2], [1, 2, 1, 3], [2, 0, 0, 1], 0, 3),
    "chain_end": (6, [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [1, 1, 1, 1, 1], 0, 3),
    "end_is_root": (3, [0, 1], [1, 2], [1, 1], 0, 0),
}
# name: (dist, prev_node, prev_edge)
PINNED = {
    "late_small": ([0, 2, 2, 3, 1], [-1, 4, 0, 2, 0], [-1, 4, 0, 3, 1]),
    "pruned": ([0, 1, 5, 2, 6, MAX], [-1, 0, 0, 1, 2, -1], [-1, 0, 1, 2, 3, -1]),
    "round_dep": ([0, 10, 1, 2, 3, 30], [-1, 0, 0, 2, 3, 0], [-1, 0, 1, 3, 4, 2]),
    "end_improves": ([0, 3, 1, 2, MAX], [-1, 3, 0, 2, -1], [-1, 3, 1, 2, -1]),
    "ulp": ([0, .25, .5, .4, float.fromhex("0x1.3333333333333p-1")], [-1, 0, 1, 0, 2], [-1, 0, 2, 1, 3]),
    "parallel_eq": ([0, 1], [-1, 0], [-1, 1]),
    "zero_cycle": ([0, 2, 2, 3], [-1, 0, 1, 2], [-1, 0, 1, 3]),
    "chain_end": ([0, 1, 2, 3, MAX, MAX], [-1, 0, 1, 2, -1, -1], [-1, 0, 1, 2, -1, -1]),
    "end_is_root": ([0, MAX, MAX], [-1, -1, -1], [-1, -1, -1]),
}
_LIT = {}


def shape(name):
    """(begin, node_idx, cost[float64], root, end) of a hand shape."""
    V, s, d, c, root, end = SHAPES[name]
    b, i = csr_of(V, s, d)
    return b, i, np.asarray(c, np.float64), root, end


def literal_of(name):
    if name not in _LIT:
        _LIT[name] = spf_literal(*shape(name))
    return _LIT[name]


def random_case(seed):
    """V up to 40, E up to 160, repeats and self loops; costs from {0, .1 .. .5} or {0, 1, 2, 3}; any root, end in -1 .. V-1."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 41))
    E = int(rng.integers(0, 161))
    s = np.sort(rng.integers(0, V, E))
    d = rng.integers(0, V, E)
    cost = rng.integers(0, 6, E) * 0.1 if seed % 2 else rng.integers(0, 4, E).astype(np.float64)
    b, i = csr_of(V, s, d)
    return b, i, np.asarray(cost, np.float64), int(rng.integers(0, V)), int(rng.integers(-1, V))


def median_end(dist):
    """The vertex at the median finite distance (ties to the lowest id): a target that prunes about half of the search."""
    fin = np.flatnonzero(dist < DBL_MAX)
    order = fin[np.argsort(dist[fin], kind="stable")]
    return int(order[len(order) // 2])


# ------------------------------------------------------------------ the definition on hand-made cases
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pinned_results(name):
    dist, pn, pe = PINNED[name]
    lit = literal_of(name)
    assert lit[0].view(np.uint64).tolist() == np.asarray(dist, np.float64).view(np.uint64).tolist()       # bits, not isclose
    assert lit[1].tolist() == pn and lit[2].tolist() == pe
    assert same(lit, spf_model(*shape(name)))


def test_round_dep_depends_on_the_target():
    b, i, c, root, _ = shape("round_dep")
    lit = spf_literal(b, i, c, root, -1)
    assert lit[0][5] == 23 and lit[1][5] == 4 and lit[2][5] == 5
    assert literal_of("round_dep")[0][5] == 30


def test_ulp_drops_by_one_ulp_a_round_later():
    assert (0.4 + 0.2).hex() == "0x1.3333333333334p-1" and (0.5 + 0.1).hex() == "0x1.3333333333333p-1"
    lit = literal_of("ulp")
    assert float(lit[0][4]).hex() == "0x1.3333333333333p-1" and lit[1][4] == 2 and lit[3] == 4
    assert spf_model(*shape("ulp"))[3:] == (4, 5, 6)                 # vertex 4 is updated twice


def test_late_small_is_not_the_smallest_tight_slot():
    """Vertex 3 is at distance 3 through slot 2 (from 1) and slot 3 (from 2): slot 3 offered it a round earlier and stays."""
    lit = literal_of("late_small")
    assert lit[2][3] == 3 and lit[1][3] == 2


def test_pruning_walks_fewer_slots():
    b, i, c, root, end = shape("pruned")
    assert spf_model(b, i, c, root, end)[4] == 4 and spf_model(b, i, c, root, -1)[4] == 5


def test_counters_of_the_corner_cases():
    assert spf_model(*shape("end_is_root"))[3:] == (1, 0, 1)         # one round, which offers nothing
    assert literal_of("end_is_root")[3] == 2
    assert spf_model(*shape("chain_end"))[3:] == (4, 3, 4)           # the round of vertex 3 walks nothing: 3 < 3 fails
    b, i, c, _, _ = shape("chain_end")
    assert spf_model(b, i, c, 0, -1)[3:] == (6, 5, 6)
    for root, end in ((7, -1), (-1, 2)):                             # a root out of range: nothing is updated
        lit, model = spf_literal(b, i, c, root, end), spf_model(b, i, c, root, end)
        assert same(lit, model) and model[3:] == (0, 0, 0) and (lit[0] == DBL_MAX).all() and (lit[1] == -1).all()
    assert spf_literal([0], [], [], 0, -1)[3] == 0                   # V = 0


def test_infinite_cost_is_never_offered():
    b, i = csr_of(3, [0, 0, 1], [1, 2, 2])
    for end in (-1, 2):
        lit = spf_literal(b, i, [np.inf, 1.0, -0.0], 0, end)
        assert lit[0].tolist() == [0, DBL_MAX, 1] and lit[2].tolist() == [-1, -1, 1]
        assert same(lit, spf_model(b, i, [np.inf, 1.0, -0.0], 0, end))
    lit = spf_literal(b, i, [-0.0, 1.0, -0.0], 0, -1)                # -0.0 is a cost like 0: no distance is ever -0.0
    assert lit[0].view(np.uint64).tolist() == [0, 0, 0] and lit[2].tolist() == [-1, 0, 2]
    assert same(lit, spf_model(b, i, [-0.0, 1.0, -0.0], 0, -1))


# ------------------------------------------------------------------ model = literal
@pytest.mark.parametrize("block", range(5))
def test_model_is_the_literal_loop_on_random_multigraphs(block):
    pruned = 0
    for seed in range(block * 90, block * 90 + 90):                  # 450 graphs
        g = random_case(seed)
        lit = spf_literal(*g)
        assert same(lit, spf_model(*g)), seed
        if g[4] >= 0:
            free = spf_model(*g[:4], -1)
            assert spf_model(*g)[4] <= free[4], seed
            pruned += lit[0].tobytes() != free[0].tobytes()
    assert pruned > 0                                                # some target changed some distance


@pytest.mark.parametrize("name", ["star33", "rmat10", "uniform"])
def test_model_is_the_literal_loop_on_named_graphs(name):
    from test_communities_host import named_graph
    b, i = named_graph(name)
    rng = np.random.default_rng(5)
    root = int(np.argmax(np.diff(b)))
    for cost in (rng.integers(0, 8, len(i)) * 0.25, rng.random(len(i))):
        free = spf_model(b, i, cost, root, -1)
        assert same(spf_literal(b, i, cost, root, -1), free)
        end = median_end(free[0])
        assert same(spf_literal(b, i, cost, root, end), spf_model(b, i, cost, root, end))


# ------------------------------------------------------------------ plumbing
GET_PATH_CC = r"""
#include "sssp_path.h"
#include "sssp_path_adj.h"
#include <stdio.h>
// both overloads of both names, in one program
void (*int_entry)(gm_graph&, int32_t*, int32_t*, node_t&, node_t*) = &sssp_path;
void (*f64_entry)(gm_graph&, double*, double*, node_t&, node_t&, node_t*, edge_t*) = &sssp_path;
void (*int_path)(gm_graph&, node_t&, node_t&, node_t*, gm_node_seq&) = &get_path;
double (*f64_path)(gm_graph&, node_t&, node_t&, node_t*, edge_t*, double*, gm_node_seq&) = &get_path;
int main() {
    gm_graph G;
    node_t prev_node[5] = {-1, 4, 0, 2, 0};          // late_small
    edge_t prev_edge[5] = {-1, 4, 0, 3, 1};
    double cost[5] = {2, 1, 1, 1, 1};
    for (node_t end = 0; end < 5; end++) {
        node_t begin = 0;
        gm_node_seq Q;
        const double total = f64_path(G, begin, end, prev_node, prev_edge, cost, Q);
        printf("%d: %.17g %d:", (int) end, total, Q.get_size());
        gm_node_seq::seq_iter it = Q.prepare_seq_iteration();
        while (it.has_next()) printf(" %d", (int) it.get_next());
        printf("\n");
    }
    return int_entry && f64_entry && int_path ? 0 : 1;
}
"""


def test_entry_is_exported_built_and_both_overloads_link(tmp_path):
    """Fails without the feature, on any box: the binding, the driver and the two overloads in one program."""
    import gmx
    from test_host_cpp import CXX_FLAGS, LINK
    assert "gmx_sssp_path_f64" in gmx.EXPORTS
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    assert hasattr(gmx.lib(), "gmx_sssp_path_f64") and hasattr(gmx.Graph, "sssp_path_f64")
    exe = os.path.join(PKG, "bin", "sssp_path_adj")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath> <root> <end>" in r.stdout
    src, prog = str(tmp_path / "get_path.cc"), str(tmp_path / "get_path")
    open(src, "w").write(GET_PATH_CC)
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-Wall", "-Werror", src, "-o", prog] + LINK)
    out = subprocess.run([prog], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    # get_path does not push begin, sums from end backwards, and gives nothing for a vertex without a predecessor
    assert out == ["0: 0 0:", "1: 2 2: 4 1", "2: 2 1: 2", "3: 3 2: 2 3", "4: 1 1: 4"]
