"""The definition of gmx_louvain (louvain_model.py) on graphs whose answer is known, its own invariants, and its quality next
to networkx's Louvain.  No device: these pin the schedule that the device tests then compare bytes with."""
import functools

import numpy as np
import pytest

import louvain_sequences   # noqa: F401  (adds louvain's row to the table of interleaved entries)
import pyoracle as po
from louvain_model import canonical, csr_of, level0, louvain_model, modularity_of, qnum_of


# ---------------------------------------------------------------- the small graphs (V, begin, idx), one stored slot per edge
def graph(V, edges):
    return (V,) + csr_of(V, edges)


def two_k5():
    k5 = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    return graph(10, k5 + [(5 + a, 5 + b) for a, b in k5] + [(4, 5)])


def ring_of_cliques(cliques=8, size=6):
    e = []
    for c in range(cliques):
        e += [(size * c + a, size * c + b) for a in range(size) for b in range(a + 1, size)]
        e.append((size * c + size - 1, size * ((c + 1) % cliques)))
    return graph(cliques * size, e)


def star(leaves):
    return graph(leaves + 1, [(0, j) for j in range(1, leaves + 1)])


def k44():
    return graph(8, [(u, 4 + w) for u in range(4) for w in range(4)])


def path(n):
    return graph(n, [(j, j + 1) for j in range(n - 1)])


def ring(n):
    return graph(n, [(j, (j + 1) % n) for j in range(n)])


def hub_and_ring(leaves):
    """A star whose leaves also form a ring: at round 0 the hub's row holds `leaves` distinct labels."""
    return graph(leaves + 1, [(0, j) for j in range(1, leaves + 1)] + [(j, j % leaves + 1) for j in range(1, leaves + 1)])


def hubs_of_degrees(degs):
    """One hub per entry of degs with exactly that many distinct neighbours (its own leaves); all leaves lie on one ring."""
    e, first, v = [], [], len(degs)
    for h, d in enumerate(degs):
        first.append(v)
        e += [(h, v + j) for j in range(d)]
        v += d
    leaves = list(range(len(degs), v))
    e += [(a, b) for a, b in zip(leaves, leaves[1:] + leaves[:1])]
    return graph(v, e)


SMALL = {"two_k5": two_k5, "ring_of_k6": ring_of_cliques, "star": lambda: star(19), "k44": k44, "path7": lambda: path(7), "path64": lambda: path(64),
         "ring5": lambda: ring(5), "ring64": lambda: ring(64), "one_edge": lambda: path(2), "loops": lambda: graph(4, [(0, 0), (0, 1), (1, 1), (2, 3), (3, 3), (1, 2)])}


@functools.lru_cache(maxsize=None)
def small(name, max_levels=32, max_rounds=64):
    V, b, i = SMALL[name]()
    return louvain_model(V, b, i, None, max_levels, max_rounds)


@functools.lru_cache(maxsize=None)
def rmat(scale, symmetrize=False):
    g = po.rmat_graph(scale)
    return po.symmetrize(g) if symmetrize else g


@functools.lru_cache(maxsize=None)
def rmat_model(scale, max_levels=32, max_rounds=64):
    g = rmat(scale)
    return louvain_model(g.N, g.begin, g.node_idx, None, max_levels, max_rounds)


def direct(V, begin, idx, weight, comm):
    """(Qnum, intra, m2) of a partition of the original graph, evaluated from the slots."""
    rows, cols, w = level0(V, begin, idx, weight)
    m2 = int(w.sum())
    return qnum_of(rows, cols, w, comm, m2) + (m2,)


# ---------------------------------------------------------------- known answers
def test_two_k5_joined_by_an_edge():
    r = small("two_k5")
    assert r["comm"].tolist() == [0] * 5 + [1] * 5 and r["num_comms"] == 2
    assert r["intra"] == 40 and r["m2"] == 42 and r["qnum"] == 42 * 40 - 2 * 21 * 21


def test_ring_of_eight_k6():
    r = small("ring_of_k6")
    assert r["comm"].tolist() == [v // 6 for v in range(48)] and r["num_comms"] == 8 and r["modularity"] == 0.8125


def test_star_is_one_community():
    r = small("star")
    assert r["num_comms"] == 1 and not r["comm"].any() and r["qnum"] == 0 and r["modularity"] == 0.0


def test_k44_stays_the_identity():
    """Every vertex of one side wants the lowest label of the other side and the other side the reverse: both half-rounds of
    round 0 lower Qnum and are rolled back."""
    r = small("k44")
    assert r["comm"].tolist() == list(range(8)) and (r["num_levels"], r["rollbacks"], r["rounds"], r["moves"]) == (0, 2, 1, 0)
    assert r["qnum"] == -8 * 16 and r["modularity"] == -0.125


@pytest.mark.parametrize("name", ["path7", "path64", "ring5", "ring64", "one_edge"])
def test_paths_and_rings(name):
    r = small(name)
    V, b, i = SMALL[name]()
    size = np.bincount(r["comm"])
    assert r["num_comms"] == len(size) and size.min() >= 2                    # nobody stays alone
    assert all(np.all(np.diff(np.flatnonzero(r["comm"] == c)) == 1) or name.startswith("ring") for c in range(len(size)))   # a path's communities are intervals
    assert r["qnum"] > 0 or name == "one_edge"
    if name == "ring64":
        assert abs(r["modularity"] - 0.742) < 5e-4
    if name == "one_edge":
        assert r["comm"].tolist() == [0, 0] and r["qnum"] == 0


def test_a_repeated_slot_is_a_weight():
    V, b, i = two_k5()
    e = [(u, int(x)) for u in range(V) for x in i[b[u]:b[u + 1]]]
    tripled = csr_of(V, [p for p in e for _ in range(3 if p == (4, 5) else 1)])
    w = np.ones(len(e), np.int32)
    w[e.index((4, 5))] = 3
    a, c = louvain_model(V, *tripled), louvain_model(V, b, i, w)
    assert a["comm"].tobytes() == c["comm"].tobytes() and {k: a[k] for k in a if k != "comm"} == {k: c[k] for k in c if k != "comm"}
    assert a["m2"] == 2 * (len(e) + 2)


def test_self_loops_count_twice_on_the_diagonal():
    V, b, i = SMALL["loops"]()
    rows, cols, w = level0(V, b, i, None)
    dense = np.zeros((V, V), np.int64)
    dense[rows, cols] = w
    assert dense.tolist() == [[2, 1, 0, 0], [1, 2, 1, 0], [0, 1, 0, 1], [0, 0, 1, 2]] and (dense == dense.T).all()
    r = small("loops")
    assert r["m2"] == 12 and r["trace"][0] == 12 * 6 - (9 + 16 + 4 + 9)   # the singletons: intra = the diagonal
    q, intra, m2 = direct(V, b, i, None, r["comm"])
    assert (q, intra, m2) == (r["qnum"], r["intra"], r["m2"])
    # a loop is no neighbour (e[] leaves w == i out): vertices that only have loops never move
    only = louvain_model(3, *csr_of(3, [(0, 0), (1, 1), (1, 1), (2, 2)]))
    assert only["comm"].tolist() == [0, 1, 2] and (only["num_levels"], only["rounds"], only["rollbacks"]) == (0, 1, 0)
    assert (only["m2"], only["intra"], only["qnum"]) == (8, 8, 8 * 8 - (4 + 16 + 4))


@pytest.mark.parametrize("name", ["ring64", "ring_of_k6", "path64"])
def test_level_limits_are_prefixes(name):
    full = small(name)
    V, b, i = SMALL[name]()
    zero = small(name, 0)
    assert zero["comm"].tolist() == list(range(V)) and zero["num_levels"] == 0 and zero["rounds"] == 0 and zero["qnum"] == full["trace"][0]
    assert zero["intra"] == 0 and zero["edges_examined"] == 0
    one = small(name, 1)
    assert one["num_levels"] == 1 and one["sizes"] == full["sizes"][:1] and one["trace"] == full["trace"][:len(one["trace"])]
    # every community of the full run is a union of communities of its first level
    assert len(set(zip(one["comm"].tolist(), full["comm"].tolist()))) == one["num_comms"]


def test_max_rounds_one_cuts_levels():
    full, cut = small("ring64"), small("ring64", 32, 1)
    assert full["cuts"] == 0 and cut["cuts"] >= 1 and cut["rounds"] == len(cut["sizes"]) and cut["qnum"] > cut["trace"][0]


@pytest.mark.parametrize("r", [small("ring64"), small("ring_of_k6"), small("two_k5"), rmat_model(10)], ids=["ring64", "ring_of_k6", "two_k5", "rmat10"])
def test_qnum_rises_strictly_and_the_result_is_the_direct_evaluation(r):
    assert all(a < b for a, b in zip(r["trace"], r["trace"][1:])) and r["trace"][-1] == r["qnum"]
    assert r["modularity"] == modularity_of(r["qnum"], r["m2"])
    assert canonical(r["comm"].tolist())[0].tobytes() == r["comm"].tobytes()


def test_result_equals_a_direct_evaluation_on_rmat():
    g, r = rmat(10), rmat_model(10)
    assert direct(g.N, g.begin, g.node_idx, None, r["comm"]) == (r["qnum"], r["intra"], r["m2"])
    w = np.random.default_rng(10).integers(1, 100, g.M).astype(np.int32)
    rw = louvain_model(g.N, g.begin, g.node_idx, w)
    assert direct(g.N, g.begin, g.node_idx, w, rw["comm"]) == (rw["qnum"], rw["intra"], rw["m2"]) and rw["comm"].tobytes() != r["comm"].tobytes()


def test_the_inputs_exercise_every_way_a_run_can_end():
    """From the model's counters: a rollback, a level cut by max_rounds, a run cut by max_levels, three levels or more."""
    assert small("k44")["rollbacks"] == 2 and rmat_model(10)["rollbacks"] >= 1
    assert small("ring64", 32, 1)["cuts"] >= 1 and rmat_model(10, 32, 1)["cuts"] >= 1
    assert small("ring64", 1)["num_levels"] == 1 < small("ring64")["num_levels"]
    assert small("ring64")["num_levels"] >= 3 and len(rmat_model(12)["sizes"]) >= 3


# ---------------------------------------------------------------- next to networkx
def nx_graph(nx, V, begin, idx):
    rows, cols, w = level0(V, begin, idx, None)
    G = nx.Graph()
    G.add_nodes_from(range(V))
    for u, x, a in zip(rows.tolist(), cols.tolist(), w.tolist()):
        if u <= x:
            G.add_edge(u, x, weight=a // 2 if u == x else a)   # (networkx counts a loop's weight twice in the degree itself)
    return G


@pytest.mark.parametrize("name", ["ring64", "ring_of_k6", "two_k5", "rmat10", "rmat12"])
def test_modularity_is_networkx_modularity(name):
    nx = pytest.importorskip("networkx")
    if name.startswith("rmat"):
        g = rmat(int(name[4:]))
        V, b, i, r = g.N, g.begin, g.node_idx, rmat_model(int(name[4:]))
    else:
        (V, b, i), r = SMALL[name](), small(name)
    parts = [set(np.flatnonzero(r["comm"] == c).tolist()) for c in range(r["num_comms"])]
    assert abs(nx.community.modularity(nx_graph(nx, V, b, i), parts, weight="weight") - r["modularity"]) < 1e-12


@pytest.mark.parametrize("scale", [10, 12])
def test_quality_is_on_par_with_networkx_louvain(scale):
    """Measured with networkx 3.4.2 on the project's RMAT generator (edge factor 16, seeds 0..2), model Q against networkx's
    lowest .. highest: scale 10: 0.095575 against 0.096797 .. 0.098269; scale 12: 0.094566 against 0.094070 .. 0.094534.  The
    model lay between 0.0012 below networkx's lowest and 0.00003 above its highest; the margin asked here is 0.005 below the
    lowest of the three seeds (four times the largest shortfall seen, 5 % of Q), with no bound from above."""
    nx = pytest.importorskip("networkx")
    g, r = rmat(scale), rmat_model(scale)
    G = nx_graph(nx, g.N, g.begin, g.node_idx)
    qs = [nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", seed=s), weight="weight") for s in range(3)]
    print("louvain quality scale %d: model %.6f networkx %s" % (scale, r["modularity"], ["%.6f" % q for q in qs]))
    assert r["modularity"] > min(qs) - 0.005
