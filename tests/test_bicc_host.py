"""The host models of gmx_biconnected against each other (no GPU): the linear Hopcroft-Tarjan that the device tests use as
their oracle equals the oracle from the definitions (remove a vertex or an edge and count components) on a few hundred
random multigraphs with loops and on a small instance of every shape test_gpu_bicc.py runs, equals NetworkX where that
imports, and the numbering rules hold.  The shapes live here so that both files build the same graphs."""
import numpy as np
import pytest

from bicc_model import canonical, csr_from_edges, definition_oracle, forest_model, hopcroft_tarjan, simple_edges, slot_ends

ARRAYS = ("bridge", "artic", "block", "tecc")
COUNTS = ("num_blocks", "num_bridges", "num_artic", "num_tecc", "num_comps", "largest_block_edges")


def same(a, b):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in COUNTS:
        assert a[k] == b[k], k


# ---- shapes: (V, src, dst)
def grid(n, permute_seed=None):
    v = np.arange(n * n).reshape(n, n)
    s = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    d = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    if permute_seed is not None:
        perm = np.random.default_rng(permute_seed).permutation(n * n)
        s, d = perm[s], perm[d]
    return n * n, s, d


def star(leaves, chords, seed=3):
    """Hub 0 with `leaves` leaves and `chords` random edges among the leaves."""
    rng = np.random.default_rng(seed)
    s = np.concatenate([np.zeros(leaves, np.int64), rng.integers(1, leaves + 1, chords)])
    d = np.concatenate([np.arange(1, leaves + 1), rng.integers(1, leaves + 1, chords)])
    return leaves + 1, s, d


def cycle(n):
    return n, np.arange(n), (np.arange(n) + 1) % n


def path(n):
    return n, np.arange(n - 1), np.arange(1, n)


def path_chords(P, span=33, every=7):
    k = np.arange(0, P - span - 7, every)
    return P, np.concatenate([np.arange(P - 1), k]), np.concatenate([np.arange(1, P), k + span])


def two_k5():
    s, d = [], []
    for base in (0, 5):
        for i in range(5):
            for j in range(i + 1, 5):
                s.append(base + i)
                d.append(base + j)
    return 12, np.array(s + [4, 10, 11]), np.array(d + [10, 11, 5])


def union(count, lo=6, hi=40, seed=5):
    """A disjoint union of `count` random multigraphs (loops and repeats included) of lo .. hi vertices."""
    rng = np.random.default_rng(seed)
    s, d, base = [], [], 0
    for _ in range(count):
        n = int(rng.integers(lo, hi + 1))
        m = int(rng.integers(n // 2, 2 * n))
        s.append(base + rng.integers(0, n, m))
        d.append(base + rng.integers(0, n, m))
        base += n
    return base, np.concatenate(s), np.concatenate(d)


SHAPES = {
    "self_loop": lambda: (1, np.array([0]), np.array([0])),
    "one_slot": lambda: (2, np.array([0]), np.array([1])),
    "both_ways": lambda: (2, np.array([0, 1]), np.array([1, 0])),
    "twice": lambda: (2, np.array([0, 0]), np.array([1, 1])),
    "triangle": lambda: cycle(3),
    "path": lambda: path(300),
    "star": lambda: star(3000, 200),
    "cycle4096": lambda: cycle(4096),
    "bowtie_low": lambda: (5, np.array([0, 1, 2, 0, 3, 4]), np.array([1, 2, 0, 3, 4, 0])),
    "bowtie_high": lambda: (5, np.array([4, 0, 1, 4, 2, 3]), np.array([0, 1, 4, 2, 3, 4])),
    "two_k5": two_k5,
    "grid64": lambda: grid(64),
    "grid64_permuted": lambda: grid(64, 9),
    "path_chords": lambda: path_chords(4096),
    "union2000": lambda: union(2000),
}
SMALL = {   # the same builders at a size the definition oracle takes
    "path": lambda: path(40),
    "star": lambda: star(60, 9),
    "cycle4096": lambda: cycle(64),
    "grid64": lambda: grid(8),
    "grid64_permuted": lambda: grid(8, 9),
    "path_chords": lambda: path_chords(64, 5, 7),
    "union2000": lambda: union(3, 6, 20),
}


def random_multigraph(rng):
    V = int(rng.integers(1, 41))
    E = int(rng.integers(0, 3 * V))
    return V, rng.integers(0, V, E), rng.integers(0, V, E)


def check_against_networkx(V, begin, idx, got):
    nx = pytest.importorskip("networkx")
    a, b = simple_edges(V, begin, idx)
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(a.tolist(), b.tolist()))
    bridges = [(min(x, y), max(x, y)) for x, y in nx.bridges(G)]
    label = {}
    for i, comp in enumerate(nx.biconnected_component_edges(G)):
        for x, y in comp:
            label[(min(x, y), max(x, y))] = i
    u, w = slot_ends(V, begin, idx)
    lab = [label.get((min(x, y), max(x, y)), -1) for x, y in zip(u.tolist(), w.tolist())]
    same(got, canonical(V, begin, idx, bridges, list(nx.articulation_points(G)), lab))


def test_hopcroft_tarjan_equals_the_definitions_on_random_multigraphs():
    rng = np.random.default_rng(2026)
    seen_bridge = seen_artic = seen_loop = 0
    for _ in range(300):
        V, s, d = random_multigraph(rng)
        begin, idx = csr_from_edges(V, s, d)
        want = definition_oracle(V, begin, idx)
        same(hopcroft_tarjan(V, begin, idx), want)
        seen_bridge += want["num_bridges"] > 0
        seen_artic += want["num_artic"] > 0
        seen_loop += int(np.any(s == d))
    assert min(seen_bridge, seen_artic, seen_loop) > 50


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hopcroft_tarjan_equals_the_definitions_on_every_shape(name):
    V, s, d = (SMALL.get(name) or SHAPES[name])()
    begin, idx = csr_from_edges(V, s, d)
    same(hopcroft_tarjan(V, begin, idx), definition_oracle(V, begin, idx))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hopcroft_tarjan_equals_networkx(name):
    V, s, d = SHAPES[name]()
    begin, idx = csr_from_edges(V, s, d)
    check_against_networkx(V, begin, idx, hopcroft_tarjan(V, begin, idx))


def test_known_counts():
    def counts(name):
        V, s, d = SHAPES[name]()
        r = hopcroft_tarjan(V, *csr_from_edges(V, s, d))
        return r["num_blocks"], r["num_bridges"], r["num_artic"], r["num_tecc"]
    assert counts("self_loop") == (0, 0, 0, 1)
    for name in ("one_slot", "both_ways", "twice"):
        assert counts(name) == (1, 1, 0, 2)
    assert counts("triangle") == (1, 0, 0, 1)
    assert counts("path") == (299, 299, 298, 300)
    assert counts("cycle4096") == (1, 0, 0, 1)
    assert counts("bowtie_low") == counts("bowtie_high") == (2, 0, 1, 1)
    assert counts("two_k5") == (5, 3, 4, 4)
    assert counts("grid64") == (1, 0, 0, 1)
    assert counts("path_chords")[:2] == (10, 9)


def test_numbering_rules():
    rng = np.random.default_rng(8)
    for _ in range(50):
        V, s, d = random_multigraph(rng)
        begin, idx = csr_from_edges(V, s, d)
        r = hopcroft_tarjan(V, begin, idx)
        u, w = slot_ends(V, begin, idx)
        blk = r["block"]
        assert np.array_equal(blk == -1, u == w)
        ids = blk[blk >= 0]
        if len(ids):   # dense, and in the order of first appearance by slot
            _, first = np.unique(ids, return_index=True)
            assert np.array_equal(np.unique(ids), np.arange(r["num_blocks"])) and np.all(np.diff(first) > 0)
        # every slot of one edge carries the same bridge flag and block
        key = np.minimum(u, w) * V + np.maximum(u, w)
        for k in np.unique(key[u != w]):
            assert len(set(blk[key == k])) == 1 and len(set(r["bridge"][key == k])) == 1
        # tecc: dense by smallest vertex; a bridge joins two of them, and the counts add up
        _, first = np.unique(r["tecc"], return_index=True)
        assert np.all(np.diff(first) > 0) and len(first) == r["num_tecc"] == r["num_comps"] + r["num_bridges"]
        assert not np.any(r["bridge"][u == w])
        b = r["bridge"] == 1
        assert np.all(r["tecc"][u[b]] != r["tecc"][w[b]]) and np.all(r["tecc"][u[~b]] == r["tecc"][w[~b]])


def test_row_order_does_not_change_the_numbering_by_uploaded_slot():
    """Sorting the rows moves slots; the block of an edge, named by the block's smallest slot of the ORIGINAL order, does not."""
    rng = np.random.default_rng(4)
    V, s, d = union(20, 6, 30, seed=12)
    sh = rng.permutation(len(s))
    begin, idx = csr_from_edges(V, s[sh], d[sh])
    r = hopcroft_tarjan(V, begin, idx)
    rows = np.repeat(np.arange(V), np.diff(begin))
    order = np.lexsort((idx, rows))
    rs = hopcroft_tarjan(V, begin, idx[order])   # numbered by sorted slot: a different, equally valid naming
    assert np.array_equal(rs["bridge"], r["bridge"][order]) and rs["num_blocks"] == r["num_blocks"]
    pairs = set(zip(rs["block"].tolist(), r["block"][order].tolist()))
    assert len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


def test_forest_model_on_known_shapes():
    V, s, d = cycle(4096)
    f = forest_model(V, *csr_from_edges(V, s, d))
    assert (f["levels"], f["roots"], f["tree"], f["walks"], f["steps"]) == (2049, 1, 4095, 1, 4095)
    V, s, d = grid(64)
    f = forest_model(V, *csr_from_edges(V, s, d))
    assert f["levels"] == 127 and f["tree"] == 4095 and f["walks"] == 2 * 64 * 63 - 4095 and f["steps"] == 257985
    assert np.array_equal(f["level"], np.add.outer(np.arange(64), np.arange(64)).ravel())
    V, s, d = path(300)
    f = forest_model(V, *csr_from_edges(V, s, d))
    assert (f["levels"], f["walks"], f["steps"]) == (300, 0, 0) and np.array_equal(f["par"][1:], np.arange(299))
    V, s, d = union(50)
    f = forest_model(V, *csr_from_edges(V, s, d))
    lvl, par = f["level"], f["par"]
    nonroot = lvl > 0
    assert np.all(lvl[par[nonroot]] == lvl[nonroot] - 1) and np.all(par[~nonroot] == np.flatnonzero(~nonroot))
