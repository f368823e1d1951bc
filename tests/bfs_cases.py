"""Boundary graphs for hop_dist's level forms (csrc/gmx_bfs.hip), shared by test_bfs_model_host.py (which proves on the CPU,
from tests/bfs_model.py, that the cases meet every boundary listed in its FACTS) and test_gpu_bfs_levels.py (which runs them).

The lever for in-row positions: rows are stored ascending, so a vertex's place in an in-row is its id.  FILLERS have
out-edges but no in-edges: they are never in a frontier, and low- and high-numbered fillers around the frontier vertices put
the one parent of a vertex at any position of its in-row, or leave it out.  A filler with more out-edges than the parent
makes the hint miss.

case(name) -> Case(begin, node_idx, r_begin, r_node_idx, rows_sorted, root, reverse): the CSRs as uploaded verbatim
(reverse False: forward-only, GMX_GRAPH_NO_REVERSE)."""
import collections
import functools

import numpy as np

import bfs_model as bm

Case = collections.namedtuple("Case", "begin node_idx r_begin r_node_idx rows_sorted root reverse")

N_LOW, N_STRONG, N_WEAK, N_HIGH, N_SINK, FILLER_PAD = 256, 8, 64, 183, 1000, 40
PAD_SINKS = 4096


def _bu_rows(pad=0, heavy=False):
    """Root -> 8 STRONG and 64 WEAK parents (level 1).  The level out of them is bottom-up: the strong parents' 1000 sinks
    each make m_f > (E - explored) / 14.  Every TARGET has an in-row LOW[:k_lo] + parents + HIGH[:k_hi] (ids in that order), so
    the parent sits at position k_lo; a strong parent has more out-edges than any filler (hint hit), a weak one fewer than
    every filler (hint miss, the row is walked).  Second-level targets hang off first-level ones, a third-level one off a
    second-level one.  Ids: 0..255 low fillers (an aligned block of 256 without an in-edge), 256 root, strong, weak, high
    fillers up to 511, 512..767 a block with 120 walkers, then the listed targets, the sinks, [pad], and three targets last
    so that V % 4 == 3.
    pad > 0: that many more fillers with TWO out-edges each into 4096 more sinks (also fed by the strong parents): V passes
    BFS_HUBS, and the BFS_HUBS-th largest out-degree is 2, so a hint with out-degree 1 is certainly no hub slot.
    heavy: one second-level target gets 1100 out-edges, so the level after the bottom-up levels takes tiles, not sparse."""
    low = np.arange(N_LOW)
    root = N_LOW
    strong = root + 1 + np.arange(N_STRONG)
    weak = strong[-1] + 1 + np.arange(N_WEAK)
    high = weak[-1] + 1 + np.arange(N_HIGH)
    assert high[-1] == 511
    src, dst = [], []
    nxt = [512]
    wk = [0]

    def new():
        nxt[0] += 1
        return nxt[0] - 1

    def weak_parent():
        wk[0] += 1
        return int(weak[wk[0] % N_WEAK])

    def target(k_lo, parents, k_hi, v=None):
        v = new() if v is None else v
        row = list(low[:k_lo]) + [weak_parent() if p == "w" else int(strong[i % N_STRONG]) if p == "s" else p for i, p in
                                  enumerate(parents, v)] + list(high[:k_hi])
        src.extend(row)
        dst.extend([v] * len(row))
        return v

    for i in range(256):                       # the block 512..767: 120 walkers, the others found by their hint
        target(1, ["w"], 0) if i % 2 == 0 and i < 240 else target(0, ["s"], 0)
    t1 = {}
    for spec in [(0, "s", 0), (1, "", 0), (1, "w", 0), (0, "w", 1), (2, "w", 0), (3, "w", 0), (4, "w", 0), (30, "w", 0), (31, "w", 0),
                 (31, "w", 1), (3, "ww", 4), (32, "w", 0), (94, "w", 0), (95, "w", 0), (96, "w", 0), (160, "w", 0), (97, "", 0),
                 (120, "", 41), (10, "s", 5), (40, "ww", 30), (32, "w", 100), (95, "w", 80), (96, "w", 100), (3, "w", 60), (40, "w", 150),
                 (0, "s", 0), (0, "s", 0), (0, "s", 0)]:
        t1[spec] = target(spec[0], list(spec[1]), spec[2])
    # second level: an only-flagged vertex whose one in-neighbour is a first-level target with that single out-edge; walkers
    a, b, c = t1[(0, "s", 0)], t1[(2, "w", 0)], t1[(10, "s", 5)]
    t2_only = target(0, [a], 0)
    t2_walk = target(5, [b], 0)
    t2_more = [target(k, [c], 2) for k in (0, 33, 100)]
    t3 = target(0, [t2_walk], 0)
    target(2, [t3], 0)
    sinks = np.array([new() for _ in range(N_SINK)])
    for s in strong:
        src.extend([s] * N_SINK)
        dst.extend(sinks)
    if heavy:
        src.extend([t2_more[0]] * 1100)
        dst.extend(list(sinks) + list(range(512, 612)))
    fillers = np.concatenate([low, high])
    for i, f in enumerate(fillers):            # every filler has more out-edges than any weak parent
        src.extend([f] * FILLER_PAD)
        dst.extend(sinks[(7 * i + 25 * np.arange(FILLER_PAD)) % N_SINK])
    if pad:
        psinks = np.array([new() for _ in range(PAD_SINKS)])
        pfill = np.array([new() for _ in range(pad)])
        for s in strong:
            src.extend([s] * PAD_SINKS)
            dst.extend(psinks)
        src.extend(np.repeat(pfill, 2))
        dst.extend(psinks[np.arange(2 * pad) % PAD_SINKS])
    while (nxt[0] + 3) % 4 != 3 or (nxt[0] + 3) % 64 == 0:
        new()                                  # (isolated)
    target(0, ["s"], 0)
    target(2, ["w"], 0)
    target(1, "", 0)
    V = nxt[0]
    src.extend([root] * (N_STRONG + N_WEAK))
    dst.extend(list(strong) + list(weak))
    return Case(*bm.build_csr(V, src, dst), True, root, True)


def _two_cluster():
    """the graph of test_gpu_parity.test_hop_dist_direction_switches_twice: two dense clusters joined by a long path"""
    rng = np.random.default_rng(7)
    nc, npath = 6000, 60
    V = 2 * nc + npath
    src, dst = [], []
    for base in (0, nc + npath):
        a = rng.integers(0, nc, 24 * nc) + base
        b = rng.integers(0, nc, 24 * nc) + base
        src += [a, b]
        dst += [b, a]
    path = np.arange(nc - 1, nc + npath + 1)
    src += [path[:-1], path[1:]]
    dst += [path[1:], path[:-1]]
    return Case(*bm.build_csr(V, np.concatenate(src), np.concatenate(dst)), True, 0, True)


def _root_row(d, reverse=False, shuffle=False, all_self=False):
    """Root 2 with a row of d slots: itself (a self-loop), vertex 3 twice (a repeat), then distinct vertices; every level-1
    vertex has one out-edge to the SAME leaf (reached from every lane and every workgroup of the level), which has five."""
    root = 2
    row = [root] * d if all_self else ([3] if d == 1 else ([root, 3, 3] + list(range(4, d + 1)))[:d])
    l1 = sorted(set(row) - {root})
    leaf = max(row) + 1
    V = leaf + 6
    src = [root] * len(row) + l1 + [leaf] * 5
    dst = row + [leaf] * len(l1) + list(range(leaf + 1, leaf + 6))
    begin, node_idx, rb, rn = bm.build_csr(V, src, dst)
    if shuffle:                                # the root's row as the caller had it: the repeats apart
        s = slice(begin[root], begin[root + 1])
        node_idx[s] = np.roll(node_idx[s][::-1], 1)
        node_idx[s][[0, -2]] = node_idx[s][[-2, 0]]   # (descending, the root last; one of the two 3s to the front)
        assert (node_idx[s][1:] < node_idx[s][:-1]).any() and (node_idx[s] == 3).sum() == 2
    return Case(begin, node_idx, rb if reverse else None, rn if reverse else None, not shuffle, root, reverse)


def _star2(d, V, reverse=True):
    """root 0 -> d vertices, each with one out-edge to a vertex of its own; behind them 40 vertices out of reach with 30 edges
    each among themselves (so that E / 14 exceeds the root's row and level 0 is top-down); the other vertices are isolated"""
    assert V >= 2 * d + 41
    far = 2 * d + 1 + np.arange(40)
    src = [0] * d + list(range(1, d + 1)) + list(np.repeat(far, 30))
    dst = list(range(1, d + 1)) + list(range(d + 1, 2 * d + 1)) + list(far[(np.arange(1200) // 30 + 1 + np.arange(1200) % 30) % 40])
    c = bm.build_csr(V, src, dst)
    return Case(c[0], c[1], c[2] if reverse else None, c[3] if reverse else None, True, 0, reverse)


def _stale_bits(reverse=True):
    """root -> 64 -> 64 (one edge each: a top-down level 1 after `first+bitmap`) -> 30 each into 700: a bottom-up level 2 whose
    frontier bitmap is the one the level out of the root wrote into"""
    l1, l2, l3 = 1 + np.arange(64), 65 + np.arange(64), 129 + np.arange(700)
    src = [0] * 64 + list(l1) + list(np.repeat(l2, 30))
    dst = list(l1) + list(l2) + list(l3[(11 * np.arange(64 * 30)) % 700])
    c = bm.build_csr(1403, src, dst)
    return Case(c[0], c[1], c[2] if reverse else None, c[3] if reverse else None, True, 0, reverse)


def _sparse_rows():
    """root -> six vertices with 0, 1, 16, 17, 80 and 81 out-edges: one wave of the sparse kernel"""
    lens = [0, 1, 16, 17, 80, 81]
    src, dst = [0] * 6, list(range(1, 7))
    for i, k in enumerate(lens):
        src += [1 + i] * k
        dst += list(7 + (13 * i + np.arange(k)) % 120)
    return Case(*bm.build_csr(131, src, dst)[:2], None, None, True, 0, False)


def _one_row(k):
    """root -> a -> k vertices: a one-vertex queue with k edges"""
    src, dst = [0] + [1] * k, [1] + list(range(2, k + 2))
    return Case(*bm.build_csr(k + 5, src, dst)[:2], None, None, True, 0, False)


def _layers(d, k, L2):
    """root -> d -> k each into L2 (the layered graphs of test_gpu_frontier_tiles.py)"""
    src = np.concatenate([np.zeros(d, np.int64), np.repeat(1 + np.arange(d), k)])
    dst = np.concatenate([1 + np.arange(d), 1 + d + (np.arange(d * k) % L2)])
    return Case(*bm.build_csr(1 + d + L2, src, dst)[:2], None, None, True, 0, False)


BUILDERS = {
    "bu_rows": _bu_rows,
    "bu_rows_heavy": lambda: _bu_rows(heavy=True),
    "bu_rows_hubs": lambda: _bu_rows(pad=131072 + 40),
    "two_cluster": _two_cluster,
    "root_1": lambda: _root_row(1),
    "root_2047": lambda: _root_row(2047),
    "root_2048": lambda: _root_row(2048),
    "root_2049": lambda: _root_row(2049),
    "root_2049_unsorted": lambda: _root_row(2049, shuffle=True),
    "root_all_self": lambda: _root_row(3, all_self=True),
    "star_63": lambda: _star2(63, 179),
    "star_64": lambda: _star2(64, 181),
    "star_64_bigV": lambda: _star2(64, 65 * 1024),
    "star_65_bigV": lambda: _star2(65, 65 * 1024),
    "stale_bits": _stale_bits,
    "stale_bits_forward": lambda: _stale_bits(reverse=False),
    "sparse_rows": _sparse_rows,
    "one_row_1026": lambda: _one_row(1026),
    "one_row_1027": lambda: _one_row(1027),
    "queue_16384": lambda: _layers(16384, 3, 4096),
    "queue_16385": lambda: _layers(16385, 3, 4096),
}
CASES = list(BUILDERS)
BOTTOM_UP_CASES = ["bu_rows", "bu_rows_heavy", "two_cluster", "stale_bits", "star_63", "star_64"]
RANK_CASES = ["bu_rows", "bu_rows_heavy", "two_cluster"]
HUB_CASE = "bu_rows_hubs"
HUB_MIN_V = 1 << 17   # GMX_BFS_HUB_MIN_V under which HUB_CASE gets its hub list


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name, rank=0, nranks=1, plain=False, hub_min_v=bm.BFS_HUB_MIN_V):
    c = case(name)
    return bm.run(c.begin, c.node_idx, c.r_begin, c.r_node_idx, c.rows_sorted, c.root, rank, nranks, plain, hub_min_v)
