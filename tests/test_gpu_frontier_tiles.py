"""The merge-path frontier tile (csrc/gmx_frontier.h) at its boundaries, through every entry that expands a queue with it:
sssp, sssp_path under both schedules, avg_teen_cnt and hop_dist on forward-only uploads.

The graphs are layered: a root with d out-edges to level 1, every level-1 vertex with k out-edges into a shared level 2 of
L2 vertices without out-edges.  Every in-edge of a vertex comes from the level before it, so a round of sssp's queue, a
top-down level of hop_dist and the teens of one level are the same queue: n vertices of ONE out-degree.  With one
out-degree per queue the cut of the merged (row ends, edges) sequence into tiles of 2048 items does not depend on the order
in which the device's appends filled the queue, so what tile_facts() finds on the CPU is what the kernels meet.
test_cases_meet_every_boundary asserts, without a device, that the cases contain every boundary condition listed in FACTS."""
import functools

import numpy as np
import pytest

import pyoracle as po
from test_gpu_sssp_path import check_exact

TILE = 2048
INT_MAX = 2**31 - 1
# name: (d, k, L2)
CASES = {
    "hub_3tiles": (6143, 3, 4097),      # 1 + d = 3 tiles exactly; rows of k + 1 = 4 items; level 2: 2 tiles of row ends + 1 item
    "library_scan": (18431, 3, 4096),   # level 1 is longer than the single-workgroup scan of hop_dist takes (16384)
    "cut_rows": (5000, 2, 2048),        # rows of 3 items: the tile boundaries cut rows
    "long_rows": (2, 5000, 5000),       # two rows of 5000 edges behind each other, neither starting at a tile boundary
}
FACTS = ["total % 2048 == 0", "total % 2048 == 1", "tile without an edge", "tile staging 2049 row ends", "row spanning >= 3 tiles",
         "tile boundary on a row boundary"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, root, levels: vertex arrays by hop level, len, sssp distances), computed once."""
    d, k, L2 = CASES[name]
    assert k <= L2
    V = 1 + d + L2
    src = np.concatenate([np.zeros(d, np.int64), np.repeat(1 + np.arange(d), k)])
    dst = np.concatenate([1 + np.arange(d), 1 + d + (np.arange(d * k) % L2)])
    order = np.lexsort((dst, src))                                    # rows ascending, as every upload form stores them
    og = po.graph_from_edges(V, src[order].astype(np.int32), dst[order].astype(np.int32))
    hop = po.bfs_queue(og, 0)
    assert hop.max() == 2 and (hop != INT_MAX).all()
    levels = [np.flatnonzero(hop == l) for l in range(3)]
    length = np.random.default_rng(d).integers(1, 101, og.M).astype(np.int32)
    return og, 0, levels, length, po.sssp(og, length, 0)[0]


def tile_facts(deg):
    """The facts of FACTS that hold for a queue whose entries have the out-degrees deg[], in that order."""
    n = len(deg)
    off = np.concatenate([[0], np.cumsum(deg, dtype=np.int64)])
    m = int(off[-1])
    ends = off[1:] + np.arange(1, n + 1)                              # the diagonal at which row i is consumed, its end included
    nb = (n + m + TILE - 1) // TILE
    diag = np.minimum(np.arange(nb + 1, dtype=np.int64) * TILE, n + m)
    rows = np.searchsorted(ends, diag, side="right")                  # rows consumed at every tile boundary
    edges = diag - rows
    first = off[:-1] + np.arange(n)                                   # item of a row's first edge, and of its last
    last = ends - 2
    out = set()
    if (n + m) % TILE == 0:
        out.add(FACTS[0])
    if (n + m) % TILE == 1:
        out.add(FACTS[1])
    if (edges[1:] == edges[:-1]).any():
        out.add(FACTS[2])
    if (rows[1:] - rows[:-1] + 1 == TILE + 1).any():
        out.add(FACTS[3])
    if ((last // TILE - first // TILE >= 2) & (deg > 0)).any():
        out.add(FACTS[4])
    if np.isin(diag[1:-1], ends).any():                               # (an interior boundary: items follow)
        out.add(FACTS[5])
    return out, n, m


def test_cases_meet_every_boundary():
    seen = set()
    topdown = False
    for name in CASES:
        og, root, levels, length, dist = case(name)
        deg = np.diff(og.begin)
        src = np.repeat(np.arange(og.N), deg)
        hop = po.bfs_queue(og, root)
        # layered: every edge goes one level down, so a vertex's in-edges are all relaxed in one round and the rounds of
        # sssp's queue are the hop levels whatever the lengths are; the oracle's distances agree with that
        assert (hop[og.node_idx] == hop[src] + 1).all()
        assert (dist != INT_MAX).all() and dist[root] == 0
        for l in (1, 2):
            assert dist[levels[l]].min() > dist[levels[l - 1]].min()
        for l, q in enumerate(levels):
            assert len(np.unique(deg[q])) == 1, (name, l)             # one out-degree: the tiles do not depend on the queue's order
            facts, n, m = tile_facts(deg[q])
            print("%s level %d: n %d, m %d: %s" % (name, l, n, m, sorted(facts)))
            seen |= facts
            topdown |= l >= 1 and m > 2 * n + 1024                     # hop_dist takes the tile kernel, not the sparse one
        assert name != "library_scan" or len(levels[1]) > 16384
    assert seen == set(FACTS), set(FACTS) - seen
    assert topdown


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(scope="module")
def uploaded(gmx):
    return {name: gmx.Graph.upload(case(name)[0].begin, case(name)[0].node_idx, flags=gmx.GMX_GRAPH_NO_REVERSE) for name in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sssp(uploaded, name):
    og, root, _, length, want = case(name)
    assert np.array_equal(uploaded[name].sssp(length, root)[0], want)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule,delta", [("round", None), ("nearfar", None), ("nearfar", "1073741824")])   # (one band: the round queue's rounds)
@pytest.mark.parametrize("name", list(CASES))
def test_sssp_path(uploaded, monkeypatch, name, schedule, delta):
    monkeypatch.setenv("GMX_SSSP_PATH_SCHEDULE", schedule)
    if delta:
        monkeypatch.setenv("GMX_SSSP_DELTA", delta)
    og, root, _, length, want = case(name)
    check_exact(og.begin, og.node_idx, length, root, want, uploaded[name].sssp_path(length, root), (name, schedule, delta))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_avg_teen_cnt(uploaded, name):
    og, _, levels, _, _ = case(name)
    for l, q in enumerate(levels):                                    # the teens are one level: the queue of that level
        age = np.full(og.N, 40, np.int32)
        age[q] = 15
        want_avg, want_cnt = po.avg_teen_cnt(og, age, 20)
        avg, cnt, _ = uploaded[name].avg_teen_cnt(age, 20)
        assert np.array_equal(cnt, want_cnt), (name, l)
        assert avg == want_avg, (name, l)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hop_dist(uploaded, name):
    og, root, _, _, _ = case(name)
    assert np.array_equal(uploaded[name].hop_dist(root)[0], po.bfs_queue(og, root))
