"""The one-workgroup tail walk (tail_rows of csrc/gmx_frontier.h) at its boundaries, through the three entries whose tail
kernels walk a queue with it: sssp_path_adj (both passes of a round), the route queries and random_bipartite_matching.

The graph is layered: a root with D out-edges to level 1, every level-1 vertex with an out-degree drawn from DEGREES into a
shared level 2 of L2 vertices without out-edges.  The queue the walk meets is the level-1 set (the second round of a search
from the root; the live lefts of the matching's first round): 8 / 9 are the two sides of the lane / wave threshold
*_TAIL_LANE = 8, 64 / 65 one and two steps of the wave loop, 1 the shortest row.  A workgroup of 1024 threads is 16 waves of
64 rows, so D > 1024 gives a wave a second pass over the queue and D % 64 != 0 a partial last group.  The order of the queue
is whatever the device's appends produced: test_queue_meets_every_boundary shows, without a device, that every order puts
lane rows and wave rows into one group of 64.  Costs are 1 .. 3, so equal offers compete for the winner word.

On a graph of two layers a two-sided route query ends after one hop from each end (the side with fewer slots walks both):
the level-1 queue is walked by the one-sided query; the two-sided ones and the transposed graph put the in-rows (one long row,
then rows of one slot) through the same walk.  For the reverse side to walk the level-1 queue the transposed graph gets a third
layer (third_layer): a vertex X in front of a sink with more parallel slots than the root's in-row and the level-1 in-rows
hold, so the side rule (the side with fewer slots is expanded) sends the reverse side from the root twice before X's row is
walked once."""
import functools

import numpy as np
import pytest

import test_gpu_random_bipartite_matching as rbm
import test_gpu_route as rt
import test_gpu_sssp_path_adj as spf
from test_random_bipartite_matching_host import rbm_model
from test_route_host import dijkstra_cost
from test_sssp_path_adj_host import sources, spf_model

D, L2 = 1100, 257
DEGREES = (1, 8, 9, 64, 65)
TAIL_LANE, WAVE, TAIL_THREADS = 8, 64, 1024


def csr(V, src, dst, w):
    order = np.lexsort((dst, src))                                    # rows ascending, as every upload form stores them
    begin = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int32)
    return begin, dst[order].astype(np.int32), w[order].astype(np.int32)


@functools.lru_cache(maxsize=None)
def case():
    """(begin, idx, w) of the layered graph and of its transpose, the level-1 vertices and the targets; computed once."""
    rng = np.random.default_rng(D)
    deg = rng.permutation(np.resize(DEGREES, D))                      # every degree D / 5 times, in random order
    first = rng.integers(0, L2, D)
    level1 = 1 + np.arange(D)
    src = np.concatenate([np.zeros(D, np.int64), np.repeat(level1, deg)])
    within = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
    dst = np.concatenate([level1, 1 + D + (np.repeat(first, deg) + within) % L2])   # a row's targets are distinct
    w = rng.integers(1, 4, len(src))
    V = 1 + D + L2
    fwd, bwd = csr(V, src, dst, w), csr(V, dst, src, w)
    for a in fwd + bwd:
        a.setflags(write=False)
    return fwd, bwd, level1, (1 + D, 1 + D + L2 // 2, V - 1)


@functools.lru_cache(maxsize=None)
def third_layer():
    """(begin, idx, w, X, K): the transposed graph and a vertex X with K parallel slots to the first target."""
    _, (tb, ti, tw), _, targets = case()
    K = len(ti)                                                          # more than D, and than the slots of the level-1 in-rows
    b = np.concatenate([tb, [tb[-1] + K]]).astype(np.int32)
    i = np.concatenate([ti, np.full(K, targets[0])]).astype(np.int32)
    w = np.concatenate([tw, np.random.default_rng(K).integers(1, 4, K)]).astype(np.int32)
    return b, i, w, len(tb) - 1, K


def test_queue_meets_every_boundary():
    (b, i, _), (tb, _, _), level1, targets = case()
    deg = np.diff(b)
    assert (sources(b)[np.isin(i, level1)] == 0).all() and deg[0] == D   # level 1 is what the root's round queues, all of it
    assert (deg[1 + D:] == 0).all()                                      # and the last queue: level 2 has no rows
    q = deg[level1]
    n = len(q)
    assert sorted(set(q.tolist())) == sorted(DEGREES)
    assert TAIL_LANE in q and TAIL_LANE + 1 in q and WAVE in q and WAVE + 1 in q
    assert n > TAIL_THREADS and n % WAVE != 0
    # groups of 64 consecutive queue entries: all but the last are full.  Were every group rows of one kind, the lane rows
    # would fill whole groups, with or without the partial one
    lane_rows = int((q <= TAIL_LANE).sum())
    assert 0 < lane_rows < n and lane_rows % WAVE not in (0, n % WAVE)
    assert deg[0] > WAVE * TAIL_LANE                                     # the first round is one row of many wave steps
    rdeg = np.diff(tb)                                                   # in-rows: the queues the two-sided queries walk
    assert (rdeg[level1] == 1).all() and all(rdeg[t] > TAIL_LANE for t in targets)
    assert int(q.sum()) > 4096                                           # with default knobs the grid takes the level-1 round
    # third_layer: the reverse side's rows are the out-rows above (the root's, then level 1 in the order queued), and X's
    # row outweighs each of its two queues, so the reverse side is expanded twice before the forward side once
    b3, i3, _, X, K = third_layer()
    assert np.array_equal(np.bincount(i3[:len(i3) - K], minlength=X)[level1], q) and np.bincount(i3[:len(i3) - K])[0] == D
    assert b3[X + 1] - b3[X] == K and K > D and K > int(q.sum()) and (i3[b3[X]:] == targets[0]).all()
    print("tail_rows queue: n %d, slots %d, lane rows %d, wave rows %d" % (n, int(q.sum()), lane_rows, n - lane_rows))


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@functools.lru_cache(maxsize=None)
def spf_want(end):
    (b, i, w), _, _, _ = case()
    want = spf_model(b, i, w.astype(np.float64), 0, end)
    for a in want[:3]:
        a.setflags(write=False)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("forced", ["all_tail", "default"])
@pytest.mark.parametrize("target", [False, True])
def test_sssp_path_adj(gmx, capfd, target, forced):
    (b, i, w), _, _, targets = case()
    end = targets[1] if target else -1
    cost = w.astype(np.float64)
    g = spf.forward_only(gmx, b, i)
    got, f = spf.logged(g, cost, 0, end, capfd, **spf.FORCED[forced])
    print("tail_rows sssp_path_f64 end %d %s: %s" % (end, forced, f))
    spf.check(spf_want(end), got, (end, forced))
    assert f["rounds"] >= 2
    if forced == "all_tail":
        assert f["grid_rounds"] == 0 and f["tail_rounds"] >= 2 and f["tail_launches"] == 1
        assert f["tail_slots"] == got[3]["edges_examined"] == len(i)     # the root's row, then every row of level 1
    else:
        assert f["grid_rounds"] > 0 and f["tail_rounds"] > 0             # the root's row by the tail, level 1 by the grid
    g.free()


@functools.lru_cache(maxsize=None)
def route_want(transposed, src, dst):
    b, i, w = case()[1 if transposed else 0]
    return dijkstra_cost(b, i, w, src, dst)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["all_tail", "default"])
@pytest.mark.parametrize("sides", ["both", "forward"])
@pytest.mark.parametrize("transposed", [False, True])
def test_route(gmx, capfd, transposed, sides, tail):
    b, i, w = case()[1 if transposed else 0]
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    env = dict(rt.SIDES[sides], **rt.TAILS[tail])
    for t in case()[3]:
        src, dst = (t, 0) if transposed else (0, t)
        got, f = rt.logged(r, src, dst, capfd, **env)
        rt.check(b, i, w, src, dst, route_want(transposed, src, dst), got, (transposed, sides, tail, t))
        assert got[0] and got[4] == 2 and f["sides"] == sides
        ran = f["f_grid"] + f["f_tail"] + f["r_grid"] + f["r_tail"]
        assert ran >= 2
        if tail == "all_tail":
            assert f["f_grid"] == f["r_grid"] == 0 and f["f_tail"] + f["r_tail"] == ran and f["tail_launches"] == 1
        if sides == "forward" and not transposed:                        # the root's row, then every row of level 1
            assert (f["f_slots"], f["r_slots"]) == (len(i), 0)
    print("tail_rows route transposed %d %s %s: %s" % (transposed, sides, tail, f))
    r.free()
    g.free()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["all_tail", "default"])
def test_route_reverse_side_walks_the_queue(gmx, capfd, tail):
    b, i, w, X, K = third_layer()
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    got, f = rt.logged(r, X, 0, capfd, **dict(rt.SIDES["both"], **rt.TAILS[tail]))
    print("tail_rows route third layer %s: %s" % (tail, f))
    rt.check(b, i, w, X, 0, dijkstra_cost(b, i, w, X, 0), got, tail)
    assert got[0] and got[4] == 3
    assert f["r_grid"] + f["r_tail"] == 2 and f["r_slots"] == len(i) - K  # the root's in-row, then every in-row of level 1
    assert f["f_grid"] + f["f_tail"] == 1 and f["f_slots"] == K
    if tail == "all_tail":
        assert (f["r_tail"], f["f_tail"], f["tail_launches"]) == (2, 1, 1)
    r.free()
    g.free()


@functools.lru_cache(maxsize=None)
def matching_case():
    """Level 1 -> level 2 as a bipartite graph of its own: the lefts are level 1, in the layered graph's order."""
    (b, i, _), _, level1, _ = case()
    lo, hi = int(b[1]), int(b[1 + D])
    mb = np.concatenate([b[1:1 + D + 1] - lo, np.full(L2, hi - lo)]).astype(np.int32)
    mi = (i[lo:hi] - 1).astype(np.int32)
    left = np.concatenate([np.ones(D, np.uint8), np.zeros(L2, np.uint8)])
    return mb, mi, left, rbm_model(mb, mi, left)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", ["all_tail", "default"])
def test_matching(gmx, capfd, forced):
    mb, mi, left, want = matching_case()
    g = gmx.Graph.upload(mb, mi)
    match, cnt, st, f = rbm.logged(g, left, capfd, **(rbm.FORCED["all_tail"] if forced == "all_tail" else {}))
    print("tail_rows random_bipartite_matching %s: %s" % (forced, f))
    rbm.check(want, match, cnt, st)
    assert f["grid_rounds"] + f["tail_rounds"] == want[2] and f["proposals"] == want[3]
    if forced == "all_tail":
        assert f["grid_rounds"] == 0 and f["tail_rounds"] == want[2] >= 2 and want[3] <= f["slots"] <= want[4]
    else:
        assert f["grid_rounds"] > 0
    g.free()
