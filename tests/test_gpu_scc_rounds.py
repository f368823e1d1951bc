"""gmx_scc's multi-workgroup rounds: what runs while more than the single-workgroup tail's share of vertices is live after
the first FW-BW -- the recount and trim rounds, colouring rounds (converging, and abandoned after their hop budget and
followed by another round), the FW-BW of later rounds, and the hand-over to the tail.  One graph gets there at its natural
size; the other tests lower the hand-over point with GMX_SCC_TAIL (a development option, like GMX_BFS_HUB_MIN_V) so the
small shapes of test_gpu_scc.py take the same path.  Every result is compared with the restated kosaraju.gm or scipy."""
import re

import numpy as np
import pytest

from test_gpu_scc import _shape, _unsorted_multigraph, check
from test_scc_host import canonical, kosaraju_check, scipy_scc

pytestmark = pytest.mark.gpu
PHASES = re.compile(r"gmx scc phases: trim [\d.]+ ms \((\d+) removed\), fwbw [\d.]+ ms \((\d+)\), colour [\d.]+ ms \((\d+)\), "
                    r"tail [\d.]+ ms \((\d+)\), relabel [\d.]+ ms; rounds (\d+), engine (\d)")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def phases(capfd, g):
    """g.scc() with the per-phase line on: (comp, count, stats, {trim, fwbw, colour, tail, rounds, engine})."""
    capfd.readouterr()
    comp, n, st = g.scc()
    err = capfd.readouterr().err
    m = PHASES.search(err)
    assert m, err
    keys = ("trim", "fwbw", "colour", "tail", "rounds", "engine")
    return comp, n, st, dict(zip(keys, (int(x) for x in m.groups())))


def _big_remainder_graph(seed=5):
    """290 K vertices whose remainder after the first FW-BW is 188 K: a strongly connected A (100 K, the pivot's), a
    strongly connected B (80 K) that A reaches one way, 1000 chains of 40 into A and 1000 out of B (removed by trim
    rounds), and three layers of 1000 10-cycles linked as a DAG below B (removed by colouring).  Ids permuted."""
    rng = np.random.default_rng(seed)
    nA, nB = 100_000, 80_000
    A, B = np.arange(nA), nA + np.arange(nB)
    s = [A, np.repeat(A, 4), B, B, rng.integers(0, nA, 1000)]
    d = [np.roll(A, -1), rng.integers(0, nA, 4 * nA), np.roll(B, -1), nA + rng.integers(0, nB, nB), nA + rng.integers(0, nB, 1000)]
    base = nA + nB
    C, L = 1000, 40
    cin = base + np.arange(C * L).reshape(C, L)
    base += C * L
    s += [cin[:, :-1].ravel(), cin[:, -1]]
    d += [cin[:, 1:].ravel(), rng.integers(0, nA, C)]
    cout = base + np.arange(C * L).reshape(C, L)
    base += C * L
    s += [cout[:, :-1].ravel(), nA + rng.integers(0, nB, C)]
    d += [cout[:, 1:].ravel(), cout[:, 0]]
    layers, per, K = 3, 1000, 10
    cyc = base + np.arange(layers * per * K).reshape(layers, per, K)
    base += layers * per * K
    flat = cyc.reshape(-1, K)
    s += [flat.ravel(), nA + rng.integers(0, nB, 500)]
    d += [np.roll(flat, -1, axis=1).ravel(), cyc[0, rng.integers(0, per, 500), rng.integers(0, K, 500)]]
    for layer in range(layers - 1):
        for _ in range(2):
            s.append(cyc[layer, np.arange(per), rng.integers(0, K, per)])
            d.append(cyc[layer + 1, rng.integers(0, per, per), rng.integers(0, K, per)])
    s, d = np.concatenate(s), np.concatenate(d)
    perm = rng.permutation(base)
    return base, perm[s], perm[d]


def test_remainder_above_the_tail_at_natural_size(gmx, capfd, monkeypatch):
    pytest.importorskip("scipy")
    V, s, d = _big_remainder_graph()
    g = gmx.Graph.from_edges(V, s, d)
    monkeypatch.setenv("GMX_SCC_PHASES", "1")
    comp, n, st, ph = phases(capfd, g)
    begin, idx, _, _ = g.download(reverse=False)
    en, ecomp = scipy_scc(V, begin, idx)
    assert n == en
    assert np.array_equal(comp, ecomp)
    assert st["vertices_reached"] == int(np.bincount(comp).max()) == 100_000
    assert ph["engine"] == 1 and ph["fwbw"] == 100_000      # A through the traversal engine
    assert ph["trim"] > 2000 + 70_000                          # beyond the 2000 seeds: the chains, by trim rounds
    assert ph["colour"] >= 80_000                              # B (and cycles) by a converging colouring round
    assert ph["trim"] + ph["fwbw"] + ph["colour"] + ph["tail"] == V


# shapes whose rounds all run as multi-workgroup launches once the tail takes over only at 64 (or 0) live vertices
ROUND_SHAPES = ["self_loops_only", "path", "reverse_path", "cycle", "triangle_chain", "triangle_chain_backwards", "star_both",
                "two_sccs_one_way", "hub_without_in_edges"]


# (the 2^16 path and cycle with tail=0 would take a launch per hop down to their last vertex: tail=64 only)
@pytest.mark.parametrize("name,tail", [(n, 64) for n in ROUND_SHAPES] +
                         [(n, 0) for n in ROUND_SHAPES if n not in ("path", "reverse_path", "cycle")])
def test_shapes_through_the_multi_workgroup_rounds(gmx, monkeypatch, name, tail):
    monkeypatch.setenv("GMX_SCC_TAIL", str(tail))
    V, s, d = _shape(name)
    check(gmx.Graph.from_edges(V, s, d))


def test_abandoned_colouring_then_another_round(gmx, capfd, monkeypatch):
    """256 triangles, each with an edge into the next: the minimum needs 768 hops down the chain, more than a colouring
    round's budget, so rounds give up and the next round's FW-BW goes on (outside the traversal engine after the first)."""
    monkeypatch.setenv("GMX_SCC_TAIL", "0")
    monkeypatch.setenv("GMX_SCC_PHASES", "1")
    V, s, d = _shape("triangle_chain")
    g = gmx.Graph.from_edges(V, s, d)
    comp, n, st, ph = phases(capfd, g)
    en, ecomp = kosaraju_check(V, *g.download())
    assert n == en == 256
    assert np.array_equal(comp, canonical(ecomp))
    assert ph["tail"] == 0 and ph["rounds"] > 1 and st["iterations"] == ph["rounds"]
    assert ph["fwbw"] > 3                                      # more than the first round's triangle
    assert ph["trim"] + ph["fwbw"] + ph["colour"] == V


def test_converging_colouring_round_with_lowered_tail(gmx, capfd, monkeypatch):
    """2000 undirected paths of 2 to 12 vertices (both directions of every edge, ids permuted): trim finds nothing, the
    first FW-BW takes one path, and one colouring round takes all the others."""
    monkeypatch.setenv("GMX_SCC_TAIL", "64")
    monkeypatch.setenv("GMX_SCC_PHASES", "1")
    rng = np.random.default_rng(3)
    sizes = rng.integers(2, 13, 2000)
    V = int(sizes.sum())
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    a = np.concatenate([np.arange(st, st + k - 1) for st, k in zip(starts, sizes)])
    perm = rng.permutation(V)
    s, d = perm[np.concatenate([a, a + 1])], perm[np.concatenate([a + 1, a])]
    g = gmx.Graph.from_edges(V, s, d)
    comp, n, st, ph = phases(capfd, g)
    en, ecomp = kosaraju_check(V, *g.download())
    assert n == en == 2000 and np.array_equal(comp, canonical(ecomp))
    assert ph["trim"] == 0 and ph["colour"] == V - ph["fwbw"] and ph["rounds"] == 1


@pytest.mark.parametrize("scale", [10, 12])
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("tail", [64, 0])
def test_rmat_through_the_multi_workgroup_rounds(gmx, monkeypatch, scale, permute, tail):
    monkeypatch.setenv("GMX_SCC_TAIL", str(tail))
    check(gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute))


@pytest.mark.parametrize("tail", [64, 0])
def test_unsorted_multigraph_through_the_multi_workgroup_rounds(gmx, monkeypatch, tail):
    """The pivot (the hub) has an unsorted row longer than V: FW-BW walks live vertices instead of using the engine."""
    monkeypatch.setenv("GMX_SCC_TAIL", str(tail))
    V = 3000
    begin, idx, rb, ri = _unsorted_multigraph(V, 8000, 17)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    comp, n, st = g.scc()
    en, mem = kosaraju_check(V, begin, idx, rb, ri)
    assert n == en and np.array_equal(comp, canonical(mem))
    assert st["vertices_reached"] == int(np.bincount(comp).max())
