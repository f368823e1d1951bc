"""Closeness, harmonic centrality and eccentricity, host side (no GPU): the one-thread BFS model that gmx.h defines
(closeness_model), which the GPU tests compare the four arrays with byte for byte; the model against networkx and against
closed forms; the fixed point's error bound; the Python helpers.

The model follows gmx.h.  D(v, s) is the hop distance in the mode's direction -- "out": from v to s along out-edges, "in":
from s to v, "both": with every stored slot read as an undirected edge.  Over the columns s with 0 < D(v, s) < infinity
(sources None: every vertex; a repeated source is another column): reach = their number, far = the sum of D, ecc = the
largest D, harm = the sum of floor(2^32 / D)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG

MODES = ("out", "in", "both")
ONE = 1 << 32


def walk_csr(V, begin, idx, mode):
    """The CSR a traversal from a SOURCE walks to find D(v, s) at v: the transpose for "out" (v reaches s), the rows as
    stored for "in", both for "both"."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V), np.diff(begin))
    if mode == "in":
        a, b = rows, idx
    elif mode == "out":
        a, b = idx, rows
    elif mode == "both":
        a, b = np.concatenate([rows, idx]), np.concatenate([idx, rows])
    else:
        raise ValueError(mode)
    o = np.argsort(a, kind="stable")
    wb = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=V))]).astype(np.int64)
    return wb, b[o]


def bfs_dist(V, wb, wi, wbl, wil, s):
    """dist[v] = the hops from s to v over the walk CSR, -1 where there is no path: one queue, one thread.  A level whose
    frontier is a few short rows is expanded slot by slot, a wide one with numpy; both take the levels in order."""
    dist = np.full(V, -1, np.int64)
    mark = np.zeros(V, bool)
    dist[s] = 0
    frontier, l = [s], 0
    while len(frontier):
        l += 1
        if len(frontier) <= 4 and sum(wbl[u + 1] - wbl[u] for u in frontier) <= 32:
            new = []
            for u in frontier:
                for w in wil[wbl[u]:wbl[u + 1]]:
                    if dist[w] < 0:
                        dist[w] = l
                        new.append(w)
            frontier = new
            continue
        frontier = np.asarray(frontier, np.int64)
        starts, cnt = wb[frontier], wb[frontier + 1] - wb[frontier]
        nb = wi[np.repeat(starts - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))]
        nb = nb[dist[nb] < 0]
        dist[nb] = l
        mark[nb] = True
        frontier = np.flatnonzero(mark)   # (each new vertex once)
        mark[frontier] = False
    return dist


def closeness_model(V, begin, idx, mode, sources=None):
    """(far[int64], reach[int32], ecc[int32], harm[uint64]) of the forward CSR (begin, idx)."""
    wb, wi = walk_csr(V, begin, idx, mode)
    wbl, wil = wb.tolist(), wi.tolist()
    far, reach, ecc, harm = np.zeros(V, np.int64), np.zeros(V, np.int32), np.zeros(V, np.int32), np.zeros(V, np.uint64)
    for s in (range(V) if sources is None else [int(x) for x in sources]):
        dist = bfs_dist(V, wb, wi, wbl, wil, s)
        at = np.flatnonzero(dist > 0)
        d = dist[at]
        far[at] += d
        reach[at] += 1
        ecc[at] = np.maximum(ecc[at], d)
        harm[at] += (ONE // d).astype(np.uint64)
    return far, reach, ecc, harm


def csr_from_edges(V, s, d):
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    o = np.argsort(s, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=V))]).astype(np.int32)
    return begin, d[o].astype(np.int32)


def random_multigraph(V, E, seed):
    """Repeated edges and self loops included."""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    loops = rng.integers(0, V, V // 10)
    rep = rng.integers(0, E, E // 10)
    return np.concatenate([s, loops, s[rep]]), np.concatenate([d, loops, d[rep]])


@pytest.fixture(scope="module")
def graphs():
    V = 300
    s, d = random_multigraph(V, 900, 21)
    return {"directed": (V, s, d), "symmetrised": (V, np.concatenate([s, d]), np.concatenate([d, s]))}


def nx_graph(V, s, d, mode):
    import networkx as nx
    G = nx.Graph() if mode == "both" else nx.DiGraph()
    G.add_nodes_from(range(V))
    G.add_edges_from((int(a), int(b)) for a, b in zip(s, d) if a != b)   # (self loops and repeats change no distance)
    return G


@pytest.mark.parametrize("name", ["directed", "symmetrised"])
@pytest.mark.parametrize("mode", MODES)
def test_model_against_networkx(graphs, name, mode):
    import networkx as nx
    V, s, d = graphs[name]
    begin, idx = csr_from_edges(V, s, d)
    far, reach, ecc, harm = closeness_model(V, begin, idx, mode)
    G = nx_graph(V, s, d, mode)
    if mode == "out":   # D(v, s) = the distance from v to s: a traversal from v along out-edges
        dist = {v: nx.single_source_shortest_path_length(G, v) for v in range(V)}
        D = lambda v, t: dist[v].get(t)
    else:
        dist = {t: nx.single_source_shortest_path_length(G, t) for t in range(V)}
        D = lambda v, t: dist[t].get(v)
    worst = 0.0
    for v in range(V):
        ds = [D(v, t) for t in range(V) if t != v and D(v, t) is not None]
        assert reach[v] == len(ds) and far[v] == sum(ds) and ecc[v] == (max(ds) if ds else 0)
        exact = sum(1.0 / x for x in ds)
        err = exact - float(harm[v]) / ONE
        assert -1e-12 * (1 + exact) <= err < reach[v] * 2.0 ** -32 + 1e-12 * (1 + exact), (v, err)
        if reach[v]:
            worst = max(worst, err / (reach[v] * 2.0 ** -32))
    print("%s %s: worst harmonic error %.2f of the bound reach * 2^-32" % (name, mode, worst))
    # networkx's own harmonic centrality sums 1 / d(u, v) over the paths INTO v: mode "in" (on the undirected graph: "both")
    if mode != "out":
        h = nx.harmonic_centrality(G)
        for v in range(V):
            assert abs(h[v] - float(harm[v]) / ONE) <= reach[v] * 2.0 ** -32 + 1e-12 * (1 + h[v])
    assert reach.max() > 100 and ecc.max() > 3


def test_eccentricity_on_a_strongly_connected_graph():
    import networkx as nx
    V = 300
    s, d = random_multigraph(V, 900, 22)
    s, d = np.concatenate([s, np.arange(V)]), np.concatenate([d, (np.arange(V) + 1) % V])   # a cycle through every vertex
    begin, idx = csr_from_edges(V, s, d)
    G = nx_graph(V, s, d, "out")
    assert nx.is_strongly_connected(G)
    far, reach, ecc, harm = closeness_model(V, begin, idx, "out")
    want = nx.eccentricity(G)   # max over t of d(v -> t)
    assert np.array_equal(ecc, [want[v] for v in range(V)]) and np.all(reach == V - 1)
    assert ecc.max() == nx.diameter(G) and ecc.min() == nx.radius(G)
    _, _, ecc_in, _ = closeness_model(V, begin, idx, "in")
    want_in = nx.eccentricity(G.reverse())
    assert np.array_equal(ecc_in, [want_in[v] for v in range(V)])


def test_directed_path_closed_forms():
    P = 97
    begin, idx = csr_from_edges(P, np.arange(P - 1), np.arange(1, P))
    v = np.arange(P, dtype=np.int64)
    far, reach, ecc, harm = closeness_model(P, begin, idx, "out")
    assert np.array_equal(far, (P - 1 - v) * (P - v) // 2) and np.array_equal(reach, P - 1 - v) and np.array_equal(ecc, P - 1 - v)
    assert np.array_equal(harm, [sum(ONE // l for l in range(1, P - x)) for x in range(P)])
    far, reach, ecc, harm = closeness_model(P, begin, idx, "in")
    assert np.array_equal(far, v * (v + 1) // 2) and np.array_equal(reach, v) and np.array_equal(ecc, v)
    far, reach, ecc, harm = closeness_model(P, begin, idx, "both")
    assert np.array_equal(far, v * (v + 1) // 2 + (P - 1 - v) * (P - v) // 2) and np.all(reach == P - 1) and np.array_equal(ecc, np.maximum(v, P - 1 - v))


def test_in_is_out_of_the_transpose(graphs):
    V, s, d = graphs["directed"]
    g, t = csr_from_edges(V, s, d), csr_from_edges(V, d, s)
    for a, b in zip(closeness_model(V, *g, "in"), closeness_model(V, *t, "out")):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(closeness_model(V, *g, "both"), closeness_model(V, *t, "both")):
        assert a.tobytes() == b.tobytes()


def test_sources_are_columns(graphs):
    """A listed source is a column, a repeated one another column; the sums are additive over the columns."""
    V, s, d = graphs["directed"]
    g = csr_from_edges(V, s, d)
    for mode in MODES:
        a = closeness_model(V, *g, mode, [3, 3, 5])
        b, c = closeness_model(V, *g, mode, [3]), closeness_model(V, *g, mode, [5])
        for k in (0, 1, 3):
            assert np.array_equal(a[k], 2 * b[k] + c[k])
        assert np.array_equal(a[2], np.maximum(b[2], c[2]))
        whole = closeness_model(V, *g, mode)
        parts = [closeness_model(V, *g, mode, range(lo, min(lo + 64, V))) for lo in range(0, V, 64)]
        for k in (0, 1, 3):
            assert np.array_equal(whole[k], sum(p[k] for p in parts))
        assert np.array_equal(whole[2], np.max([p[2] for p in parts], axis=0))
        for x in closeness_model(V, *g, mode, []):
            assert not x.any()


def test_python_helpers():
    import gmx
    far, reach = np.array([0, 6, 3]), np.array([0, 3, 2])
    assert np.array_equal(gmx.closeness_of(far, reach), [0.0, 0.5, 2 / 3])
    assert np.array_equal(gmx.closeness_of(far, reach, wasserman_faust=True), [0.0, 0.5 * 3 / 2, 2 / 3 * 2 / 2])
    assert np.array_equal(gmx.harmonic_of(np.array([0, ONE, ONE // 2 + ONE // 3], np.uint64)), [0.0, 1.0, (ONE // 2 + ONE // 3) / ONE])


def test_closeness_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    out = np.zeros(4, np.int64)
    src = np.zeros(1, np.int32)
    assert L.gmx_closeness(None, 0, None, 0, out.ctypes.data, None, None, None, None) == -1   # GMX_ERR_ARG
    assert L.gmx_closeness(None, 2, src.ctypes.data, 1, None, None, None, None, None) == -1
    assert L.gmx_closeness(None, 3, None, 0, None, None, None, None, None) == -1
    assert not out.any()
    assert "gmx_closeness" in gmx.EXPORTS and hasattr(L, "gmx_closeness") and hasattr(gmx.Graph, "closeness")
    assert gmx.Graph.CLOSE_MODES == {m: i for i, m in enumerate(MODES)}
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert ("int gmx_closeness(gmx_graph_t* g, int mode, const gmx_node_t* sources, int32_t nsources, int64_t* far_host, int32_t* reach_host, "
            "int32_t* ecc_host,\n                  uint64_t* harm_host, gmx_stats_t* stats);") in hdr
    for name, value in (("OUT", 0), ("IN", 1), ("BOTH", 2)):
        assert "#define GMX_CLOSE_%-4s %d " % (name, value) in hdr
    assert "EQUAL A ONE-THREAD BFS" in hdr


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_closeness.cc"
    src.write_text('#include "closeness.h"\n#include "gmx.h"\nint main() { gm_graph G; gm_node_seq Q; std::vector<node_t> p; '
                   'closeness(G, GMX_CLOSE_OUT, (double*) 0, (double*) 0, (int32_t*) 0); closeness(G, GMX_CLOSE_IN, Q, (double*) 0, (double*) 0, (int32_t*) 0); '
                   'closeness(G, GMX_CLOSE_BOTH, p, (double*) 0, (double*) 0, (int32_t*) 0); return 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_closeness")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "closeness.cc"))
