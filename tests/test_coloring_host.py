"""Greedy vertex colouring, host side (no GPU): the one-thread first fit that gmx.h defines (greedy_model) and the synchronous
rounds that compute it (schedule_model), which the GPU tests compare color, depth and the log line with; the two against
each other and against networkx; a certificate; the C entry's argument checks; the drop-in header.

The models follow gmx.h.  Every stored slot u -> w with u != w makes u and w neighbours.  u is earlier than w when
(prio[u], -u) > (prio[w], -w); prio None is outdeg + indeg with every stored slot counted.  color[v] is the smallest colour
no earlier neighbour holds; depth[v] the longest chain of successively earlier neighbours that ends at v, in edges; npred[v]
the slots of v (out-row + in-row) whose other end is earlier, a repeated slot counted again."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG, csr_of


def neighbourhood(V, begin, idx):
    """(nb, ni, L): the rows of the symmetrised slot list without self loops (repeats kept) and outdeg + indeg of the
    stored slots, self loops included."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V), np.diff(begin))
    L = np.diff(begin) + np.bincount(idx, minlength=V)
    keep = rows != idx
    a, b = np.concatenate([rows[keep], idx[keep]]), np.concatenate([idx[keep], rows[keep]])
    o = np.argsort(a, kind="stable")
    nb = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=V))])
    return nb, b[o], L.astype(np.int64)


def order_of(V, L, prio):
    """The vertices from the earliest to the latest, and rank[v] = v's place in that order."""
    p = L if prio is None else np.asarray(prio, np.int64)
    order = np.lexsort((np.arange(V), -p))
    rank = np.empty(V, np.int64)
    rank[order] = np.arange(V)
    return order, rank


def greedy_model(V, begin, idx, prio=None):
    """dict(color, depth, npred, rounds, class0, num_colors, L, passes) of the forward CSR (begin, idx): one thread that takes
    the vertices in the order.  passes(W): the extra window passes if every row went through the block regime."""
    nb, ni, L = neighbourhood(V, begin, idx)
    order, rank = order_of(V, L, prio)
    a = np.repeat(np.arange(V), np.diff(nb))
    npred = np.bincount(a[rank[ni] < rank[a]], minlength=V).astype(np.int32)
    nbl, nil = nb.tolist(), ni.tolist()
    color, depth = [-1] * V, [0] * V
    for v in order.tolist():
        used, d = set(), -1
        for w in nil[nbl[v]:nbl[v + 1]]:
            c = color[w]
            if c >= 0:
                used.add(c)
                if depth[w] > d:
                    d = depth[w]
        c = 0
        while c in used:
            c += 1
        color[v], depth[v] = c, d + 1
    color, depth = np.array(color, np.int32).reshape(V), np.array(depth, np.int32).reshape(V)
    return {"color": color, "depth": depth, "npred": npred, "rounds": int(depth.max()) + 1 if V else 0, "class0": int((color == 0).sum()),
            "num_colors": int(color.max()) + 1 if V else 0, "L": L, "passes": lambda W: int((color.astype(np.int64) // W).sum())}


def schedule_model(V, begin, idx, prio=None):
    """dict(color, depth, rounds) by the schedule: round 0 colours the vertices without an earlier neighbour, round r + 1
    those whose last earlier neighbour was coloured in round r; a coloured vertex lowers the pending count of every
    neighbour that has no colour yet, once per slot."""
    nb, ni, L = neighbourhood(V, begin, idx)
    _, rank = order_of(V, L, prio)
    a = np.repeat(np.arange(V), np.diff(nb))
    pend = np.bincount(a[rank[ni] < rank[a]], minlength=V)
    color, depth = np.full(V, -1, np.int32), np.zeros(V, np.int32)
    ready = np.nonzero(pend == 0)[0]
    rounds = 0
    while len(ready):
        new = np.empty(len(ready), np.int32)
        for i, v in enumerate(ready):   # all of them read the colours of the rounds before
            cs = color[ni[nb[v]:nb[v + 1]]]
            new[i] = np.setdiff1d(np.arange(len(cs) + 1), cs[cs >= 0])[0]
        color[ready], depth[ready] = new, rounds
        rounds += 1
        lens = nb[ready + 1] - nb[ready]
        pos = np.repeat(nb[ready] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
        t = ni[pos]
        t, dec = np.unique(t[color[t] < 0], return_counts=True)
        pend[t] -= dec
        ready = t[pend[t] == 0]
    assert V == 0 or color.min() >= 0
    return {"color": color, "depth": depth, "rounds": rounds}


def certificate(V, begin, idx, color, num_colors):
    """What makes color a greedy colouring of some order, vectorised: proper, every vertex sees every smaller colour, class
    0 independent and maximal, the degree bound."""
    nb, ni, L = neighbourhood(V, begin, idx)
    color = np.asarray(color, np.int64)
    a = np.repeat(np.arange(V), np.diff(nb))
    assert not np.any(color[a] == color[ni])                                 # proper (class 0 independent among the rest)
    below = color[ni] < color[a]
    pairs = np.unique(a[below] * (num_colors + 1) + color[ni][below])
    assert np.array_equal(np.bincount(pairs // (num_colors + 1), minlength=V), color)   # a neighbour of every smaller colour
    sees0 = np.zeros(V, bool)
    sees0[a[color[ni] == 0]] = True
    assert np.array_equal(sees0, color > 0)                                  # class 0 is maximal, and independent
    assert num_colors == (color.max() + 1 if V else 0) and num_colors <= (L.max() + 1 if V else 0)


def _random_multigraph(rng, vmax):
    V = int(rng.integers(1, vmax + 1))
    E = int(rng.integers(0, 4 * V + 1))
    return V, rng.integers(0, V, E), rng.integers(0, V, E)   # repeats and self loops included


def _prios(rng, V):
    return {"degree": None, "id": np.zeros(V, np.int32), "random": rng.integers(-5, 5, V).astype(np.int32),
            "extremes": rng.choice([-2**31, 2**31 - 1, 0], V).astype(np.int32)}


def test_models_agree_with_each_other_and_with_networkx():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(21)
    for trial in range(150):
        V, s, d = _random_multigraph(rng, 50)
        begin, idx, _, _ = csr_of(V, s, d)
        G = nx.Graph()
        G.add_nodes_from(range(V))
        G.add_edges_from((int(u), int(w)) for u, w in zip(s, d) if u != w)
        for name, prio in _prios(rng, V).items():
            m, sm = greedy_model(V, begin, idx, prio), schedule_model(V, begin, idx, prio)
            assert np.array_equal(m["color"], sm["color"]) and np.array_equal(m["depth"], sm["depth"]) and m["rounds"] == sm["rounds"], (trial, name)
            order, _ = order_of(V, m["L"], prio)
            ref = nx.greedy_color(G, strategy=lambda G, c: order.tolist())
            assert np.array_equal(m["color"], [ref[v] for v in range(V)]), (trial, name)
            assert np.all(m["color"] <= np.minimum(m["npred"], m["L"]))


def test_certificate_on_directed_multigraphs_with_self_loops():
    rng = np.random.default_rng(22)
    for trial in range(150):
        V, s, d = _random_multigraph(rng, 60)
        begin, idx, _, _ = csr_of(V, s, d)
        for name, prio in _prios(rng, V).items():
            m = greedy_model(V, begin, idx, prio)
            certificate(V, begin, idx, m["color"], m["num_colors"])
            assert m["class0"] == int((m["color"] == 0).sum()) and m["rounds"] == m["depth"].max() + 1


def test_one_direction_its_transpose_and_the_symmetrised_form_give_the_same_arrays():
    rng = np.random.default_rng(23)
    for trial in range(60):
        V, s, d = _random_multigraph(rng, 40)
        prio = rng.integers(0, 4, V).astype(np.int32)
        forms = [csr_of(V, s, d)[:2], csr_of(V, d, s)[:2], csr_of(V, np.concatenate([s, d]), np.concatenate([d, s]))[:2]]
        for p in (None, prio, np.zeros(V, np.int32)):   # (None: the symmetrised form doubles every degree, the order stays)
            ms = [greedy_model(V, b, i, p) for b, i in forms]
            for m in ms[1:]:
                assert np.array_equal(m["color"], ms[0]["color"]) and np.array_equal(m["depth"], ms[0]["depth"])
            assert np.array_equal(2 * ms[0]["npred"], ms[2]["npred"]) and np.array_equal(ms[0]["npred"], ms[1]["npred"])


def path(P):
    return P, np.arange(P - 1), np.arange(1, P)


def clique_upper(n):
    a, b = np.nonzero(np.triu(np.ones((n, n), bool), 1))
    return n, a, b


def crown(n):
    """a_i = 2 i, b_i = 2 i + 1, a_i - b_j for i != j."""
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    return 2 * n, 2 * i, 2 * j + 1


def test_pinned_small_shapes():
    P = 257
    V, s, d = path(P)
    m = greedy_model(V, *csr_of(V, s, d)[:2], np.zeros(V, np.int32))
    assert np.array_equal(m["color"], np.arange(P) % 2) and m["rounds"] == P and np.array_equal(m["depth"], np.arange(P))
    V, s, d = clique_upper(300)
    m = greedy_model(V, *csr_of(V, s, d)[:2], np.zeros(V, np.int32))
    assert np.array_equal(m["color"], np.arange(300)) and m["rounds"] == 300 and m["passes"](64) == 560 and m["num_colors"] == 300
    assert np.array_equal(m["npred"], np.arange(300))
    V, s, d = crown(40)
    m = greedy_model(V, *csr_of(V, s, d)[:2], np.zeros(V, np.int32))
    assert m["num_colors"] == 40 and np.array_equal(m["color"], np.arange(80) // 2)
    m = greedy_model(0, [0], [])
    assert (m["rounds"], m["num_colors"], m["class0"]) == (0, 0, 0)
    m = greedy_model(3, [0, 1, 2, 3], [0, 1, 2])   # self loops only
    assert not m["color"].any() and m["rounds"] == 1 and m["class0"] == 3


def test_coloring_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n = C.c_int32(7)
    color = np.zeros(4, np.int32)
    assert L.gmx_coloring(None, None, color.ctypes.data, None, C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_coloring(None, None, None, None, None, None) == -1
    assert L.gmx_coloring(C.c_void_p(8), None, None, None, C.byref(n), None) == -1   # color_host is checked before g is touched
    assert L.gmx_coloring(None, color.ctypes.data, color.ctypes.data, color.ctypes.data, None, None) == -1
    assert "gmx_coloring" in gmx.EXPORTS and hasattr(L, "gmx_coloring") and hasattr(gmx.Graph, "coloring")
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_coloring(gmx_graph_t* g, const int32_t* prio_host, int32_t* color_host, int32_t* depth_host, int32_t* num_colors, gmx_stats_t* stats);" in hdr


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_coloring.cc"
    src.write_text('#include "coloring.h"\nint main() { gm_graph G; return coloring(G, (int32_t*) 0) + coloring(G, (int32_t*) 0, (int32_t*) 0) < 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_coloring")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "coloring.cc"))
