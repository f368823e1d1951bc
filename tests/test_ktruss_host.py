"""k-truss decomposition and per-edge triangle support, host side (no GPU): the one-thread model of gmx_ktruss's schedule
(ktruss_model.py), which the GPU tests compare bytes with, against networkx.k_truss, against closed forms and against the
clustering model's triangle count; the C entry's argument checks; what build() must leave behind."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from ktruss_model import book, ktruss_model, star_with_a_triangle, triangulated_grid, two_cliques_and_a_path
from test_clustering_host import clique, clustering_model, cycle, friendship, nx_graph
from test_scc_host import PKG, csr_of


def check_against_networkx(nx, V, begin, idx, m):
    """truss(e) >= k <=> e is an edge of networkx.k_truss(G, k), for every k up to max_truss + 1 (where nothing is left)."""
    G = nx_graph(nx, V, begin, idx)
    assert m["num_edges"] == G.number_of_edges()
    et = {e: int(t) for e, t in zip(m["edges"], m["edge_truss"])}
    for k in range(2, m["max_truss"] + 2):
        H = nx.k_truss(G, k)
        got = {(min(a, b), max(a, b)) for a, b in H.edges()}
        assert got == {e for e, t in et.items() if t >= k}, k
    es = {e: int(s) for e, s in zip(m["edges"], m["edge_support"])}
    for (a, b), s in es.items():
        assert s == len(set(G[a]) & set(G[b]))


def consistent(V, begin, idx, m):
    """What holds for every graph: slots of one edge carry one value, self loops 0, real edges at least 2, truss <= support + 2."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V), np.diff(begin))
    loop = rows == idx
    assert not m["truss"][loop].any() and not m["support"][loop].any()
    assert np.all(m["truss"][~loop] >= 2) and np.all(m["truss"][~loop] <= m["support"][~loop] + 2)
    key = np.minimum(rows, idx) * V + np.maximum(rows, idx)
    for arr in (m["truss"], m["support"]):
        seen = {}
        for k, x in zip(key[~loop].tolist(), arr[~loop].tolist()):
            assert seen.setdefault(k, x) == x
    assert m["max_truss"] == (int(m["truss"].max()) if len(idx) else 0) and m["top"] == int((m["edge_truss"] == m["max_truss"]).sum()) * (m["num_edges"] > 0)
    assert m["rounds"] == sum(m["rounds_per_level"]) and m["levels"] == len(m["rounds_per_level"])
    assert m["levels"] == len(set(m["edge_truss"].tolist()))   # every level removes at least one edge, and s only rises


def test_model_against_networkx_on_random_multigraphs():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(31)
    tri = 0
    for V, slots in ((30, 120), (60, 400), (300, 4000)):
        for trial in range(4):
            s, d = np.sort(rng.integers(0, V, slots)), rng.integers(0, V, slots)   # self loops and repeats included
            begin, idx = csr_of(V, s, d)[:2]
            m = ktruss_model(V, begin, idx)
            consistent(V, begin, idx, m)
            check_against_networkx(nx, V, begin, idx, m)
            tri += m["triangles"]
    assert tri > 1000


def shapes():
    return {"K5": clique(5), "K9": clique(9), "cycle7": cycle(7), "friendship6": friendship(6), "cliques_and_path": two_cliques_and_a_path(),
            "book40": book(40), "star_triangle": star_with_a_triangle(50), "grid8": triangulated_grid(8)}


def test_model_against_networkx_on_the_named_shapes():
    nx = pytest.importorskip("networkx")
    for name, (V, s, d) in shapes().items():
        o = np.argsort(s, kind="stable")
        begin, idx = csr_of(V, np.asarray(s)[o], np.asarray(d)[o])[:2]
        m = ktruss_model(V, begin, idx)
        consistent(V, begin, idx, m)
        check_against_networkx(nx, V, begin, idx, m)


def model_of_shape(V, s, d):
    o = np.argsort(s, kind="stable")
    return ktruss_model(V, *csr_of(V, np.asarray(s)[o], np.asarray(d)[o])[:2])


def test_closed_forms():
    for n in (3, 4, 9, 65):
        m = model_of_shape(*clique(n))
        assert np.all(m["support"] == n - 2) and np.all(m["truss"] == n) and (m["levels"], m["rounds"]) == (1, 1)
        assert m["slots"] == n * (n - 1) // 2 * (n - 1) and m["max_truss"] == n and m["top"] == m["num_edges"] == n * (n - 1) // 2
    V, s, d = two_cliques_and_a_path()
    m = model_of_shape(V, s, d)
    want = np.where(np.asarray(s) >= 12, 2, np.where(np.asarray(d) <= 4, 5, 9))
    o = np.argsort(s, kind="stable")
    assert np.array_equal(m["truss"], want[o]) and m["levels"] == 3 and m["max_truss"] == 9 and m["top"] == 36
    mb = model_of_shape(*book(500))
    assert mb["support"][0] == 500 and np.all(mb["support"][1:] == 1) and np.all(mb["truss"] == 3) and (mb["levels"], mb["rounds"]) == (1, 2)
    assert mb["triangles"] == 500 and mb["slots"] == 501 + 2 * 500 * 2
    ms = model_of_shape(*star_with_a_triangle(300))
    assert ms["levels"] == 2 and ms["max_truss"] == 3 and ms["top"] == 3 and int((ms["truss"] == 2).sum()) == 298 and ms["triangles"] == 1
    for n in (8, 16, 32):
        mg = model_of_shape(*triangulated_grid(n))
        assert np.all(mg["truss"] == 3) and (mg["levels"], mg["rounds"]) == (1, n) and mg["triangles"] == 2 * (n - 1) ** 2
    for V, begin, idx in ((0, [0], []), (3, [0, 0, 0, 0], []), (3, [0, 1, 2, 3], [0, 1, 2])):
        m = ktruss_model(V, begin, idx)
        assert (m["max_truss"], m["num_edges"], m["triangles"], m["levels"], m["rounds"], m["slots"], m["top"]) == (0,) * 7
        assert len(m["truss"]) == len(idx) and not m["truss"].any() and not m["support"].any()
    assert model_of_shape(*cycle(5))["truss"].tolist() == [2] * 5
    m = ktruss_model(*(lambda V, s, d: (V,) + tuple(csr_of(V, s, d)[:2]))(*clique(6)), peel=False)
    assert np.all(m["support"] == 4) and not m["truss"].any() and (m["max_truss"], m["rounds"], m["slots"]) == (0, 0, 0)


def test_support_sums_to_three_times_the_clustering_models_triangles(golden):
    rng = np.random.default_rng(32)
    cases = []
    for trial in range(30):
        V = int(rng.integers(1, 80))
        E = int(rng.integers(0, 6 * V + 1))
        cases.append((V,) + tuple(csr_of(V, np.sort(rng.integers(0, V, E)), rng.integers(0, V, E))[:2]))
    c = golden["cases"]["rmat8_noperm"]
    cases.append((256, c["begin"], c["node_idx"]))
    total = 0
    for V, begin, idx in cases:
        m, cm = ktruss_model(V, begin, idx), clustering_model(V, begin, idx)
        assert int(m["edge_support"].sum()) == 3 * cm["triangles"] and m["triangles"] == cm["triangles"] and m["num_edges"] == cm["up"]
        total += m["triangles"]
    assert total > 1000


def test_entry_is_declared_exported_bound_and_built():
    import gmx
    L = gmx.lib()
    assert "gmx_ktruss" in gmx.EXPORTS and hasattr(L, "gmx_ktruss") and hasattr(gmx.Graph, "ktruss")
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_ktruss(gmx_graph_t* g, int32_t* truss_host, int32_t* support_host, int32_t* max_truss, int64_t* num_edges, gmx_stats_t* stats);" in hdr
    assert os.path.exists(os.path.join(PKG, "bin", "ktruss")), "bin/ktruss not built"
    assert os.path.exists(os.path.join(PKG, "generated", "ktruss.cc")) and os.path.exists(os.path.join(PKG, "generated", "ktruss.h"))


def test_ktruss_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    k, n = C.c_int32(7), C.c_int64(7)
    tr = np.full(4, 5, np.int32)
    assert L.gmx_ktruss(None, tr.ctypes.data, None, C.byref(k), C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_ktruss(None, None, None, None, None, None) == -1
    assert L.gmx_ktruss(C.c_void_p(8), None, None, None, C.byref(n), None) == -1   # max_truss is checked before g is touched
    assert (k.value, n.value) == (7, 7) and np.all(tr == 5)
    with pytest.raises(gmx.GmxError):
        gmx.Graph(None).ktruss()
