"""k-clique counting, host side (no GPU): the one-thread model of gmx_kclique's recursion (kclique_model.py), which the GPU
tests compare bytes with, against networkx.enumerate_all_cliques, against the closed forms of the named shapes and, at k = 3,
against the clustering model's triangle counts; the C entry's argument checks; what build() must leave behind."""
import ctypes as C
import os
import subprocess
from math import comb

import numpy as np
import pytest

from conftest import ROOT
import kclique_sequences   # (adds kclique's row to the table of interleaved entries)
from kclique_model import (clique, clique_counts, esym, hub_over, hub_over_counts, kclique_model, multipartite, multipartite_counts)
from test_clustering_host import clustering_model, nx_graph, random_multigraph
from test_scc_host import CXX_FLAGS, PKG, csr_of
from test_upload_forms_host import unsorted_multigraph

KS = (3, 4, 5, 6, 7, 8)


def csr_of_shape(shape):
    V, s, d = shape
    o = np.argsort(np.asarray(s), kind="stable")
    return (V,) + tuple(csr_of(V, np.asarray(s)[o], np.asarray(d)[o])[:2])


def consistent(V, m, k):
    assert m["count"].dtype == np.int64 and len(m["count"]) == V and int(m["count"].sum()) == k * m["cliques"]
    assert len(m["up_len"]) == V and int(m["up_len"].sum()) == m["up"]


def by_enumeration(nx, V, begin, idx):
    """{k: (count, cliques)} for k = 3 .. 8 from networkx's list of all cliques (by size, ascending)."""
    out = {k: [np.zeros(V, np.int64), 0] for k in KS}
    for c in nx.enumerate_all_cliques(nx_graph(nx, V, begin, idx)):
        if len(c) > 8:
            break
        if len(c) >= 3:
            out[len(c)][0][c] += 1
            out[len(c)][1] += 1
    return out


def test_model_against_networkx_on_random_multigraphs_and_the_named_shapes():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(41)
    cases = []
    for trial in range(40):
        V, s, d = random_multigraph(rng, 60)   # self loops and repeats included
        cases.append((V,) + tuple(csr_of(V, s, d)[:2]))
    for V, slots in ((24, 400), (40, 900), (60, 1500)):   # dense enough for 7- and 8-cliques
        cases.append((V,) + tuple(csr_of(V, rng.integers(0, V, slots), rng.integers(0, V, slots))[:2]))
    cases += [csr_of_shape(sh) for sh in (clique(9), clique(12), multipartite((3, 2, 4, 1, 2)), multipartite((2,) * 8), hub_over(clique(8)),
                                           hub_over(multipartite((3, 3, 3, 3))))]
    seen = {k: 0 for k in KS}
    for V, begin, idx in cases:
        want = by_enumeration(nx, V, begin, idx)
        for k in KS:
            for ordered in (True, False):
                m = kclique_model(V, begin, idx, k, ordered)
                consistent(V, m, k)
                assert m["cliques"] == want[k][1] and m["count"].tobytes() == want[k][0].tobytes(), (V, k, ordered)
            seen[k] += want[k][1]
    assert all(seen[k] > 100 for k in KS), seen


def test_closed_forms():
    assert [esym((2, 3, 4), j) for j in range(5)] == [1, 9, 26, 24, 0]
    for n in (3, 4, 5, 20, 66):
        for k in (3, 4):
            m = kclique_model(*csr_of_shape(clique(n)), k)
            cnt, tot = clique_counts(n, k)
            assert m["cliques"] == tot == comb(n, k) and m["count"].tobytes() == cnt.tobytes() and np.all(cnt == comb(n - 1, k - 1))
            assert sorted(m["up_len"].tolist()) == list(range(n))   # every order is a tie: vertex v has n - 1 - v upper neighbours
    for k in KS:
        m = kclique_model(*csr_of_shape(clique(12)), k)
        assert (m["cliques"], m["count"].tolist()) == (comb(12, k), [comb(11, k - 1)] * 12)
    assert kclique_model(*csr_of_shape(clique(7)), 8)["cliques"] == 0
    sizes = (5, 6, 3, 1, 4, 7, 2, 3)
    for k in KS:
        m = kclique_model(*csr_of_shape(multipartite(sizes)), k)
        cnt, tot = multipartite_counts(sizes, k)
        assert m["cliques"] == tot and m["count"].tobytes() == cnt.tobytes()
    assert multipartite_counts(sizes, 8)[1] == int(np.prod(sizes))   # one clique per choice of a vertex from every part
    m = kclique_model(*csr_of_shape(multipartite((4, 4, 4))), 4)
    assert m["cliques"] == 0 and not m["count"].any() and kclique_model(*csr_of_shape(multipartite((4, 4, 4))), 3)["cliques"] == 64
    parts = (6, 5, 4, 3)
    for k in (3, 4, 5):
        m = kclique_model(*csr_of_shape(hub_over(multipartite(parts))), k)
        cnt, tot = hub_over_counts(lambda j: multipartite_counts(parts, j), k)
        assert m["cliques"] == tot == esym(parts, k) + esym(parts, k - 1) and m["count"].tobytes() == cnt.tobytes()
        m = kclique_model(*csr_of_shape(hub_over(clique(9))), k)
        cnt, tot = hub_over_counts(lambda j: clique_counts(9, j), k)
        assert m["cliques"] == tot == comb(10, k) and m["count"].tobytes() == cnt.tobytes()
    # no vertex, no edge, self loops only
    for V, begin, idx in ((0, [0], []), (3, [0, 0, 0, 0], []), (3, [0, 1, 2, 3], [0, 1, 2])):
        m = kclique_model(V, begin, idx, 3)
        assert m["cliques"] == 0 and len(m["count"]) == V and not m["count"].any() and m["up"] == 0


def test_k3_is_the_clustering_models_tri_byte_for_byte(golden):
    cases = [(256, golden["cases"][name]["begin"], golden["cases"][name]["node_idx"]) for name in sorted(golden["cases"])
             if len(golden["cases"][name]["begin"]) == 257]
    assert cases
    for V, hub_edges in ((64, 200), (3000, 8000)):
        cases.append((V,) + tuple(unsorted_multigraph(V, hub_edges, V)[:2]))
    total = 0
    for V, begin, idx in cases:
        m, cm = kclique_model(V, begin, idx, 3), clustering_model(V, begin, idx)
        assert m["count"].tobytes() == cm["tri"].tobytes() and m["cliques"] == cm["triangles"] and m["up"] == cm["up"]
        assert int(m["up_len"].max()) == cm["max_up"]
        total += m["cliques"]
    assert total > 1000


def test_kclique_is_a_row_of_the_table_of_interleaved_entries():
    import gmx
    import handle_sequences as hs
    assert "kclique" in vars(gmx.Graph) and list(hs.ROWS).count("kclique") == 1 and hs.ROWS["kclique"].args == kclique_sequences.ARGS
    assert [s.entry for s in hs.forward()].count("kclique") == 1 and [s.entry for s in hs.shuffled()].count("kclique") == 2
    for k, (label, a) in enumerate(kclique_sequences.ARGS):
        step = hs.Step("kclique", k, label)
        hs.check_step(step, hs.fake_call(step))
    wrong = list(hs.fake_call(hs.Step("kclique", 0, "S")))
    wrong[0] = wrong[0].copy()
    wrong[0][int(np.argmax(wrong[0]))] += 1
    with pytest.raises(AssertionError):
        hs.check_step(hs.Step("kclique", 0, "S"), tuple(wrong))


def test_entry_is_declared_exported_bound_and_built(tmp_path):
    import gmx
    L = gmx.lib()
    assert "gmx_kclique" in gmx.EXPORTS and hasattr(L, "gmx_kclique") and hasattr(gmx.Graph, "kclique")
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_kclique(gmx_graph_t* g, int32_t k, int64_t* count_host, int64_t* cliques, gmx_stats_t* stats);" in hdr
    assert "wrap modulo 2^64" in hdr
    assert os.path.exists(os.path.join(PKG, "bin", "kclique")), "bin/kclique not built"
    assert os.path.exists(os.path.join(PKG, "generated", "kclique.h"))
    obj = tmp_path / "kclique.o"
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), "-c", os.path.join(PKG, "generated", "kclique.cc"), "-o", str(obj)])
    assert obj.exists()
    src = tmp_path / "use_kclique.cc"
    src.write_text('#include "kclique.h"\nint main() { gm_graph G; return kclique(G, 4, (int64_t*) 0) < 0; }\n')
    link = [os.path.join(PKG, "libgmgraph.a"), "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), str(src), "-o", str(tmp_path / "use_kclique")] + link)


def test_kclique_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n = C.c_int64(7)
    cnt = np.full(4, 5, np.int64)
    bogus = C.c_void_p(8)   # never touched: every check comes before g is read
    assert L.gmx_kclique(bogus, 2, cnt.ctypes.data, C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_kclique(bogus, 9, cnt.ctypes.data, C.byref(n), None) == -1
    assert L.gmx_kclique(bogus, 4, cnt.ctypes.data, None, None) == -1
    assert L.gmx_kclique(None, 4, cnt.ctypes.data, C.byref(n), None) == -1
    assert L.gmx_kclique(None, 4, None, None, None) == -1
    assert n.value == 7 and np.all(cnt == 5)
    for k in (-1, 0, 2, 9, 1 << 20):
        assert L.gmx_kclique(None, k, None, C.byref(n), None) == -1
    with pytest.raises(gmx.GmxError):
        gmx.Graph(None).kclique(4)
