"""The 4-node graphlet census, host side (no GPU): the two one-thread forms of gmx_graphlets (graphlets_model.py), which the GPU
tests compare bytes with, against each other on random graphs, on the named shapes and on the golden RMAT-8 graph; the closed
forms; the sum identities; multigraph slots and self loops; the C entry's argument checks; what build() must leave behind."""
import ctypes as C
import os
import subprocess
from math import comb

import numpy as np
import pytest

from conftest import ROOT
import graphlets_sequences   # (adds graphlets' row to the table of interleaved entries)
from graphlets_model import (GRAPHLETS, NAMES, ORBITS, SHAPES, bipartite_gdv, clique_gdv, clique_subgraph_gdv, cycle_gdv, graphlets_definition, graphlets_formulas, grid_closed,
                             identities_hold, induced_from, nonzero_of, path_gdv, star_gdv, totals_of)
from squares_model import bipartite, clique, cycle, grid, path, squares_definition, star
from test_kclique_host import csr_of_shape
from test_scc_host import CXX_FLAGS, PKG, csr_of


def both(V, begin, idx):
    """The definition's result, after the formulas have been found to give the same bytes; the non-induced rows alongside."""
    d = graphlets_definition(V, begin, idx)
    f = graphlets_formulas(V, begin, idx, True)
    n = graphlets_formulas(V, begin, idx, False)
    assert d["gdv"].dtype == np.int64 and d["gdv"].shape == (V, ORBITS) and d["totals"].shape == (GRAPHLETS,)
    assert f["gdv"].tobytes() == d["gdv"].tobytes() and f["totals"].tobytes() == d["totals"].tobytes(), (V, d["totals"], f["totals"])
    assert induced_from(n["gdv"]).tobytes() == d["gdv"].tobytes() and (d["gdv"] >= 0).all() and (n["gdv"] >= d["gdv"])[:, 3:].all()
    for m in (d, n):
        assert identities_hold(m["gdv"]) and totals_of(m["gdv"]).tobytes() == m["totals"].tobytes()
    assert f["nonzero"] == nonzero_of(d["gdv"]) and f["triangles"] == int(d["totals"][2]) == int(n["totals"][2]) and f["up"] == int(d["totals"][0])
    return d, n


def random_graph(rng, V, density):
    a, b = np.nonzero(np.triu(rng.random((V, V)) < density, 1))
    return csr_of(V, a, b)[:2]


def test_both_forms_agree_on_random_graphs():
    rng = np.random.default_rng(15)
    seen = np.zeros(ORBITS, np.int64)
    for trial in range(200):
        V = int(rng.integers(5, 15))
        begin, idx = random_graph(rng, V, 0.1 + 0.8 * (trial % 9) / 8)
        d, n = both(V, begin, idx)
        seen += d["gdv"].sum(axis=0)
    assert (seen > 1000).all(), seen


def test_named_shapes_and_every_orbit():
    seen = np.zeros(ORBITS, np.int64)
    for name, (shape, closed) in sorted(SHAPES.items()):
        V, begin, idx = csr_of_shape(shape)
        d, n = both(V, begin, idx)
        if closed is not None:
            assert d["gdv"].tobytes() == closed[0].tobytes() and d["totals"].tobytes() == closed[1].tobytes(), name
        seen += d["gdv"].sum(axis=0) > 0
    assert (seen[4:] > 0).all(), seen   # each 4-node orbit is non-zero on at least one named shape
    V, begin, idx = csr_of_shape(SHAPES["paw"][0])
    assert graphlets_definition(V, begin, idx)["gdv"][:, 9:12].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]
    V, begin, idx = csr_of_shape(SHAPES["diamond"][0])
    assert graphlets_definition(V, begin, idx)["gdv"][:, 12:14].tolist() == [[0, 1], [0, 1], [1, 0], [1, 0]]


def test_closed_forms():
    for n in (4, 5, 9, 20):
        gdv, totals = clique_gdv(n)
        d, nn = both(*csr_of_shape(clique(n)))
        assert d["gdv"].tobytes() == gdv.tobytes() and totals.tolist() == [comb(n, 2), 0, comb(n, 3), 0, 0, 0, 0, 0, comb(n, 4)]
        # the subgraph counts of K_n: every 4-subset holds 12 paths, 4 claws, 3 cycles, 12 paws, 6 diamonds and one K4
        assert nn["totals"][3:].tolist() == [x * comb(n, 4) for x in (12, 4, 3, 12, 6, 1)]
        assert nn["gdv"].tobytes() == clique_subgraph_gdv(n)[0].tobytes() and nn["totals"].tobytes() == clique_subgraph_gdv(n)[1].tobytes()
    for n in (3, 9, 30):
        gdv, totals = star_gdv(n)
        d, _ = both(*csr_of_shape(star(n)))
        assert d["gdv"].tobytes() == gdv.tobytes() and totals.tolist() == [n, comb(n, 2), 0, 0, comb(n, 3), 0, 0, 0, 0]
    for n in (4, 5, 6, 11):
        gdv, totals = cycle_gdv(n)
        d, _ = both(*csr_of_shape(cycle(n)))
        assert d["gdv"].tobytes() == gdv.tobytes() and totals.tolist() == ([4, 4, 0, 0, 0, 1, 0, 0, 0] if n == 4 else [n, n, 0, n, 0, 0, 0, 0, 0])
    for n in (2, 3, 4, 5, 9):
        gdv, totals = path_gdv(n)
        d, _ = both(*csr_of_shape(path(n)))
        assert d["gdv"].tobytes() == gdv.tobytes() and totals.tolist() == [n - 1, max(n - 2, 0), 0, max(n - 3, 0), 0, 0, 0, 0, 0]
    for a, b in ((1, 4), (2, 2), (2, 9), (3, 12), (5, 5)):
        gdv, totals = bipartite_gdv(a, b)
        d, _ = both(*csr_of_shape(bipartite(a, b)))
        assert d["gdv"].tobytes() == gdv.tobytes()
        assert totals.tolist() == [a * b, a * comb(b, 2) + b * comb(a, 2), 0, 0, a * comb(b, 3) + b * comb(a, 3), comb(a, 2) * comb(b, 2), 0, 0, 0]
    for m, n in ((2, 2), (3, 3), (5, 7)):
        cols, totals = grid_closed(m, n)
        d, _ = both(*csr_of_shape(grid(m, n)))
        assert d["totals"].tobytes() == totals.tobytes()
        for k, col in cols.items():
            assert d["gdv"][:, k].tolist() == col.tolist(), (m, n, k)
    # no vertex, no edge, self loops only
    for V, begin, idx in ((0, [0], []), (3, [0, 0, 0, 0], []), (3, [0, 1, 2, 3], [0, 1, 2])):
        for m in (graphlets_formulas(V, begin, idx), graphlets_formulas(V, begin, idx, False)) + ((graphlets_definition(V, begin, idx),) if V else ()):
            assert m["gdv"].shape == (V, ORBITS) and not m["gdv"].any() and not m["totals"].any()


def test_both_forms_agree_on_the_golden_rmat8(golden):
    c = golden["cases"]["rmat8_noperm"]
    d, n = both(256, c["begin"], c["node_idx"])
    assert (d["totals"] > 0).all(), d["totals"]
    assert n["gdv"][:, 8].tobytes() == squares_definition(256, c["begin"], c["node_idx"])["count"].tobytes()


def test_multigraph_slots_and_self_loops_change_nothing():
    rng = np.random.default_rng(16)
    for trial in range(10):
        V = int(rng.integers(6, 13))
        a, b = np.nonzero(np.triu(rng.random((V, V)) < 0.5, 1))
        want = graphlets_formulas(V, *csr_of(V, a, b)[:2])
        loops = rng.integers(0, V, 4)
        s = np.concatenate([a, b[:5], a[:3], loops])   # antiparallel slots, repeats, self loops
        t = np.concatenate([b, a[:5], b[:3], loops])
        o = rng.permutation(len(s))
        begin, idx = csr_of(V, s[o], t[o])[:2]
        assert graphlets_formulas(V, begin, idx)["gdv"].tobytes() == want["gdv"].tobytes()
        assert graphlets_definition(V, begin, idx)["gdv"].tobytes() == want["gdv"].tobytes()


def test_graphlets_is_a_row_of_the_table_of_interleaved_entries():
    import gmx
    import handle_sequences as hs
    assert "graphlets" in vars(gmx.Graph) and list(hs.ROWS).count("graphlets") == 1 and hs.ROWS["graphlets"].args == graphlets_sequences.ARGS
    assert [s.entry for s in hs.forward()].count("graphlets") == 1 and [s.entry for s in hs.shuffled()].count("graphlets") == 2
    for label, a in graphlets_sequences.ARGS:
        assert label == "D" or "_env" not in a   # (an identity-order call on S would make test_workspace's clustering rebuild S's plan)
    for k, (label, a) in enumerate(graphlets_sequences.ARGS):
        step = hs.Step("graphlets", k, label)
        hs.check_step(step, hs.fake_call(step))
    wrong = list(hs.fake_call(hs.Step("graphlets", 0, "S")))
    wrong[0] = wrong[0].copy()
    wrong[0][5, 12] += 1
    with pytest.raises(AssertionError):
        hs.check_step(hs.Step("graphlets", 0, "S"), tuple(wrong))
    s, b = hs.want_of("graphlets", 0, "S"), hs.want_of("graphlets", 1, "B")
    assert (s["totals"] > 0).all() and b["totals"][2] == 0 and b["totals"][5] > 0   # B has no triangle, but butterflies
    line = ("gmx graphlets: plan V 4096 E 9 up 8 order degree built 1 adj_built 1 groups_built 1 squares_built 1 kclique_built 1; cap 512 long 2048 counts lds induced 1; "
            "items 7 staged + 0 memory; long_rows 0; triangles 5; totals 1 2 3 4 5 6 7 8 9\n")
    f = graphlets_sequences.log_fields("noise\n" + line)
    assert f["totals"] == list(range(1, 10)) and f["order"] == "degree" and f["counts"] == "lds" and f["triangles"] == 5 and f["V"] == 4096


def test_entry_is_declared_exported_bound_and_built(tmp_path):
    import gmx
    L = gmx.lib()
    assert "gmx_graphlets" in gmx.EXPORTS and hasattr(L, "gmx_graphlets") and hasattr(gmx.Graph, "graphlets")
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_graphlets(gmx_graph_t* g, int induced, int64_t* gdv_host, int64_t* totals, gmx_stats_t* stats);" in hdr
    assert "divide before they multiply" in hdr
    assert os.path.exists(os.path.join(PKG, "bin", "graphlets")), "bin/graphlets not built"
    assert os.path.exists(os.path.join(PKG, "generated", "graphlets.h"))
    obj = tmp_path / "graphlets.o"
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), "-c", os.path.join(PKG, "generated", "graphlets.cc"), "-o", str(obj)])
    assert obj.exists()
    src = tmp_path / "use_graphlets.cc"
    src.write_text('#include "graphlets.h"\nint main() { gm_graph G; int64_t t[9]; graphlets(G, (int64_t*) 0, t); return t[0] != 0; }\n')
    link = [os.path.join(PKG, "libgmgraph.a"), "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), str(src), "-o", str(tmp_path / "use_graphlets")] + link)


def test_graphlets_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    totals = np.full(9, 7, np.int64)
    gdv = np.full(30, 5, np.int64)
    bogus = C.c_void_p(8)   # never touched: every check comes before g is read
    assert L.gmx_graphlets(bogus, 1, gdv.ctypes.data, None, None) == -1   # GMX_ERR_ARG
    assert L.gmx_graphlets(bogus, 2, gdv.ctypes.data, totals.ctypes.data, None) == -1
    assert L.gmx_graphlets(bogus, -1, None, totals.ctypes.data, None) == -1
    assert L.gmx_graphlets(None, 1, gdv.ctypes.data, totals.ctypes.data, None) == -1
    assert L.gmx_graphlets(None, 0, None, None, None) == -1
    assert np.all(totals == 7) and np.all(gdv == 5)
    with pytest.raises(gmx.GmxError):
        gmx.Graph(None).graphlets()
    assert NAMES[0] == "edges" and len(NAMES) == GRAPHLETS
