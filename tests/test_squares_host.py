"""4-cycle (square) counting, host side (no GPU): the two one-thread forms of gmx_squares (squares_model.py), which the GPU
tests compare bytes with, against each other, against a brute force over 4-subsets and against the closed forms of the named
shapes; the class prediction; the C entry's argument checks; what build() must leave behind."""
import ctypes as C
import os
import subprocess
from math import comb

import numpy as np
import pytest

from conftest import ROOT
import squares_sequences   # (adds squares' row to the table of interleaved entries)
from kclique_model import orientation
from squares_model import (_simple_pairs, plan_ids, binary_tree, bipartite, bipartite_counts, brute_force, classes_of, clique, clique_counts, cycle, grid, grid_counts, hypercube,
                           hypercube_counts, knobs_in_force, path, squares_definition, squares_schedule, star)
from test_clustering_host import random_multigraph
from test_kclique_host import csr_of_shape
from test_scc_host import CXX_FLAGS, PKG, csr_of
from test_upload_forms_host import unsorted_multigraph


def consistent(V, m):
    assert m["count"].dtype == np.int64 and len(m["count"]) == V and int(m["count"].sum()) == 4 * m["squares"]


def both(V, begin, idx):
    """The definition's result, after the schedule under both orders has been found to give the same bytes."""
    d = squares_definition(V, begin, idx)
    consistent(V, d)
    for ordered in (True, False):
        s = squares_schedule(V, begin, idx, ordered)
        consistent(V, s)
        assert s["squares"] == d["squares"] and s["count"].tobytes() == d["count"].tobytes(), (V, ordered)
        assert len(s["D"]) == len(s["W"]) == V and int(s["D"].sum()) == s["up"] and s["wedges"] == int(s["W"][s["D"] >= 2].sum())
    return d


def test_both_forms_against_brute_force_on_random_multigraphs():
    rng = np.random.default_rng(43)
    seen = 0
    for trial in range(24):
        V = int(rng.integers(9, 13))
        n = int(rng.integers(V, 4 * V))
        s, d = rng.integers(0, V, n), rng.integers(0, V, n)
        s, d = np.concatenate([s, d[:5], s[:4], [0, 1]]), np.concatenate([d, s[:5], d[:4], [0, 1]])   # antiparallel slots, repeats, self loops
        begin, idx = csr_of(V, s, d)[:2]
        m = both(V, begin, idx)
        cnt, n = brute_force(V, begin, idx)
        assert m["squares"] == n and m["count"].tobytes() == cnt.tobytes(), trial
        seen += n
    assert seen > 200
    for trial in range(10):
        V, s, d = random_multigraph(rng, 60)   # self loops and repeats included
        begin, idx = csr_of(V, s, d)[:2]
        both(V, begin, idx)
        for ordered in (True, False):   # the schedule's numbering is the one the k-clique model uses
            assert np.array_equal(plan_ids(V, _simple_pairs(V, begin, idx)[0], ordered), orientation(V, begin, idx, ordered)[0])


def test_closed_forms():
    for shape in (cycle(3), cycle(5), cycle(6), path(7), star(9), binary_tree(31)):
        m = both(*csr_of_shape(shape))
        assert m["squares"] == 0 and not m["count"].any()
    m = both(*csr_of_shape(cycle(4)))
    assert m["squares"] == 1 and m["count"].tolist() == [1, 1, 1, 1]
    assert clique_counts(4)[0].tolist() == [3, 3, 3, 3] and clique_counts(4)[1] == 3   # K4 holds three squares, on one vertex set
    for n in (4, 5, 12, 65):
        cnt, tot = clique_counts(n)
        m = both(*csr_of_shape(clique(n)))
        assert m["squares"] == tot == 3 * comb(n, 4) and m["count"].tobytes() == cnt.tobytes() and np.all(cnt == 3 * comb(n - 1, 3))
    for a, b in ((2, 2), (2, 9), (3, 30), (7, 7), (40, 40)):
        cnt, tot = bipartite_counts(a, b)
        m = both(*csr_of_shape(bipartite(a, b)))
        assert m["squares"] == tot == comb(a, 2) * comb(b, 2) and m["count"].tobytes() == cnt.tobytes()
        assert cnt[0] == (a - 1) * comb(b, 2) and cnt[-1] == (b - 1) * comb(a, 2)
    for d in range(1, 9):
        cnt, tot = hypercube_counts(d)
        m = both(*csr_of_shape(hypercube(d)))
        assert m["squares"] == tot == (2 ** (d - 2) * comb(d, 2) if d >= 2 else 0) and m["count"].tobytes() == cnt.tobytes()
    for rows, cols in ((2, 2), (5, 7), (33, 65)):
        cnt, tot = grid_counts(rows, cols)
        m = both(*csr_of_shape(grid(rows, cols)))
        assert m["squares"] == tot == (rows - 1) * (cols - 1) and m["count"].tobytes() == cnt.tobytes()
        assert cnt[0] == 1 and ((rows, cols) == (2, 2) or (sorted(set(cnt.tolist())) == [1, 2, 4] and cnt[1] == 2 and cnt[cols + 1] == 4))   # by position
    # no vertex, no edge, self loops only
    for V, begin, idx in ((0, [0], []), (3, [0, 0, 0, 0], []), (3, [0, 1, 2, 3], [0, 1, 2])):
        for m in (squares_definition(V, begin, idx), squares_schedule(V, begin, idx)):
            assert m["squares"] == 0 and len(m["count"]) == V and not m["count"].any()


def test_both_forms_agree_on_the_inputs_of_the_gpu_tests(golden):
    cases = [(256, golden["cases"][name]["begin"], golden["cases"][name]["node_idx"]) for name in sorted(golden["cases"])
             if len(golden["cases"][name]["begin"]) == 257]
    assert cases
    for V, hub_edges in ((64, 200), (3000, 8000)):
        cases.append((V,) + tuple(unsorted_multigraph(V, hub_edges, V)[:2]))
    total = 0
    for V, begin, idx in cases:
        total += both(V, begin, idx)["squares"]
    assert total > 1000


def test_the_schedule_of_a_two_hub_graph_and_its_classes():
    """K_{2,n} under the degree order: the leaves come first, the higher hub walks one wedge per leaf, all to the other hub."""
    n = 300
    V, begin, idx = csr_of_shape(bipartite(2, n))
    m = squares_schedule(V, begin, idx)
    assert m["squares"] == comb(n, 2) and m["D"].tolist() == [0] * n + [n, n] and m["W"].tolist() == [0] * n + [0, n] and m["wedges"] == n
    assert classes_of(m["D"], m["W"]) == {"wave": 1, "block": 1, "glob": 0, "split": 0, "skipped": n, "batches": 0}
    assert classes_of(m["D"], m["W"], wave_max=0, lds_slots=2 * n) == {"wave": 0, "block": 2, "glob": 0, "split": 0, "skipped": n, "batches": 0}
    assert classes_of(m["D"], m["W"], wave_max=0, lds_slots=2 * n - 2, split=n - 1) == {"wave": 0, "block": 1, "glob": 1, "split": 1, "skipped": n, "batches": 1}
    assert classes_of(m["D"], m["W"], wave_max=n) == classes_of(m["D"], m["W"], wave_max=128)   # clamped
    assert knobs_in_force(wave_max=1000, lds_slots=1, split=0, batch_bytes=0) == {"wave_max": 128, "lds_slots": 64, "split": 1, "batch_bytes": 1}
    # the identity order: the two hubs are the lowest ids, every leaf walks the wedges through both
    i = squares_schedule(V, begin, idx, False)
    assert i["D"].tolist() == [0, 0] + [2] * n and i["W"].tolist() == [0, 0] + [2 * k for k in range(n)] and i["count"].tobytes() == m["count"].tobytes()
    c = classes_of(i["D"], i["W"], wave_max=0, lds_slots=64, batch_bytes=1)
    assert c["glob"] == c["batches"] == int((i["W"] > 32).sum()) and c["block"] == n - c["glob"] and c["skipped"] == 2
    three = classes_of(i["D"], i["W"], wave_max=0, lds_slots=64, batch_bytes=3 * 4 * 320)   # every global vertex needs at most 320 counters
    assert 1 < three["batches"] <= -(-c["glob"] // 3)


def test_squares_is_a_row_of_the_table_of_interleaved_entries():
    import gmx
    import handle_sequences as hs
    assert "squares" in vars(gmx.Graph) and list(hs.ROWS).count("squares") == 1 and hs.ROWS["squares"].args == squares_sequences.ARGS
    assert [s.entry for s in hs.forward()].count("squares") == 1 and [s.entry for s in hs.shuffled()].count("squares") == 2
    for label, a in squares_sequences.ARGS:
        assert label == "D" or "_env" not in a   # (an identity-order call on S would make test_workspace's clustering rebuild S's plan)
    for k, (label, a) in enumerate(squares_sequences.ARGS):
        step = hs.Step("squares", k, label)
        hs.check_step(step, hs.fake_call(step))
    wrong = list(hs.fake_call(hs.Step("squares", 0, "S")))
    wrong[0] = wrong[0].copy()
    wrong[0][int(np.argmax(wrong[0]))] += 1
    with pytest.raises(AssertionError):
        hs.check_step(hs.Step("squares", 0, "S"), tuple(wrong))
    want = hs.want_of("squares", 0, "S")
    d = squares_definition(hs.inputs()["S"].V, hs.inputs()["S"].begin, hs.inputs()["S"].idx)   # V = 4096: the dense product's upper end
    assert d["squares"] == want[True]["squares"] == want[False]["squares"] > 0 and d["count"].tobytes() == want[True]["count"].tobytes() == want[False]["count"].tobytes()
    assert hs.want_of("squares", 1, "B")[True]["squares"] > 0   # butterflies: B has no triangle


def test_entry_is_declared_exported_bound_and_built(tmp_path):
    import gmx
    L = gmx.lib()
    assert "gmx_squares" in gmx.EXPORTS and hasattr(L, "gmx_squares") and hasattr(gmx.Graph, "squares")
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_squares(gmx_graph_t* g, int64_t* count_host, int64_t* squares, gmx_stats_t* stats);" in hdr
    assert "2 * count[v] < 2^63" in hdr
    assert os.path.exists(os.path.join(PKG, "bin", "squares")), "bin/squares not built"
    assert os.path.exists(os.path.join(PKG, "generated", "squares.h"))
    obj = tmp_path / "squares.o"
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), "-c", os.path.join(PKG, "generated", "squares.cc"), "-o", str(obj)])
    assert obj.exists()
    src = tmp_path / "use_squares.cc"
    src.write_text('#include "squares.h"\nint main() { gm_graph G; return squares(G, (int64_t*) 0) < 0; }\n')
    link = [os.path.join(PKG, "libgmgraph.a"), "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + os.path.join(PKG, "generated"), str(src), "-o", str(tmp_path / "use_squares")] + link)


def test_squares_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n = C.c_int64(7)
    cnt = np.full(4, 5, np.int64)
    bogus = C.c_void_p(8)   # never touched: every check comes before g is read
    assert L.gmx_squares(bogus, cnt.ctypes.data, None, None) == -1   # GMX_ERR_ARG
    assert L.gmx_squares(None, cnt.ctypes.data, C.byref(n), None) == -1
    assert L.gmx_squares(None, None, None, None) == -1
    assert n.value == 7 and np.all(cnt == 5)
    with pytest.raises(gmx.GmxError):
        gmx.Graph(None).squares()
