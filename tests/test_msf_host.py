"""Minimum spanning forests, host side (no GPU): Kruskal's algorithm in (weight, slot) order, a vectorised numpy model of
the device's schedule (gmx.h at gmx_msf) that the GPU tests compare bytes and statistics with, the checks of one against the
other, the C entry's argument checks and the drop-in header.

The model: round 0 lists every vertex that has an out-slot; a round reads every slot of every listed row; a slot is cross
when its ends lie in different trees at the round's start; every tree takes the smallest key (weight, uploaded slot) among
the cross slots that touch it; the chosen slots are selected and their trees merged; the next round lists the vertices that
had a cross out-slot; the run ends when the list is empty or a round finds no cross slot."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG, canonical
from test_wcc_host import scipy_wcc

pytest.importorskip("scipy")
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def kruskal(V, src, dst, w):
    """in_forest[E] of Kruskal's algorithm over the slots in (weight, slot) order; self loops never join anything."""
    src, dst, w = (np.asarray(x).tolist() for x in (src, dst, w))
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    sel = np.zeros(len(src), bool)
    for e in sorted(range(len(src)), key=lambda i: (w[i], i)):
        a, b = find(src[e]), find(dst[e])
        if a != b:
            parent[a] = b
            sel[e] = True
    return sel


def keys_of(w, slot):
    """(weight biased to unsigned) << 32 | slot."""
    return ((np.asarray(w, np.int64) + (1 << 31)).astype(np.uint64) << np.uint64(32)) | np.asarray(slot, np.uint64)


def msf_model(V, src, dst, w=None, slot=None):
    """The schedule on the host.  src / dst: the ends of every stored slot in the device's slot order, slot: the uploaded
    slot of each (None: the same), w: weights by UPLOADED slot (None: all 0).  Returns a dict: in_forest (bool, by uploaded
    slot), rounds (those that merged), slots (read over all rounds), comp (canonical), total, per_round (slots read by each
    round) and unlisted_cross (cross slots whose tail was not listed: the listing rule says 0)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = len(src)
    slot = np.arange(E, dtype=np.int64) if slot is None else np.asarray(slot, np.int64)
    w = np.zeros(E, np.int64) if w is None else np.asarray(w, np.int64)
    key = keys_of(w[slot], slot)
    dev_of = np.empty(E, np.int64)
    dev_of[slot] = np.arange(E)
    tree = np.arange(V)
    listed = np.zeros(V, bool)
    listed[src] = True
    in_forest = np.zeros(E, bool)
    rounds = slots = unlisted_cross = 0
    per_round = []
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    while listed.any():
        read = listed[src]
        per_round.append(int(read.sum()))
        slots += per_round[-1]
        cross_anywhere = tree[src] != tree[dst]
        unlisted_cross += int((cross_anywhere & ~read).sum())
        e = np.flatnonzero(read & cross_anywhere)
        if len(e) == 0:
            break
        best = np.full(V, NONE, np.uint64)
        np.minimum.at(best, tree[src[e]], key[e])
        np.minimum.at(best, tree[dst[e]], key[e])
        chosen = np.unique(best[best != NONE] & np.uint64(0xFFFFFFFF)).astype(np.int64)   # uploaded slots
        in_forest[chosen] = True
        ce = dev_of[chosen]
        m = csr_matrix((np.ones(len(ce), np.int8), (tree[src[ce]], tree[dst[ce]])), shape=(V, V))
        tree = connected_components(m, directed=True, connection="weak")[1][tree]
        listed = np.zeros(V, bool)
        listed[src[e]] = True
        rounds += 1
    return {"in_forest": in_forest, "rounds": rounds, "slots": slots, "comp": canonical(tree), "total": int(w[in_forest].sum()),
            "count": int(in_forest.sum()), "per_round": per_round, "unlisted_cross": unlisted_cross}


def ruler(n):
    """1, 2, 1, 3, 1, 2, 1, 4, ...: the number of trailing zero bits of 1 .. n, plus one."""
    i = np.arange(1, n + 1)
    return (np.log2(i & -i) + 1).astype(np.int32)


def ceil_log2(V):
    return int(np.ceil(np.log2(V))) if V > 1 else 0


def random_multigraph(rng):
    """Heavy ties, negative weights, self loops and repeats; rows in slot order (sorted by tail, stable)."""
    V = int(rng.integers(1, 40))
    E = int(rng.integers(0, 4 * V + 1))
    src, dst = np.sort(rng.integers(0, V, E)), rng.integers(0, V, E)
    if E > 2:
        dst[E // 2] = src[E // 2]                       # a self loop
        src[1], dst[1] = src[0], dst[0]                 # a repeat
    w = rng.integers(-3, 4, E)
    return V, src, dst, w


def begin_of(V, src):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(src, np.int64), minlength=V))])


def test_model_equals_kruskal_on_random_multigraphs():
    rng = np.random.default_rng(2026)
    for _ in range(300):
        V, src, dst, w = random_multigraph(rng)
        m = msf_model(V, src, dst, w)
        assert np.array_equal(m["in_forest"], kruskal(V, src, dst, w)), (V, src, dst, w)
        assert m["unlisted_cross"] == 0                       # a cross slot never has an unlisted tail
        assert m["rounds"] <= ceil_log2(V)
        n, comp = scipy_wcc(V, begin_of(V, src), dst)
        assert np.array_equal(m["comp"], comp) and m["count"] == V - n
        assert not m["in_forest"][src == dst].any()
        assert m["slots"] == sum(m["per_round"]) and len(m["per_round"]) in (m["rounds"], m["rounds"] + 1)


def test_model_with_permuted_slots_ties_to_the_uploaded_slot():
    rng = np.random.default_rng(7)
    for _ in range(100):
        V, src, dst, w = random_multigraph(rng)               # as uploaded
        order = np.lexsort((dst, src))                        # the device sorts every row: device slot -> uploaded slot
        m = msf_model(V, src[order], dst[order], w, slot=order)
        assert np.array_equal(m["in_forest"], kruskal(V, src, dst, w))
        plain = msf_model(V, src, dst, w)
        assert m["rounds"] == plain["rounds"] and m["slots"] == plain["slots"]


def test_total_equals_scipy_minimum_spanning_tree():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    rng = np.random.default_rng(5)
    for _ in range(100):
        V, src, dst, _ = random_multigraph(rng)
        w = rng.integers(1, 6, len(src))                      # >= 1: scipy reads 0 as "no edge"
        lo, hi = np.minimum(src, dst), np.maximum(src, dst)
        pair = {}
        for a, b, x in zip(lo.tolist(), hi.tolist(), w.tolist()):
            if a != b:
                pair[(a, b)] = min(x, pair.get((a, b), x))    # the minimum over repeated pairs, both directions
        a = np.array([k[0] for k in pair], np.int64)
        b = np.array([k[1] for k in pair], np.int64)
        want = int(minimum_spanning_tree(csr_matrix((np.array(list(pair.values()), np.int64), (a, b)), shape=(V, V))).sum())
        assert msf_model(V, src, dst, w)["total"] == want == int(w[kruskal(V, src, dst, w)].sum())


def test_paths_ascending_and_ruler():
    P = 1 << 10
    s, d = np.arange(P - 1), np.arange(1, P)
    m = msf_model(P, s, d, np.arange(P - 1))                  # every vertex but the last picks the edge to its left ... one chain
    assert m["rounds"] == 1 and m["in_forest"].all() and m["slots"] == 2 * (P - 1)
    m = msf_model(P, s, d, ruler(P - 1))
    assert m["rounds"] == 10 and m["in_forest"].all()
    assert np.array_equal(m["in_forest"], kruskal(P, s, d, ruler(P - 1)))


def test_extreme_weights_and_the_lower_slot():
    lo, hi = -(1 << 31), (1 << 31) - 1
    V, src, dst = 4, [0, 0, 1, 1, 2, 3], [1, 1, 2, 2, 3, 0]
    w = [hi, -1, 0, lo, hi, hi]
    m = msf_model(V, src, dst, w)
    assert m["in_forest"].tolist() == kruskal(V, src, dst, w).tolist() == [False, True, False, True, True, False]
    assert m["total"] == lo - 1 + hi
    both = msf_model(2, [0, 1], [1, 0], [5, 5])
    assert both["in_forest"].tolist() == [True, False]
    tri = msf_model(3, [0, 1, 2], [1, 2, 0], [1, 1, 1])       # the classic tie cycle: slot order breaks it
    assert tri["in_forest"].tolist() == [True, True, False] and tri["rounds"] == 1


def test_msf_is_declared_exported_and_bound():
    import gmx
    L = gmx.lib()
    with open(os.path.join(ROOT, "include", "gmx.h")) as f:
        header = f.read()
    assert "int gmx_msf(gmx_graph_t* g, const int32_t* weight_host, uint8_t* in_forest_host" in header
    assert "gmx_msf" in gmx.EXPORTS and hasattr(L, "gmx_msf") and hasattr(gmx.Graph, "msf")


def test_msf_null_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n, t, c = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    sel = np.zeros(4, np.uint8)
    assert L.gmx_msf(None, None, sel.ctypes.data, C.byref(n), C.byref(t), None, C.byref(c), None) == -1   # GMX_ERR_ARG
    assert L.gmx_msf(None, None, None, None, None, None, None, None) == -1
    assert b"NULL" in L.gmx_last_error()


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_msf.cc"
    src.write_text('#include "msf.h"\nint main() { gm_graph G; return msf(G, (int32_t*) 0, (bool*) 0) < 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_msf")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "msf.cc"))
