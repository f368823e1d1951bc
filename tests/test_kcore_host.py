"""k-core decomposition, host side (no GPU): a numpy model of the schedule in gmx.h that the GPU tests compare core, layer
and the log line with; the model against networkx, against a certificate and against the definition by brute force; the C
entry's argument checks; the drop-in header.

The model follows gmx.h round by round.  Every stored slot u -> w with u != w counts once.  mode "in": a vertex's degree
is its in-slots and removing v lowers the heads of v's out-row; "out": the out-slots, and the tails of v's in-row; "both":
the sum, and both rows.  Level k is the smallest degree of a live vertex; round 0 of a level removes every live vertex of
degree <= k, round r+1 those whose degree fell to <= k because of round r's removals; the rounds that removed something
are numbered across the run and layer[v] is the round that removed v.  The live list is compacted by every level's scan
alone, so at a level's start it holds the vertices that were live after round 0 of the level before: `scanned` sums its
lengths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG, csr_of

MODES = ("in", "out", "both")


def kcore_model(V, begin, idx, mode="in"):
    """dict(core, layer, levels, rounds, scanned, max_core, top, slots) of the forward CSR (begin, idx)."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V), np.diff(begin))
    keep = rows != idx
    u, w = rows[keep], idx[keep]
    # lowered[kb[v] : kb[v + 1]]: the vertices that lose a counted slot when v is removed
    if mode == "in":
        key, tgt = u, w
    elif mode == "out":
        key, tgt = w, u
    else:
        key, tgt = np.concatenate([u, w]), np.concatenate([w, u])
    deg = np.bincount(tgt, minlength=V).astype(np.int64)
    o = np.argsort(key, kind="stable")
    lowered = tgt[o]
    kb = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=V))])
    core = np.zeros(V, np.int32)
    layer = np.zeros(V, np.int32)
    live = np.ones(V, bool)
    lst = np.arange(V)
    levels = rounds = scanned = 0
    k, top = 0, 0
    while len(lst):
        alive = lst[live[lst]]
        if not len(alive):
            break
        levels += 1
        scanned += len(lst)
        k = int(deg[alive].min())
        q = alive[deg[alive] <= k]
        lst = alive[deg[alive] > k]
        top = 0
        while len(q):
            core[q] = k
            layer[q] = rounds
            live[q] = False
            rounds += 1
            top += len(q)
            lens = kb[q + 1] - kb[q]
            total = int(lens.sum())
            pos = np.repeat(kb[q] - (np.cumsum(lens) - lens), lens) + np.arange(total)
            t = lowered[pos]
            t, dec = np.unique(t[live[t]], return_counts=True)
            deg[t] -= dec
            q = t[deg[t] <= k]
    return {"core": core, "layer": layer, "levels": levels, "rounds": rounds, "scanned": scanned, "max_core": k if V else 0, "top": top,
            "slots": len(idx) * (2 if mode == "both" else 1)}


def transpose(V, begin, idx):
    rows = np.repeat(np.arange(V), np.diff(np.asarray(begin, np.int64)))
    b, i, _, _ = csr_of(V, np.asarray(idx, np.int64), rows)
    return b, i


def _random_simple_undirected(rng):
    V = int(rng.integers(1, 61))
    p = rng.choice([0.03, 0.1, 0.3, 0.6])
    a = np.triu(rng.random((V, V)) < p, 1)
    s, d = np.nonzero(a)
    return V, s, d


def test_model_against_networkx_core_number_and_onion_layers():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(7)
    for trial in range(300):
        V, s, d = _random_simple_undirected(rng)
        G = nx.Graph()
        G.add_nodes_from(range(V))
        G.add_edges_from(zip(s.tolist(), d.tolist()))
        cn, ol = nx.core_number(G), nx.onion_layers(G)
        want_core = np.array([cn[v] for v in range(V)], np.int32)
        want_layer = np.array([ol[v] - 1 for v in range(V)], np.int32)
        sym = csr_of(V, np.concatenate([s, d]), np.concatenate([d, s]))
        one = csr_of(V, s, d)
        for mode, (begin, idx) in (("in", sym[:2]), ("out", sym[:2]), ("both", one[:2])):
            m = kcore_model(V, begin, idx, mode)
            assert np.array_equal(m["core"], want_core), (trial, mode)
            assert np.array_equal(m["layer"], want_layer), (trial, mode)
            assert m["max_core"] == want_core.max() and m["top"] == int((want_core == want_core.max()).sum())
            assert m["rounds"] == want_layer.max() + 1


def _counts(V, begin, idx, mode):
    """cnt[v, w]: the counted slots of v whose other end is w."""
    rows = np.repeat(np.arange(V), np.diff(np.asarray(begin, np.int64)))
    idx = np.asarray(idx, np.int64)
    keep = rows != idx
    u, w = rows[keep], idx[keep]
    cnt = np.zeros((V, V), np.int64)
    if mode in ("in", "both"):
        np.add.at(cnt, (w, u), 1)
    if mode in ("out", "both"):
        np.add.at(cnt, (u, w), 1)
    return cnt


def _random_multigraph(rng, vmax):
    V = int(rng.integers(1, vmax + 1))
    E = int(rng.integers(0, 4 * V + 1))
    return V, rng.integers(0, V, E), rng.integers(0, V, E)   # repeats and self loops included


def test_certificate_on_directed_multigraphs_with_self_loops():
    rng = np.random.default_rng(8)
    for trial in range(200):
        V, s, d = _random_multigraph(rng, 60)
        begin, idx, _, _ = csr_of(V, s, d)
        for mode in MODES:
            m = kcore_model(V, begin, idx, mode)
            cnt, core = _counts(V, begin, idx, mode), m["core"].astype(np.int64)
            # every v has at least core[v] counted slots to vertices of core >= core[v] ...
            into = (cnt * (core[None, :] >= core[:, None])).sum(axis=1)
            assert np.all(into >= core), (trial, mode)
            # ... and no more than core[v] to the vertices that were live when its round began: the peeling order is the
            # witness that no larger k holds (and core never falls along it)
            assert np.all(np.diff(core[np.argsort(m["layer"], kind="stable")]) >= 0)
            at_removal = (cnt * (m["layer"][None, :] >= m["layer"][:, None])).sum(axis=1)
            assert np.all(at_removal <= core), (trial, mode)
            assert m["slots"] == len(idx) * (2 if mode == "both" else 1)


def test_definition_by_brute_force():
    rng = np.random.default_rng(9)
    for trial in range(60):
        V, s, d = _random_multigraph(rng, 12)
        begin, idx, _, _ = csr_of(V, s, d)
        member = ((np.arange(1 << V)[:, None] >> np.arange(V)[None, :]) & 1).astype(np.int64)   # every subset S
        for mode in MODES:
            cnt = _counts(V, begin, idx, mode)
            inside = member @ cnt.T                                   # [S, v]: the slots of v with the other end in S
            low = np.where(member == 1, inside, np.iinfo(np.int64).max).min(axis=1)   # the smallest degree within S
            low[0] = 0
            want = (member * low[:, None]).max(axis=0)
            assert np.array_equal(kcore_model(V, begin, idx, mode)["core"], want), (trial, mode)


def test_out_is_in_on_the_transpose_and_both_is_twice_in_on_a_symmetric_graph():
    rng = np.random.default_rng(10)
    for trial in range(100):
        V, s, d = _random_multigraph(rng, 60)
        begin, idx, _, _ = csr_of(V, s, d)
        tb, ti = transpose(V, begin, idx)
        a, b = kcore_model(V, begin, idx, "out"), kcore_model(V, tb, ti, "in")
        for f in ("core", "layer"):
            assert np.array_equal(a[f], b[f]), (trial, f)
        assert (a["levels"], a["rounds"], a["scanned"]) == (b["levels"], b["rounds"], b["scanned"])
        sb, si, _, _ = csr_of(V, np.concatenate([s, d]), np.concatenate([d, s]))
        i, o, both = (kcore_model(V, sb, si, m) for m in MODES)
        assert np.array_equal(i["core"], o["core"]) and np.array_equal(both["core"], 2 * i["core"])
        assert np.array_equal(i["layer"], o["layer"]) and np.array_equal(both["layer"], i["layer"])
        assert both["slots"] == 2 * i["slots"] and both["scanned"] == i["scanned"]


def test_model_on_small_shapes():
    # a triangle with a pendant path 3 - 4 - 5, symmetric: the path peels in three rounds of level 1, the triangle at level 2
    s = [0, 1, 2, 2, 3, 4]
    d = [1, 2, 0, 3, 4, 5]
    begin, idx, _, _ = csr_of(6, s + d, d + s)
    m = kcore_model(6, begin, idx, "in")
    assert m["core"].tolist() == [2, 2, 2, 1, 1, 1] and m["layer"].tolist() == [3, 3, 3, 2, 1, 0]
    assert (m["levels"], m["rounds"], m["scanned"], m["max_core"], m["top"]) == (2, 4, 6 + 5, 2, 3)
    # self loops only, and no vertex at all
    m = kcore_model(3, [0, 1, 2, 3], [0, 1, 2], "both")
    assert m["core"].tolist() == [0, 0, 0] and m["layer"].tolist() == [0, 0, 0] and (m["levels"], m["rounds"], m["scanned"]) == (1, 1, 3)
    m = kcore_model(0, [0], [], "in")
    assert (m["levels"], m["rounds"], m["scanned"], m["max_core"]) == (0, 0, 0, 0)
    # a directed path in mode in: the degrees fall one behind the other, a round each
    m = kcore_model(4, [0, 1, 2, 3, 3], [1, 2, 3], "in")
    assert m["core"].tolist() == [0, 0, 0, 0] and m["layer"].tolist() == [0, 1, 2, 3] and m["levels"] == 1


def test_kcore_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    k = C.c_int32(7)
    core = np.zeros(4, np.int32)
    assert L.gmx_kcore(None, 0, core.ctypes.data, None, C.byref(k), None) == -1   # GMX_ERR_ARG
    assert L.gmx_kcore(None, 0, None, None, None, None) == -1
    assert L.gmx_kcore(C.c_void_p(8), 0, None, None, C.byref(k), None) == -1   # core_host is checked before g is touched
    assert L.gmx_kcore(None, 3, core.ctypes.data, None, None, None) == -1
    assert "gmx_kcore" in gmx.EXPORTS and hasattr(L, "gmx_kcore") and hasattr(gmx.Graph, "kcore")
    assert gmx.Graph.KCORE_MODES == {"in": 0, "out": 1, "both": 2}
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    for name, value in (("GMX_KCORE_IN", 0), ("GMX_KCORE_OUT", 1), ("GMX_KCORE_BOTH", 2)):
        assert "#define %-14s %d" % (name, value) in hdr


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_kcore.cc"
    src.write_text('#include "kcore.h"\nint main() { gm_graph G; return kcore(G, (int32_t*) 0) < 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_kcore")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "kcore.cc"))
