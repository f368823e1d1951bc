"""Weakly connected components, host side (no GPU): a numpy/scipy model of the device scheme (neighbour sampling, the
skipped tree, the live rows of the final pass) that the GPU tests compare the log line and the statistics with, the proof
by exhaustion that skipping a tree is sound, the C entry's argument checks, and the drop-in header.

The model follows gmx.h: sampling round r reads slot r of every out-row that has one; the trees of the sampled forest are
named by their smallest vertex; g* is the most frequent root among 1024 fixed probes (every vertex when V <= 1024), ties to
the smallest root; the live vertices are the ones outside g*'s tree; the final pass walks their whole out-rows and in-rows,
or -- without a reverse CSR or with GMX_WCC_SKIP=0 -- the out-rows of every vertex."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG, canonical, csr_of

PROBES = 1024


def _components(V, src, dst):
    """Weak components of an edge list: every vertex's component named by its smallest vertex."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    m = csr_matrix((np.ones(len(src), np.int8), (np.asarray(src, np.int64), np.asarray(dst, np.int64))), shape=(V, V))
    _, lab = connected_components(m, directed=True, connection="weak")
    smallest = np.full(lab.max() + 1 if V else 0, V, np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    return smallest[lab]


def scipy_wcc(V, begin, idx):
    """(count, canonical comp) of the weak components of a CSR from scipy."""
    if V == 0:
        return 0, np.zeros(0, np.int32)
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    idx = np.asarray(idx, np.int32)
    m = csr_matrix((np.ones(len(idx), np.int8), idx, np.asarray(begin, np.int64)), shape=(V, V))
    n, lab = connected_components(m, directed=True, connection="weak")
    return int(n), canonical(lab)


def probe_positions(V):
    if V <= PROBES:
        return np.arange(V)
    return ((np.arange(PROBES, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) % np.uint64(V)


def wcc_model(V, begin, idx, rb=None, K=2, giant=None):
    """The scheme on the host.  giant: None (the probes decide) or a vertex whose tree is skipped."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    outdeg = np.diff(begin)
    indeg = np.diff(np.asarray(rb, np.int64)) if rb is not None else np.bincount(idx, minlength=V)
    su, sw = [], []
    for r in range(K):
        v = np.flatnonzero(outdeg > r)
        su.append(v)
        sw.append(idx[begin[v] + r])
    su = np.concatenate(su) if su else np.zeros(0, np.int64)
    sw = np.concatenate(sw) if sw else np.zeros(0, np.int64)
    root = _components(V, su, sw)   # the sampled forest
    if giant is None:
        r, c = np.unique(root[probe_positions(V).astype(np.int64)], return_counts=True)
        gstar = int(r[np.argmax(c)])   # (argmax takes the first maximum: the smallest root)
    else:
        gstar = int(root[giant])
    live = root != gstar
    rows = np.repeat(np.arange(V), outdeg)
    n, comp = scipy_wcc(V, begin, idx)
    return {
        "sampled": (su, sw),
        "root": root,
        "gstar": gstar,
        "live": live,
        "edges_skip": len(su) + int(outdeg[live].sum() + indeg[live].sum()),
        "edges_noskip": len(su) + len(idx),
        # what the skipping final pass links: every edge with a live end
        "final": (rows[live[rows] | live[idx]], idx[live[rows] | live[idx]]),
        "count": n,
        "comp": comp,
    }


def late_attachment(V0, src, dst, extra):
    """`extra` new vertices V0 .. V0+extra-1, each with one in-edge from the vertex of most out-edges and no out-edge: they
    sort to the end of the hub's row, where no sampling round looks."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    hub = int(np.argmax(np.bincount(src, minlength=V0)))
    new = np.arange(V0, V0 + extra)
    return V0 + extra, np.concatenate([src, np.full(extra, hub)]), np.concatenate([dst, new]), hub


def _sorted_csr(V, src, dst):
    o = np.lexsort((dst, src))
    return csr_of(V, np.asarray(src)[o], np.asarray(dst)[o])


def _assert_skip_sound(V, begin, idx, rb, tag):
    for K in (0, 1, 2, 4):
        base = wcc_model(V, begin, idx, rb, K)
        rows = np.repeat(np.arange(V), np.diff(begin))
        trees = np.unique(base["root"])
        for t in trees:   # every tree of the sampled forest as the skipped one
            live = base["root"] != t
            keep = live[rows] | live[idx]   # the slots of the live vertices' out-rows and in-rows
            u = np.concatenate([base["sampled"][0], rows[keep]])
            w = np.concatenate([base["sampled"][1], np.asarray(idx)[keep]])
            assert np.array_equal(canonical(_components(V, u, w)), base["comp"]), (tag, K, int(t))
        m = wcc_model(V, begin, idx, rb, K, giant=int(trees[-1]))   # the model's own form of the same choice
        assert m["gstar"] == trees[-1] and np.array_equal(m["live"], base["root"] != trees[-1])
        assert np.array_equal(m["final"][0], rows[m["live"][rows] | m["live"][idx]])


def test_skipping_a_tree_is_sound():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(5)
    for trial in range(300):
        V = int(rng.integers(1, 61))
        E = int(rng.integers(0, 3 * V + 1))
        src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
        begin, idx, rb, _ = _sorted_csr(V, src, dst) if trial % 2 else csr_of(V, src, dst)
        _assert_skip_sound(V, begin, idx, rb, trial)
    V0 = 40
    V, src, dst, hub = late_attachment(V0, rng.integers(0, V0, 400), rng.integers(0, V0, 400), 20)
    begin, idx, rb, _ = _sorted_csr(V, src, dst)
    assert begin[hub + 1] - begin[hub] > 4 + 20 and np.all(idx[begin[hub + 1] - 20:begin[hub + 1]] >= V0)
    m = wcc_model(V, begin, idx, rb, 4)
    assert np.all(m["live"][V0:]) and np.all(m["comp"][V0:] == m["comp"][hub])   # never sampled, yet in the hub's component
    _assert_skip_sound(V, begin, idx, rb, "late")


def test_model_probes_and_counts():
    pytest.importorskip("scipy")
    # two out-stars and an isolated vertex: K = 1 samples one leaf per hub only
    src = [0] * 5 + [6] * 3
    dst = [1, 2, 3, 4, 5, 7, 8, 9]
    begin, idx, rb, _ = csr_of(11, src, dst)
    m = wcc_model(11, begin, idx, rb, 1)
    assert len(m["sampled"][0]) == 2 and m["gstar"] == 0   # every tree is probed once or twice: {0,1} wins, ties to the smallest
    assert m["live"].tolist() == [False, False] + [True] * 9
    assert m["edges_noskip"] == 2 + 8
    assert m["edges_skip"] == 2 + 3 + 7   # the out-row of 6, the in-rows of 2..5 and 7..9
    assert m["count"] == 3 and m["comp"].tolist() == [0] * 6 + [1] * 4 + [2]
    p = probe_positions(5000)
    assert len(p) == PROBES and p[0] == 0 and p[1] == 0x9E3779B1 % 5000 and p[3] == ((3 * 0x9E3779B1) % (1 << 32)) % 5000


def test_wcc_null_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n = C.c_int64(0)
    comp = np.zeros(4, np.int32)
    assert L.gmx_wcc(None, comp.ctypes.data, C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_wcc(None, None, None, None) == -1
    assert L.gmx_wcc(C.c_void_p(8), None, C.byref(n), None) == -1   # comp_host is checked before g is touched
    assert "gmx_wcc" in gmx.EXPORTS and hasattr(L, "gmx_wcc") and hasattr(gmx.Graph, "wcc")


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_wcc.cc"
    src.write_text('#include "wcc.h"\nint main() { gm_graph G; return wcc(G, (node_t*) 0) < 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_wcc")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "wcc.cc"))
