"""Strongly connected components, host side (no GPU): the kosaraju drop-in builds against the reference's driver, the
restated checker the GPU tests compare with, and the C entry's argument checks.

The checker restates apps/src/kosaraju.gm: phase 1 is an iterative DFS over G (the out-rows in slot order, as
gm_dfs_template.h walks them) that pushes every vertex to the front of a sequence at its post-visit; phase 2 walks that
sequence and starts, from each vertex still without a component, a BFS over G^ restricted to `mem == -1` that gives every
vertex it reaches the next component id.  The device numbers the components canonically (ids in increasing order of each
component's smallest vertex), so both sides are compared after canonicalisation."""
import ctypes as C
import os
import subprocess
from collections import deque

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "green-marl_amd")
REF_APPS = "/root/reference/apps/output_cpp/src"
CXX_FLAGS = ["-O2", "-fopenmp", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "gm_graph", "inc"),
             "-I" + os.path.join(PKG, "generated")]
LINK = [os.path.join(PKG, "libgmgraph.a"), "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib",
        "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]


def kosaraju_check(V, begin, node_idx, r_begin, r_node_idx):
    """kosaraju.gm restated: returns (count, mem) with the reference's own (DFS finish order) ids."""
    begin, node_idx = np.asarray(begin).tolist(), np.asarray(node_idx).tolist()
    r_begin, r_node_idx = np.asarray(r_begin).tolist(), np.asarray(r_node_idx).tolist()
    checked = [False] * V
    seq = []   # post-order; Seq.PushFront makes the walk of phase 2 its reverse
    for t in range(V):
        if checked[t]:
            continue
        checked[t] = True
        stack = [(t, begin[t])]
        while stack:
            v, j = stack[-1]
            if j < begin[v + 1]:
                stack[-1] = (v, j + 1)
                w = node_idx[j]
                if not checked[w]:
                    checked[w] = True
                    stack.append((w, begin[w]))
            else:
                stack.pop()
                seq.append(v)
    mem = [-1] * V
    comp = 0
    for t in reversed(seq):
        if mem[t] != -1:
            continue
        mem[t] = comp
        q = deque([t])
        while q:
            v = q.popleft()
            for j in range(r_begin[v], r_begin[v + 1]):
                w = r_node_idx[j]
                if mem[w] == -1:
                    mem[w] = comp
                    q.append(w)
        comp += 1
    return comp, np.array(mem, np.int64)


def canonical(mem):
    """Component ids renumbered 0 .. count-1 in increasing order of each component's smallest vertex."""
    mem = np.asarray(mem)
    if len(mem) == 0:
        return mem.astype(np.int32)
    _, first, inv = np.unique(mem, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv].astype(np.int32)


def csr_of(V, src, dst):
    """Forward and reverse CSR of an edge list, rows in input order (stable)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    o = np.argsort(src, kind="stable")
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    begin = np.cumsum(begin)
    r = np.argsort(dst, kind="stable")
    r_begin = np.zeros(V + 1, np.int64)
    np.add.at(r_begin, dst + 1, 1)
    r_begin = np.cumsum(r_begin)
    return begin, dst[o], r_begin, src[r]


def scipy_scc(V, begin, node_idx):
    """(count, canonical comp) from scipy, or None when scipy is not importable."""
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    begin = np.asarray(begin, np.int64)
    node_idx = np.asarray(node_idx, np.int32)
    m = csr_matrix((np.ones(len(node_idx), np.int8), node_idx, begin), shape=(V, V))
    n, lab = connected_components(m, directed=True, connection="strong")
    return n, canonical(lab)


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present")
def test_reference_kosaraju_driver_compiles_unchanged(tmp_path):
    """The reference's kosaraju_main.cc and common_main.h, untouched, build and link against this tree (kosaraju.h)."""
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "kosaraju")
    subprocess.check_call(["g++"] + CXX_FLAGS + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "kosaraju_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)   # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout


def test_checker_on_the_reference_drivers_small_graph():
    """TEST_LARGE 0 branch of kosaraju_main.cc: 5 components, {0,1,2,3,4,9} being one."""
    src = [0, 1, 2, 3, 5, 7, 9, 1, 2, 4]
    dst = [1, 2, 3, 0, 8, 4, 1, 4, 5, 9]
    n, mem = kosaraju_check(10, *csr_of(10, src, dst))
    assert n == 5
    assert canonical(mem).tolist() == [0, 0, 0, 0, 0, 1, 2, 3, 4, 0]


def test_checker_agrees_with_scipy_on_random_digraphs():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(7)
    for trial in range(300):
        V = int(rng.integers(1, 40))
        E = int(rng.integers(0, 3 * V + 1))
        src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
        begin, idx, rb, ri = csr_of(V, src, dst)
        n, mem = kosaraju_check(V, begin, idx, rb, ri)
        sn, slab = scipy_scc(V, begin, idx)
        assert n == sn, trial
        assert np.array_equal(canonical(mem), slab), trial


def test_scc_null_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    n = C.c_int64(0)
    comp = np.zeros(4, np.int32)
    assert L.gmx_scc(None, comp.ctypes.data, C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_scc(None, None, None, None) == -1
    assert "gmx_scc" in gmx.EXPORTS and hasattr(L, "gmx_scc")
