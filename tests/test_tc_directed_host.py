"""triangle_counting_directed.gm's result contract restated on the host (no GPU).

    Foreach(v) Foreach(u: v.Nbrs) Foreach(w: v.Nbrs)(w > u)
        If (w.HasEdgeFrom(u) || w.HasEdgeTo(u)) T++;

    T = sum over v of #{ ordered slot pairs (i, j) of row v : node_idx[i] < node_idx[j], adj(node_idx[i], node_idx[j]) },
    adj(u, w) = (u -> w in E or w -> u in E)

tcd_literal is the triple loop with Python sets for HasEdgeTo / HasEdgeFrom (set membership: the reference binary-searches a
semi-sorted row and its prologue semi-sorts); tcd_ref is the sparse-product restatement the device tests
(test_gpu_tc_directed.py) count against.  The two agree wherever the loop is affordable, T does not depend on the vertex
numbering, T = 3 x triangle_counting on a symmetric simple graph, and the totals of the named graphs are pinned.  The
reference ships no generated triangle_counting_directed.cc and no driver for it, so there is no reference-compiled fixture.
Also: the entry is declared, exported, bound and built."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT
from test_communities_host import csr, named_graph
from test_upload_forms_host import rows_of, unsorted_multigraph

PKG = os.path.join(ROOT, "green-marl_amd")


def tcd_literal(begin, node_idx):
    """The .gm as written."""
    begin = [int(x) for x in begin]
    idx = [int(x) for x in node_idx]
    V = len(begin) - 1
    out = [set(idx[begin[v]:begin[v + 1]]) for v in range(V)]          # w in out[u]: u.HasEdgeTo(w) = w.HasEdgeFrom(u)
    T = 0
    for v in range(V):
        row = idx[begin[v]:begin[v + 1]]
        for u in row:
            ou = out[u]
            for w in row:
                if w > u and (w in ou or u in out[w]):
                    T += 1
    return T


def tcd_ref(begin, node_idx):
    """T by formula: with c_v(x) = multiplicity of x in row v, T = sum over the unordered pairs {u, w}, u != w, joined by an
    edge in either direction, of sum over v of c_v(u) c_v(w).  Exact, any row order."""
    from scipy.sparse import csr_matrix
    V = len(begin) - 1
    rows = rows_of(begin).astype(np.int64)
    idx = np.asarray(node_idx, np.int64)
    if len(idx) == 0:
        return 0
    Ct = csr_matrix((np.ones(len(idx), np.int64), (idx, rows)), shape=(V, V))   # Ct[x, v] = c_v(x)
    Ct.sum_duplicates()
    lo, hi = np.minimum(rows, idx), np.maximum(rows, idx)
    key = np.unique(lo[lo != hi] * V + hi[lo != hi])
    u, w = key // V, key % V
    T = 0
    for a in range(0, len(u), 1 << 16):
        T += int(Ct[u[a:a + (1 << 16)]].multiply(Ct[w[a:a + (1 << 16)]]).sum())
    return T


MULTI = {"multi300": (300, 2000, 3), "multi2000": (2000, 3000, 1)}
_G, _REF = {}, {}


def tcd_graph(name):
    """(begin, node_idx) of a named graph of test_communities_host, or of one of the two unsorted multigraphs."""
    if name in MULTI:
        if name not in _G:
            b, i, _, _ = unsorted_multigraph(*MULTI[name])
            _G[name] = (np.ascontiguousarray(b, np.int32), np.ascontiguousarray(i, np.int32))
        return _G[name]
    return named_graph(name)


def tcd_ref_of(name, begin=None, node_idx=None):
    """tcd_ref, computed once per named graph and shared between the tests."""
    if name not in _REF:
        if begin is None:
            begin, node_idx = tcd_graph(name)
        _REF[name] = tcd_ref(begin, node_idx)
    return _REF[name]


# ------------------------------------------------------------------ the definition on tiny graphs

def both(V, s, d):
    b, i = csr(V, s, d)
    T = tcd_literal(b, i)
    assert tcd_ref(b, i) == T
    return T


def test_tiny_cases():
    # row 0 = {1, 1, 2, 0}: pairs (0,1) x2 and (0,2) count through the self loop's own edges 0 -> 1, 0 -> 2; (1,2) x2
    # through 1 -> 2: duplicates count multiply, the self loop takes part literally
    assert both(3, [0, 0, 0, 0, 1], [1, 1, 2, 0, 2]) == 5
    assert both(3, [0, 1, 2], [1, 2, 0]) == 0          # directed 3-cycle: no vertex has two out-neighbours
    assert both(3, [0, 0], [1, 2]) == 0                # an open wedge
    assert both(3, [0, 0, 2], [1, 2, 1]) == 1          # the closing edge runs "backwards" (w -> u)
    assert both(3, [0, 0, 1], [1, 2, 2]) == 1          # ... or forwards
    assert both(3, [0, 0, 1, 2], [1, 2, 2, 1]) == 1    # the adjacency test is boolean: both directions count once
    assert both(2, [0, 0], [0, 0]) == 0                # a pair needs two distinct values
    assert both(1, [], []) == 0


@pytest.mark.parametrize("name", ["star33", "chain4096", "path4096", "planted16", "multi300", "multi2000"])
def test_formula_is_the_literal_loop(name):
    b, i = tcd_graph(name)
    assert tcd_ref_of(name) == tcd_literal(b, i)


def test_rows_may_be_in_any_order():
    b, i = tcd_graph("multi300")
    o = np.lexsort((i, rows_of(b)))
    assert np.any(np.asarray(i)[o] != i)
    assert tcd_ref(b, np.asarray(i)[o]) == tcd_ref_of("multi300")


def test_count_does_not_depend_on_the_numbering():
    b, i = named_graph("rmat12")
    V = len(b) - 1
    perm = np.random.default_rng(12).permutation(V)
    pb, pi = csr(V, perm[rows_of(b)], perm[np.asarray(i, np.int64)])
    assert tcd_ref(pb, pi) == tcd_ref_of("rmat12") == 3093471


@pytest.mark.parametrize("name", ["rmat10s", "rmat12s"])
def test_three_times_the_undirected_count_on_a_symmetric_simple_graph(name):
    og = po.symmetrize(po.rmat_graph(int(name[4:6])))
    assert np.array_equal(og.begin, named_graph(name)[0])
    assert tcd_ref_of(name) == 3 * po.triangle_counting(og)


PINNED = {"star33": 0, "chain4096": 0, "path4096": 0, "uniform": 85, "planted16": 265404, "rmat10": 635428, "rmat10p": 635428,
          "rmat10s": 232512, "rmat12": 3093471, "rmat12p": 3093471, "rmat12s": 1441512, "rmat14": 15308531, "multi300": 47650,
          "multi2000": 19620}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_totals(name):
    T = tcd_ref_of(name)
    print("triangle_counting_directed %s: %d" % (name, T))
    assert T == PINNED[name]


# ------------------------------------------------------------------ plumbing

def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    for sym in ("gmx_triangle_counting_directed", "gmx_triangle_counting_directed_part"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in gmx.EXPORTS
        assert hasattr(gmx.lib(), sym)
    assert hasattr(gmx.Graph, "triangle_counting_directed")
    gen = open(os.path.join(PKG, "generated", "triangle_counting_directed.h")).read()
    assert "GM_GENERATED_CPP_TRIANGLE_COUNTING_DIRECTED_H" in gen
    assert re.search(r"\bint64_t\s+triangle_counting_directed\s*\(\s*gm_graph&\s*G\s*\)", gen)
    exe = os.path.join(PKG, "bin", "triangle_counting_directed")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout
