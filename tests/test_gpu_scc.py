"""gmx_scc (kosaraju.gm) on the device: the partition and count against the restated kosaraju.gm checker (small graphs)
or scipy (larger ones), both canonicalised; shapes that stress each phase; unsorted multigraphs; the drop-in driver."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_scc_host import canonical, kosaraju_check, scipy_scc
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
INT_MAX = 2147483647


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def expect(g, V=None):
    """(count, canonical comp) of the downloaded graph: the checker up to 2^16 vertices, scipy above."""
    begin, idx, rb, ri = g.download()
    V = len(begin) - 1
    if V <= (1 << 16):
        n, mem = kosaraju_check(V, begin, idx, rb, ri)
        return n, canonical(mem)
    r = scipy_scc(V, begin, idx)
    if r is None:
        pytest.skip("scipy does not import")
    return r


def check(g):
    comp, n, st = g.scc()
    en, ecomp = expect(g)
    assert n == en
    assert np.array_equal(comp, ecomp)
    if n:
        assert st["vertices_reached"] == int(np.bincount(comp).max())
    return comp, n, st


def test_reference_drivers_ten_vertex_graph(gmx):
    src = [0, 1, 2, 3, 5, 7, 9, 1, 2, 4]
    dst = [1, 2, 3, 0, 8, 4, 1, 4, 5, 9]
    g = gmx.Graph.from_edges(10, src, dst)
    comp, n, st = g.scc()
    assert n == 5
    assert comp.tolist() == [0, 0, 0, 0, 0, 1, 2, 3, 4, 0]
    assert st["vertices_reached"] == 6


def _shape(name):
    rng = np.random.default_rng(11)
    P = 1 << 16
    if name == "no_edges":
        return 1000, [], []
    if name == "one_vertex":
        return 1, [], []
    if name == "one_vertex_self_loop":
        return 1, [0, 0], [0, 0]
    if name == "self_loops_only":
        return 300, list(range(300)), list(range(300))
    if name == "path":
        return P, np.arange(P - 1), np.arange(1, P)
    if name == "reverse_path":
        return P, np.arange(1, P), np.arange(P - 1)
    if name == "cycle":
        return P, np.arange(P), (np.arange(P) + 1) % P
    if name == "triangle_chain":   # 256 triangles, each with an edge into the next: a DAG of non-trivial SCCs
        t = np.arange(256)
        s = np.concatenate([3 * t, 3 * t + 1, 3 * t + 2, 3 * t[:-1] + 2])
        d = np.concatenate([3 * t + 1, 3 * t + 2, 3 * t, 3 * t[1:]])
        return 768, s, d
    if name == "triangle_chain_backwards":
        t = np.arange(256)
        s = np.concatenate([3 * t, 3 * t + 1, 3 * t + 2, 3 * t[1:]])
        d = np.concatenate([3 * t + 1, 3 * t + 2, 3 * t, 3 * t[:-1] + 2])
        return 768, s, d
    if name == "star_out":
        return 5000, np.zeros(4999, np.int64), np.arange(1, 5000)
    if name == "star_in":
        return 5000, np.arange(1, 5000), np.zeros(4999, np.int64)
    if name == "star_both":
        return 5000, np.concatenate([np.zeros(4999, np.int64), np.arange(1, 5000)]), np.concatenate([np.arange(1, 5000), np.zeros(4999, np.int64)])
    if name == "two_sccs_one_way":   # two random strongly connected halves (a cycle each + chords), edges A -> B only
        h = 40000
        perm = rng.permutation(2 * h)
        s, d = [], []
        for base in (0, h):
            c = np.arange(h)
            s += [base + c, base + rng.integers(0, h, 3 * h)]
            d += [base + (c + 1) % h, base + rng.integers(0, h, 3 * h)]
        s.append(rng.integers(0, h, 500))
        d.append(h + rng.integers(0, h, 500))
        s, d = np.concatenate(s), np.concatenate(d)
        return 2 * h, perm[s], perm[d]
    if name == "hub_without_in_edges":   # the vertex with the most out-edges has no in-edge, the rest is a cycle
        V = 20000
        c = np.arange(1, V)
        s = np.concatenate([np.zeros(3 * V, np.int64), c])
        d = np.concatenate([rng.integers(1, V, 3 * V), np.where(c + 1 < V, c + 1, 1)])
        return V, s, d
    raise KeyError(name)


SHAPES = ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only", "path", "reverse_path", "cycle", "triangle_chain",
          "triangle_chain_backwards", "star_out", "star_in", "star_both", "two_sccs_one_way", "hub_without_in_edges"]


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_against_checker(gmx, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    check(g)


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    comp, n, st = g.scc()
    assert n == 0 and len(comp) == 0


def test_symmetrised_rmat_gives_weak_components(gmx):
    g = gmx.Graph.rmat(1 << 14, 4 << 14, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    comp, n, st = check(g)
    assert n > 1


@pytest.mark.parametrize("scale", [8, 10, 12, 14])
@pytest.mark.parametrize("permute", [False, True])
def test_rmat_small_against_checker(gmx, scale, permute):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
    check(g)


@pytest.mark.parametrize("scale", [16, 18, 20, 22])
def test_rmat_against_scipy(gmx, scale):
    pytest.importorskip("scipy")
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, scale % 4 == 2)
    check(g)


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (150000, 400000)])
def test_unsorted_multigraph_uploaded_verbatim(gmx, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    comp, n, st = g.scc()
    r = scipy_scc(V, begin, idx) if V > 4096 else None
    if r is None:
        en, mem = kosaraju_check(V, begin, idx, rb, ri)
        r = (en, canonical(mem))
    assert n == r[0]
    assert np.array_equal(comp, r[1])
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)   # the same graph with sorted rows
    comp2, n2, _ = sorted_g.scc()
    assert n2 == n and np.array_equal(comp2, comp)


def test_no_reverse_csr_is_a_state_error(gmx):
    import ctypes as C
    g = gmx.Graph.from_edges(4, [0, 1, 2], [1, 2, 0], flags=gmx.GMX_GRAPH_NO_REVERSE)
    comp = np.zeros(4, np.int32)
    n = C.c_int64(0)
    assert gmx.lib().gmx_scc(g._h, comp.ctypes.data, C.byref(n), None) == -5   # GMX_ERR_STATE
    assert b"reverse" in gmx.lib().gmx_last_error()
    with pytest.raises(gmx.GmxError):
        g.scc()


def test_repeatable_and_hop_dist_unchanged(gmx):
    g = gmx.Graph.rmat(1 << 18, 16 << 18, 1997, 0.57, 0.19, 0.19, False)
    roots = [0, 1, 777, 123456]
    before = [g.hop_dist(r)[0] for r in roots]
    c1, n1, s1 = g.scc()
    c2, n2, s2 = g.scc()
    assert n1 == n2 and np.array_equal(c1, c2)
    assert s1["vertices_reached"] == int(np.bincount(c1).max()) == s2["vertices_reached"]
    assert s1["kernel_ms"] > 0 and s1["edges_examined"] > 0 and s1["iterations"] >= 1
    after = [g.hop_dist(r)[0] for r in roots]
    for b, a in zip(before, after):
        assert np.array_equal(a, b)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "kosaraju")
    assert os.path.exists(exe), "bin/kosaraju not built"
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    n, _ = kosaraju_check(256, c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
    assert "num_membership = %d\n" % n in out.stdout
    out = subprocess.run([exe, "RMAT:12", "1", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    n, _ = kosaraju_check(1 << 12, *g.download())
    assert "num_membership = %d\n" % n in out.stdout


def test_rmat24_against_scipy(gmx):
    pytest.importorskip("scipy")
    g = gmx.Graph.rmat(1 << 24, 16 << 24, 1997, 0.57, 0.19, 0.19, True)
    comp, n, st = g.scc()
    begin, idx, _, _ = g.download(reverse=False)
    en, ecomp = scipy_scc(1 << 24, begin, idx)
    assert n == en
    assert np.array_equal(comp, ecomp)


def test_rmat26_giant_component_from_two_traversals(gmx):
    """Count and largest SCC at RMAT-26: the largest is FW(p) n BW(p) of a vertex p inside it, computed from hop_dist on
    the graph and on a transposed upload; the other components are the SCCs of the graph without it (scipy)."""
    V = 1 << 26
    g = gmx.Graph.rmat(V, 16 << 26, 1997, 0.57, 0.19, 0.19, False)
    comp, n, st = g.scc()
    sizes = np.bincount(comp)
    big = int(sizes.argmax())
    assert st["vertices_reached"] == int(sizes[big])
    p = int(np.flatnonzero(comp == big)[0])
    fw, _ = g.hop_dist(p)
    begin, idx, rb, ri = g.download()
    gt = gmx.Graph.upload(rb, ri, begin, idx, flags=0)
    bw, _ = gt.hop_dist(p)
    del gt
    inside = (fw != INT_MAX) & (bw != INT_MAX)
    assert int(inside.sum()) == int(sizes[big])
    assert np.array_equal(inside, comp == big)
    pytest.importorskip("scipy")
    keep = ~inside
    src = np.repeat(np.arange(V, dtype=np.int32), np.diff(begin))
    m = keep[src] & keep[idx]
    new_id = np.cumsum(keep) - 1
    rest = int(keep.sum())
    del rb, ri, bw, fw
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    a = csr_matrix((np.ones(int(m.sum()), np.int8), (new_id[src[m]], new_id[idx[m]])), shape=(rest, rest))
    del src, m
    n_rest, _ = connected_components(a, directed=True, connection="strong")
    assert n == n_rest + 1
