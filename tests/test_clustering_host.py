"""Per-vertex triangle counts and clustering coefficients, host side (no GPU): a numpy model of gmx_clustering's scheme that
the GPU tests compare bytes with; the model against the definition on a dense matrix, against closed forms and against
networkx; the C entry's argument checks; the drop-in header.

The stored slots are read as an undirected simple graph: N(v) = { u != v : v -> u or u -> v is stored }, deg = |N|,
tri[v] = #{ unordered {u, w} in N(v) : w in N(u) }, lcc[v] = float64(2 tri) / float64(deg (deg - 1)) (0.0 below degree 2),
triangles = sum(tri) / 3, wedges = sum(deg (deg - 1) / 2).  The model follows the device: N as sorted unique keys, a stable
ascending-degree renumbering, UP' (the neighbours above a vertex in that numbering), and for every oriented edge (v, u) the
entries w of UP'(u) that are neighbours of v, each credited to v, u and w."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scc_host import CXX_FLAGS, PKG, csr_of


def lcc_of(tri, deg):
    tri, deg = np.asarray(tri, np.int64), np.asarray(deg, np.int64)
    pairs = deg * (deg - 1)
    out = np.zeros(len(tri), np.float64)
    ok = deg >= 2
    out[ok] = (2 * tri[ok]).astype(np.float64) / pairs[ok].astype(np.float64)
    return out


def clustering_model(V, begin, idx):
    """dict(tri[int64], deg[int32], lcc[float64], triangles, wedges, up, max_up, slots, items) of the forward CSR (begin, idx):
    up = |UP'|, max_up = the longest UP' row, slots and items = the work of the degree-ordered plan (a row of d >= 2 upper
    neighbours has d - 1 slots in ceil((d - 1) / 64) work items)."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin))
    keep = rows != idx
    s, d = rows[keep], idx[keep]
    keys = np.unique(np.concatenate([s * V + d, d * V + s]))           # N, sorted, repeats dropped
    a, b = (keys // V, keys % V) if V else (keys, keys)
    deg = np.bincount(a, minlength=V).astype(np.int64)
    order = np.argsort(deg, kind="stable")                             # ascending |N|, ties by id
    perm = np.empty(V, np.int64)
    perm[order] = np.arange(V)
    pa, pb = perm[a], perm[b]
    upk = np.sort((pa * V + pb)[pa < pb])                              # UP' in the new numbering, row-major and sorted
    x, y = (upk // V, upk % V) if V else (upk, upk)
    ub = np.concatenate([[0], np.cumsum(np.bincount(x, minlength=V))]).astype(np.int64)
    tri_new = np.zeros(V, np.int64)
    lens = ub[y + 1] - ub[y] if len(y) else np.zeros(0, np.int64)      # |UP'(u)| for every oriented edge (v, u)
    step = 1 << 16
    for lo in range(0, len(y), step):                                  # in pieces: the expansion is sum |UP'(u)| long
        ln = lens[lo:lo + step]
        total = int(ln.sum())
        pos = np.repeat(ub[y[lo:lo + step]] - (np.cumsum(ln) - ln), ln) + np.arange(total)
        w = y[pos]
        v, u = np.repeat(x[lo:lo + step], ln), np.repeat(y[lo:lo + step], ln)
        q = v * V + w
        f = np.searchsorted(upk, q)
        hit = (f < len(upk)) & (upk[np.minimum(f, len(upk) - 1)] == q)
        for c in (v, u, w):
            tri_new += np.bincount(c[hit], minlength=V)
    tri = tri_new[perm] if V else tri_new
    return {"tri": tri.astype(np.int64), "deg": deg.astype(np.int32), "lcc": lcc_of(tri, deg), "triangles": int(tri.sum()) // 3,
            "wedges": int((deg * (deg - 1) // 2).sum()), "up": len(upk), "max_up": int(np.diff(ub).max()) if V else 0,
            "slots": int(np.maximum(np.diff(ub) - 1, 0).sum()), "items": int(((np.maximum(np.diff(ub) - 1, 0) + 63) // 64).sum())}


def by_definition(V, begin, idx):
    """(tri, deg) from the dense 0/1 matrix of N."""
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    rows = np.repeat(np.arange(V), np.diff(begin))
    A = np.zeros((V, V), np.int64)
    A[rows, idx] = 1
    A[idx, rows] = 1
    A[np.arange(V), np.arange(V)] = 0
    return ((A @ A) * A).sum(1) // 2, A.sum(1)


def check_against_definition(V, begin, idx):
    m = clustering_model(V, begin, idx)
    tri, deg = by_definition(V, begin, idx)
    assert np.array_equal(m["tri"], tri) and np.array_equal(m["deg"], deg)
    assert m["tri"].dtype == np.int64 and m["deg"].dtype == np.int32 and m["lcc"].dtype == np.float64
    assert m["lcc"].tobytes() == lcc_of(tri, deg).tobytes()
    assert 3 * m["triangles"] == tri.sum() and m["wedges"] == (deg * (deg - 1) // 2).sum() and 2 * m["up"] == deg.sum()
    return m


# ---- named shapes (also uploaded by the GPU tests)
def clique(n):
    a, b = np.nonzero(np.triu(np.ones((n, n), bool), 1))
    return n, a, b


def cycle(n):
    return n, np.arange(n), (np.arange(n) + 1) % n


def star(n):
    return n + 1, np.zeros(n, np.int64), np.arange(1, n + 1)


def friendship(k):
    """k triangles sharing vertex 0: n = 2 k rim vertices."""
    r = 1 + 2 * np.arange(k)
    return 2 * k + 1, np.concatenate([np.zeros(2 * k, np.int64), r]), np.concatenate([np.arange(1, 2 * k + 1), r + 1])


TRIANGLES = {
    "one_way_round": ([0, 1, 2], [1, 2, 0]),
    "both_directions": ([0, 1, 2, 1, 2, 0], [1, 2, 0, 0, 1, 2]),
    "repeats_and_self_loops": ([0, 0, 0, 1, 2, 2, 1, 1, 2], [1, 1, 0, 2, 0, 2, 1, 2, 0]),
}


def random_multigraph(rng, vmax):
    V = int(rng.integers(1, vmax + 1))
    E = int(rng.integers(0, 6 * V + 1))
    return V, rng.integers(0, V, E), rng.integers(0, V, E)   # repeats and self loops included


def test_model_against_the_definition_on_random_directed_multigraphs():
    rng = np.random.default_rng(21)
    seen = 0
    for trial in range(150):
        V, s, d = random_multigraph(rng, 80)
        begin, idx, _, _ = csr_of(V, s, d)
        seen += check_against_definition(V, begin, idx)["triangles"]
    assert seen > 1000
    V, s, d = random_multigraph(np.random.default_rng(22), 1024)
    check_against_definition(1024, *csr_of(1024, s % 1024, d % 1024)[:2])


def test_model_against_the_definition_on_rmat8(golden):
    c = golden["cases"]["rmat8_noperm"]
    m = check_against_definition(256, c["begin"], c["node_idx"])
    assert m["triangles"] > 0 and m["wedges"] > m["triangles"]


def test_named_shapes_have_their_closed_forms():
    for n in (3, 4, 5, 65, 130):
        V, s, d = clique(n)
        m = check_against_definition(V, *csr_of(V, s, d)[:2])
        assert np.all(m["tri"] == (n - 1) * (n - 2) // 2) and np.all(m["lcc"] == 1.0) and np.all(m["deg"] == n - 1)
        assert m["triangles"] == n * (n - 1) * (n - 2) // 6 and m["wedges"] == 3 * m["triangles"]
    for n in (4, 5, 1000):
        V, s, d = cycle(n)
        m = check_against_definition(V, *csr_of(V, s, d)[:2])
        assert not m["tri"].any() and not m["lcc"].any() and np.all(m["deg"] == 2) and m["wedges"] == n
    for name, (s, d) in TRIANGLES.items():
        m = check_against_definition(3, *csr_of(3, s, d)[:2])
        assert m["tri"].tolist() == [1, 1, 1] and m["lcc"].tolist() == [1.0, 1.0, 1.0] and (m["triangles"], m["wedges"]) == (1, 3), name
    V, s, d = star(500)
    m = check_against_definition(V, *csr_of(V, s, d)[:2])
    assert not m["tri"].any() and not m["lcc"].any() and m["deg"][0] == 500 and m["wedges"] == 500 * 499 // 2
    for k in (1, 2, 50):
        V, s, d = friendship(k)
        m = check_against_definition(V, *csr_of(V, s, d)[:2])
        n = 2 * k
        assert m["tri"][0] == n // 2 and np.all(m["tri"][1:] == 1) and np.all(m["lcc"][1:] == 1.0) and m["triangles"] == k
        assert m["lcc"][0] == (2.0 * k) / (n * (n - 1))
    # no vertex, no edge, self loops only
    m = clustering_model(0, [0], [])
    assert len(m["tri"]) == 0 and (m["triangles"], m["wedges"], m["up"]) == (0, 0, 0)
    for begin, idx in (([0, 0, 0, 0], []), ([0, 1, 2, 3], [0, 1, 2])):
        m = check_against_definition(3, begin, idx)
        assert not m["tri"].any() and not m["deg"].any() and m["lcc"].tobytes() == np.zeros(3).tobytes()


def nx_graph(nx, V, begin, idx):
    rows = np.repeat(np.arange(V), np.diff(np.asarray(begin, np.int64)))
    idx = np.asarray(idx, np.int64)
    keep = rows != idx
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(rows[keep].tolist(), idx[keep].tolist()))
    return G


def check_against_networkx(nx, V, begin, idx, tri, lcc, triangles, wedges):
    """tri equal; lcc equal as BYTES: networkx divides the Python integers 2 tri by deg (deg - 1), one correctly rounded
    division of the same two integers (found equal on every case here; no 1-ulp allowance is needed).  Transitivity is
    6 T / (2 W) there, the same rational."""
    G = nx_graph(nx, V, begin, idx)
    t, c = nx.triangles(G), nx.clustering(G)
    assert np.array_equal(tri, np.array([t[v] for v in range(V)], np.int64))
    assert np.asarray(lcc, np.float64).tobytes() == np.array([c[v] for v in range(V)], np.float64).tobytes()
    assert nx.transitivity(G) == ((3 * triangles) / wedges if wedges else 0)


def test_model_against_networkx(golden):
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(23)
    cases = [random_multigraph(rng, 60) for _ in range(100)]
    cases += [clique(9), cycle(7), star(9), friendship(6)]
    for V, s, d in cases:
        begin, idx, _, _ = csr_of(V, s, d)
        m = clustering_model(V, begin, idx)
        check_against_networkx(nx, V, begin, idx, m["tri"], m["lcc"], m["triangles"], m["wedges"])
    c = golden["cases"]["rmat8_noperm"]
    m = clustering_model(256, c["begin"], c["node_idx"])
    check_against_networkx(nx, 256, c["begin"], c["node_idx"], m["tri"], m["lcc"], m["triangles"], m["wedges"])


def test_clustering_arguments_rejected_without_a_device():
    import gmx
    L = gmx.lib()
    assert "gmx_clustering" in gmx.EXPORTS and hasattr(L, "gmx_clustering") and hasattr(gmx.Graph, "clustering")
    T, W = C.c_int64(7), C.c_int64(7)
    tri = np.zeros(4, np.int64)
    assert L.gmx_clustering(None, tri.ctypes.data, None, None, C.byref(T), C.byref(W), None) == -1   # GMX_ERR_ARG
    assert L.gmx_clustering(None, None, None, None, None, None, None) == -1
    assert L.gmx_clustering(C.c_void_p(8), None, None, None, None, C.byref(W), None) == -1   # triangles is checked before g is touched
    assert (T.value, W.value) == (7, 7) and not tri.any()
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert "int gmx_clustering(gmx_graph_t* g, int64_t* tri_host, int32_t* deg_host, double* lcc_host, int64_t* triangles, int64_t* wedges," in hdr


@pytest.mark.parametrize("edge64", [False, True])
def test_dropin_header_compiles_and_links(tmp_path, edge64):
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host", "host64"], stdout=subprocess.DEVNULL)
    src = tmp_path / "use_clustering.cc"
    src.write_text('#include "clustering.h"\nint main() { gm_graph G; int64_t w = 0; return clustering(G, (int64_t*) 0, (double*) 0, w) < 0; }\n')
    lib = os.path.join(PKG, "libgmgraph_e64.a" if edge64 else "libgmgraph.a")
    link = [lib, "-L" + PKG, "-lgmx", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + [str(src), "-o", str(tmp_path / "use_clustering")] + link)
    assert os.path.exists(os.path.join(ROOT, "green-marl_amd", "generated", "clustering.cc"))
