"""gmx_wcc on the device: every result against scipy's weak components of the downloaded CSR (canonicalised), together
with the count and the largest component; the shapes that stress the compress depth, the skipped tree and the merge-path
tile; every knob; the path that ran, from the log line, against the host model; unsorted multigraphs; the driver."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph
from test_wcc_host import late_attachment, scipy_wcc, wcc_model

pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_WCC_SAMPLE_ROUNDS", "GMX_WCC_SKIP", "GMX_WCC_GIANT", "GMX_WCC_LOG", "GMX_WCC_PHASES")
LOG = re.compile(r"gmx wcc: V (\d+) E (\d+) sample_rounds (\d+) sampled (\d+) giant (\d+) skipped (\d+) live (\d+) reverse ([01]) "
                 r"final_slots (\d+) comps (\d+) largest (\d+)\n")
LOG_FIELDS = ("V", "E", "sample_rounds", "sampled", "giant", "skipped", "live", "reverse", "final_slots", "comps", "largest")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def expect(g):
    begin, idx, _, _ = g.download(reverse=False) if g.V else (np.zeros(1, np.int32), np.zeros(0, np.int32), None, None)
    return scipy_wcc(g.V, begin, idx)


def check(g, want=None):
    """wcc() equal to scipy (want: a result computed before) in comp, count and largest component."""
    comp, n, st = g.wcc()
    en, ecomp = want if want is not None else expect(g)
    assert n == en
    assert comp.dtype == np.int32 and np.array_equal(comp, ecomp)
    if n:
        assert st["vertices_reached"] == int(np.bincount(ecomp).max())
    return comp, n, st


def logged(gmx_graph, capfd, monkeypatch):
    """One call with GMX_WCC_LOG: (comp, count, stats, the log line's fields)."""
    monkeypatch.setenv("GMX_WCC_LOG", "1")
    capfd.readouterr()
    comp, n, st = gmx_graph.wcc()
    err = capfd.readouterr().err
    monkeypatch.delenv("GMX_WCC_LOG")
    m = LOG.search(err)
    assert m, err
    f = dict(zip(LOG_FIELDS, map(int, m.groups())))
    assert f["V"] == gmx_graph.V and f["E"] == gmx_graph.E
    assert f["skipped"] + f["live"] == f["V"]
    assert f["sampled"] + f["final_slots"] == st["edges_examined"]
    assert f["comps"] == n and f["largest"] == st["vertices_reached"] and st["iterations"] == f["sample_rounds"] + 1
    return comp, n, st, f


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    comp, n, st = g.wcc()
    assert n == 0 and len(comp) == 0


def _wcc_shape(name):
    if name == "one_vertex_self_loop":
        return 1, [0], [0]
    if name == "permuted_path":   # the smallest id sits deep inside the chain: the compress depth
        P = 1 << 16
        perm = np.random.default_rng(3).permutation(P)
        return P, perm[:-1], perm[1:]
    return _shape(name)


SHAPES = ["no_edges", "one_vertex_self_loop", "self_loops_only", "path", "reverse_path", "cycle", "permuted_path", "star_out", "star_in",
          "triangle_chain"]


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_against_scipy(gmx, name):
    V, s, d = _wcc_shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    comp, n, st = check(g)
    if name in ("no_edges", "self_loops_only"):
        assert n == V and np.array_equal(comp, np.arange(V))
    if name in ("path", "reverse_path", "cycle", "permuted_path", "star_out", "star_in", "triangle_chain"):
        assert n == 1 and st["vertices_reached"] == V


@pytest.fixture(scope="module")
def late(gmx):
    """RMAT-12 plus 2000 vertices that hang on the end of the hub's row: (V, src, dst, hub, scipy's result)."""
    g0 = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g0.download(reverse=False)
    src = np.repeat(np.arange(g0.V), np.diff(begin))
    V, s, d, hub = late_attachment(g0.V, src, idx, 2000)
    o = np.lexsort((d, s))
    b = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=V))])
    return V, s, d, hub, scipy_wcc(V, b, d[o])


@pytest.mark.parametrize("form", ["reverse", "no_reverse", "skip0"])
def test_late_attachment(gmx, late, form, capfd, monkeypatch):
    V, s, d, hub, want = late
    g = gmx.Graph.from_edges(V, s, d, flags=gmx.GMX_GRAPH_NO_REVERSE if form == "no_reverse" else 0)
    begin, idx, _, _ = g.download(reverse=False)
    assert np.array_equal(idx[begin[hub + 1] - 2000:begin[hub + 1]], np.arange(V - 2000, V))   # behind every sampled slot
    if form == "skip0":
        monkeypatch.setenv("GMX_WCC_SKIP", "0")
    comp, n, st, f = logged(g, capfd, monkeypatch)
    assert n == want[0] and np.array_equal(comp, want[1])
    assert np.all(comp[V - 2000:] == comp[hub])
    assert st["vertices_reached"] == int(np.bincount(want[1]).max())
    assert f["reverse"] == (0 if form == "no_reverse" else 1)
    m = wcc_model(V, begin, idx, None, 2, giant=f["giant"])
    if form == "reverse":
        assert f["live"] == int(m["live"].sum()) >= 2000 and st["edges_examined"] == m["edges_skip"]
    else:
        assert f["live"] == V and f["skipped"] == 0 and st["edges_examined"] == m["edges_noskip"]


@pytest.fixture(scope="module")
def two_stars(gmx):
    """In-stars A (hub 0, 60 000 leaves) and B (hub 60 001, 50 000 leaves) and an isolated vertex."""
    a, b = 60000, 50000
    s = np.concatenate([np.arange(1, a + 1), np.arange(a + 2, a + 2 + b)])
    d = np.concatenate([np.zeros(a, np.int64), np.full(b, a + 1)])
    V = a + b + 3
    g = gmx.Graph.from_edges(V, s, d)
    return g, expect(g), a, b


@pytest.mark.parametrize("giant", ["A", "B", "isolated"])
def test_long_live_row_goes_through_the_tile(gmx, two_stars, giant, capfd, monkeypatch):
    g, want, a, b = two_stars
    forced = {"A": 17, "B": a + 1 + 23, "isolated": g.V - 1}[giant]
    monkeypatch.setenv("GMX_WCC_GIANT", str(forced))
    comp, n, st, f = logged(g, capfd, monkeypatch)
    assert n == 3 == want[0] and np.array_equal(comp, want[1]) and st["vertices_reached"] == a + 1
    assert f["giant"] == {"A": 0, "B": a + 1, "isolated": g.V - 1}[giant]
    assert f["skipped"] == {"A": a + 1, "B": b + 1, "isolated": 1}[giant]
    # the live hubs' in-rows and the live leaves' out-rows, every slot once each
    assert f["final_slots"] == 2 * {"A": b, "B": a, "isolated": a + b}[giant]


@pytest.fixture(scope="module")
def rmat_case(gmx):
    cache = {}

    def get(scale, permute):
        if (scale, permute) not in cache:
            cache.clear()   # (one graph at a time)
            g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
            cache[(scale, permute)] = (g, expect(g))
        return cache[(scale, permute)]
    return get


@pytest.mark.parametrize("scale,permute", [(s, p) for s in (8, 10, 12, 14) for p in (False, True)] + [(16, False), (18, True), (20, False)])
def test_rmat_against_scipy_under_every_knob(gmx, rmat_case, scale, permute, monkeypatch):
    g, want = rmat_case(scale, permute)
    comp, n, st = check(g, want)
    assert n > 1 and st["kernel_ms"] > 0
    for K in (0, 1, 4):
        monkeypatch.setenv("GMX_WCC_SAMPLE_ROUNDS", str(K))
        ck, nk, sk = check(g, want)
        assert ck.tobytes() == comp.tobytes() and sk["iterations"] == K + 1
    monkeypatch.delenv("GMX_WCC_SAMPLE_ROUNDS")
    monkeypatch.setenv("GMX_WCC_SKIP", "0")
    c0, n0, s0 = check(g, want)
    assert c0.tobytes() == comp.tobytes()


def test_the_path_that_ran_rmat14(gmx, rmat_case, capfd, monkeypatch):
    g, want = rmat_case(14, False)
    begin, idx, rb, _ = g.download()
    V = g.V
    ratios = {}
    for K in (1, 2, 4):
        monkeypatch.setenv("GMX_WCC_SAMPLE_ROUNDS", str(K))
        comp, n, st, f = logged(g, capfd, monkeypatch)
        assert n == want[0] and np.array_equal(comp, want[1])
        assert f["sample_rounds"] == K and f["reverse"] == 1
        assert f["skipped"] > 0 and f["skipped"] + f["live"] == V
        m = wcc_model(V, begin, idx, rb, K, giant=f["giant"])
        assert f["giant"] == m["gstar"] == wcc_model(V, begin, idx, rb, K)["gstar"]   # the probes' choice, and a root
        assert f["live"] == int(m["live"].sum())
        assert st["edges_examined"] == m["edges_skip"]
        monkeypatch.setenv("GMX_WCC_SKIP", "0")
        comp0, n0, st0, f0 = logged(g, capfd, monkeypatch)
        monkeypatch.delenv("GMX_WCC_SKIP")
        assert np.array_equal(comp0, comp)
        assert f0["live"] == V and f0["skipped"] == 0 and f0["final_slots"] == g.E
        assert st0["edges_examined"] == m["edges_noskip"] == int(np.minimum(np.diff(begin), K).sum()) + g.E
        ratios[K] = st["edges_examined"] / st0["edges_examined"]
        print("RMAT-14 K=%d: skip %d / no-skip %d slots = %.3f" % (K, st["edges_examined"], st0["edges_examined"], ratios[K]))
        assert 2 * st["edges_examined"] <= st0["edges_examined"]


def test_no_reverse_csr_gives_the_same_arrays(gmx, rmat_case, capfd, monkeypatch):
    g, want = rmat_case(14, False)
    begin, idx, _, _ = g.download(reverse=False)
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    comp, n, st, f = logged(h, capfd, monkeypatch)
    assert n == want[0] and np.array_equal(comp, want[1])
    assert f["reverse"] == 0 and f["live"] == g.V
    assert st["edges_examined"] == int(np.minimum(np.diff(begin), 2).sum()) + g.E


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (150000, 400000)])
def test_unsorted_multigraph_uploaded_verbatim(gmx, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    want = scipy_wcc(V, begin, idx)
    comp, n, st = check(g, want)
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)   # the same graph with sorted rows
    comp2, n2, _ = check(sorted_g, want)
    assert n2 == n and np.array_equal(comp2, comp)


def test_symmetrised_rmat_equals_scc(gmx):
    g = gmx.Graph.rmat(1 << 14, 4 << 14, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    comp, n, st = check(g)
    scomp, sn, sst = g.scc()
    assert n == sn > 1 and np.array_equal(comp, scomp)
    assert st["vertices_reached"] == sst["vertices_reached"]


def test_repeatable_and_hop_dist_unchanged(gmx):
    g = gmx.Graph.rmat(1 << 18, 16 << 18, 1997, 0.57, 0.19, 0.19, False)
    roots = [0, 1, 777, 123456]
    before = [g.hop_dist(r)[0] for r in roots]
    c1, n1, s1 = g.wcc()
    c2, n2, s2 = g.wcc()
    assert n1 == n2 and c1.tobytes() == c2.tobytes()
    assert s1["vertices_reached"] == int(np.bincount(c1).max()) == s2["vertices_reached"]
    assert s1["edges_examined"] == s2["edges_examined"] > 0 and s1["kernel_ms"] > 0 and s1["iterations"] == 3
    after = [g.hop_dist(r)[0] for r in roots]
    for b, a in zip(before, after):
        assert np.array_equal(a, b)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "wcc")
    assert os.path.exists(exe), "bin/wcc not built"
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    n, comp = scipy_wcc(256, c["begin"], c["node_idx"])
    assert (n, int(np.bincount(comp).max())) == (25, 232)
    assert "num_components = %d\n" % n in out.stdout and "largest_component = %d\n" % np.bincount(comp).max() in out.stdout
    out = subprocess.run([exe, "RMAT:12", "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    comp, n, st = g.wcc()
    assert "num_components = %d\n" % n in out.stdout and "largest_component = %d\n" % st["vertices_reached"] in out.stdout
