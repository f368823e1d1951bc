"""gmx_ktruss on the device: truss and support byte for byte against the one-thread model (ktruss_model.py) or a closed form,
the counts and statistics with them, and the log line's levels, rounds and slots against the model's: the shapes at which
the 64-slot steps of the wave's row walk, the same-round rule, many decrements of one word and rows far longer than a tile
can go wrong; rounds on the grid and in the one-workgroup tail; the plan shared with gmx_clustering and
gmx_triangle_counting_directed; unsorted multigraphs uploaded three ways; the array selection; the driver."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from ktruss_model import book, ktruss_model, star_with_a_triangle, triangulated_grid, two_cliques_and_a_path
from test_clustering_host import clique, nx_graph
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_KTRUSS_NO_ORDER", "GMX_KTRUSS_TAIL", "GMX_KTRUSS_LOG", "GMX_KTRUSS_PHASES", "GMX_LCC_NO_ORDER", "GMX_LCC_LOG", "GMX_TCD_NO_ORDER", "GMX_TCD_LOG")
LOG = re.compile(r"gmx ktruss: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) adj_built (?P<adj_built>\d); "
                 r"support (?P<support>\w+) triangles (?P<triangles>\d+); levels (?P<levels>\d+) rounds (?P<rounds>\d+) scanned (?P<scanned>\d+) "
                 r"grid_rounds (?P<grid_rounds>\d+) tail_rounds (?P<tail_rounds>\d+) slots (?P<slots>\d+) max_truss (?P<max_truss>\d+) top (?P<top>\d+)\n")
BIG = 1 << 30
LCC_BUILT = re.compile(r"gmx clustering: plan V \d+ E \d+ up \d+ order \w+ built (\d)")
TCD_BUILT = re.compile(r"gmx triangle_counting_directed: plan V \d+ out \d+ up \d+ order \w+ built (\d)")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def run(capfd, monkeypatch):
    def call(g, truss=True, support=True, **knobs):
        """One call with GMX_KTRUSS_LOG and the knobs given (no_order=1, tail=0, ...; the others unset): (truss, support, max_truss,
        num_edges, stats, the log line's fields), the line checked against the results."""
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMX_KTRUSS_LOG", "1")
        for k, v in knobs.items():
            monkeypatch.setenv("GMX_KTRUSS_" + k.upper(), str(v))
        capfd.readouterr()
        tr, su, k, n, st = g.ktruss(truss=truss, support=support)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {key: (v if key in ("order", "support") else int(v)) for key, v in m.groupdict().items()}
        assert f["V"] == g.V and f["E"] == g.E and f["up"] == n and st["kernel_ms"] > 0 and st["h2d_ms"] == 0
        assert f["order"] == ("identity" if "no_order" in knobs else "degree")
        if knobs.get("tail") == 0:
            assert f["tail_rounds"] == 0
        if knobs.get("tail") == BIG:
            assert f["grid_rounds"] == 0
        assert f["rounds"] == st["iterations"] == f["grid_rounds"] + f["tail_rounds"]
        assert f["slots"] == st["edges_examined"] and f["top"] == st["vertices_reached"] and f["max_truss"] == k
        if truss:
            assert tr.dtype == np.int32 and len(tr) == g.E and k == int(tr.max()) and k >= 2 and f["levels"] >= 1 and f["rounds"] >= f["levels"]
        else:
            assert tr is None and (k, f["levels"], f["rounds"], f["scanned"], f["slots"], f["top"]) == (0,) * 6
        if support:
            assert su.dtype == np.int32 and len(su) == g.E
            if truss:
                assert np.all(tr[tr > 0] <= su[tr > 0] + 2) and np.all((tr == 0) <= (su == 0))
        return tr, su, k, n, st, f
    return call


def agrees(res, want, peel=True):
    tr, su, k, n, st, f = res
    if tr is not None:
        assert tr.tobytes() == want["truss"].tobytes()
    if su is not None:
        assert su.tobytes() == want["support"].tobytes()
    assert n == want["num_edges"] and f["triangles"] == want["triangles"]
    if peel:
        assert (k, f["levels"], f["rounds"], f["slots"], f["top"], f["scanned"]) == tuple(want[x] for x in ("max_truss", "levels", "rounds", "slots", "top", "scanned"))


def model_of(g, peel=True):
    begin, idx, _, _ = g.download(reverse=False)
    return ktruss_model(g.V, begin, idx, peel)


def graph_of(gmx, shape):
    V, s, d = shape
    return gmx.Graph.from_edges(V, s, d)


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    tr, su, k, n, st = g.ktruss()
    assert len(tr) == 0 and len(su) == 0 and (k, n) == (0, 0) and st["iterations"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, capfd, monkeypatch, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    monkeypatch.setenv("GMX_KTRUSS_LOG", "1")
    capfd.readouterr()
    tr, su, k, n, st = g.ktruss()
    assert "gmx ktruss" not in capfd.readouterr().err   # answered without a plan
    assert len(tr) == len(su) == g.E and not tr.any() and not su.any() and (k, n) == (0, 0)
    assert (st["iterations"], st["vertices_reached"], st["edges_examined"]) == (0, 0, 0)
    g.clustering()                                       # ... and with the plan another entry built
    assert g.ktruss()[2:4] == (0, 0)


@pytest.mark.parametrize("n", [3, 4, 65, 66, 130])
def test_cliques(gmx, run, n):
    """The lowest vertex has n - 1 upper neighbours and every row n - 1 slots: 64, 65 and 129 are the 64-slot steps of the
    wave's row walk, 2 and 3 rows a lane walks alone."""
    g = graph_of(gmx, clique(n))
    for knobs in ({}, {"tail": 0}, {"tail": BIG}, {"no_order": 1}):
        tr, su, k, ne, st, f = run(g, **knobs)
        assert np.all(su == n - 2) and np.all(tr == n) and (k, ne) == (n, n * (n - 1) // 2)
        assert (f["levels"], f["rounds"], f["top"], f["triangles"]) == (1, 1, ne, n * (n - 1) * (n - 2) // 6)
        assert st["edges_examined"] == n * (n - 1) // 2 * (n - 1)


def test_long_rows_of_a_big_clique(gmx, run):
    g = graph_of(gmx, clique(1100))   # rows of 1099 slots: 18 steps of the wave, the last one of 11 lanes
    tr, su, k, ne, st, f = run(g, truss=False)
    assert np.all(su == 1098) and ne == 1100 * 1099 // 2 and f["triangles"] == 1100 * 1099 * 1098 // 6


def test_two_cliques_sharing_a_vertex_and_a_pendant_path(gmx, run):
    V, s, d = two_cliques_and_a_path()
    g = gmx.Graph.from_edges(V, s, d)
    want = model_of(g)
    for knobs in ({}, {"tail": 0}, {"tail": BIG}, {"no_order": 1}):
        res = run(g, **knobs)
        agrees(res, want)
        begin, idx, _, _ = g.download(reverse=False)
        rows = np.repeat(np.arange(V), np.diff(begin))
        assert np.array_equal(res[0], np.where(rows >= 12, 2, np.where(idx <= 4, 5, 9)))
        assert res[5]["levels"] == 3 and res[2] == 9 and res[5]["top"] == 36   # s jumps 0 -> 3 -> 7


def test_book_with_70000_pages(gmx, run):
    """Both page edges of every triangle are in round 0's queue (the same-round rule: exactly one of them decrements the
    spine), the spine's word takes 70000 decrements and exactly one of them queues it, and the spine's rows are far longer
    than a tile."""
    m = 70000
    V, s, d = book(m)
    g = gmx.Graph.from_edges(V, s, d)
    begin, idx, _, _ = g.download(reverse=False)
    spine = (np.repeat(np.arange(V), np.diff(begin)) == 0) & (idx == 1)
    assert spine.sum() == 1
    for knobs in ({}, {"tail": 0}, {"tail": BIG}, {"no_order": 1}):
        tr, su, k, ne, st, f = run(g, **knobs)
        assert su[spine] == m and np.all(su[~spine] == 1) and np.all(tr == 3) and (k, ne) == (3, 2 * m + 1)
        assert (f["levels"], f["rounds"], f["triangles"], f["top"]) == (1, 2, m, 2 * m + 1)
        assert f["slots"] == (m + 1) + 2 * (2 * m)


def test_star_with_a_triangle(gmx, run):
    n = 70000
    V, s, d = star_with_a_triangle(n)
    g = gmx.Graph.from_edges(V, s, d)
    begin, idx, _, _ = g.download(reverse=False)
    rows = np.repeat(np.arange(V), np.diff(begin))
    in_triangle = np.maximum(rows, idx) <= 2
    assert in_triangle.sum() == 3
    for knobs in ({}, {"tail": 0}, {"tail": BIG}, {"no_order": 1}):
        tr, su, k, ne, st, f = run(g, **knobs)
        assert np.all(tr[in_triangle] == 3) and np.all(tr[~in_triangle] == 2) and np.all(su == in_triangle)
        assert (k, ne, f["levels"], f["rounds"], f["top"], f["triangles"]) == (3, n + 1, 2, 2, 3, 1)
        assert f["slots"] == (n - 2) + 3 * 2


def test_triangulated_grid_peels_one_ring_per_round(gmx, run):
    n = 40
    g = graph_of(gmx, triangulated_grid(n))
    want = model_of(g)
    assert (want["levels"], want["rounds"], want["max_truss"]) == (1, n, 3)
    for knobs in ({"tail": 0}, {"tail": BIG}, {}):   # all rounds on the grid, all in the tail, the default
        res = run(g, **knobs)
        agrees(res, want)
        assert np.all(res[0] == 3) and res[5]["grid_rounds"] + res[5]["tail_rounds"] == n


@pytest.mark.parametrize("scale,permute", [(s, p) for s in (8, 10, 12) for p in (False, True)])
def test_rmat_against_the_model(gmx, run, scale, permute):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
    want = model_of(g)
    assert want["triangles"] > 0 and want["levels"] > 3 and want["rounds"] > want["levels"]
    print("RMAT-%d%s: edges %d triangles %d max_truss %d levels %d rounds %d slots %d" % (
        scale, "p" if permute else "", want["num_edges"], want["triangles"], want["max_truss"], want["levels"], want["rounds"], want["slots"]))
    a = run(g)
    agrees(a, want)
    seen = {"grid_rounds": a[5]["grid_rounds"], "tail_rounds": a[5]["tail_rounds"]}
    for knobs in ({"tail": 0}, {"tail": BIG}, {"tail": 64}):
        r = run(g, **knobs)
        agrees(r, want)
        assert r[0].tobytes() == a[0].tobytes() and r[1].tobytes() == a[1].tobytes()
        for key in seen:
            seen[key] += r[5][key]
    assert seen["grid_rounds"] > 0 and seen["tail_rounds"] > 0
    assert scale < 12 or (a[5]["grid_rounds"] > 0 and a[5]["tail_rounds"] > 0)   # the default hands over in both directions
    b = run(g, no_order=1)
    agrees(b, want)
    assert b[5]["built"] == 1 and b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes()


def test_symmetrised_rmat10_against_the_counting_entries_and_networkx(gmx, run):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    res = run(g)
    want = model_of(g)
    agrees(res, want)
    assert res[5]["triangles"] == g.clustering()[3] == g.triangle_counting()[0]
    try:
        import networkx as nx
    except ImportError:
        return
    begin, idx, _, _ = g.download(reverse=False)
    G = nx_graph(nx, g.V, begin, idx)
    rows = np.repeat(np.arange(g.V), np.diff(begin))
    for k in range(2, res[2] + 2):
        got = {(min(a, b), max(a, b)) for a, b in nx.k_truss(G, k).edges()}
        keep = res[0] >= k
        assert got == set(zip(np.minimum(rows, idx)[keep].tolist(), np.maximum(rows, idx)[keep].tolist())), k


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (30000, 80000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    want = ktruss_model(V, begin, idx)
    assert want["triangles"] > 0
    rows = np.repeat(np.arange(V), np.diff(begin))
    loops = rows == idx
    key = np.minimum(rows, idx).astype(np.int64) * V + np.maximum(rows, idx)
    assert loops.any() and len(np.unique(key[~loops])) < (~loops).sum()   # self loops, and repeats or both directions
    graphs = (gmx.Graph.upload(begin, idx, rb, ri, flags=0), gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS),
              gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE))
    for g in graphs:
        agrees(run(g, tail=0), want)
        res = run(g)
        agrees(res, want)
        for arr in res[:2]:
            assert not arr[loops].any()
            first = {}
            for k, x in zip(key[~loops].tolist(), arr[~loops].tolist()):
                assert first.setdefault(k, x) == x


def test_plan_is_shared_with_clustering_and_triangle_counting_directed(gmx, run, capfd, monkeypatch):
    def other(g, entry, var, pattern):
        monkeypatch.setenv(var, "1")
        capfd.readouterr()
        out = entry()
        m = pattern.search(capfd.readouterr().err)
        assert m
        return out, int(m.group(1))

    def lcc(g):
        out, built = other(g, g.clustering, "GMX_LCC_LOG", LCC_BUILT)
        return (out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), out[3], out[4]), built

    def tcd(g):
        out, built = other(g, g.triangle_counting_directed, "GMX_TCD_LOG", TCD_BUILT)
        return out[0], built

    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    roots = [0, 1, 777, 4000]
    before = [g.hop_dist(r)[0] for r in roots]
    c0, b0 = lcc(g)
    assert b0 == 1
    a = run(g)
    assert (a[5]["built"], a[5]["adj_built"]) == (0, 1)      # the plan clustering built, plus the adjacency
    assert (run(g)[5]["built"], run(g)[5]["adj_built"]) == (0, 0)
    assert lcc(g) == (c0, 0)
    h = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    b = run(h)
    assert (b[5]["built"], b[5]["adj_built"]) == (1, 1)
    assert lcc(h) == (c0, 0) and tcd(h) == (tcd(g)[0], 0)   # ... and the plan ktruss built
    c = run(h, no_order=1)
    assert (c[5]["built"], c[5]["adj_built"]) == (1, 1)      # the other order: rebuilt
    d = run(h)
    assert (d[5]["built"], d[5]["adj_built"]) == (1, 1)      # and back
    for r in (b, c, d):
        assert r[0].tobytes() == a[0].tobytes() and r[1].tobytes() == a[1].tobytes() and r[2:4] == a[2:4]
    agrees(a, model_of(g))
    after = [g.hop_dist(r)[0] for r in roots]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_array_selection(gmx, run):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, True)
    tr, su, k, n, st, f = run(g)
    t2, s2, k2, n2, st2, f2 = run(g, truss=False)
    assert t2 is None and s2.tobytes() == su.tobytes() and (k2, n2) == (0, n) and st2["iterations"] == 0 and f2["triangles"] == f["triangles"] > 0
    t3, s3, k3, n3, st3, f3 = run(g, support=False)
    assert s3 is None and t3.tobytes() == tr.tobytes() and (k3, n3) == (k, n) and st3["iterations"] == st["iterations"]
    assert g.ktruss(truss=False, support=False)[:4] == (None, None, 0, n)


def test_two_calls_give_the_same_bytes_and_statistics(gmx, run):
    g = gmx.Graph.rmat(1 << 11, 16 << 11, 7, 0.57, 0.19, 0.19, True)
    a, b = run(g), run(g)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:4] == b[2:4]
    for key in ("iterations", "edges_examined", "vertices_reached"):
        assert a[4][key] == b[4][key]
    assert a[4]["iterations"] > 0 and a[4]["edges_examined"] > 0


def report_lines(max_truss, top, num_edges, triangles, rounds):
    return ["max_truss = %d\n" % max_truss, "max_truss_edges = %d\n" % top, "num_edges = %d\n" % num_edges, "triangles = %d\n" % triangles,
            "rounds = %d\n" % rounds]


def test_dropin_driver(gmx, run, golden):
    exe = os.path.join(PKG, "bin", "ktruss")
    assert os.path.exists(exe), "bin/ktruss not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stdout
    m = ktruss_model(256, c["begin"], c["node_idx"])
    for line in report_lines(m["max_truss"], m["top"], m["num_edges"], m["triangles"], m["rounds"]):
        assert line in out.stdout, (line, out.stdout)
    out = subprocess.run([exe, "RMAT:12", "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    tr, su, k, n, st, f = run(g)
    for line in report_lines(k, st["vertices_reached"], n, f["triangles"], st["iterations"]):
        assert line in out.stdout, (line, out.stdout)
