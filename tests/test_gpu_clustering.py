"""gmx_clustering on the device: tri, deg and lcc byte for byte against the host model (test_clustering_host.clustering_model)
or a closed form, the totals and the statistics with them, and the log line as the proof that a regime ran: the shapes at
which the 64-slot groups, the staging cap, the packed position counters and the 64-bit sums can go wrong; every knob; the
plan shared with gmx_triangle_counting_directed; unsorted multigraphs; the graph without a reverse CSR; the driver."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_clustering_host import check_against_networkx, clique, clustering_model, lcc_of
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_LCC_CAP", "GMX_LCC_ALONE", "GMX_LCC_RATIO", "GMX_LCC_HUB_TAIL", "GMX_LCC_HUBS", "GMX_LCC_NO_ORDER", "GMX_LCC_PLAIN", "GMX_LCC_LOG",
         "GMX_TCD_NO_ORDER", "GMX_TCD_LOG")
LOG = re.compile(r"gmx clustering: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) build_ms [\d.]+ "
                 r"hubs (?P<hubs>\d+) hub_ms [\d.]+; cap (?P<cap>\d+) alone (?P<alone_max>\d+) ratio (?P<ratio>\d+) hub_tail (?P<hub_tail>\d+) "
                 r"w (?P<w>\w+); items (?P<staged>\d+) staged \+ (?P<memory>\d+) memory; slots (?P<alone>\d+) alone \+ (?P<list>\d+) list \+ "
                 r"(?P<tail>\d+) tail \+ (?P<hub>\d+) hub \+ (?P<empty>\d+) empty; credits (?P<lds>\d+) lds \+ (?P<glob>\d+) global\n")
TCD_LOG = re.compile(r"gmx triangle_counting_directed: plan V \d+ out \d+ up \d+ order \w+ built (\d)")
BIG = 1 << 30


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
    def call(g, **knobs):
        """One call with GMX_LCC_LOG and the knobs given (hubs=0, cap=64, no_order=1, ...; the others unset):
        (tri, deg, lcc, triangles, wedges, stats, the log line's fields), the line checked against the results."""
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMX_LCC_LOG", "1")
        for k, v in knobs.items():
            monkeypatch.setenv("GMX_LCC_" + k.upper(), str(v))
        capfd.readouterr()
        tri, deg, lcc, T, W, st = g.clustering()
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {k: (v if k in ("order", "w") else int(v)) for k, v in m.groupdict().items()}
        assert tri.dtype == np.int64 and deg.dtype == np.int32 and lcc.dtype == np.float64
        assert f["V"] == g.V and f["E"] == g.E and f["up"] == st["edges_examined"] and 2 * f["up"] == int(deg.sum(dtype=np.int64))
        assert f["lds"] + f["glob"] == T and int(tri.sum()) == 3 * T
        assert st["iterations"] == 1 and st["vertices_reached"] == int((tri > 0).sum()) and st["kernel_ms"] > 0
        assert f["order"] == ("identity" if "no_order" in knobs else "degree")
        if "no_order" in knobs or knobs.get("hubs") == 0:
            assert f["hubs"] == 0 and f["hub"] == 0
        if f["memory"] == 0 and f["w"] == "lds":
            assert f["glob"] == 0
        if f["staged"] == 0:
            assert f["lds"] == 0
        return tri, deg, lcc, T, W, st, f
    return call


def agrees(res, want):
    tri, deg, lcc, T, W, st, f = res
    assert tri.tobytes() == want["tri"].tobytes()
    assert deg.tobytes() == want["deg"].tobytes()
    assert lcc.tobytes() == want["lcc"].tobytes()
    assert T == want["triangles"] and W == want["wedges"] and f["up"] == want["up"]
    if f["order"] == "degree" and "slots" in want:   # the work of the degree-ordered plan
        assert f["staged"] + f["memory"] == want["items"]
        assert f["alone"] + f["list"] + f["tail"] + f["hub"] + f["empty"] == want["slots"]


def model_of(g):
    begin, idx, _, _ = g.download(reverse=False)
    return clustering_model(g.V, begin, idx)


def clique_expectation(n):
    """K_n: every order is a tie, so the plan keeps the ids and vertex v has n - 1 - v upper neighbours."""
    tri = np.full(n, (n - 1) * (n - 2) // 2, np.int64)
    deg = np.full(n, n - 1, np.int32)
    d = np.arange(n - 1, -1, -1)
    return {"tri": tri, "deg": deg, "lcc": lcc_of(tri, deg), "triangles": n * (n - 1) * (n - 2) // 6, "wedges": n * (n - 1) * (n - 2) // 2,
            "up": n * (n - 1) // 2, "max_up": n - 1, "slots": int(np.maximum(d - 1, 0).sum()), "items": int(((np.maximum(d - 1, 0) + 63) // 64).sum())}


@pytest.fixture(scope="module")
def cliques(gmx):
    out = {}
    for n in (65, 66, 67, 130, 1100):
        V, s, d = clique(n)
        out[n] = gmx.Graph.from_edges(V, s, d)
    return out


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    tri, deg, lcc, T, W, st = g.clustering()
    assert len(tri) == 0 and len(deg) == 0 and len(lcc) == 0 and (T, W) == (0, 0) and st["iterations"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, run, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    if g.E == 0:   # answered before any plan: no log line
        res = g.clustering()
    else:
        res = run(g)
        assert res[6]["up"] == 0 and res[6]["staged"] + res[6]["memory"] == 0
    tri, deg, lcc, T, W, st = res[:6]
    assert len(tri) == V and not tri.any() and not deg.any() and lcc.tobytes() == np.zeros(V).tobytes() and (T, W) == (0, 0)
    assert st["iterations"] == 1 and st["vertices_reached"] == 0


@pytest.mark.parametrize("n", [65, 66, 67, 130])
def test_group_boundary_cliques(gmx, run, cliques, n):
    """The lowest vertex has 64, 65, 66 and 129 upper neighbours, so 63, 64, 65 and 128 slots: a group that is not full, one
    that is, and a second group of one slot and of 64.  In K_130 the positions from 64 on take exactly 64 credits from group
    0, the most a packed byte counter ever holds."""
    g, want = cliques[n], clique_expectation(n)
    assert all(np.array_equal(model_of(g)[k], want[k]) for k in ("tri", "deg", "lcc")) and model_of(g)["up"] == want["up"]
    for hubs in (0, None):
        for alone in (0, BIG):
            knobs = {"alone": alone}
            if hubs is not None:
                knobs["hubs"] = hubs
            res = run(g, **knobs)
            agrees(res, want)
            f = res[6]
            assert f["memory"] == 0 and f["glob"] == 0 and f["lds"] == want["triangles"]
            if alone == BIG:
                assert f["alone"] > 0 and f["list"] + f["tail"] + f["hub"] == 0
            elif hubs == 0:
                assert f["alone"] == 0 and f["list"] + f["tail"] > 0 and f["hub"] == 0
            else:
                assert f["hubs"] == (n & ~63) and f["hub"] > 0 and f["alone"] == 0
    agrees(run(g), want)
    agrees(run(g, plain=1), want)


def test_cap_boundary(gmx, run, cliques):
    g, want = cliques[130], clique_expectation(130)
    for extra in ({}, {"hubs": 0}, {"alone": 0}, {"hubs": 0, "alone": BIG}):
        res = run(g, cap=64, **extra)
        agrees(res, want)
        f = res[6]
        assert f["cap"] == 64 and f["memory"] > 0 and f["staged"] > 0 and f["glob"] > 0 and f["lds"] > 0
    g, want = cliques[1100], clique_expectation(1100)   # |UP'| = 1099 > 1024 at the default cap
    for extra in ({}, {"hubs": 0}):
        res = run(g, **extra)
        agrees(res, want)
        f = res[6]
        assert f["cap"] == 1024 and f["memory"] > 0 and f["staged"] > 0 and f["glob"] > 0 and f["lds"] > 0
        assert np.all(res[0] == 1099 * 1098 // 2)
    assert run(g, cap=1)[6]["cap"] == 64 and run(g, cap=5000)[6]["cap"] == 1024   # clamped


@pytest.fixture(scope="module")
def big_star(gmx):
    n = 70000   # leaves 1 .. n, and the edge {1, 2}
    s = np.concatenate([np.zeros(n, np.int64), [2]])
    d = np.concatenate([np.arange(1, n + 1), [1]])
    return gmx.Graph.from_edges(n + 1, s, d), n


def test_64_bit_arithmetic_on_a_big_star(gmx, run, big_star):
    g, n = big_star
    for knobs in ({}, {"hubs": 0}, {"no_order": 1}):
        tri, deg, lcc, T, W, st, f = run(g, **knobs)
        assert T == 1 and W == n * (n - 1) // 2 + 2 and W > 1 << 31 and int(deg[0]) * (int(deg[0]) - 1) > 1 << 32
        assert tri[0] == tri[1] == tri[2] == 1 and int(tri.sum()) == 3 and st["vertices_reached"] == 3
        assert deg[0] == n and deg[1] == deg[2] == 2 and np.all(deg[3:] == 1)
        assert lcc[0].tobytes() == np.float64(2.0 / (70000 * 69999)).tobytes()
        assert lcc[1] == lcc[2] == 1.0 and not lcc[3:].any()
        want_lcc = lcc_of(tri, deg)
        assert lcc.tobytes() == want_lcc.tobytes()


def test_order_knob_gives_the_same_bytes(gmx, run, cliques, big_star):
    rm = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    for g, extras in ((cliques[130], ({}, {"cap": 64}, {"alone": 0})), (cliques[1100], ({},)), (big_star[0], ({},)), (rm, ({}, {"cap": 64}, {"ratio": 0}))):
        a = run(g)
        for extra in extras:
            b = run(g, no_order=1, **extra)
            assert b[6]["hubs"] == 0 and b[6]["order"] == "identity" and b[6]["built"] == 1
            for k in range(3):
                assert a[k].tobytes() == b[k].tobytes()
            assert a[3:5] == b[3:5] and a[5]["vertices_reached"] == b[5]["vertices_reached"]
            assert run(g, no_order=1, **extra)[6]["built"] == 0
            c = run(g)   # back to the degree order: rebuilt
            assert c[6]["built"] == 1 and c[0].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("scale,permute", [(s, p) for s in (8, 10, 12, 14) for p in (False, True)])
def test_rmat_against_the_model_under_every_knob(gmx, run, scale, permute):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
    want = model_of(g)
    assert want["triangles"] > 0
    seen = {"hub": 0, "list": 0, "tail": 0, "alone": 0, "memory": 0}
    for hubs in (0, 64, None):
        for cap in (64, None):
            for ratio in (0, None):
                knobs = {k: v for k, v in (("hubs", hubs), ("cap", cap), ("ratio", ratio)) if v is not None}
                res = run(g, **knobs)
                agrees(res, want)
                tri, deg, lcc, T, W, st, f = res
                assert int(tri.sum()) == 3 * T and W == want["wedges"] and st["vertices_reached"] == int((tri > 0).sum())
                if hubs == 64:
                    assert f["hubs"] == 64
                if ratio == 0:
                    assert f["list"] == 0
                for k in seen:
                    seen[k] += f[k]
    print("RMAT-%d%s: triangles %d wedges %d, slots over the knobs %s" % (scale, "p" if permute else "", want["triangles"], want["wedges"], seen))
    assert seen["alone"] > 0 and seen["tail"] > 0 and seen["hub"] > 0 and seen["list"] > 0
    assert (seen["memory"] > 0) == (want["max_up"] > 64)   # cap 64
    assert scale < 12 or want["max_up"] > 64
    agrees(run(g, plain=1), want)
    agrees(run(g, alone=0, hub_tail=0), want)
    agrees(run(g, alone=BIG), want)


def test_symmetrised_rmat12_against_the_counting_entries_and_networkx(gmx, run):
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    res = run(g)
    tri, deg, lcc, T, W, st, f = res
    assert T == g.triangle_counting()[0]
    assert 3 * T == g.triangle_counting_directed()[0]   # the identity in gmx.h
    agrees(res, model_of(g))
    try:
        import networkx as nx
    except ImportError:
        return
    begin, idx, _, _ = g.download(reverse=False)
    check_against_networkx(nx, g.V, begin, idx, tri, lcc, T, W)


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (30000, 80000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    want = clustering_model(V, begin, idx)
    assert want["triangles"] > 0
    graphs = (gmx.Graph.upload(begin, idx, rb, ri, flags=0), gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS),
              gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE))
    for g in graphs:
        for knobs in ({}, {"hubs": 0, "cap": 64}):
            agrees(run(g, **knobs), want)


def test_plan_is_shared_with_triangle_counting_directed(gmx, run, capfd, monkeypatch):
    def tcd(g):
        monkeypatch.setenv("GMX_TCD_LOG", "1")
        capfd.readouterr()
        t = g.triangle_counting_directed()[0]
        m = TCD_LOG.search(capfd.readouterr().err)
        assert m
        return t, int(m.group(1))

    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    roots = [0, 1, 777, 4000]
    before = [g.hop_dist(r)[0] for r in roots]
    t0, b0 = tcd(g)
    assert b0 == 1
    a = run(g)
    assert a[6]["built"] == 0          # the plan tcd built
    t1, b1 = tcd(g)
    assert (t1, b1) == (t0, 0)
    h = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    c1, c2 = run(h), run(h)
    assert c1[6]["built"] == 1 and c2[6]["built"] == 0
    assert tcd(h) == (t0, 0)           # ... and the plan clustering built
    c3 = run(h)
    for r in (c1, c2, c3):
        for k in range(3):
            assert r[k].tobytes() == a[k].tobytes()
        assert r[3:5] == a[3:5]
    agrees(a, model_of(g))
    after = [g.hop_dist(r)[0] for r in roots]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_array_selection(gmx):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, True)
    tri, deg, lcc, T, W, st = g.clustering()
    t2, d2, l2, T2, W2, st2 = g.clustering(tri=False, deg=False, lcc=True)
    assert t2 is None and d2 is None and l2.tobytes() == lcc.tobytes() and (T2, W2) == (T, W) and T > 0
    assert st2["vertices_reached"] == st["vertices_reached"] == int((tri > 0).sum())
    t3, d3, l3, T3, W3, _ = g.clustering(lcc=False)
    assert l3 is None and t3.tobytes() == tri.tobytes() and d3.tobytes() == deg.tobytes() and (T3, W3) == (T, W)
    assert g.clustering(tri=False, deg=False, lcc=False)[:5] == (None, None, None, T, W)


def report_lines(tri, lcc, T, W):
    s = 0.0
    for x in lcc.tolist():   # in id order, sequentially in double
        s += x
    return ["triangles = %d\n" % T, "wedges = %d\n" % W, "transitivity = %.17g\n" % (float(3 * T) / float(W) if W else 0.0),
            "avg_clustering = %.17g\n" % (s / len(lcc)), "top = %d\n" % int(np.argmax(tri))]


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "clustering")
    assert os.path.exists(exe), "bin/clustering not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stdout
    m = clustering_model(256, c["begin"], c["node_idx"])
    for line in report_lines(m["tri"], m["lcc"], m["triangles"], m["wedges"]):
        assert line in out.stdout, (line, out.stdout)
    out = subprocess.run([exe, "RMAT:12", "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    tri, deg, lcc, T, W, _ = g.clustering()
    for line in report_lines(tri, lcc, T, W):
        assert line in out.stdout, (line, out.stdout)
