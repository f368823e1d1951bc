"""gmx_graphlets on the device: the graphlet degree vectors and the totals byte for byte against the one-thread forms
(graphlets_model.py) or a closed form, induced and not, per vertex and totals only, under the degree and the identity order,
with the staged walk and its plain form: degenerate and named shapes, rows at the boundaries of the row passes, a list longer
than a wave's LDS slice, wide credits, a binomial whose product wraps, RMAT graphs, upload forms, one handle shared with the
rest of the counting family, the columns the family also returns, the driver."""
import os
import subprocess
from math import comb

import numpy as np
import pytest

from conftest import GOLD, ROOT
from graphlets_sequences import log_fields   # (importing it also adds graphlets' row to the table of interleaved entries)
from graphlets_model import NAMES, SHAPES, clique_gdv, clique_subgraph_gdv, graphlets_definition, graphlets_formulas, star_gdv
from squares_model import clique, star
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_GRAPHLETS_NO_ORDER", "GMX_GRAPHLETS_PLAIN", "GMX_GRAPHLETS_CAP", "GMX_GRAPHLETS_LONG", "GMX_GRAPHLETS_LOG", "GMX_GRAPHLETS_PHASES",
         "GMX_SQUARES_NO_ORDER", "GMX_SQUARES_LOG", "GMX_KCLIQUE_NO_ORDER", "GMX_KCLIQUE_LOG", "GMX_KTRUSS_NO_ORDER", "GMX_KTRUSS_LOG", "GMX_LCC_NO_ORDER", "GMX_LCC_LOG",
         "GMX_TCD_NO_ORDER")
EVERY_WAY = [(induced, per_vertex, knobs) for induced in (True, False) for per_vertex in (True, False)
             for knobs in ({}, {"plain": 1}, {"no_order": 1}, {"no_order": 1, "plain": 1})]


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
    def call(g, per_vertex=True, induced=True, **knobs):
        """One call with GMX_GRAPHLETS_LOG and the knobs given (no_order=1, plain=1, cap=64, long=64; the others unset): (gdv,
        totals, stats, the log line's fields), the line and the statistics checked against the results."""
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("GMX_GRAPHLETS_LOG", "1")
        for name, v in knobs.items():
            monkeypatch.setenv("GMX_GRAPHLETS_" + name.upper(), str(v))
        capfd.readouterr()
        gdv, totals, st = g.graphlets(per_vertex=per_vertex, induced=induced)
        f = log_fields(capfd.readouterr().err)
        assert f["V"] == g.V and f["E"] == g.E and f["totals"] == totals.tolist() and f["induced"] == int(induced)
        assert f["order"] == ("identity" if "no_order" in knobs else "degree")
        assert f["counts"] == ("none" if not per_vertex else "global" if "plain" in knobs else "lds")
        assert totals.dtype == np.int64 and totals.shape == (9,) and f["up"] == totals[0]
        assert st["iterations"] == 1 and st["h2d_ms"] == 0 and st["kernel_ms"] > 0 and st["edges_examined"] == f["triangles"]
        if per_vertex:
            assert gdv.dtype == np.int64 and gdv.shape == (g.V, 15) and st["vertices_reached"] == int((gdv[:, 4:] != 0).any(axis=1).sum())
            assert f["triangles"] == totals[2] and ("plain" not in knobs or f["staged"] + f["memory"] == 0)
        else:
            assert gdv is None and st["vertices_reached"] == 0 and f["triangles"] == 0 and f["staged"] + f["memory"] + f["long_rows"] == 0
        return gdv, totals, st, f
    return call


def graph_of(gmx, shape):
    V, s, d = shape
    return gmx.Graph.from_edges(V, s, d)


def models_of(g):
    """{induced: the formulas' result} for the rows the device holds."""
    begin, idx, _, _ = g.download(reverse=False)
    out = {induced: graphlets_formulas(g.V, begin, idx, induced) for induced in (True, False)}
    for m in out.values():
        m["gdv"].setflags(write=False)
    return out


def agrees(res, want):
    gdv, totals, st, f = res
    assert totals.tobytes() == want["totals"].tobytes(), (totals, want["totals"])
    if gdv is not None:
        assert gdv.tobytes() == want["gdv"].tobytes(), np.argwhere(gdv != want["gdv"])[:8]
        assert st["vertices_reached"] == want["nonzero"] and st["edges_examined"] == want["triangles"]


def every_way(run, g, want, ways=EVERY_WAY, **more):
    for induced, per_vertex, knobs in ways:
        agrees(run(g, per_vertex, induced, **knobs, **more), want[induced])


# ---- 1: degenerate shapes
def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    for per_vertex in (True, False):
        gdv, totals, st = g.graphlets(per_vertex=per_vertex)
        assert (gdv is None or gdv.shape == (0, 15)) and not totals.any() and st["iterations"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, capfd, monkeypatch, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    monkeypatch.setenv("GMX_GRAPHLETS_LOG", "1")
    for again in (False, True):
        capfd.readouterr()
        for induced in (True, False):
            gdv, totals, st = g.graphlets(induced=induced)
            assert gdv.shape == (V, 15) and not gdv.any() and not totals.any() and (st["vertices_reached"], st["edges_examined"], st["iterations"]) == (0, 0, 1)
            gdv, totals, st = g.graphlets(per_vertex=False, induced=induced)
            assert gdv is None and not totals.any() and st["iterations"] == 1
        assert "gmx graphlets" not in capfd.readouterr().err   # answered without a plan
        g.clustering()                                         # ... and again with the plan another entry built
        g.ktruss()


# ---- 2: named shapes, every way
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shapes(gmx, run, name):
    shape, closed = SHAPES[name]
    g = graph_of(gmx, shape)
    want = models_of(g)
    if closed is not None:
        assert want[True]["gdv"].tobytes() == closed[0].tobytes() and want[True]["totals"].tobytes() == closed[1].tobytes()
    every_way(run, g, want)
    every_way(run, g, want, [(True, True, {}), (False, True, {"no_order": 1})], cap=64, long=1)


# ---- 3: row-length boundaries
def wheel_path(n):
    """Vertex 0 joined to 1 .. n, which are joined in a path: t(e) = 2 on the inner spokes, 1 on the path's edges."""
    return n + 1, np.concatenate([np.zeros(n, np.int64), np.arange(1, n)]), np.concatenate([np.arange(1, n + 1), np.arange(2, n + 1)])


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_rows_at_the_boundaries_of_the_passes(gmx, run, n):
    g = graph_of(gmx, wheel_path(n))
    want = models_of(g)
    assert want[True]["triangles"] == n - 1 and want[True]["totals"][7] == n - 2
    ways = [(True, True, {}), (False, True, {"no_order": 1}), (True, True, {"plain": 1}), (True, False, {})]
    every_way(run, g, want, ways)
    for long_min in (63, 64, 128):   # the hub's row on either side of the cut into groups
        res = run(g, True, True, long=long_min)
        agrees(res, want[True])
        assert res[3]["long_rows"] == int(n > long_min)
        agrees(run(g, True, False, long=long_min, no_order=1, cap=64), want[False])


@pytest.fixture(scope="module")
def hub_and_clique(gmx):
    """Vertex 0 joined to 1 .. 5000, of which 1 .. 64 are a clique: under the identity order UP'(0) holds 5000 entries."""
    a, b = np.nonzero(np.triu(np.ones((64, 64), bool), 1))
    g = gmx.Graph.from_edges(5001, np.concatenate([np.zeros(5000, np.int64), a + 1]), np.concatenate([np.arange(1, 5001), b + 1]))
    return g, models_of(g)


def test_a_list_longer_than_a_waves_slice(gmx, run, hub_and_clique):
    g, want = hub_and_clique
    assert want[True]["triangles"] == comb(65, 3) and want[True]["totals"][8] == comb(65, 4)
    res = run(g, True, True, no_order=1)
    agrees(res, want[True])
    assert res[3]["memory"] > 0 and res[3]["staged"] > 0 and res[3]["long_rows"] == 1   # the fallback did run
    assert res[3]["memory"] == sum(1 for grp in range((5000 - 1 + 63) // 64) if 5000 - 64 * grp > 512)
    res = run(g, True, False, no_order=1, cap=1024)
    agrees(res, want[False])
    assert res[3]["memory"] == sum(1 for grp in range((5000 - 1 + 63) // 64) if 5000 - 64 * grp > 1024)
    res = run(g, True, True)   # under the degree order every list is short
    agrees(res, want[True])
    assert res[3]["memory"] == 0
    for ways in ([(True, True, {"plain": 1}), (False, True, {"no_order": 1, "plain": 1}), (True, False, {}), (False, False, {"no_order": 1})],):
        every_way(run, g, want, ways)
    agrees(run(g, True, True, cap=64, long=1), want[True])


# ---- 4: wide credits
def test_credits_past_two_to_the_sixteenth(gmx, run):
    """K257: every support is 255, a corner's share of one triangle 254, a vertex's orbit-12 count before the transform 3 C(256, 3)."""
    g = graph_of(gmx, clique(257))
    want = {True: {"gdv": clique_gdv(257)[0], "totals": clique_gdv(257)[1]}, False: {"gdv": clique_subgraph_gdv(257)[0], "totals": clique_subgraph_gdv(257)[1]}}
    for m in want.values():
        m.update(nonzero=257, triangles=comb(257, 3))
    assert want[False]["gdv"][0, 12] == 3 * comb(256, 3) > 1 << 16
    every_way(run, g, want, [(True, True, {}), (False, True, {}), (False, True, {"no_order": 1}), (True, True, {"plain": 1}), (False, False, {}), (True, False, {})])
    agrees(run(g, True, False, cap=64), want[False])   # lists of 65 .. 256 entries searched in memory


# ---- 5: a product that wraps
def test_a_binomial_whose_product_wraps(gmx, run):
    n = 3400000
    assert n * (n - 1) * (n - 2) > 1 << 64 and comb(n, 3) < 1 << 63
    g = graph_of(gmx, star(n))
    gdv, totals = star_gdv(n)
    res = run(g, True, True)
    assert res[0][0, 7] == comb(n, 3) and res[0][1, 6] == res[0][n, 6] == comb(n - 1, 2)   # the centre's o7 and the leaves' o6
    assert res[0].tobytes() == gdv.tobytes() and res[1].tobytes() == totals.tobytes() and res[3]["long_rows"] == 1
    assert res[1].tolist() == [n, comb(n, 2), 0, 0, comb(n, 3), 0, 0, 0, 0]
    for induced in (True, False):   # (a star's induced and subgraph counts are the same)
        assert run(g, False, induced)[1].tobytes() == totals.tobytes()


# ---- 6: RMAT against the models
RMATS = {"rmat10": (10, False, False), "rmat10p": (10, True, False), "rmat10s": (10, False, True), "rmat12": (12, False, False)}


@pytest.fixture(scope="module")
def rmats(gmx):
    out = {}
    for name, (scale, permute, sym) in RMATS.items():
        g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
        g = g.symmetrize() if sym else g
        out[name] = (g, models_of(g))
    return out


@pytest.mark.parametrize("name", sorted(RMATS))
def test_rmat_against_the_formulas(gmx, run, rmats, name):
    g, want = rmats[name]
    assert (want[True]["totals"] > 0).all()
    a = run(g, True, True)
    agrees(a, want[True])
    print("%s: %s, items %d staged + %d memory, long rows %d" % (name, dict(zip(NAMES, a[1].tolist())), a[3]["staged"], a[3]["memory"], a[3]["long_rows"]))
    every_way(run, g, want, EVERY_WAY[1:])
    agrees(run(g, True, True, cap=64, long=100), want[True])
    agrees(run(g, True, False, cap=64, long=100, no_order=1), want[False])


def test_rmat8_against_the_definition(gmx, run, golden):
    c = golden["cases"]["rmat8_noperm"]
    g = gmx.Graph.upload(c["begin"], c["node_idx"], flags=gmx.GMX_GRAPH_NO_REVERSE)
    d = graphlets_definition(256, c["begin"], c["node_idx"])
    for knobs in ({}, {"plain": 1}, {"no_order": 1}):
        gdv, totals, st, f = run(g, True, True, **knobs)
        assert gdv.tobytes() == d["gdv"].tobytes() and totals.tobytes() == d["totals"].tobytes()
    assert run(g, False, True)[1].tobytes() == d["totals"].tobytes()


# ---- 7: upload forms
@pytest.mark.parametrize("V,hub_edges", [(64, 200), (3000, 8000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    graphs = (gmx.Graph.upload(begin, idx, rb, ri, flags=0), gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS),
              gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE))
    want = {induced: graphlets_formulas(V, begin, idx, induced) for induced in (True, False)}   # on the rows as stored
    assert want[True]["totals"][2] > 0
    for g in graphs:
        every_way(run, g, want, [(True, True, {}), (False, True, {"no_order": 1}), (True, False, {}), (True, True, {"plain": 1})])


# ---- 8: one handle
def test_one_handle_with_the_rest_of_the_family(gmx, run, rmats, capfd, monkeypatch):
    make = lambda: gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    want = rmats["rmat10"][1]
    built = lambda r: tuple(r[3][k] for k in ("built", "adj_built", "groups_built", "squares_built", "kclique_built"))
    family = (("clustering", "GMX_LCC_LOG", lambda g: g.clustering()[:5]), ("ktruss", "GMX_KTRUSS_LOG", lambda g: g.ktruss()[:4]),
              ("squares", "GMX_SQUARES_LOG", lambda g: g.squares()[:2]), ("kclique", "GMX_KCLIQUE_LOG", lambda g: g.kclique(4)[:2]))

    def logged(g, name, knob, call):
        """(the result's bytes, the entry's log line) of a call."""
        monkeypatch.setenv(knob, "1")
        capfd.readouterr()
        got = tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in call(g))
        err = capfd.readouterr().err
        monkeypatch.delenv(knob)
        lines = [line for line in err.splitlines() if line.startswith("gmx %s:" % name)]
        assert len(lines) == 1, err
        return got, lines[0]

    # on handles of their own: the first call's bytes, the second call's line (nothing is built any more)
    alone = {}
    for name, knob, call in family:
        h = make()
        first = logged(h, name, knob, call)
        alone[name] = (first[0], logged(h, name, knob, call)[1])
    g = make()
    a = run(g)
    assert built(a) == (1, 1, 1, 1, 1)
    agrees(a, want[True])
    for name, knob, call in family:   # after graphlets: the same bytes, every part found, and then the very line of a warm call
        got, line = logged(g, name, knob, call)
        assert got == alone[name][0], name
        assert " built 0" in line and " adj_built 1" not in line and " classes_built 1" not in line, line
        assert logged(g, name, knob, call) == alone[name], name
    b = run(g, True, False)
    assert built(b) == (0, 0, 0, 0, 0)
    agrees(b, want[False])
    h = make()   # the other way round: graphlets finds what the four built
    for name, knob, call in family:
        assert logged(h, name, knob, call)[0] == alone[name][0]
    c = run(h)
    assert built(c) == (0, 0, 0, 0, 0)
    agrees(c, want[True])
    d = run(h, True, True, no_order=1)   # the other order: everything again
    assert built(d) == (1, 1, 1, 1, 1)
    agrees(d, want[True])
    assert built(run(h, False, True, no_order=1)) == (0, 0, 0, 0, 0)
    L = gmx.lib()
    used = None
    for again in (False, True):   # a second pass does not grow the workspace
        agrees(run(g), want[True])
        for name, knob, call in family:
            assert logged(g, name, knob, call)[0] == alone[name][0]
        agrees(run(g, False, False), want[False])
        agrees(run(g, True, True, plain=1), want[True])
        if again:
            assert L.gmx_workspace_bytes() == used
        used = L.gmx_workspace_bytes()
    assert used > 0


# ---- 9: the columns the family returns as well
def test_columns_agree_with_the_family(gmx, rmats):
    for name in ("rmat10s", "rmat12"):
        g = rmats[name][0]
        tri, deg = g.clustering()[:2]
        for induced in (True, False):
            gdv = g.graphlets(induced=induced)[0]
            assert gdv[:, 0].tobytes() == deg.astype(np.int64).tobytes() and gdv[:, 3].tobytes() == tri.tobytes()
        assert gdv[:, 8].tobytes() == g.squares()[0].tobytes() and gdv[:, 14].tobytes() == g.kclique(4)[0].tobytes()
        assert int(gdv[:, 8].sum()) == 4 * g.squares(per_vertex=False)[1]


# ---- 10: the driver
def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "graphlets")
    assert os.path.exists(exe), "bin/graphlets not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    m = graphlets_formulas(256, c["begin"], c["node_idx"])
    assert (m["totals"] > 0).all()
    top = int(np.argmax(m["gdv"][:, 14]))   # the lowest id with the largest count
    for line in ["%s = %d\n" % (n, t) for n, t in zip(NAMES, m["totals"].tolist())] + ["top = %d\n" % top]:
        assert line in out.stdout, (line, out.stdout)
