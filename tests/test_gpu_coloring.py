"""gmx_coloring on the device: color and depth byte for byte against the one-thread first fit of the downloaded CSR
(test_coloring_host.greedy_model), num_colors, the statistics and every field of the log line with them; the shapes at
which the three mex regimes, the release tile, the tail workgroup and the hand-over between them can go wrong; every knob;
unsorted multigraphs; the graph without a reverse CSR; the driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_coloring_host import certificate, clique_upper, crown, greedy_model
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_COLOR_TAIL", "GMX_COLOR_WAVE_MIN", "GMX_COLOR_BLOCK_MIN", "GMX_COLOR_WINDOW", "GMX_COLOR_LOG", "GMX_COLOR_PHASES")
LOG_FIELDS = ("V", "E", "user_prio", "rounds", "grid_rounds", "tail_rounds", "group", "wave", "block", "passes", "colors", "class0")
LOG = re.compile(r"gmx color: " + " ".join(r"%s (\d+)" % f for f in LOG_FIELDS) + r"\n")
TAILS = (0, None, 1 << 30)   # never, the default, always
HUGE = str(1 << 30)
WAVE_MIN, BLOCK_MIN, WINDOW = 65, 256, 1 << 18   # the defaults
BLOCK_MAX = 8192                               # GMX_COLOR_BLOCK_MIN is clamped to the bits of a wave's LDS slice
REGIMES = {"default": {}, "wave": {"GMX_COLOR_WAVE_MIN": "1", "GMX_COLOR_BLOCK_MIN": HUGE}, "block": {"GMX_COLOR_BLOCK_MIN": "1"}}


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
    def call(g, prio=None, tail=None, env=None):
        """One call with GMX_COLOR_LOG: (color, depth, num_colors, stats, the log line's fields), the line checked against them."""
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMX_COLOR_LOG", "1")
        if tail is not None:
            monkeypatch.setenv("GMX_COLOR_TAIL", str(tail))
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        color, depth, n, st = g.coloring(prio, depth=True)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = dict(zip(LOG_FIELDS, map(int, m.groups())))
        f["env"] = dict(env or {})
        assert f["V"] == g.V and f["E"] == g.E and f["user_prio"] == (prio is not None)
        assert f["grid_rounds"] + f["tail_rounds"] == f["rounds"] == st["iterations"]
        assert f["group"] + f["wave"] + f["block"] == g.V
        assert f["colors"] == n and f["class0"] == st["vertices_reached"]
        assert color.dtype == np.int32 and depth.dtype == np.int32
        if tail == 0:
            assert f["tail_rounds"] == 0
        if tail == 1 << 30:
            assert f["grid_rounds"] == 0
        return color, depth, n, st, f
    return call


def agrees(res, want, E):
    color, depth, n, st, f = res
    assert color.tobytes() == want["color"].tobytes()
    assert depth.tobytes() == want["depth"].tobytes()
    assert n == want["num_colors"] and st["vertices_reached"] == want["class0"]
    assert st["iterations"] == want["rounds"] and st["edges_examined"] == 6 * E
    # the regimes by row length under the call's thresholds, and the block regime's extra passes under its window
    wave_min = min(int(f["env"].get("GMX_COLOR_WAVE_MIN", WAVE_MIN)), WAVE_MIN)
    block_min = min(int(f["env"].get("GMX_COLOR_BLOCK_MIN", BLOCK_MIN)), BLOCK_MAX)
    window = int(f["env"].get("GMX_COLOR_WINDOW", WINDOW))
    L = want["L"]
    block = L >= block_min
    wave = ~block & (L >= wave_min)
    assert (f["group"], f["wave"], f["block"]) == (int((~block & ~wave).sum()), int(wave.sum()), int(block.sum()))
    assert f["passes"] == int((want["color"][block].astype(np.int64) // window).sum())


def model_of(g, prio=None):
    begin, idx, _, _ = g.download(reverse=False)
    return greedy_model(g.V, begin, idx, prio)


def zeros(g):
    return np.zeros(g.V, np.int32)


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    color, depth, n, st = g.coloring(depth=True)
    assert len(color) == 0 and len(depth) == 0 and n == 0 and st["iterations"] == 0 and st["vertices_reached"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_one_round_of_colour_zero(gmx, run, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    for prio in (None, zeros(g)):
        want = model_of(g, prio)
        for tail in TAILS:
            for env in REGIMES.values():
                res = run(g, prio, tail, env)
                agrees(res, want, g.E)
                assert not res[0].any() and not res[1].any() and res[2] == 1 and res[3]["iterations"] == 1 and res[3]["vertices_reached"] == V


@pytest.mark.parametrize("P,tail,permuted", [(1 << 16, None, False), (1 << 16, None, True), (1 << 12, 0, False), (1 << 12, 0, True),
                                             (1 << 12, 1 << 30, False), (1 << 12, 1 << 30, True)])
def test_path_in_id_order(gmx, run, P, tail, permuted):
    """Plain: P rounds of one vertex, colours alternate -- the tail's round loop, or the hand-over every round.  Permuted: the
    ids along the path are shuffled, the order stays the id order."""
    at = np.random.default_rng(3).permutation(P) if permuted else np.arange(P)
    g = gmx.Graph.from_edges(P, at[:-1], at[1:])
    want = model_of(g, zeros(g))
    if not permuted:
        assert np.array_equal(want["color"], np.arange(P) % 2) and want["rounds"] == P
    res = run(g, zeros(g), tail)
    agrees(res, want, g.E)
    if tail is None and not permuted:
        assert res[4]["tail_rounds"] == P   # the round loop ran in the tail workgroup


@pytest.fixture(scope="module")
def k300(gmx):
    V, s, d = clique_upper(300)
    g = gmx.Graph.from_edges(V, s, d)
    prios = {"id": np.zeros(V, np.int32), "reversed": np.arange(V, dtype=np.int32)}
    return g, prios, {k: model_of(g, p) for k, p in prios.items()}


@pytest.mark.parametrize("order", ["id", "reversed"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_clique_stored_one_way(gmx, run, k300, order, regime):
    """K_300, upper triangle only: in id order the earlier neighbours come from the in-rows alone, reversed from the out-rows
    alone; color is the rank, 300 rounds."""
    g, prios, want = k300
    w = want[order]
    assert np.array_equal(w["color"], np.arange(300) if order == "id" else 299 - np.arange(300)) and w["rounds"] == 300
    for tail in TAILS:
        agrees(run(g, prios[order], tail, REGIMES[regime]), w, g.E)
    if regime == "block":
        for tail in (0, 1 << 30):
            res = run(g, prios[order], tail, dict(REGIMES["block"], GMX_COLOR_WINDOW="64"))
            agrees(res, w, g.E)
            assert res[4]["passes"] == 560 == w["passes"](64)
    if regime == "default":
        assert run(g, prios[order], None)[4]["block"] == 300   # every row has 299 slots


@pytest.mark.parametrize("order", ["id", "reversed"])
def test_group_regime_with_a_full_mask(gmx, run, order):
    """K_65: every row has 64 slots, the longest the group regime takes, and the last vertex sees all 64 colours of the mask."""
    V, s, d = clique_upper(65)
    g = gmx.Graph.from_edges(V, s, d)
    prio = np.zeros(V, np.int32) if order == "id" else np.arange(V, dtype=np.int32)
    want = model_of(g, prio)
    assert want["num_colors"] == 65
    for tail in TAILS:
        res = run(g, prio, tail)
        agrees(res, want, g.E)
        assert res[4]["group"] == 65 and res[0].max() == 64


@pytest.mark.parametrize("regime", list(REGIMES) + ["block64"])
def test_a_high_colour_does_not_alias_a_low_one(gmx, run, regime):
    """K_80 in id order plus vertex 80 joined to 65 and 0: colour 65 must fall outside every bitmap, not onto bit 1."""
    V, s, d = clique_upper(80)
    g = gmx.Graph.from_edges(81, np.concatenate([s, [65, 0]]), np.concatenate([d, [80, 80]]))
    want = model_of(g, zeros(g))
    assert want["npred"][80] == 2 and want["color"][80] == 1 and want["rounds"] == 80
    env = dict(REGIMES["block"], GMX_COLOR_WINDOW="64") if regime == "block64" else REGIMES[regime]
    for tail in TAILS:
        res = run(g, zeros(g), tail, env)
        agrees(res, want, g.E)
        assert res[0][80] == 1


@pytest.mark.parametrize("regime", list(REGIMES))
def test_crown_graph_needs_forty_colours(gmx, run, regime):
    V, s, d = crown(40)
    g = gmx.Graph.from_edges(V, s, d)
    want = model_of(g, zeros(g))
    assert want["num_colors"] == 40
    for tail in TAILS:
        agrees(run(g, zeros(g), tail, REGIMES[regime]), want, g.E)
    agrees(run(g, None, None, REGIMES[regime]), model_of(g), g.E)


@pytest.fixture(scope="module")
def stars(gmx):
    n = 1 << 17
    leaves, hub = np.arange(n), np.full(n, n, np.int64)   # the hub holds the highest id
    out = {}
    for name, (s, d) in (("star_out", (hub, leaves)), ("star_in", (leaves, hub)),
                         ("star_both", (np.concatenate([hub, leaves]), np.concatenate([leaves, hub])))):
        g = gmx.Graph.from_edges(n + 1, s, d)
        out[name] = (g, model_of(g), model_of(g, np.zeros(n + 1, np.int32)))
    return out


@pytest.mark.parametrize("name", ["star_out", "star_in", "star_both"])
def test_stars(gmx, run, stars, name):
    """Default order: the hub is first, every leaf takes colour 1 in round 1.  Id order with the hub last: 131072 (262144)
    earlier slots, colour 1 in the second round -- the block regime at its default window, and with a window of 64 bits."""
    g, by_degree, by_id = stars[name]
    n = g.V - 1
    for tail in TAILS:
        res = run(g, None, tail)
        agrees(res, by_degree, g.E)
        assert res[0][n] == 0 and np.all(res[0][:n] == 1) and res[3]["iterations"] == 2 and res[3]["vertices_reached"] == 1
        for env in ({}, {"GMX_COLOR_WINDOW": "64"}):
            res = run(g, zeros(g), tail, env)
            agrees(res, by_id, g.E)
            assert by_id["npred"][n] == g.E and res[0][n] == 1 and not res[0][:n].any() and res[3]["iterations"] == 2
            assert res[4]["block"] == 1 and res[4]["passes"] == 0


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (150000, 400000)])
def test_unsorted_multigraph_uploaded_verbatim(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)
    rng = np.random.default_rng(5)
    for prio in (None, np.zeros(V, np.int32), rng.integers(0, 50, V).astype(np.int32)):
        want = greedy_model(V, begin, idx, prio)
        res = run(g, prio)
        agrees(res, want, g.E)
        res2 = run(sorted_g, prio)
        agrees(res2, want, g.E)
        assert res2[0].tobytes() == res[0].tobytes() and res2[1].tobytes() == res[1].tobytes()


@pytest.fixture(scope="module")
def rmats(gmx):
    out = {}
    rng = np.random.default_rng(6)
    for name, permute, symmetrize in (("plain", False, False), ("permuted", True, False), ("symmetrised", False, True)):
        g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, permute)
        if symmetrize:
            g = g.symmetrize()
        prios = {"degree": None, "id": np.zeros(g.V, np.int32), "random": rng.integers(0, 50, g.V).astype(np.int32)}
        out[name] = (g, prios, {k: model_of(g, p) for k, p in prios.items()})
    return out


@pytest.mark.parametrize("name", ["plain", "permuted", "symmetrised"])
@pytest.mark.parametrize("order", ["degree", "id", "random"])
def test_rmat_against_the_model_under_every_knob(gmx, run, rmats, name, order):
    g, prios, want = rmats[name]
    w = want[order]
    splits = []
    for regime, env in REGIMES.items():
        for tail in TAILS:
            res = run(g, prios[order], tail, env)
            agrees(res, w, g.E)
            splits.append((res[4]["grid_rounds"], res[4]["tail_rounds"]))
    res = run(g, prios[order], None, dict(REGIMES["block"], GMX_COLOR_WINDOW="64"))
    agrees(res, w, g.E)
    print("RMAT-12 %s %s: rounds %d colors %d class0 %d regimes %s grid/tail rounds %s" % (
        name, order, w["rounds"], w["num_colors"], w["class0"], (res[4]["group"], res[4]["wave"], res[4]["block"]), splits[:3]))
    assert w["rounds"] > 10 and w["num_colors"] > 5
    if name == "symmetrised" and order == "id":   # one direction only gives the same bytes as the symmetrised form
        assert w["color"].tobytes() == rmats["plain"][2]["id"]["color"].tobytes() and w["depth"].tobytes() == rmats["plain"][2]["id"]["depth"].tobytes()


def test_certificate_at_rmat16(gmx, run):
    g = gmx.Graph.rmat(1 << 16, 16 << 16, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g.download(reverse=False)
    res = run(g)
    certificate(g.V, begin, idx, res[0], res[2])
    agrees(res, greedy_model(g.V, begin, idx), g.E)
    assert res[3]["vertices_reached"] == int((res[0] == 0).sum()) and res[3]["iterations"] == int(res[1].max()) + 1 and res[3]["kernel_ms"] > 0


def test_errors(gmx):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g.download()
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    with pytest.raises(gmx.GmxError, match="gmx status -5"):   # GMX_ERR_STATE
        h.coloring()
    with pytest.raises(ValueError):
        g.coloring(np.zeros(g.V + 1, np.int32))
    L = gmx.lib()
    n = C.c_int32(0)
    color = np.zeros(g.V, np.int32)
    assert L.gmx_coloring(g._h, None, None, None, C.byref(n), None) == -1   # GMX_ERR_ARG
    assert L.gmx_coloring(None, None, color.ctypes.data, None, None, None) == -1
    assert L.gmx_coloring(g._h, None, color.ctypes.data, None, None, None) == 0   # depth, num_colors and stats may be NULL
    assert color.tobytes() == g.coloring()[0].tobytes()


def test_runs_are_repeatable(gmx):
    g = gmx.Graph.rmat(1 << 16, 16 << 16, 1997, 0.57, 0.19, 0.19, True)
    c1, d1, n1, s1 = g.coloring(depth=True)
    c2, d2, n2, s2 = g.coloring(depth=True)
    assert n1 == n2 > 0 and c1.tobytes() == c2.tobytes() and d1.tobytes() == d2.tobytes()
    for f in ("iterations", "vertices_reached", "edges_examined"):
        assert s1[f] == s2[f] > 0
    c3, n3, s3 = g.coloring()
    assert c3.tobytes() == c1.tobytes() and n3 == n1 and s3["iterations"] == s1["iterations"]


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "coloring")
    assert os.path.exists(exe), "bin/coloring not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    for order in ("degree", "id"):
        out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null", order], stdout=subprocess.PIPE, text=True,
                             timeout=120, cwd=ROOT)
        assert out.returncode == 0, out.stdout
        m = greedy_model(256, c["begin"], c["node_idx"], None if order == "degree" else np.zeros(256, np.int32))
        for line in ("num_colors = %d\n" % m["num_colors"], "independent_set = %d\n" % m["class0"], "rounds = %d\n" % m["rounds"]):
            assert line in out.stdout, out.stdout
