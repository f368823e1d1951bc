"""gmx_kcore on the device: core, layer and max_core byte for byte against the host model of the schedule
(test_kcore_host.kcore_model), the statistics and the log line's levels, rounds and scanned with them; the shapes at which
the level scan, the round tile, the tail workgroup and the hand-over between them can go wrong; every mode and knob; the
symmetric graph against networkx; unsorted multigraphs; the graph without a reverse CSR; the driver."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_gpu_scc import _shape
from test_kcore_host import MODES, kcore_model, transpose
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_KCORE_TAIL", "GMX_KCORE_LOG", "GMX_KCORE_PHASES")
LOG_FIELDS = ("V", "E", "mode", "reverse", "levels", "rounds", "scanned", "grid_rounds", "tail_rounds", "slots", "max_core", "top")
LOG = re.compile(r"gmx kcore: " + " ".join(r"%s (\d+)" % f for f in LOG_FIELDS) + r"\n")
TAILS = (0, None, 1 << 30)   # never, the default, always


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
    def call(g, mode, tail=None):
        """One call with GMX_KCORE_LOG: (core, layer, max_core, stats, the log line's fields), the line checked against them."""
        monkeypatch.setenv("GMX_KCORE_LOG", "1")
        if tail is None:
            monkeypatch.delenv("GMX_KCORE_TAIL", raising=False)
        else:
            monkeypatch.setenv("GMX_KCORE_TAIL", str(tail))
        capfd.readouterr()
        core, layer, k, st = g.kcore(mode, layers=True)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = dict(zip(LOG_FIELDS, map(int, m.groups())))
        assert f["V"] == g.V and f["E"] == g.E and f["mode"] == MODES.index(mode)
        assert f["grid_rounds"] + f["tail_rounds"] == f["rounds"] == st["iterations"]
        assert f["slots"] == st["edges_examined"] and f["top"] == st["vertices_reached"] and f["max_core"] == k
        assert core.dtype == np.int32 and layer.dtype == np.int32
        if tail == 0:
            assert f["tail_rounds"] == 0
        if tail == 1 << 30:
            assert f["grid_rounds"] == 0
        return core, layer, k, st, f
    return call


def agrees(res, want, E, mode):
    core, layer, k, st, f = res
    assert core.tobytes() == want["core"].tobytes()
    assert layer.tobytes() == want["layer"].tobytes()
    assert k == want["max_core"] and st["vertices_reached"] == want["top"]
    assert st["iterations"] == want["rounds"]
    assert st["edges_examined"] == E * (2 if mode == "both" else 1) == want["slots"]
    assert (f["levels"], f["rounds"], f["scanned"]) == (want["levels"], want["rounds"], want["scanned"])


def model_of(g, mode):
    begin, idx, _, _ = g.download(reverse=False)
    return kcore_model(g.V, begin, idx, mode)


def sym(s, d):
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    return np.concatenate([s, d]), np.concatenate([d, s])


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    core, layer, k, st = g.kcore("in", layers=True)
    assert len(core) == 0 and len(layer) == 0 and k == 0 and st["iterations"] == 0


@pytest.mark.parametrize("name", ["one_vertex_self_loop", "no_edges", "self_loops_only"])
@pytest.mark.parametrize("mode", MODES)
def test_trivial_shapes_are_one_round_of_core_zero(gmx, run, name, mode):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    for tail in TAILS:
        res = run(g, mode, tail)
        agrees(res, model_of(g, mode), g.E, mode)
        assert not res[0].any() and not res[1].any() and res[2] == 0 and res[3]["iterations"] == 1 and res[3]["vertices_reached"] == V


def path_expectation(order):
    """The symmetric path through the vertices `order`: both ends go in every round of the one level."""
    P = len(order)
    layer = np.empty(P, np.int32)
    layer[order] = np.minimum(np.arange(P), P - 1 - np.arange(P))
    return {"core": np.ones(P, np.int32), "layer": layer, "levels": 1, "rounds": P // 2, "scanned": P, "max_core": 1, "top": P, "slots": 2 * (P - 1)}


@pytest.mark.parametrize("P,tail,permuted", [(1 << 16, None, False), (1 << 16, None, True), (1 << 12, 0, False), (1 << 12, 1 << 30, True)])
def test_path_is_one_level_of_half_as_many_rounds(gmx, run, P, tail, permuted):
    order = np.random.default_rng(3).permutation(P) if permuted else np.arange(P)
    g = gmx.Graph.from_edges(P, *sym(order[:-1], order[1:]))
    want = path_expectation(order)
    if P == 1 << 12:
        m = model_of(g, "in")
        assert all(np.array_equal(m[f], want[f]) for f in ("core", "layer")) and all(m[f] == want[f] for f in ("levels", "rounds", "scanned", "top"))
    res = run(g, "in", tail)
    agrees(res, want, g.E, "in")
    if tail is None:
        assert res[4]["tail_rounds"] >= P // 2 - 1   # the round loop ran in the tail workgroup


def test_cycle_and_triangle_chain(gmx, run):
    P = 1 << 16
    g = gmx.Graph.from_edges(P, *sym(np.arange(P), (np.arange(P) + 1) % P))
    for mode in MODES:
        res = run(g, mode)
        agrees(res, model_of(g, mode), g.E, mode)
        assert res[3]["iterations"] == 1 and np.all(res[0] == (4 if mode == "both" else 2))
    V, s, d = _shape("triangle_chain")
    g = gmx.Graph.from_edges(V, s, d)
    for mode in MODES:
        for tail in TAILS:
            agrees(run(g, mode, tail), model_of(g, mode), g.E, mode)


@pytest.fixture(scope="module")
def stars(gmx):
    n = 60000
    leaves, hub = np.arange(1, n + 1), np.zeros(n, np.int64)
    out = {}
    for name, (s, d) in (("in_star", (leaves, hub)), ("out_star", (hub, leaves))):
        g = gmx.Graph.from_edges(n + 1, s, d)
        out[name] = (g, {mode: model_of(g, mode) for mode in MODES})
    return out


@pytest.mark.parametrize("name", ["in_star", "out_star"])
@pytest.mark.parametrize("mode", MODES)
def test_stars(gmx, run, stars, name, mode):
    """in-star, mode in: 60000 decrements of one word in one round and one append; out-star, mode in: one row of 60000 slots
    over ~30 tiles and 60000 appends."""
    g, want = stars[name]
    for tail in TAILS:
        res = run(g, mode, tail)
        agrees(res, want[mode], g.E, mode)
    core, layer = res[0], res[1]
    if (name, mode) in (("in_star", "in"), ("out_star", "out")):   # the leaves go first, the hub falls to 0 behind them
        assert core[0] == 0 and layer[0] == 1 and not layer[1:].any() and res[3]["iterations"] == 2
    if (name, mode) in (("out_star", "in"), ("in_star", "out")):   # the hub goes first, all leaves in the next round
        assert not core.any() and layer[0] == 0 and np.all(layer[1:] == 1)
    if mode == "both":
        assert np.all(core == 1) and not layer[1:].any() and layer[0] == 1


def test_clique_with_a_pendant_path_jumps_from_level_1_to_63(gmx, run):
    a, b = np.nonzero(np.triu(np.ones((64, 64), bool), 1))
    chain = np.arange(63, 64 + 1000)
    g = gmx.Graph.from_edges(64 + 1000, *sym(np.concatenate([a, chain[:-1]]), np.concatenate([b, chain[1:]])))
    for tail in TAILS:
        res = run(g, "in", tail)
        agrees(res, model_of(g, "in"), g.E, "in")
        assert res[4]["levels"] == 2 and res[2] == 63 and res[3]["vertices_reached"] == 64 and res[3]["iterations"] == 1001
        assert np.all(res[0][:64] == 63) and np.all(res[0][64:] == 1)


def test_parallel_slots_count_again_and_self_loops_do_not(gmx, run):
    n = 5000
    s = np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64), [0, 0, 1]])
    d = np.concatenate([np.ones(n, np.int64), np.zeros(n, np.int64), [0, 0, 1]])
    g = gmx.Graph.from_edges(2, s, d)
    for mode, k in (("in", n), ("out", n), ("both", 2 * n)):
        for tail in TAILS:
            res = run(g, mode, tail)
            agrees(res, model_of(g, mode), g.E, mode)
            assert res[0].tolist() == [k, k] and res[1].tolist() == [0, 0]


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (150000, 400000)])
def test_unsorted_multigraph_uploaded_verbatim(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)
    for mode in MODES:
        want = kcore_model(V, begin, idx, mode)
        res = run(g, mode)
        agrees(res, want, g.E, mode)
        res2 = run(sorted_g, mode)
        agrees(res2, want, g.E, mode)
        assert res2[0].tobytes() == res[0].tobytes() and res2[1].tobytes() == res[1].tobytes()


@pytest.mark.parametrize("scale,permute", [(s, p) for s in (8, 10, 12, 14) for p in (False, True)] + [(16, False)])
def test_rmat_against_the_model_under_every_knob(gmx, run, scale, permute):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
    begin, idx, _, _ = g.download(reverse=False)
    for mode in MODES:
        want = kcore_model(g.V, begin, idx, mode)
        splits = []
        for tail in TAILS:
            res = run(g, mode, tail)
            agrees(res, want, g.E, mode)
            splits.append((res[4]["grid_rounds"], res[4]["tail_rounds"]))
        print("RMAT-%d%s %s: levels %d rounds %d scanned/V %.2f max_core %d grid/tail rounds %s" % (
            scale, "p" if permute else "", mode, want["levels"], want["rounds"], want["scanned"] / g.V, want["max_core"], splits))
        assert want["levels"] > 2 and want["rounds"] > want["levels"]


def test_symmetrised_rmat_against_networkx(gmx, run):
    nx = pytest.importorskip("networkx")
    for scale, onion in ((14, False), (12, True)):
        g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, False).symmetrize()
        begin, idx, _, _ = g.download(reverse=False)
        rows = np.repeat(np.arange(g.V), np.diff(begin))
        G = nx.Graph()
        G.add_nodes_from(range(g.V))
        G.add_edges_from(zip(rows.tolist(), idx.tolist()))
        assert 2 * G.number_of_edges() == g.E   # symmetric and simple
        ref = nx.onion_layers(G) if onion else nx.core_number(G)
        want = np.array([ref[v] for v in range(g.V)], np.int32) - (1 if onion else 0)
        i, o, both = (run(g, mode) for mode in MODES)
        assert np.array_equal(i[1] if onion else i[0], want)
        assert i[0].tobytes() == o[0].tobytes() and i[1].tobytes() == o[1].tobytes()
        assert np.array_equal(both[0], 2 * i[0]) and both[1].tobytes() == i[1].tobytes()
        assert both[3]["edges_examined"] == 2 * g.E and i[3]["edges_examined"] == g.E


def test_no_reverse_csr(gmx, run):
    g = gmx.Graph.rmat(1 << 14, 16 << 14, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, rb, ri = g.download()
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    a, b = run(g, "in"), run(h, "in")
    agrees(b, kcore_model(g.V, begin, idx, "in"), g.E, "in")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[4]["reverse"] == 1 and b[4]["reverse"] == 0
    for mode in ("out", "both"):
        with pytest.raises(gmx.GmxError, match="gmx status -5"):   # GMX_ERR_STATE
            h.kcore(mode)
    # out on G is in on the transpose
    t = gmx.Graph.upload(rb, ri, begin, idx)
    o, ti = run(g, "out"), run(t, "in")
    assert o[0].tobytes() == ti[0].tobytes() and o[1].tobytes() == ti[1].tobytes()
    tb, tidx = transpose(g.V, begin, idx)
    agrees(o, kcore_model(g.V, tb, tidx, "in") | {"slots": g.E}, g.E, "out")


def test_repeatable_and_hop_dist_unchanged(gmx):
    g = gmx.Graph.rmat(1 << 18, 16 << 18, 1997, 0.57, 0.19, 0.19, False)
    roots = [0, 1, 777, 123456]
    before = [g.hop_dist(r)[0] for r in roots]
    c1, l1, k1, s1 = g.kcore("in", layers=True)
    c2, l2, k2, s2 = g.kcore("in", layers=True)
    assert k1 == k2 > 0 and c1.tobytes() == c2.tobytes() and l1.tobytes() == l2.tobytes()
    for f in ("iterations", "vertices_reached", "edges_examined"):
        assert s1[f] == s2[f] > 0
    assert s1["edges_examined"] == g.E and s1["kernel_ms"] > 0
    assert s1["vertices_reached"] == int((c1 == k1).sum()) and c1.max() == k1 and s1["iterations"] == int(l1.max()) + 1
    c3, k3, s3 = g.kcore("in")
    assert c3.tobytes() == c1.tobytes() and k3 == k1 and s3["iterations"] == s1["iterations"]
    after = [g.hop_dist(r)[0] for r in roots]
    for b, a in zip(before, after):
        assert np.array_equal(a, b)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "kcore")
    assert os.path.exists(exe), "bin/kcore not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    for mode in MODES:
        out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null", mode], stdout=subprocess.PIPE, text=True,
                             timeout=120, cwd=ROOT)
        assert out.returncode == 0, out.stdout
        m = kcore_model(256, c["begin"], c["node_idx"], mode)
        for line in ("max_core = %d\n" % m["max_core"], "max_core_size = %d\n" % m["top"], "rounds = %d\n" % m["rounds"]):
            assert line in out.stdout, out.stdout
    out = subprocess.run([exe, "RMAT:12", "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    core, k, st = g.kcore()
    for line in ("max_core = %d\n" % k, "max_core_size = %d\n" % st["vertices_reached"], "rounds = %d\n" % st["iterations"]):
        assert line in out.stdout, out.stdout
