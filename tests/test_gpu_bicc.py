"""gmx_biconnected on the device: bridge, artic, block and tecc byte for byte against the host oracles (bicc_model: the
definitions up to 64 vertices, Hopcroft-Tarjan above), the counts, the statistics and the log line with them; every shape
under every knob; the forest and the walks' work against the schedule model; both upload forms; the driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from bicc_model import csr_from_edges, definition_oracle, forest_model, hopcroft_tarjan, slot_ends
from conftest import GOLD, ROOT
from test_bicc_host import ARRAYS, SHAPES, same
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_BICC_TAIL", "GMX_BICC_SKIP", "GMX_BICC_WALKS", "GMX_BICC_LOG", "GMX_BICC_PHASES")
FIELDS = ("V", "E", "levels", "roots", "tree", "walks", "steps", "jumps", "links", "grid_levels", "tail_levels", "blocks", "bridges", "artic", "tecc")
LOG = re.compile("gmx bicc: " + " ".join(r"%s (?P<%s>-?\d+)" % (f, f) for f in FIELDS) + "\n")
MATRIX = [dict(skip=s, walks=w, **t) for s in (0, 1) for w in (0, 64, 256) for t in ({"tail": 0}, {})]


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
        """One call with GMX_BICC_LOG and the knobs given (skip=0, walks=64, tail=0; the others unset): the results as the
        oracles name them, the stats and the log line's fields, the line checked against the results."""
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMX_BICC_LOG", "1")
        for k, v in knobs.items():
            monkeypatch.setenv("GMX_BICC_" + k.upper(), str(v))
        capfd.readouterr()
        bridge, artic, block, tecc, nblocks, nbridges, nartic, ntecc, st = g.biconnected()
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {k: int(v) for k, v in m.groupdict().items()}
        assert bridge.dtype == bool and artic.dtype == bool and block.dtype == np.int32 and tecc.dtype == np.int32
        assert (len(bridge), len(artic), len(block), len(tecc)) == (g.E, g.V, g.E, g.V)
        assert (f["V"], f["E"]) == (g.V, g.E)
        assert f["grid_levels"] + f["tail_levels"] == f["levels"] == st["iterations"]
        assert f["tree"] == st["vertices_reached"] == g.V - f["roots"] and f["steps"] == st["edges_examined"]
        assert (f["blocks"], f["bridges"], f["artic"], f["tecc"]) == (nblocks, nbridges, nartic, ntecc)
        assert f["steps"] >= f["walks"] and f["jumps"] <= f["steps"] and f["links"] <= f["steps"]
        if knobs.get("tail") == 0:
            assert f["tail_levels"] == 0
        if knobs.get("skip") == 0:
            assert f["jumps"] == 0
        assert st["kernel_ms"] > 0 and st["d2h_ms"] > 0 and st["h2d_ms"] == 0
        return {"bridge": bridge.astype(np.uint8), "artic": artic.astype(np.uint8), "block": block, "tecc": tecc, "num_blocks": nblocks,
                "num_bridges": nbridges, "num_artic": nartic, "num_tecc": ntecc, "stats": st, "log": f}
    return call


def oracle_of(g):
    """(the oracle's results, the schedule model) on the graph's stored forward CSR: its slots are the uploaded slots of a
    graph built from an edge list or on the device."""
    begin, idx, _, _ = g.download(reverse=False)
    want = hopcroft_tarjan(g.V, begin, idx)
    if g.V <= 64:
        same(want, definition_oracle(g.V, begin, idx))
    return want, forest_model(g.V, begin, idx)


def agrees(res, want, model=None):
    for k in ARRAYS:
        assert res[k].tobytes() == want[k].tobytes(), k
    for k in ("num_blocks", "num_bridges", "num_artic", "num_tecc"):
        assert res[k] == want[k], k
    if model is not None:
        f = res["log"]
        for k in ("levels", "roots", "tree", "walks"):
            assert f[k] == model[k], k


def check_all_knobs(run, g, want, model):
    """Every combination of the knobs gives the same bytes; without jumps the walks' work is the model's, exactly."""
    steps = {}
    for knobs in MATRIX:
        res = run(g, **knobs)
        agrees(res, want, model)
        if knobs["skip"] == 0:
            assert res["log"]["steps"] == model["steps"], knobs
        steps[tuple(sorted(knobs.items()))] = res["log"]["steps"]
    return steps


# ---- arguments and states
def test_null_graph_and_null_outputs(gmx, run):
    L = gmx.lib()
    assert L.gmx_biconnected(None, None, None, None, None, None, None, None, None, None) == -1   # GMX_ERR_ARG
    V, s, d = SHAPES["two_k5"]()
    g = gmx.Graph.from_edges(V, s, d)
    assert L.gmx_biconnected(g._h, None, None, None, None, None, None, None, None, None) == 0    # everything may be NULL
    full = g.biconnected()
    for i in range(4):   # one array at a time: the others are neither built nor downloaded
        ask = [j == i for j in range(4)]
        got = g.biconnected(*ask)
        assert all(got[j] is None for j in range(4) if j != i)
        assert got[i].tobytes() == full[i].tobytes() and got[4:8] == full[4:8]
    n = C.c_int64(-1)
    for pos in range(4):   # one count at a time, no array
        args = [None] * 4
        args[pos] = C.byref(n)
        assert L.gmx_biconnected(g._h, None, None, None, None, *args, None) == 0
        assert n.value == full[4 + pos]


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    bridge, artic, block, tecc, *counts, st = g.biconnected()
    assert (len(bridge), len(artic), len(block), len(tecc)) == (0, 0, 0, 0) and counts == [0, 0, 0, 0]
    assert st["iterations"] == 0 and st["edges_examined"] == 0


def test_no_edges(gmx, run):
    g = gmx.Graph.from_edges(1000, [], [])
    res = run(g)
    assert (res["num_blocks"], res["num_bridges"], res["num_artic"], res["num_tecc"]) == (0, 0, 0, 1000)
    assert np.array_equal(res["tecc"], np.arange(1000)) and not res["artic"].any()
    assert res["log"]["levels"] == 1 and res["log"]["roots"] == 1000 and res["log"]["walks"] == 0


def test_needs_the_reverse_csr(gmx):
    V, s, d = SHAPES["two_k5"]()
    begin, idx = csr_from_edges(V, s, d)
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    with pytest.raises(gmx.GmxError, match="gmx status -5"):   # GMX_ERR_STATE
        h.biconnected()


# ---- shapes
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_under_every_knob(gmx, run, name):
    V, s, d = SHAPES[name]()
    g = gmx.Graph.from_edges(V, s, d)
    want, model = oracle_of(g)
    check_all_knobs(run, g, want, model)
    res = run(g)
    comp, ncomp, _ = g.wcc()
    assert res["num_tecc"] - ncomp == res["num_bridges"] and ncomp == model["roots"]
    if name == "path_chords":
        assert (res["num_bridges"], res["num_blocks"]) == (9, 10)
    if name == "cycle4096":
        assert res["log"]["levels"] == 2049 and res["log"]["tail_levels"] == 2049 and run(g, tail=0)["log"]["grid_levels"] == 2049
    if name == "star":   # the hub's row is longer than a merge-path tile
        assert np.diff(g.download(reverse=False)[0]).max() >= 3000 > 2048
    if name == "union2000":
        assert model["roots"] >= 2000


def test_bowtie_root_rule_and_child_rule(gmx, run):
    """The shared vertex as the forest's root (its children span two classes) and as a non-root (a child of another class)."""
    for name, cut in (("bowtie_low", 0), ("bowtie_high", 4)):
        V, s, d = SHAPES[name]()
        res = run(gmx.Graph.from_edges(V, s, d))
        assert np.flatnonzero(res["artic"]).tolist() == [cut] and res["num_blocks"] == 2 and res["num_bridges"] == 0


@pytest.fixture(scope="module")
def rmats(gmx):
    """RMAT 8 / 10 / 12 / 14 plain, permuted and symmetrised, each with its oracle and model (computed once)."""
    out = {}
    for scale in (8, 10, 12, 14):
        for form in ("plain", "permuted", "symmetrised"):
            g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, form == "permuted")
            if form == "symmetrised":
                g = g.symmetrize()
            out[scale, form] = (g,) + oracle_of(g)
    return out


@pytest.mark.parametrize("form", ["plain", "permuted", "symmetrised"])
@pytest.mark.parametrize("scale", [8, 10, 12, 14])
def test_rmat_under_every_knob(run, rmats, scale, form):
    g, want, model = rmats[scale, form]
    check_all_knobs(run, g, want, model)
    assert want["num_bridges"] > 0 and want["num_artic"] > 0


def test_jumps_on_the_grid(gmx, run):
    """With 256 slots per launch later walks see the facts of earlier ones: jumps happen, and the cursor moves fall below
    half of the count without jumps.  A condition, not a measurement: the model with facts visible between batches of 256
    walks gives 30768 moves against 257985."""
    V, s, d = SHAPES["grid64"]()
    g = gmx.Graph.from_edges(V, s, d)
    want, model = oracle_of(g)
    plain = run(g, skip=0, walks=256)
    jumped = run(g, skip=1, walks=256)
    agrees(plain, want, model)
    agrees(jumped, want, model)
    print("grid64 walks=256: steps %d without jumps, %d with (%d jumps)" % (plain["log"]["steps"], jumped["log"]["steps"], jumped["log"]["jumps"]))
    assert plain["log"]["steps"] == model["steps"] == 257985
    assert jumped["log"]["jumps"] > 0 and 2 * jumped["log"]["steps"] < plain["log"]["steps"]


# ---- upload forms
def test_verbatim_and_sorted_upload_agree_by_uploaded_slot(gmx, run):
    begin, idx, rb, ri = unsorted_multigraph(3000, 2500, 7)
    V = len(begin) - 1
    want = hopcroft_tarjan(V, begin, idx)   # on the caller's arrays: their slots are the uploaded slots of both forms
    verbatim = gmx.Graph.upload(begin, idx, rb, ri)
    sorted_ = gmx.Graph.upload(begin, idx, rb, ri, flags=gmx.GMX_GRAPH_SORT_ROWS)
    assert sorted_.edge_order() is not None and verbatim.edge_order() is None
    a, b = run(verbatim), run(sorted_)
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    agrees(a, want)
    agrees(b, want)
    for knobs in MATRIX:
        agrees(run(sorted_, **knobs), want)


# ---- cross-checks
def test_tecc_of_a_bridgeless_graph_is_wcc(gmx, run, rmats):
    g, want, _ = rmats[10, "symmetrised"]
    begin, idx, _, _ = g.download(reverse=False)
    u, w = slot_ends(g.V, begin, idx)
    keep = want["bridge"] == 0   # without its bridges a graph has none: what is left are its 2-edge-connected components
    h = gmx.Graph.from_edges(g.V, u[keep], w[keep])
    res = run(h)
    comp, ncomp, _ = h.wcc()
    assert res["num_bridges"] == 0 and not res["bridge"].any()
    assert res["num_tecc"] == ncomp == want["num_tecc"] and res["tecc"].tobytes() == comp.tobytes() == want["tecc"].tobytes()


def test_calls_repeat_and_leave_the_graph_alone(gmx, run, rmats):
    g, want, model = rmats[12, "plain"]
    dist0, _ = g.hop_dist(0)
    comp0, n0, st0 = g.wcc()
    a, b = run(g), run(g)
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    agrees(a, want, model)
    dist1, _ = g.hop_dist(0)
    comp1, n1, st1 = g.wcc()
    assert dist0.tobytes() == dist1.tobytes() and comp0.tobytes() == comp1.tobytes() and n0 == n1
    assert all(st0[k] == st1[k] for k in ("iterations", "vertices_reached", "edges_examined"))


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "biconnected")
    assert os.path.exists(exe), "bin/biconnected not built"

    def report(m):
        return ["num_blocks = %d\n" % m["num_blocks"], "num_bridges = %d\n" % m["num_bridges"], "num_articulation_points = %d\n" % m["num_artic"],
                "num_2edge_components = %d\n" % m["num_tecc"], "largest_block_edges = %d\n" % m["largest_block_edges"]]
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    for line in report(hopcroft_tarjan(256, c["begin"], c["node_idx"])):
        assert line in out.stdout, (line, out.stdout)
