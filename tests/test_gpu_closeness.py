"""gmx_closeness on the device: far, reach, ecc and harm byte for byte against the one-thread BFS model of the downloaded
CSR (test_closeness_host.closeness_model) and the log line's invariants, at the shapes where each piece can go wrong: partly
filled sweeps at every width, more levels than a byte holds, dead columns, repeated sources, both row regimes and the wave
walk's early exit, unsorted multigraphs, the graph without a reverse CSR, the argument checks and the driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_closeness_host import MODES, closeness_model
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_CLOSE_WORDS", "GMX_CLOSE_LONG_MIN", "GMX_CLOSE_BATCH", "GMX_CLOSE_LOG")
LOG_FIELDS = ("V", "E", "mode", "sources", "words", "sweeps", "levels", "lane", "wave", "saturated", "slots", "pairs")
LOG = re.compile(r"gmx close: " + " ".join(r"%s (\d+)" % f for f in LOG_FIELDS) + r"\n")
WORDS = (1, 2, 4)
HUGE = 1 << 30
LONG_MINS = (1, None, HUGE)   # every row by a wave, the default, every row by a lane
BATCHES = (1, 2, 3, 4)         # levels launched per host read


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
    def call(g, mode, sources=None, words=None, long_min=None, batch=None):
        """One call with GMX_CLOSE_LOG: ((far, reach, ecc, harm), stats, the log line's fields), the line's invariants checked."""
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMX_CLOSE_LOG", "1")
        if words is not None:
            monkeypatch.setenv("GMX_CLOSE_WORDS", str(words))
        if long_min is not None:
            monkeypatch.setenv("GMX_CLOSE_LONG_MIN", str(long_min))
        if batch is not None:
            monkeypatch.setenv("GMX_CLOSE_BATCH", str(batch))
        capfd.readouterr()
        far, reach, ecc, harm, st = g.closeness(mode, sources)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = dict(zip(LOG_FIELDS, map(int, m.groups())))
        n = g.V if sources is None else len(sources)
        assert (far.dtype, reach.dtype, ecc.dtype, harm.dtype) == (np.int64, np.int32, np.int32, np.uint64)
        assert f["V"] == g.V and f["E"] == g.E and f["mode"] == MODES.index(mode) and f["sources"] == n
        want_words = words or f["words"]
        while want_words > 1 and 64 * (want_words // 2) >= n:   # no wider than the sources need
            want_words //= 2
        assert f["words"] == want_words
        assert f["sweeps"] == -(-n // (64 * f["words"]))
        assert f["lane"] + f["wave"] + f["saturated"] == g.V * f["levels"]
        assert f["pairs"] == int(reach.sum(dtype=np.int64)) == st["vertices_reached"]
        assert f["slots"] == st["edges_examined"] <= f["levels"] * g.E * (2 if mode == "both" else 1)
        assert f["levels"] == st["iterations"] >= f["sweeps"]
        if batch is not None:
            assert f["levels"] % batch == 0 and f["levels"] >= batch * f["sweeps"]
        if long_min == HUGE:
            assert f["wave"] == 0
        if long_min == 1:
            assert f["lane"] == 0
        return (far, reach, ecc, harm), st, f
    return call


def same(got, want):
    for a, b, name in zip(got, want, ("far", "reach", "ecc", "harm")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def model_of(g, mode, sources=None):
    begin, idx, _, _ = g.download(reverse=False)
    return closeness_model(g.V, begin, idx, mode, sources)


def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    for mode in MODES:
        far, reach, ecc, harm, st = g.closeness(mode)
        assert len(far) == len(reach) == len(ecc) == len(harm) == 0 and st["iterations"] == 0 and st["vertices_reached"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, run, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    for mode in MODES:
        want = model_of(g, mode)
        for long_min in LONG_MINS:
            for batch in (1, 4):
                got, st, f = run(g, mode, long_min=long_min, batch=batch)
                for a in got:
                    assert len(a) == V and not a.any()
                assert f["pairs"] == 0 and f["levels"] == batch * f["sweeps"]   # every sweep's first level finds nothing
                same(got, want)


@pytest.fixture(scope="module")
def paths(gmx):
    """700 = 10 * 64 + 60 = 2 * 256 + 188: the last sweep is partly filled at every width; levels pass 255 and 256."""
    P = 700
    out = {}
    for name, at in (("plain", np.arange(P)), ("shuffled", np.random.default_rng(3).permutation(P))):
        g = gmx.Graph.from_edges(P, at[:-1], at[1:])
        out[name] = (g, at, {mode: model_of(g, mode) for mode in MODES})
    return out


@pytest.mark.parametrize("name", ["plain", "shuffled"])
@pytest.mark.parametrize("mode", MODES)
def test_directed_path_all_sources(gmx, run, paths, name, mode):
    g, at, models = paths[name]
    P = g.V
    want = models[mode]
    if name == "plain":
        v = np.arange(P, dtype=np.int64)
        if mode == "out":
            assert np.array_equal(want[0], (P - 1 - v) * (P - v) // 2) and want[2][0] == P - 1
        if mode == "in":
            assert np.array_equal(want[0], v * (v + 1) // 2) and want[2][P - 1] == P - 1
    assert want[2].max() == P - 1
    passes = {}
    for words in WORDS:
        got, st, f = run(g, mode, words=words, batch=1)
        same(got, want)
        assert f["words"] == words and f["levels"] > 256
        passes[words] = f["levels"]
    for batch in BATCHES[1:]:   # the ring of per-level words turns many times; a batch may end past the sweep's last level
        got, st, f = run(g, mode, words=2, batch=batch)
        same(got, want)
        assert passes[2] <= f["levels"] < passes[2] + batch * f["sweeps"]


def test_ten_vertices_leave_dead_columns(gmx, run):
    rng = np.random.default_rng(4)
    g = gmx.Graph.from_edges(10, rng.integers(0, 10, 25), rng.integers(0, 10, 25))
    for mode in MODES:
        want = model_of(g, mode)
        assert want[1].max() > 3
        for words in WORDS:
            for long_min in LONG_MINS:
                got, st, f = run(g, mode, words=words, long_min=long_min)
                same(got, want)
                assert f["words"] == 1 and f["sweeps"] == 1
                assert got[1].max() <= 9   # a column past the sources would show as extra reach


def test_repeated_and_restricted_sources(gmx, run):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    for mode in MODES:
        a, _, f = run(g, mode, [3, 3, 5])
        b, _, _ = run(g, mode, [3])
        c, _, _ = run(g, mode, [5])
        same(a, model_of(g, mode, [3, 3, 5]))
        for k in (0, 1, 3):
            assert np.array_equal(a[k], 2 * b[k] + c[k])
        assert np.array_equal(a[2], np.maximum(b[2], c[2]))
        assert a[1].max() == 3 and f["sweeps"] == 1
    # a list that fills one sweep exactly, one more, and none at all
    rng = np.random.default_rng(5)
    for n in (64, 65, 129, 0):
        src = rng.integers(0, g.V, n).astype(np.int32)
        for words in (1, 2):
            got, st, f = run(g, "in", src, words=words)
            same(got, model_of(g, "in", src))
        if n == 0:
            assert f["sweeps"] == 0 and f["levels"] == 0 and not any(x.any() for x in got)


@pytest.mark.parametrize("name", ["star_out", "star_in", "star_both"])
def test_stars_in_both_row_regimes(gmx, run, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    for mode in MODES:
        want = model_of(g, mode)
        waves = {}
        for long_min in LONG_MINS:
            got, st, f = run(g, mode, long_min=long_min)
            same(got, want)
            waves[long_min] = f["wave"]
        hub_row = {"out": name != "star_in", "in": name != "star_out", "both": True}[mode]   # does the mode walk the hub's long row
        assert (waves[None] > 0) == hub_row
    assert model_of(g, "both")[2].max() == 2


def test_wave_walk_stops_at_the_first_covering_piece(gmx, run):
    """t = 1024 has in-edges from a_i = i, i < 1024, its reverse row sorted: from a_0 the first piece of the row covers the one
    missing column, from a_1023 only the last."""
    n = 1024
    g = gmx.Graph.from_edges(n + 1, np.arange(n), np.full(n, n))
    first, _, f0 = run(g, "in", [0])
    last, _, f1 = run(g, "in", [n - 1])
    for got, src in ((first, [0]), (last, [n - 1])):
        assert got[0][n] == 1 and got[1][n] == 1 and got[2][n] == 1 and got[3][n] == 1 << 32
        same(got, model_of(g, "in", src))
    assert f0["wave"] == f1["wave"] == 1 and 0 < f0["slots"] < f1["slots"] == n
    # the lane walk stops early as well
    _, _, l0 = run(g, "in", [0], long_min=HUGE)
    _, _, l1 = run(g, "in", [n - 1], long_min=HUGE)
    assert 0 < l0["slots"] < l1["slots"] == n


@pytest.fixture(scope="module")
def rmats(gmx):
    out = {}
    for name, permute, symmetrize in (("plain", False, False), ("permuted", True, False), ("symmetrised", False, True)):
        g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, permute)
        if symmetrize:
            g = g.symmetrize()
        out[name] = g
    return out


@pytest.mark.parametrize("name", ["plain", "permuted", "symmetrised"])
@pytest.mark.parametrize("mode", MODES)
def test_rmat_against_the_model_under_every_knob(gmx, run, rmats, name, mode):
    g = rmats[name]
    want = model_of(g, mode)
    levels = {}
    for words in WORDS:
        for long_min in (1, None):
            got, st, f = run(g, mode, words=words, long_min=long_min)
            same(got, want)
            levels[words] = f["levels"]
            assert f["words"] == words and st["kernel_ms"] > 0
    print("RMAT-12 %s %s: pairs %d max ecc %d levels by width %s" % (name, mode, f["pairs"], want[2].max(), levels))
    assert f["pairs"] > g.V and want[2].max() >= 3
    if name == "symmetrised" and mode == "both":   # one undirected graph: the direction does not matter
        same(run(g, "out")[0], got)
        same(run(g, "in")[0], got)
    if name == "plain" and mode == "in":   # IN is OUT of the transposed edge list
        begin, idx, _, _ = g.download(reverse=False)
        t = gmx.Graph.from_edges(g.V, idx, np.repeat(np.arange(g.V), np.diff(begin)))
        same(run(t, "out")[0], got)
        t.free()


@pytest.mark.parametrize("V,hub_edges,pivots", [(64, 200, None), (64, 200, 20), (150000, 400000, 64)])
def test_unsorted_multigraph_uploaded_verbatim(gmx, run, V, hub_edges, pivots):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)
    src = None if pivots is None else np.random.default_rng(7).integers(0, V, pivots).astype(np.int32)
    if pivots == 64:
        src[:3] = 5   # the hub, three times
    for mode in MODES:
        want = closeness_model(V, begin, idx, mode, src)
        got, _, _ = run(g, mode, src)
        same(got, want)
        same(run(sorted_g, mode, src)[0], got)
        same(run(g, mode, src, words=2, long_min=1, batch=2)[0], got)
        assert want[1].max() > 1


def test_graph_without_reverse_csr(gmx, run):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g.download()
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    want = closeness_model(g.V, begin, idx, "out")
    same(run(h, "out")[0], want)
    same(run(g, "out")[0], want)
    for mode in ("in", "both"):
        with pytest.raises(gmx.GmxError, match="gmx status -5"):   # GMX_ERR_STATE
            h.closeness(mode)


def test_errors_and_null_outputs(gmx):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    L = gmx.lib()
    V = g.V
    far, reach, ecc, harm = np.zeros(V, np.int64), np.zeros(V, np.int32), np.zeros(V, np.int32), np.zeros(V, np.uint64)
    outs = (far.ctypes.data, reach.ctypes.data, ecc.ctypes.data, harm.ctypes.data)
    src = np.array([1, 2, V], np.int32)
    assert L.gmx_closeness(None, 0, None, 0, *outs, None) == -1   # GMX_ERR_ARG
    assert L.gmx_closeness(g._h, 3, None, 0, *outs, None) == -1
    assert L.gmx_closeness(g._h, -1, None, 0, *outs, None) == -1
    assert L.gmx_closeness(g._h, 0, src.ctypes.data, 3, *outs, None) == -1    # a source out of range
    assert L.gmx_closeness(g._h, 0, src.ctypes.data, -1, *outs, None) == -1
    src[2] = -1
    assert L.gmx_closeness(g._h, 0, src.ctypes.data, 3, *outs, None) == -1
    assert not far.any() and not reach.any()
    with pytest.raises(gmx.GmxError, match="gmx status -1"):
        g.closeness("in", [V])
    with pytest.raises(KeyError):
        g.closeness("sideways")
    assert L.gmx_closeness(g._h, 0, src.ctypes.data, -1, None, None, None, None, None) == -1
    assert L.gmx_closeness(g._h, 0, None, -1, None, None, None, None, None) == 0   # every vertex: nsources is ignored; all outputs may be NULL
    whole = g.closeness("out")
    for k in range(4):   # one output at a time
        only = [None] * 4
        only[k] = outs[k]
        assert L.gmx_closeness(g._h, 0, None, 0, *only, None) == 0
        assert (far, reach, ecc, harm)[k].tobytes() == whole[k].tobytes()


def test_runs_are_repeatable(gmx, run):
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, True)
    a, sa, fa = run(g, "both")
    b, sb, fb = run(g, "both")
    same(a, b)
    assert fa == fb and fa["pairs"] > 0
    for k in ("iterations", "vertices_reached", "edges_examined"):
        assert sa[k] == sb[k] > 0
    for words, batch in ((4, 1), (1, 2), (2, 3), (4, 4)):
        c, _, fc = run(g, "both", words=words, batch=batch)
        same(a, c)
        assert fc["pairs"] == fa["pairs"]


def test_derived_centralities(gmx):
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    far, reach, ecc, harm, _ = g.closeness("both")
    c, h = gmx.closeness_of(far, reach), gmx.harmonic_of(harm)
    at = reach > 0
    assert np.all(c[~at] == 0) and np.all(h[~at] == 0) and np.all((c[at] > 0) & (c[at] <= 1)) and np.all(h[at] <= reach[at])
    assert np.all(h[at] >= reach[at] / ecc[at] - reach[at] * 2.0 ** -32)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "closeness")
    assert os.path.exists(exe), "bin/closeness not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    for mode in ("in", "out", "both"):
        out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null", mode], stdout=subprocess.PIPE, text=True,
                             timeout=120, cwd=ROOT)
        assert out.returncode == 0, out.stdout
        far, reach, ecc, harm = closeness_model(256, c["begin"], c["node_idx"], mode)
        radius = int(ecc[reach > 0].min()) if (reach > 0).any() else 0
        for line in ("diameter = %d\n" % ecc.max(), "radius = %d\n" % radius, "wiener = %d\n" % far.sum(), "top = %d\n" % int(np.argmax(harm))):
            assert line in out.stdout, (mode, line, out.stdout)
