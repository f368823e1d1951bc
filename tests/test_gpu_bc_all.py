"""gmx_bc_all (comp_BC of bc_adj.gm: every vertex a source, in node order) and the multi-source traversal behind it
(GMX_BCB_MSBFS): the bytes of gmx_bc over arange(V) and the oracle's bits for every width, gmx_bc_batch's bytes and stats
with the knob on and off, both row-length regimes of the traversal forced, the depth cap at its edge, every upload form,
the argument checks, the memory fallback and the bin/bc_adj driver.  The trace lines say which path ran."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import GOLD, ROOT
from test_bc_random_host import GRAPHS, NSEEDS, graph, same_f32, seeds_of
from test_communities_host import undirected_path
from test_scc_host import csr_of
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_BCB_WIDTH", "GMX_BCB_MAX_DEPTH", "GMX_BCB_LONG_MIN", "GMX_BCB_MEM_MB", "GMX_BCB_TRACE", "GMX_BCB_MSBFS", "GMX_BCB_MS_LONG_MIN")
HUGE = str(1 << 30)
WIDTHS = (16, 32, 64, 0)
TRACE = re.compile(r"gmx bc_batch batch (\d+): seeds (\d+) width (\d+) depth (\d+) path (batched|per-seed) rows (\d+) short \+ (\d+) long, slots (\d+)\n"
                   r"(?:gmx bc_batch msbfs batch (\d+): levels (\d+) rows (\d+) short \+ (\d+) long slots (\d+) saturated (\d+)\n)?")
FIELDS = ("batch", "seeds", "width", "depth", "path", "short", "long", "slots", "ms_batch", "ms_levels", "ms_short", "ms_long", "ms_slots", "ms_saturated")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@contextlib.contextmanager
def knobs(**kw):
    """The library reads its knobs from the environment at every call."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def traced(capfd, call, **kw):
    """(BC, stats, the call's batches as dicts: the batch line's fields and, where one follows, the msbfs line's)"""
    capfd.readouterr()
    with knobs(GMX_BCB_TRACE="1", **kw):
        out, st = call()
    lines = [dict(zip(FIELDS, (x if x is None or not x.isdigit() else int(x) for x in m.groups()))) for m in TRACE.finditer(capfd.readouterr().err)]
    return out, st, lines


def bytes_equal(a, b):
    return a.tobytes() == b.tobytes()


def both_csr(V, src, dst):
    b, i, rb, ri = csr_of(V, src, dst)
    return [np.ascontiguousarray(x, np.int32) for x in (b, i, rb, ri)]


def small_random(V):
    """3 V random edges on V vertices, self-loops and repeats included, rows in drawing order."""
    rng = np.random.default_rng(V)
    return both_csr(V, rng.integers(0, V, 3 * V), rng.integers(0, V, 3 * V))


def complete(V):
    s, d = np.divmod(np.arange(V * V), V)
    return both_csr(V, s[s != d], d[s != d])


def star(leaves, both_ways):
    """vertex 0 is the centre; leaf -> centre, and with both_ways centre -> leaf too"""
    l = np.arange(1, leaves + 1)
    z = np.zeros(leaves, np.int64)
    return both_csr(leaves + 1, np.concatenate([z, l]) if both_ways else l, np.concatenate([l, z]) if both_ways else z)


def chain(V):
    return both_csr(V, np.arange(V - 1), np.arange(1, V))


def upath(V):
    return both_csr(*undirected_path(V))


MADE = {"rmat10": None, "rmat12p": None, "v1": lambda: small_random(1), "v2": lambda: small_random(2), "v17": lambda: small_random(17),
        "v65": lambda: small_random(65), "v257": lambda: small_random(257), "e0": lambda: both_csr(100, [], []), "k70": lambda: complete(70)}


class Case:
    """A graph on the device with its references, each computed once: gmx_bc over arange(V) and the oracle's comp_BC."""

    def __init__(self, gmx, arrays):
        self.og = po.Graph(len(arrays[0]) - 1, *[a.copy() for a in arrays])
        self.V = self.og.N
        self.g = gmx.Graph.upload(*arrays)
        self.all = np.arange(self.V, dtype=np.int32)
        self._ref = {}

    def ref(self, skip):
        if skip not in self._ref:
            with knobs():
                got, st = self.g.bc(self.all, skip)
            assert same_f32(got, po.bc(self.og, self.all, skip))
            self._ref[skip] = (got, st)
        return self._ref[skip]

    def batch_stats(self, skip, width):
        """gmx_bc_batch's stats for the same seeds (its default: the staged traversals)"""
        if (skip, width) not in self._ref:
            with knobs():
                self._ref[skip, width] = self.g.bc_batch(self.all, skip, width)[1]
        return self._ref[skip, width]


@pytest.fixture(scope="module")
def case(gmx, golden):
    cache = {}

    def get(name):
        if name not in cache:
            if name in GRAPHS:
                og = graph(name)
                arrays = [og.begin, og.node_idx, og.r_begin, og.r_node_idx]
            elif name in MADE:
                arrays = MADE[name]()
            else:
                c = golden["cases"][name]
                arrays = [c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"]]
            cache[name] = Case(gmx, arrays)
        return cache[name]
    yield get
    for c in cache.values():
        c.g.free()


def check_a(capfd, c, skip, **kw):
    """Comparison A on one graph: every width against gmx_bc's bytes, the oracle's bits (Case.ref) and bc_batch's stats."""
    ref, ref_st = c.ref(skip)
    for width in WIDTHS:
        got, st, tr = traced(capfd, lambda: c.g.bc_all(skip, width), **kw)
        assert bytes_equal(got, ref), width
        bst = c.batch_stats(skip, width)
        assert st["iterations"] == c.V == bst["iterations"]
        assert st["vertices_reached"] == ref_st["vertices_reached"] == bst["vertices_reached"], width
        assert st["edges_examined"] == bst["edges_examined"], width
        assert len(tr) == (-(-c.V // tr[0]["width"]) if c.V else 0)
        for t in tr:   # a batch that ran batched got its levels from the multi-source traversal
            assert t["path"] == "per-seed" or (t["ms_batch"] == t["batch"] and t["ms_levels"] == t["depth"]), t
    return tr


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", list(MADE))
def test_all_sources_made_graphs(case, capfd, name, skip):
    """rmat10, rmat12p, V in {1, 2, 17, 65, 257} (a partial last batch at every width), no edges, K_70."""
    c = case(name)
    tr = check_a(capfd, c, skip)
    assert all(t["path"] == "batched" for t in tr), tr
    if name == "k70":   # every vertex has every live column after level 1: level 2 walks no row
        assert all(t["ms_levels"] == 1 and t["ms_saturated"] >= 70 for t in tr), tr
    if name == "e0":
        assert all(t["ms_levels"] == 0 and t["ms_slots"] == 0 for t in tr) and not c.ref(skip)[0].any()


def golden_names():
    """The golden cases that carry a reverse CSR (every graph case does; the uniform generator's outputs do not)."""
    keys = np.load(os.path.join(GOLD, "golden.npz"), allow_pickle=False).files
    return sorted({k.split("/")[0] for k in keys if k.endswith("/r_begin")})


@pytest.mark.parametrize("name", golden_names())
def test_all_sources_golden(case, capfd, name):
    """Hand graphs (empty, isolated, self-loop, multi-edge, the adjacency samples) and the RMAT fixtures."""
    for skip in (False, True):
        check_a(capfd, case(name), skip)


def test_golden_cases_are_covered():
    assert len(golden_names()) >= 15 and "hand_adj_very_small_sample" in golden_names()


@pytest.mark.parametrize("skip", [False, True])
def test_batch_knob_same_bytes_and_stats(gmx, capfd, skip):
    """Comparison B: bc_batch with the multi-source traversal against the staged traversals, 70 seeds of rmat14 (a
    duplicated hub, a vertex without out-edges) and the prefixes around a batch's end."""
    og, seeds = graph("rmat14"), seeds_of("rmat14")
    g = gmx.Graph.upload(og.begin, og.node_idx, og.r_begin, og.r_node_idx)
    for n in (NSEEDS, 1, 16, 17, 64, 65):
        for width in WIDTHS:
            off, ost, otr = traced(capfd, lambda: g.bc_batch(seeds[:n], skip, width), GMX_BCB_MSBFS="0")
            on, st, tr = traced(capfd, lambda: g.bc_batch(seeds[:n], skip, width), GMX_BCB_MSBFS="1")
            assert bytes_equal(on, off), (n, width)
            assert st["vertices_reached"] == ost["vertices_reached"] and st["edges_examined"] == ost["edges_examined"] and st["iterations"] == n
            assert all(t["ms_batch"] is None for t in otr) and all(t["ms_batch"] == t["batch"] for t in tr)
            assert [{k: t[k] for k in FIELDS[:8]} for t in tr] == [{k: t[k] for k in FIELDS[:8]} for t in otr]   # the batch lines are unchanged
    capfd.readouterr()
    with knobs(GMX_BCB_TRACE="1"):   # off by default for gmx_bc_batch
        assert bytes_equal(g.bc_batch(seeds[:65], skip, 0)[0], on)
    assert "msbfs" not in capfd.readouterr().err
    g.free()


@pytest.mark.parametrize("both_ways", [True, False])
def test_regimes_star(gmx, capfd, both_ways):
    """A reverse row of 5000 slots (the centre's): by a wave (GMX_BCB_MS_LONG_MIN=1 and the default) and by a lane (a huge
    value).  Seeds: the centre, leaves and a repeated leaf."""
    arrays = star(5000, both_ways)
    og = po.Graph(5001, *[a.copy() for a in arrays])
    g = gmx.Graph.upload(*arrays)
    seeds = np.concatenate([[0, 7, 7], np.arange(1, 5000, 75)]).astype(np.int32)
    assert len(seeds) == 70
    for skip in (False, True):
        with knobs():
            ref, ref_st = g.bc(seeds, skip)
        assert same_f32(ref, po.bc(og, seeds, skip))
        for kw, want in (({"GMX_BCB_MS_LONG_MIN": "1"}, (False, True)), ({"GMX_BCB_MS_LONG_MIN": HUGE}, (True, False)), ({}, (True, True))):
            got, st, tr = traced(capfd, lambda: g.bc_batch(seeds, skip, 64), GMX_BCB_MSBFS="1", **kw)
            assert bytes_equal(got, ref) and st["vertices_reached"] == ref_st["vertices_reached"], kw
            assert len(tr) == 2 and all(t["path"] == "batched" and (t["ms_short"] > 0, t["ms_long"] > 0) == want for t in tr), (kw, tr)
    g.free()


@pytest.mark.parametrize("skip", [False, True])
def test_regimes_rmat12p(case, capfd, skip):
    c = case("rmat12p")
    tr = check_a(capfd, c, skip, GMX_BCB_MS_LONG_MIN="1")
    assert all(t["ms_short"] == 0 and t["ms_long"] > 0 for t in tr), tr[:2]
    tr = check_a(capfd, c, skip, GMX_BCB_MS_LONG_MIN=HUGE)
    assert all(t["ms_long"] == 0 and t["ms_short"] > 0 for t in tr), tr[:2]
    tr = check_a(capfd, c, skip, GMX_BCB_MS_LONG_MIN="64")
    assert all(t["ms_long"] > 0 and t["ms_short"] > 0 for t in tr), tr[:2]


def test_depth_cap_chain(gmx, capfd):
    """A directed chain of 320 vertices: seed s is 319 - s levels deep.  Seeds 0..63 reach level 319 and seeds 64..127 level
    255, one past the cap: both batches run per seed; seeds 128..191 reach level 191 and stay batched."""
    arrays = chain(320)
    og = po.Graph(320, *[a.copy() for a in arrays])
    g = gmx.Graph.upload(*arrays)
    seeds = np.arange(192, dtype=np.int32)
    got, st, tr = traced(capfd, lambda: g.bc_batch(seeds, True, 64), GMX_BCB_MSBFS="1")
    with knobs():
        ref, ref_st = g.bc(seeds, True)
    assert bytes_equal(got, ref) and same_f32(got, po.bc(og, seeds, True)) and st["vertices_reached"] == ref_st["vertices_reached"]
    assert [t["path"] for t in tr] == ["per-seed", "per-seed", "batched"] and tr[2]["depth"] == 191 == tr[2]["ms_levels"], tr
    got, _, tr = traced(capfd, lambda: g.bc_batch(seeds[128:], False, 64), GMX_BCB_MSBFS="1")   # the literal form on the batched part
    assert same_f32(got, po.bc(og, seeds[128:], False)) and [t["path"] for t in tr] == ["batched"]
    g.free()


@pytest.mark.parametrize("V", [255, 256])
def test_depth_cap_path(gmx, capfd, V):
    """An undirected path: 254 levels from an end are exactly the cap and stay batched; 255 are not (the batches that hold
    an end vertex run per seed)."""
    arrays = upath(V)
    og = po.Graph(V, *[a.copy() for a in arrays])
    g = gmx.Graph.upload(*arrays)
    every = np.arange(V, dtype=np.int32)
    got, st, tr = traced(capfd, lambda: g.bc_all(True, 64))
    assert same_f32(got, po.bc(og, every, True)) and st["vertices_reached"] == V * V
    assert [t["path"] for t in tr] == (["batched"] * 4 if V == 255 else ["per-seed", "batched", "batched", "per-seed"]), tr
    assert V != 255 or (tr[0]["depth"] == 254 == tr[0]["ms_levels"] and tr[3]["depth"] == 254)
    g.free()


def test_depth_cap_lowered(case, capfd):
    """The environment lowers the cap: every batch of rmat10 per seed, the bytes of comparison A."""
    c = case("rmat10")
    got, st, tr = traced(capfd, lambda: c.g.bc_all(True, 32), GMX_BCB_MAX_DEPTH="3")
    assert bytes_equal(got, c.ref(True)[0]) and st["vertices_reached"] == c.ref(True)[1]["vertices_reached"]
    assert len(tr) == 32 and all(t["path"] == "per-seed" and t["ms_levels"] == 4 for t in tr), tr[:2]


@pytest.mark.parametrize("form", ["F0", "F1", "F2", "F3", "F4"])
def test_unsorted_multigraph_every_upload_form(gmx, capfd, form):
    """The upload forms of test_gpu_bc_batch.py: a hub row of 5000 slots with repeats, rows in shuffled order."""
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    rev, flags = {"F0": (True, S), "F1": (True, 0), "F2": (False, N), "F3": (False, 0), "F4": (False, S | N)}[form]
    b, i, rb, ri = unsorted_multigraph(2048, 5000, 2048)
    d = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
    if flags & N:
        with pytest.raises(gmx.GmxError, match="reverse"):
            d.bc_all()
        d.free()
        return
    hb, hi, hrb, hri = d.download()
    held = po.Graph(2048, hb, hi, hrb, hri)
    every = np.arange(2048, dtype=np.int32)
    with knobs():
        ref, _ = d.bc(every, True)
    assert same_f32(ref, po.bc(held, every, True))
    for kw in ({}, {"GMX_BCB_MS_LONG_MIN": "1"}, {"GMX_BCB_MS_LONG_MIN": HUGE}):
        got, _, tr = traced(capfd, lambda: d.bc_all(True, 32), **kw)
        assert bytes_equal(got, ref), kw
        assert len(tr) == 64 and all(t["path"] == "batched" and t["ms_batch"] == t["batch"] for t in tr)
    d.free()


def test_errors_and_memory_fallback(gmx, case, capfd):
    c = case("rmat10")
    L = gmx.lib()
    out = np.zeros(1024, np.float32)
    ok = np.array([1, 2], np.int32)
    with knobs():
        assert L.gmx_bc_all(c.g._h, 1, 16, None, None) == GMX_ERR_ARG == L.gmx_bc_batch(c.g._h, ok.ctypes.data, 2, 1, 16, None, None)
        assert L.gmx_bc_all(None, 1, 16, out.ctypes.data, None) == GMX_ERR_ARG
        for width in (3, 128, -16, 2):
            assert L.gmx_bc_all(c.g._h, 1, width, out.ctypes.data, None) == GMX_ERR_ARG == L.gmx_bc_batch(c.g._h, ok.ctypes.data, 2, 1, width, out.ctypes.data, None)
        assert L.gmx_bc_all(c.g._h, 1, 16, out.ctypes.data, None) == 0           # stats may be NULL
        assert bytes_equal(out, c.ref(True)[0])
        og = graph("rmat10")
        nr = gmx.Graph.upload(og.begin, og.node_idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
        st = gmx.Stats()
        want = L.gmx_bc_batch(nr._h, ok.ctypes.data, 2, 0, 16, out.ctypes.data, C.byref(st))
        assert want != 0 and L.gmx_bc_all(nr._h, 0, 16, out.ctypes.data, C.byref(st)) == want
        assert b"reverse" in L.gmx_last_error()
        nr.free()
        e = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))          # V = 0
        assert e.bc_all(True, 16)[0].shape == (0,)
        e.free()
    with knobs(GMX_BCB_WIDTH="5"):
        assert L.gmx_bc_all(c.g._h, 1, 0, out.ctypes.data, None) == GMX_ERR_ARG
    got, st, tr = traced(capfd, lambda: c.g.bc_all(True, 64), GMX_BCB_MEM_MB="0")   # no room for a batch: gmx_bc itself
    assert bytes_equal(got, c.ref(True)[0]) and st["edges_examined"] == 0 and st["vertices_reached"] == c.ref(True)[1]["vertices_reached"]
    assert len(tr) == 1 and tr[0]["path"] == "per-seed" and tr[0]["width"] == 1 and tr[0]["ms_batch"] is None, tr


def test_deterministic_and_leaves_the_graph_alone(case):
    c = case("rmat12p")
    with knobs():
        dist0, _ = c.g.hop_dist(0)
        a, _ = c.g.bc_all(True, 64)
        b, _ = c.g.bc_all(True, 64)
        assert bytes_equal(a, b) and bytes_equal(a, c.ref(True)[0])
        assert np.array_equal(c.g.hop_dist(0)[0], dist0)
    with knobs(GMX_BCB_MSBFS="0"):   # the staged traversals behind the same entry
        assert bytes_equal(c.g.bc_all(True, 64)[0], a)


def test_dropin_driver(gmx, golden, tmp_path):
    """bin/bc_adj on the committed sample (one double per vertex and per edge): the lines bc_adj_main.cc prints, the BC
    values those of comp_BC(G, BC) on the graph the loader builds, looked up by key."""
    exe = os.path.join(PKG, "bin", "bc_adj")
    assert os.path.exists(exe), "bin/bc_adj not built"
    cfg = tmp_path / "config.txt"
    cfg.write_text("1908 128\t99 333\nignored\n")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe, os.path.join(GOLD, "very_small_sample.adj"), str(cfg), "3", "d"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout
    c = golden["cases"]["hand_adj_very_small_sample"]
    og = po.Graph(4, c["begin"].copy(), c["node_idx"].copy(), c["r_begin"].copy(), c["r_node_idx"].copy())
    want = po.bc(og, np.arange(4, dtype=np.int32), True)
    ids = {128: 0, 99: 1, 333: 2, 1908: 3}
    lines = r.stdout.splitlines()
    assert lines[0] == "running with 3 threads"
    assert re.fullmatch(r"BC \(threads: 3\) - COMPUTATION RUNNING TIME \(ms\): \d+\.\d+", lines[1])
    assert lines[2:6] == ["%d :  %f" % (k, float(want[ids[k]])) for k in (1908, 128, 99, 333)]
    assert want[1] == 1.0   # 128 -> 99 -> 333: the one vertex on a shortest path between two others
