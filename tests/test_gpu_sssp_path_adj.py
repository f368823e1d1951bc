"""gmx_sssp_path_f64 (sssp_path_adj.gm) on the device against test_sssp_path_adj_host: the pinned shapes and the parallel
statement (spf_model, which the host tests confirm against the loop as written) byte for byte on every vertex -- dist compared
as bit patterns -- with the tail threshold forced to each path (shown to be the path that ran by the library's
GMX_SSSP_F64_LOG line), targets that prune, thousands of rounds on a chain, every upload form with cost and prev_edge in the
caller's slots, errors, the counters (which are the model's) and the driver."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_communities_host import named_graph
from test_gpu_sssp_path import gm_rand32_lengths
from test_sssp_path_adj_host import DBL_MAX, PINNED, SHAPES, csr_of, median_end, random_case, shape, spf_model
from test_upload_forms_host import rows_unsorted, ugraph, unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_SSSP_F64_TAIL", "GMX_SSSP_F64_LOG")
HUGE = "2000000000"
FORCED = {"default": {}, "no_tail": {"GMX_SSSP_F64_TAIL": "0"}, "all_tail": {"GMX_SSSP_F64_TAIL": HUGE}}
LINE = re.compile(r"gmx sssp_path_f64: V (\d+) E (\d+) root (-?\d+) end (-?\d+); tail (\d+); rounds (\d+): (\d+) grid \+ (\d+) tail in (\d+) launches; "
                  r"queued (\d+); slots (\d+) grid \+ (\d+) tail; ms ([0-9.]+) grid \+ ([0-9.]+) tail")
FIELDS = ("V", "E", "root", "end", "tail_from", "rounds", "grid_rounds", "tail_rounds", "tail_launches", "queued", "grid_slots", "tail_slots",
          "grid_ms", "tail_ms")
_MODEL = {}


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


def logged(g, cost, root, end, capfd, **env):
    """(the call's result, the fields of the library's line)."""
    capfd.readouterr()
    with knobs(GMX_SSSP_F64_LOG="1", **env):
        got = g.sssp_path_f64(cost, root, end)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    return got, {k: (float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, lines[0])}


def check(want, got, label=None):
    """Bytes of the three arrays, and the counters."""
    dist, pn, pe, st = got
    assert dist.dtype == np.float64 and pn.dtype == np.int32 and pe.dtype == np.int32
    assert np.array_equal(dist.view(np.uint64), want[0].view(np.uint64)), label
    assert np.array_equal(pn, want[1]), label
    assert np.array_equal(pe, want[2]), label
    if st is not None and len(want) > 3:
        assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == want[3:], label


def model_of(key, b, i, cost, root, end):
    """spf_model, computed once per case and shared between the tests."""
    if key not in _MODEL:
        _MODEL[key] = spf_model(b, i, cost, root, end)
        for a in _MODEL[key][:3]:
            a.setflags(write=False)
    return _MODEL[key]


def forward_only(gmx, b, i):
    return gmx.Graph.upload(np.ascontiguousarray(b, np.int32), np.ascontiguousarray(i, np.int32), flags=gmx.GMX_GRAPH_NO_REVERSE)


# ---------------------------------------------------------------- the pinned shapes, every path
@pytest.mark.parametrize("forced", sorted(FORCED))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pinned_shapes(gmx, capfd, name, forced):
    b, i, cost, root, end = shape(name)
    g = forward_only(gmx, b, i)
    got, f = logged(g, cost, root, end, capfd, **FORCED[forced])
    dist, pn, pe = PINNED[name]
    want = (np.asarray(dist, np.float64), np.asarray(pn, np.int32), np.asarray(pe, np.int32)) + spf_model(b, i, cost, root, end)[3:]
    check(want, got, (name, forced))
    assert f["rounds"] == got[3]["iterations"] and f["grid_slots"] + f["tail_slots"] == got[3]["edges_examined"]
    if forced == "no_tail":
        assert f["tail_rounds"] == 0 and f["tail_launches"] == 0 and f["tail_slots"] == 0
    if forced == "all_tail":
        assert f["grid_rounds"] == 0 and f["grid_slots"] == 0 and f["tail_launches"] <= 1


def test_round_dep_without_a_target(gmx):
    b, i, cost, root, _ = shape("round_dep")
    dist, pn, pe, _ = forward_only(gmx, b, i).sssp_path_f64(cost, root)
    assert dist[5] == 23 and pn[5] == 4 and pe[5] == 5


def test_ulp_bits(gmx):
    b, i, cost, root, end = shape("ulp")
    for env in FORCED.values():
        with knobs(**env):
            dist = forward_only(gmx, b, i).sssp_path_f64(cost, root, end)[0]
        assert float(dist[4]).hex() == "0x1.3333333333333p-1"


def test_infinite_and_negative_zero_costs(gmx):
    b, i = csr_of(3, [0, 0, 1], [1, 2, 2])
    g = forward_only(gmx, b, i)
    for cost in ([np.inf, 1.0, -0.0], [-0.0, 1.0, -0.0]):
        for end in (-1, 2):
            check(spf_model(b, i, cost, 0, end), g.sssp_path_f64(cost, 0, end), (cost, end))


# ---------------------------------------------------------------- edge shapes
def test_no_edges_and_roots_out_of_range(gmx):
    g = gmx.Graph.upload(np.zeros(6, np.int32), np.zeros(0, np.int32))
    for end in (-1, 4, 2):
        dist, pn, pe, st = g.sssp_path_f64(np.zeros(0), 2, end)
        assert dist.tolist() == [DBL_MAX, DBL_MAX, 0, DBL_MAX, DBL_MAX] and (pn == -1).all() and (pe == -1).all()
        assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == (1, 0, 1)
    b, i, cost, _, _ = shape("chain_end")
    g = forward_only(gmx, b, i)
    for root in (6, -1, -7, 1 << 30):
        for end in (-1, 3):
            dist, pn, pe, st = g.sssp_path_f64(cost, root, end)
            assert (dist == DBL_MAX).all() and (pn == -1).all() and (pe == -1).all()
            assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == (0, 0, 0)


def test_empty_graph_through_the_c_abi(gmx):
    L = gmx.lib()
    e = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))
    out = [np.full(1, 77.0), np.full(1, 77, np.int32), np.full(1, 77, np.int32)]
    st = gmx.Stats()
    assert L.gmx_sssp_path_f64(e._h, 0, -1, None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, C.byref(st)) == 0
    assert st.iterations == 0 and all((o == 77).all() for o in out)
    dist, pn, pe, st = e.sssp_path_f64(np.zeros(0), 0, -1)
    assert len(dist) == len(pn) == len(pe) == 0 and st["iterations"] == 0


# ---------------------------------------------------------------- named graphs: two cost draws, four targets
def costs_of(draw, E):
    rng = np.random.default_rng(E + 17)
    return rng.integers(0, 8, E) * 0.25 if draw == "ties" else rng.random(E)      # many exact ties and zeros / none to speak of


@pytest.mark.parametrize("draw", ["ties", "uniform01"])
@pytest.mark.parametrize("name", ["rmat10", "rmat12", "rmat12s", "uniform", "star33"])
def test_named_graphs(gmx, capfd, name, draw):
    b, i = named_graph(name)
    cost = costs_of(draw, len(i))
    root = int(np.argmax(np.diff(b)))                                             # the top hub
    free = model_of((name, draw, -1), b, i, cost, root, -1)
    ends = {"none": -1, "root": root, "median": median_end(free[0])}
    far = np.flatnonzero(free[0] == DBL_MAX)
    if len(far):
        ends["unreachable"] = int(far[0])
    g = forward_only(gmx, b, i)
    unpruned = None
    for label, end in ends.items():
        want = model_of((name, draw, end), b, i, cost, root, end)
        for forced in ("default", "no_tail"):
            got, f = logged(g, cost, root, end, capfd, **FORCED[forced])
            check(want, got, (name, draw, label, forced))
        st = got[3]
        print("sssp_path_f64 %s %s end %s: %s" % (name, draw, label, f))
        assert st["iterations"] > 0
        if end == -1:
            unpruned = st
        else:
            assert st["edges_examined"] <= unpruned["edges_examined"], label
        if label == "unreachable":                                               # the bound never falls: the unpruned run
            check(free, got, label)
        if label == "median" and name != "star33":
            assert st["edges_examined"] < unpruned["edges_examined"]
    g.free()


def test_random_multigraphs(gmx):
    for seed in range(60):
        b, i, cost, root, end = random_case(seed)
        g = forward_only(gmx, b, i)
        with knobs(**(FORCED["no_tail"] if seed % 2 else {})):
            check(spf_model(b, i, cost, root, end), g.sssp_path_f64(cost, root, end), seed)
        g.free()


@pytest.mark.parametrize("tail", ["64", "1024"])
def test_the_tail_hands_back_to_the_grid(gmx, capfd, tail):
    """rmat12 from its hub: the first queue is small, the next ones are not, the last ones are again."""
    b, i = named_graph("rmat12")
    cost = costs_of("ties", len(i))
    root = int(np.argmax(np.diff(b)))
    want = model_of(("rmat12", "ties", -1), b, i, cost, root, -1)
    root2 = int(np.flatnonzero(np.diff(b) == 1)[0])                               # a root with one slot: the tail starts
    g = forward_only(gmx, b, i)
    got, f = logged(g, cost, root, -1, capfd, GMX_SSSP_F64_TAIL=tail)
    check(want, got, tail)
    got2, f2 = logged(g, cost, root2, -1, capfd, GMX_SSSP_F64_TAIL=tail)
    check(spf_model(b, i, cost, root2, -1), got2, tail)
    print("sssp_path_f64 rmat12 tail %s: %s / %s" % (tail, f, f2))
    assert f["grid_rounds"] > 0 and f["tail_rounds"] > 0
    assert f2["grid_rounds"] > 0 and f2["tail_launches"] >= 2                     # tail, grid, tail


def test_default_threshold(gmx, capfd):
    b, i, cost, root, end = shape("pruned")
    _, f = logged(forward_only(gmx, b, i), cost, root, end, capfd)
    assert f["tail_from"] == 4096


# ---------------------------------------------------------------- thousands of rounds
@pytest.mark.parametrize("forced", sorted(FORCED))
@pytest.mark.parametrize("name", ["path4096", "chain4096"])
def test_long_chains(gmx, capfd, name, forced):
    b, i = named_graph(name)
    cost = np.random.default_rng(4096).integers(1, 4, len(i)) * 0.5
    want = model_of((name, 3000), b, i, cost, 0, 3000)
    assert want[3] >= 3000 and want[0][3000] < DBL_MAX and (want[0][3002:] == DBL_MAX).all()
    g = forward_only(gmx, b, i)
    g.sssp_path_f64(cost, 0, 3000)                                                # (the first call allocates)
    t0 = time.perf_counter()
    got, f = logged(g, cost, 0, 3000, capfd, **FORCED[forced])
    dt = time.perf_counter() - t0
    print("sssp_path_f64 %s %s: %.3f s, %s" % (name, forced, dt, f))
    check(want, got, (name, forced))
    assert dt < 10.0, "a round costs %.1f us" % (1e6 * dt / want[3])


# ---------------------------------------------------------------- upload forms: cost and prev_edge in the caller's slots
def _forms(gmx, b, i, rb, ri):
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"verbatim both CSRs": (True, 0, False), "SORT_ROWS": (True, S, True), "device-built reverse": (False, 0, True),
             "NO_REVERSE verbatim": (False, N, False), "SORT_ROWS|NO_REVERSE": (False, S | N, True)}
    for label, (rev, flags, mapped) in forms.items():
        g = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
        assert (g.edge_order() is not None) == mapped, label
        yield label, g
    L = gmx.lib()
    b64, rb64 = b.astype(np.int64), rb.astype(np.int64)
    for rev in (True, False):
        h = C.c_void_p()
        assert L.gmx_graph_upload_e64(b64.ctypes.data, i.ctypes.data, rb64.ctypes.data if rev else None, ri.ctypes.data if rev else None,
                                      len(b) - 1, len(i), 0, C.byref(h)) == 0
        yield "e64 %s" % ("verbatim" if rev else "device-built reverse"), gmx.Graph(h)


@pytest.mark.parametrize("name", ["multi64", "multi300", "rmat16_shuffled"])
def test_upload_forms(gmx, name):
    if name == "multi300":
        b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(300, 2000, 3))
        root = 5
    else:
        u = ugraph(name)
        b, i, rb, ri, root = u.begin, u.idx, u.rb, u.ri, u.hub
    assert rows_unsorted(b, i)
    cost = costs_of("ties", len(i))
    free = model_of((name, -1), b, i, cost, root, -1)                              # the loop on the rows as stored
    end = median_end(free[0])
    want = {-1: free, end: model_of((name, end), b, i, cost, root, end)}
    assert want[end][0].tobytes() != free[0].tobytes()
    for label, g in _forms(gmx, b, i, rb, ri):
        for e, w in want.items():
            for env in ({}, FORCED["no_tail"]) if name != "rmat16_shuffled" else ({},):
                with knobs(**env):
                    check(w, g.sssp_path_f64(cost, root, e), (name, label, e))
        g.free()


def test_ties_go_to_the_smallest_uploaded_slot(gmx):
    """Row 0 = [1, 2, 1, 1, 2] with costs [5, 1, 3, 3, 9]: vertex 1 is offered 3 by the uploaded slots 2 and 3 in round 1.  Slot
    2 must win, kept verbatim or sorted on the device (where it is device slot 1)."""
    begin = np.array([0, 5, 5, 5], np.int32)
    idx = np.array([1, 2, 1, 1, 2], np.int32)
    cost = np.array([5, 1, 3, 3, 9], np.float64)
    for sort in (False, True):
        flags = gmx.GMX_GRAPH_NO_REVERSE | (gmx.GMX_GRAPH_SORT_ROWS if sort else 0)
        g = gmx.Graph.upload(begin, idx, flags=flags)
        assert (g.edge_order() is not None) == sort
        for env in FORCED.values():
            with knobs(**env):
                dist, pn, pe, _ = g.sssp_path_f64(cost, 0)
            assert dist.tolist() == [0, 3, 1] and pn.tolist() == [-1, 0, 0] and pe.tolist() == [-1, 2, 1]


# ---------------------------------------------------------------- errors
def test_errors_leave_the_outputs_and_the_graph_alone(gmx):
    b, i, cost, root, end = shape("pruned")
    V, E = len(b) - 1, len(i)
    g = forward_only(gmx, b, i)
    L = gmx.lib()
    f = L.gmx_sssp_path_f64
    out = [np.full(V, 77.0), np.full(V, 77, np.int32), np.full(V, 77, np.int32)]
    ptr = [o.ctypes.data for o in out]
    for bad, word in ((-1.0, b"cost[4]"), (np.nan, b"cost[4]"), (-np.inf, b"cost[4]")):
        c = cost.copy()
        c[E - 1] = bad                                                            # the last slot
        assert f(g._h, root, end, c.ctypes.data, ptr[0], ptr[1], ptr[2], None) == GMX_ERR_ARG
        assert word in L.gmx_last_error(), L.gmx_last_error()
        with pytest.raises(gmx.GmxError, match="cost"):
            g.sssp_path_f64(c, root, end)
    c = cost.copy()
    c[1], c[3] = -2.0, np.nan
    assert f(g._h, root, end, c.ctypes.data, ptr[0], ptr[1], ptr[2], None) == GMX_ERR_ARG
    assert b"cost[1]" in L.gmx_last_error()                                       # the first offending slot
    for e in (V, -2, 1 << 30):
        assert f(g._h, root, e, cost.ctypes.data, ptr[0], ptr[1], ptr[2], None) == GMX_ERR_ARG
        assert b"end" in L.gmx_last_error()
    assert f(None, root, end, cost.ctypes.data, ptr[0], ptr[1], ptr[2], None) == GMX_ERR_ARG
    assert f(g._h, root, end, None, ptr[0], ptr[1], ptr[2], None) == GMX_ERR_ARG
    assert f(g._h, root, end, cost.ctypes.data, None, ptr[1], ptr[2], None) == GMX_ERR_ARG
    assert f(g._h, root, end, cost.ctypes.data, ptr[0], None, ptr[2], None) == GMX_ERR_ARG
    assert all((o == 77).all() for o in out)                                      # refused before anything is written
    # prev_edge and stats are optional; the graph is still usable
    assert f(g._h, root, end, cost.ctypes.data, ptr[0], ptr[1], None, None) == 0
    dist, pn, pe = PINNED["pruned"]
    assert out[0].tolist() == dist and out[1].tolist() == pn and (out[2] == 77).all()
    check(spf_model(b, i, cost, root, end), g.sssp_path_f64(cost, root, end))
    assert np.array_equal(g.hop_dist(0)[0][:4], [0, 1, 1, 2])


# ---------------------------------------------------------------- counters and scratch reuse
def test_pruning_walks_fewer_slots(gmx):
    b, i, cost, root, end = shape("pruned")
    g = forward_only(gmx, b, i)
    assert g.sssp_path_f64(cost, root, end)[3]["edges_examined"] == 4 and g.sssp_path_f64(cost, root, -1)[3]["edges_examined"] == 5


def test_calls_on_one_graph_are_independent(gmx):
    """The scratch is kept on the graph: a call after another one -- another root, another target, another path, the graph's
    other entries in between -- gives the bytes of a first call."""
    b, i = named_graph("rmat10")
    cost = costs_of("ties", len(i))
    root = int(np.argmax(np.diff(b)))
    free = model_of(("rmat10", "ties", -1), b, i, cost, root, -1)
    end = median_end(free[0])
    g = forward_only(gmx, b, i)
    first = g.sssp_path_f64(cost, root, end)
    again = g.sssp_path_f64(cost, root, end)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:3], again[:3]))
    assert first[3]["iterations"] == again[3]["iterations"] and first[3]["edges_examined"] == again[3]["edges_examined"]
    hop = g.hop_dist(root)[0]
    for r, e, env in ((root, -1, {}), (end, root, FORCED["no_tail"]), (root, end, FORCED["all_tail"]), (7, -1, {}), (root, end, {})):
        with knobs(**env):
            check(spf_model(b, i, cost, r, e), g.sssp_path_f64(cost, r, e), (r, e))
    check(spf_model(b, i, cost * 2, root, end), g.sssp_path_f64(cost * 2, root, end))
    assert np.array_equal(g.hop_dist(root)[0], hop)
    g.free()


# ---------------------------------------------------------------- the driver
def _driver(args):
    exe = os.path.join(PKG, "bin", "sssp_path_adj")
    assert os.path.exists(exe), "bin/sssp_path_adj not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"] + [str(a) for a in args],
                         stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0 and out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n"), out.stdout
    return out.stdout.splitlines()


def test_driver(gmx, golden):
    c = golden["cases"]["rmat8_noperm"]                                           # the graph of that file
    b, i = c["begin"], c["node_idx"]
    cost = gm_rand32_lengths(len(i)) / 10.0                                       # ((rand() % 100) + 1) / 10.0 in slot order
    root = int(np.argmax(np.diff(b)))
    free = spf_model(b, i, cost, root, -1)
    end = median_end(free[0])
    dist, pn, pe = spf_model(b, i, cost, root, end)[:3]
    path, total, n = [], 0.0, end
    while n != root:                                                              # get_path: from end backwards
        path.insert(0, n)
        total += float(cost[pe[n]])
        n = int(pn[n])
    lines = _driver([root, end])
    at = lines.index("%d -> %d" % (root, end))
    assert lines[at + 1] == "    Costs are %f" % total and lines[at + 2] == "    Number of links is %d" % len(path)
    links = ["        %d: %d - %d" % (pe[v], u, v) for u, v in zip([root] + path[:-1], path)][:20]
    assert lines[at + 3:at + 3 + len(links)] == links and len(path) >= 2
    far = np.flatnonzero(free[0] == DBL_MAX)
    assert len(far)
    lines = _driver([root, int(far[0])])
    assert "PATH NOT FOUND" in lines and not any("Costs are" in l for l in lines)
