"""gmx_route_* and gmx_bidir_dijkstra (bidir_dijkstra.gm / sssp_dijkstra.gm) on the device against test_route_host: flag and
cost are dijkstra_cost's, exactly; the returned route passes valid_route on the caller's arrays (which route is not
specified).  Every hand shape under both searches and every tail setting -- shown to be what ran by the library's
GMX_ROUTE_LOG line -- random multigraphs, named graphs with many pairs interleaved on one route object, every upload form
with path_edge in the caller's slots, the shape on which searching from both ends must pay off, early exit, thousands of
rounds on a chain, cap, errors, the driver and the generated entries on a gm_graph."""
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
from test_gpu_sssp_path_adj import _forms
from test_route_host import (INT_MAX, SHAPES, dijkstra_all, dijkstra_cost, random_case, route_of_parents, shape, tree4, valid_route)
from test_upload_forms_host import rows_unsorted, ugraph, unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_ROUTE_SIDES", "GMX_ROUTE_TAIL", "GMX_ROUTE_LOG")
HUGE = "2000000000"
TAILS = {"default": {}, "no_tail": {"GMX_ROUTE_TAIL": "0"}, "all_tail": {"GMX_ROUTE_TAIL": HUGE}}
SIDES = {"both": {"GMX_ROUTE_SIDES": "both"}, "forward": {"GMX_ROUTE_SIDES": "forward"}}
LINE = re.compile(r"gmx route: V (\d+) E (\d+) src (-?\d+) dst (-?\d+) sides (both|forward); tail (\d+); rounds F (\d+) grid \+ (\d+) tail, "
                  r"R (\d+) grid \+ (\d+) tail in (\d+) launches; slots F (\d+) R (\d+); queued (\d+); found ([01]) cost (-?\d+) meet (-?\d+) "
                  r"hops (\d+); ms ([0-9.]+)")
FIELDS = ("V", "E", "src", "dst", "sides", "tail_from", "f_grid", "f_tail", "r_grid", "r_tail", "tail_launches", "f_slots", "r_slots", "queued",
          "found", "cost", "meet", "hops", "ms")
_DIST = {}


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


def logged(route, src, dst, capfd, cap=None, **env):
    """(the query's result, the fields of the library's line)."""
    capfd.readouterr()
    with knobs(GMX_ROUTE_LOG="1", **env):
        got = route.query(src, dst, cap)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    return got, {k: (v if k == "sides" else float(v) if k == "ms" else int(v)) for k, v in zip(FIELDS, lines[0])}


def check(b, i, w, src, dst, want, got, label=None):
    """Flag and cost exactly, the route on the caller's arrays, the counters of an answer."""
    found, cost, pn, pe, hops, st = got
    assert pn.dtype == np.int32 and pe.dtype == np.int32
    assert (found, cost) == (want is not None, want), label
    if found:
        assert hops == len(pn) == len(pe), label
        assert valid_route(b, i, w, src, dst, pn, pe, cost) is None, (label, valid_route(b, i, w, src, dst, pn, pe, cost))
    else:
        assert hops == 0 and len(pn) == 0, label
    assert st["kernel_ms"] >= 0 and st["h2d_ms"] == 0, label


def dist_of(key, b, i, w, src):
    """dijkstra_all, computed once per case and shared between the tests."""
    if key not in _DIST:
        _DIST[key] = dijkstra_all(b, i, w, src)
        _DIST[key].setflags(write=False)
    return _DIST[key]


def want_of(dist, v):
    return None if dist[v] == INT_MAX else int(dist[v])


# ---------------------------------------------------------------- the hand shapes, both searches, every tail setting
@pytest.mark.parametrize("tail", sorted(TAILS))
@pytest.mark.parametrize("sides", sorted(SIDES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hand_shapes(gmx, capfd, name, sides, tail):
    b, i, w, src, dst, found, cost = shape(name)
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    env = dict(SIDES[sides], **TAILS[tail])
    got, f = logged(r, src, dst, capfd, **env)
    check(b, i, w, src, dst, cost, got, (name, sides, tail))
    st = got[5]
    assert f["sides"] == sides and (f["found"], f["cost"]) == (int(found), cost if found else -1) and f["hops"] == got[4]
    assert st["iterations"] == f["f_grid"] + f["f_tail"] + f["r_grid"] + f["r_tail"] and st["edges_examined"] == f["f_slots"] + f["r_slots"]
    assert st["vertices_reached"] == f["queued"]
    if sides == "forward":
        assert f["r_grid"] == f["r_tail"] == f["r_slots"] == 0
    if tail == "no_tail":
        assert f["f_tail"] == f["r_tail"] == f["tail_launches"] == 0
    if tail == "all_tail":
        assert f["f_grid"] == f["r_grid"] == 0 and f["tail_launches"] <= 1
    if src != dst and name != "tiny_reverse" and name != "one_way":
        assert st["iterations"] > 0
    with knobs(**env):
        hit, parent, parent_edge, st2 = g.bidir_dijkstra(w, src, dst)
    assert hit == found and st2["h2d_ms"] > 0
    nodes, edges = route_of_parents(parent, parent_edge, src, dst)
    if found:
        assert valid_route(b, i, w, src, dst, nodes, edges, cost) is None
    on = np.zeros(len(b) - 1, bool)
    on[nodes] = True                                                               # -1 everywhere off the route, and on src
    assert (parent[~on] == -1).all() and (parent_edge[~on] == -1).all() and (parent[on] != -1).all() and not on[src]
    r.free()
    g.free()


def test_default_knobs(gmx, capfd):
    b, i, w, src, dst, _, _ = shape("meet_not_best")
    g = gmx.Graph.upload(b, i)
    _, f = logged(g.route(w), src, dst, capfd)
    assert f["sides"] == "both" and f["tail_from"] == 4096
    g2 = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE)
    _, f = logged(g2.route(w), src, dst, capfd)
    assert f["sides"] == "forward"


# ---------------------------------------------------------------- random multigraphs
@pytest.mark.parametrize("block", range(4))
def test_random_multigraphs(gmx, capfd, block):
    envs = [dict(s, **t) for s in SIDES.values() for t in TAILS.values()] + [{}]
    for seed in range(block * 100, block * 100 + 100):                            # 400 graphs
        b, i, w, src, dst = random_case(seed)
        want = dijkstra_cost(b, i, w, src, dst)
        no_reverse = seed % 3 == 0
        g = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE if no_reverse else 0)
        r = g.route(w)
        env = envs[seed % len(envs)]
        got, f = logged(r, src, dst, capfd, **env)
        check(b, i, w, src, dst, want, got, seed)
        if no_reverse:
            assert f["sides"] == "forward" and f["r_slots"] == 0, seed
        r.free()
        g.free()


# ---------------------------------------------------------------- named graphs: two weight draws, many pairs on one object
def weights_of(draw, E):
    rng = np.random.default_rng(E + 23)
    return (rng.integers(0, 4, E) if draw == "ties" else rng.integers(1, 101, E)).astype(np.int32)   # many ties with zeros / 1 .. 100


@pytest.mark.parametrize("draw", ["ties", "1to100"])
@pytest.mark.parametrize("name", ["rmat10", "rmat12", "rmat12s", "uniform", "star33"])
def test_named_graphs(gmx, capfd, name, draw):
    b, i = named_graph(name)
    w = weights_of(draw, len(i))
    hub = int(np.argmax(np.diff(b)))                                               # the top hub
    dist = dist_of((name, draw), b, i, w, hub)
    fin = np.flatnonzero(dist != INT_MAX)
    order = fin[np.argsort(dist[fin], kind="stable")]
    targets = {"median": int(order[len(order) // 2]), "farthest": int(order[-1]), "hub": hub}
    far = np.flatnonzero(dist == INT_MAX)
    if len(far):
        targets["unreachable"] = int(far[0])
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    first = None
    for env in ({}, dict(SIDES["forward"], **TAILS["no_tail"]), TAILS["all_tail"] if name in ("rmat10", "star33") else TAILS["no_tail"]):
        for label, t in targets.items():                                           # interleaved on ONE object
            got, f = logged(r, hub, t, capfd, **env)
            check(b, i, w, hub, t, want_of(dist, t), got, (name, draw, label, env))
            if first is None:
                first = (t, got)
                print("route %s %s -> %s: %s" % (name, draw, label, f))
    t, got = first
    again = r.query(hub, t)                                                        # the scratch is reused: same answer
    assert again[:2] == got[:2]
    check(b, i, w, hub, t, want_of(dist, t), again, "again")
    back = r.query(targets["median"], hub)                                         # and the other way round
    check(b, i, w, targets["median"], hub, dijkstra_cost(b, i, w, targets["median"], hub), back, "back")
    r.free()
    g.free()


# ---------------------------------------------------------------- upload forms: weight and path_edge in the caller's slots
@pytest.mark.parametrize("name", ["multi64", "multi300", "rmat16_shuffled"])
def test_upload_forms(gmx, capfd, name):
    if name == "multi300":
        b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(300, 2000, 3))
        hub = 5
    else:
        u = ugraph(name)
        b, i, rb, ri, hub = u.begin, u.idx, u.rb, u.ri, u.hub
    assert rows_unsorted(b, i)
    w = weights_of("ties" if name != "rmat16_shuffled" else "1to100", len(i))
    dist = dist_of((name, "forms"), b, i, w, hub)
    fin = np.flatnonzero(dist != INT_MAX)
    order = fin[np.argsort(dist[fin], kind="stable")]
    targets = [int(order[len(order) // 2]), int(order[-1]), int(order[len(order) // 4])]
    for label, g in _forms(gmx, b, i, rb, ri):
        r = g.route(w)
        reverse_found_edges = 0
        for t in targets:
            got, f = logged(r, hub, t, capfd)
            check(b, i, w, hub, t, want_of(dist, t), got, (name, label, t))        # path_edge: a slot of b / i as uploaded
            assert f["sides"] == ("forward" if "NO_REVERSE" in label else "both"), label
            reverse_found_edges += f["meet"] != t
        if "NO_REVERSE" not in label:
            assert reverse_found_edges > 0, label                                  # edges after the meeting vertex are the reverse side's
            with knobs(**SIDES["forward"]):
                check(b, i, w, hub, targets[0], want_of(dist, targets[0]), r.query(hub, targets[0]), (name, label, "forward"))
        hit, parent, parent_edge, _ = g.bidir_dijkstra(w, hub, targets[0])
        nodes, edges = route_of_parents(parent, parent_edge, hub, targets[0])
        assert hit and valid_route(b, i, w, hub, targets[0], nodes, edges, int(dist[targets[0]])) is None, label
        r.free()
        g.free()


# ---------------------------------------------------------------- searching from both ends must pay off
def test_both_ends_walk_a_fraction_of_the_tree(gmx):
    """A complete 4-ary out-tree of depth 6, root -> a leaf: one-sided search settles every level above the leaf (about 5460
    slots), the reverse side walks a chain of six in-edges.  The ratio is above 100 for any policy that prefers the smaller
    queue; 4 is slack."""
    V, b, i = tree4(6)
    w = np.ones(len(i), np.int32)
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    res = {}
    for sides in SIDES:
        with knobs(**SIDES[sides]):
            res[sides] = r.query(0, V - 1)
        check(b, i, w, 0, V - 1, 6, res[sides], sides)
    both, fwd = res["both"][5]["edges_examined"], res["forward"][5]["edges_examined"]
    print("route tree4(6): slots both %d forward %d" % (both, fwd))
    assert both * 4 <= fwd
    r.free()
    g.free()


def test_early_exit_when_a_side_drains(gmx):
    """tiny_reverse at V = 5461: dst has no in-edges, so the answer is known before the forward ball is walked."""
    V, b, i = tree4(6, cut_last=True)
    w = np.ones(len(i), np.int32)
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    got = r.query(0, V - 1)
    check(b, i, w, 0, V - 1, None, got)
    assert got[5]["edges_examined"] < len(i)
    with knobs(**SIDES["forward"]):                                               # one-sided: the whole ball, the same flag
        check(b, i, w, 0, V - 1, None, r.query(0, V - 1))
    r.free()
    g.free()


# ---------------------------------------------------------------- thousands of rounds
@pytest.mark.parametrize("tail", sorted(TAILS))
@pytest.mark.parametrize("name", ["path4096", "chain4096"])
def test_long_chains(gmx, capfd, name, tail):
    b, i = named_graph(name)
    w = np.random.default_rng(4096).integers(1, 4, len(i)).astype(np.int32)
    dist = dist_of((name, "chain"), b, i, w, 0)
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    r.query(0, 1)                                                                  # (warm-up: code objects)
    t0 = time.perf_counter()
    got, f = logged(r, 0, 3000, capfd, **TAILS[tail])
    dt = time.perf_counter() - t0
    print("route %s %s: %.3f s, %s" % (name, tail, dt, f))
    check(b, i, w, 0, 3000, int(dist[3000]), got, (name, tail))
    assert got[4] == 3000 and got[5]["iterations"] >= 2900                         # a hop per round, from one end or the other
    if tail == "default":
        assert dt < 10.0, "a round costs %.1f us" % (1e6 * dt / got[5]["iterations"])
    r.free()
    g.free()


# ---------------------------------------------------------------- cap
def test_cap_smaller_than_hops(gmx):
    b, i = named_graph("chain4096")
    w = np.ones(len(i), np.int32)
    g = gmx.Graph.upload(b, i)
    r = g.route(w)
    found, cost, pn, pe, hops, _ = r.query(5, 105, cap=10)
    assert found and cost == 100 and hops == 100 and pn.tolist() == list(range(6, 16)) and pe.tolist() == list(range(5, 15))
    found, cost, pn, pe, hops, _ = r.query(5, 105, cap=0)
    assert found and cost == 100 and hops == 100 and len(pn) == 0
    L = gmx.lib()
    out = [np.full(12, 77, np.int32), np.full(12, 77, np.int32)]
    hit, c, h = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    assert L.gmx_route_query(r._h, 5, 105, C.byref(hit), C.byref(c), out[0].ctypes.data, out[1].ctypes.data, 10, C.byref(h), None) == 0
    assert h.value == 100 and out[0].tolist() == list(range(6, 16)) + [77, 77] and out[1].tolist() == list(range(5, 15)) + [77, 77]
    assert L.gmx_route_query(r._h, 5, 105, C.byref(hit), C.byref(c), None, None, 10, C.byref(h), None) == 0 and h.value == 100
    r.free()
    g.free()


# ---------------------------------------------------------------- errors
def test_errors_leave_the_outputs_and_the_graph_alone(gmx):
    b, i, w, src, dst, _, cost = shape("meet_not_best")
    V, E = len(b) - 1, len(i)
    g = gmx.Graph.upload(b, i)
    L = gmx.lib()
    h = C.c_void_p(77)
    bad = w.copy()
    bad[E - 1] = -1                                                               # the last slot
    assert L.gmx_route_create(g._h, bad.ctypes.data, C.byref(h)) == GMX_ERR_ARG and h.value is None
    assert b"weight[%d]" % (E - 1) in L.gmx_last_error(), L.gmx_last_error()
    bad[1], bad[3] = -2, -5
    assert L.gmx_route_create(g._h, bad.ctypes.data, C.byref(h)) == GMX_ERR_ARG and h.value is None
    assert b"weight[1]" in L.gmx_last_error()                                     # the first offending slot
    with pytest.raises(gmx.GmxError, match="weight"):
        g.route(bad)
    assert L.gmx_route_create(None, w.ctypes.data, C.byref(h)) == GMX_ERR_ARG
    assert L.gmx_route_create(g._h, None, C.byref(h)) == GMX_ERR_ARG
    assert L.gmx_route_create(g._h, w.ctypes.data, None) == GMX_ERR_ARG
    r = g.route(w)
    hit, c, hops = C.c_int32(77), C.c_int64(77), C.c_int64(77)
    out = [np.full(V, 77, np.int32), np.full(V, 77, np.int32)]
    q = L.gmx_route_query
    for s, d, word in ((V, dst, b"src"), (-1, dst, b"src"), (src, V, b"dst"), (src, -2, b"dst"), (1 << 30, dst, b"src")):
        assert q(r._h, s, d, C.byref(hit), C.byref(c), out[0].ctypes.data, out[1].ctypes.data, V, C.byref(hops), None) == GMX_ERR_ARG
        assert word in L.gmx_last_error()
        with pytest.raises(gmx.GmxError):
            r.query(s, d)
    assert q(None, src, dst, C.byref(hit), C.byref(c), out[0].ctypes.data, out[1].ctypes.data, V, C.byref(hops), None) == GMX_ERR_ARG
    assert q(r._h, src, dst, None, C.byref(c), out[0].ctypes.data, out[1].ctypes.data, V, C.byref(hops), None) == GMX_ERR_ARG
    assert q(r._h, src, dst, C.byref(hit), None, out[0].ctypes.data, out[1].ctypes.data, V, C.byref(hops), None) == GMX_ERR_ARG
    assert q(r._h, src, dst, C.byref(hit), C.byref(c), out[0].ctypes.data, out[1].ctypes.data, V, None, None) == GMX_ERR_ARG
    assert q(r._h, src, dst, C.byref(hit), C.byref(c), out[0].ctypes.data, out[1].ctypes.data, -1, C.byref(hops), None) == GMX_ERR_ARG
    par = [np.full(V, 77, np.int32), np.full(V, 77, np.int32)]
    f = L.gmx_bidir_dijkstra
    assert f(g._h, bad.ctypes.data, src, dst, par[0].ctypes.data, par[1].ctypes.data, C.byref(hit), None) == GMX_ERR_ARG
    assert f(g._h, w.ctypes.data, V, dst, par[0].ctypes.data, par[1].ctypes.data, C.byref(hit), None) == GMX_ERR_ARG
    assert f(g._h, w.ctypes.data, src, dst, None, par[1].ctypes.data, C.byref(hit), None) == GMX_ERR_ARG
    assert f(g._h, w.ctypes.data, src, dst, par[0].ctypes.data, par[1].ctypes.data, None, None) == GMX_ERR_ARG
    assert f(g._h, None, src, dst, par[0].ctypes.data, par[1].ctypes.data, C.byref(hit), None) == GMX_ERR_ARG
    # refused before anything is written
    assert (hit.value, c.value, hops.value) == (77, 77, 77) and all((o == 77).all() for o in out + par)
    # parent_edge and stats are optional; the route object and the graph are still usable
    assert f(g._h, w.ctypes.data, src, dst, par[0].ctypes.data, None, C.byref(hit), None) == 0 and hit.value == 1
    assert (par[1] == 77).all() and par[0][src] == -1 and par[0][dst] != -1
    check(b, i, w, src, dst, cost, r.query(src, dst))
    assert np.array_equal(g.hop_dist(0)[0], [0, 1, 1, 2, 3, 2])
    r.free()
    g.free()


def test_empty_graphs(gmx):
    L = gmx.lib()
    e = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))           # V = 0
    h = C.c_void_p()
    assert L.gmx_route_create(e._h, None, C.byref(h)) == 0 and h.value
    hit, c, hops = C.c_int32(77), C.c_int64(77), C.c_int64(77)
    assert L.gmx_route_query(h, 0, 0, C.byref(hit), C.byref(c), None, None, 0, C.byref(hops), None) == GMX_ERR_ARG   # no vertex to ask for
    assert L.gmx_route_free(h) == 0
    par = np.full(1, 77, np.int32)
    assert L.gmx_bidir_dijkstra(e._h, None, 0, 0, par.ctypes.data, None, C.byref(hit), None) == 0 and hit.value == 0 and par[0] == 77
    g = gmx.Graph.upload(np.zeros(6, np.int32), np.zeros(0, np.int32))           # E = 0
    r = g.route(np.zeros(0, np.int32))
    for sides in SIDES.values():
        with knobs(**sides):
            assert r.query(2, 4)[:2] == (False, None) and r.query(3, 3)[:2] == (True, 0) and r.query(3, 3)[4] == 0
    hit, parent, parent_edge, _ = g.bidir_dijkstra(np.zeros(0, np.int32), 2, 4)
    assert not hit and (parent == -1).all() and (parent_edge == -1).all()
    hit, parent, parent_edge, _ = g.bidir_dijkstra(np.zeros(0, np.int32), 2, 2)
    assert hit and (parent == -1).all() and (parent_edge == -1).all()
    r.free()


# ---------------------------------------------------------------- the driver
QUERY = re.compile(r"(TEST \[ +(\d+) \] )?weight +(-?\d+) ,hops +(-?\d+), time +([0-9]+\.[0-9]{2}) path=(NO_PATH_EXISTS|(?:v\d+=>)+)$")


def _driver(args):
    exe = os.path.join(PKG, "bin", "bidir_dijkstra")
    assert os.path.exists(exe), "bin/bidir_dijkstra not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"] + [str(a) for a in args],
                         stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0 and out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n"), out.stdout
    return [m.groups() for m in map(QUERY.match, out.stdout.splitlines()) if m]


def test_driver(gmx, golden, tmp_path):
    c = golden["cases"]["rmat8_noperm"]                                           # the graph of that file
    b, i = c["begin"], c["node_idx"]
    w = gm_rand32_lengths(len(i))                                                 # (rand() % 100) + 1 in slot order
    hub = int(np.argmax(np.diff(b)))
    dist = dijkstra_all(b, i, w, hub)
    fin = np.flatnonzero(dist != INT_MAX)
    order = fin[np.argsort(dist[fin], kind="stable")]
    far = np.flatnonzero(dist == INT_MAX)
    assert len(far)
    end = int(order[-1])

    def expect(line, n, s, d):
        prefix, k, weight, hops, _, path = line
        want = dijkstra_cost(b, i, w, s, d)
        assert (prefix is None) == (n is None) and (n is None or int(k) == n)
        if want is None:
            assert (int(weight), int(hops), path) == (-1, -1, "NO_PATH_EXISTS")
        else:
            vs = [int(x) for x in re.findall(r"v(\d+)=>", path)]
            assert int(weight) == want and vs[0] == s and len(vs) == min(int(hops), 4) and int(hops) >= 2
            if int(hops) <= 4:
                assert vs[-1] == d
            assert all(v2 in i[b[v1]:b[v1 + 1]] for v1, v2 in zip(vs, vs[1:]))    # the printed vertices are joined by edges

    lines = _driver([hub, end])
    assert len(lines) == 1
    expect(lines[0], None, hub, end)
    pairs = [(hub, end), (hub, int(far[0])), (int(order[len(order) // 2]), hub), (end, hub)]
    path = tmp_path / "pairs.txt"
    path.write_text("".join("%d %d\n" % p for p in pairs))
    lines = _driver([0, 0, path, 3])                                              # the first three lines of the file
    assert len(lines) == 3
    for n, (line, (s, d)) in enumerate(zip(lines, pairs)):
        expect(line, n + 1, s, d)


# ---------------------------------------------------------------- the drop-in entries, through gm_graph
DROPIN_CC = r"""
#include "bidir_dijkstra.h"
#include "sssp_dijkstra.h"
#include <stdio.h>
#include <vector>
typedef bool (*entry_t)(gm_graph&, int32_t*, node_t&, node_t&, node_t*, edge_t*);
static void run(const char* what, entry_t f, gm_graph& G, std::vector<int32_t>& w, node_t src, node_t dst) {
    std::vector<node_t> parent((size_t) G.num_nodes(), 77);
    std::vector<edge_t> parent_edge((size_t) G.num_nodes(), 77);
    gm_node_seq Q;
    const bool found = f(G, w.data(), src, dst, parent.data(), parent_edge.data());
    const int32_t total = found ? get_path(G, src, dst, parent.data(), parent_edge.data(), w.data(), Q) : -1;
    printf("%s %d -> %d: %d %d:", what, (int) src, (int) dst, (int) found, (int) total);
    gm_node_seq::seq_iter it = Q.prepare_seq_iteration();
    while (it.has_next()) printf(" %d", (int) it.get_next());
    int off = 0;
    for (node_t v = 0; v < G.num_nodes(); v++) off += parent[(size_t) v] == gm_graph::NIL_NODE && parent_edge[(size_t) v] == gm_graph::NIL_EDGE;
    printf(" | %d\n", off);
}
int main() {
    gm_graph G;                                       // meet_not_best plus 5 -> 0, rows in slot order
    const int s[7] = {0, 0, 1, 2, 3, 4, 5}, d[7] = {1, 2, 5, 3, 4, 5, 0};
    std::vector<int32_t> w = {3, 1, 3, 1, 1, 1, 7};
    for (int v = 0; v < 7; v++) G.add_node();         // vertex 6 has no edges
    for (int e = 0; e < 7; e++) G.add_edge(s[e], d[e]);
    G.freeze();
    run("bidir", &bidir_dijkstra, G, w, 0, 5);
    run("dijkstra", &dijkstra, G, w, 0, 5);
    run("bidir", &bidir_dijkstra, G, w, 4, 2);
    run("dijkstra", &dijkstra, G, w, 0, 6);
    run("bidir", &bidir_dijkstra, G, w, 6, 0);
    run("bidir", &bidir_dijkstra, G, w, 3, 3);
    return 0;
}
"""


@pytest.mark.parametrize("edge64", [False, True])
def test_drop_in_entries(gmx, tmp_path, edge64):
    """bidir_dijkstra() and dijkstra() of the generated headers on a gm_graph, get_path on what they return; with edge_t
    64 bits wide the slots pass through a temporary."""
    from test_host_cpp import CXX_FLAGS, LINK, LINK64
    src, prog = str(tmp_path / "dropin.cc"), str(tmp_path / "dropin")
    open(src, "w").write(DROPIN_CC)
    lib = LINK64 if edge64 else LINK
    assert os.path.exists(lib[0]), "%s not built" % lib[0]
    subprocess.check_call(["g++"] + CXX_FLAGS + (["-DGM_EDGE64"] if edge64 else []) + ["-Wall", "-Werror", src, "-o", prog] + lib)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([prog], stdout=subprocess.PIPE, text=True, check=True, timeout=120, env=env).stdout.splitlines()
    # found, the route's weight, the vertices after src | vertices with NIL parent and NIL parent edge (all but the route's)
    assert out == ["bidir 0 -> 5: 1 4: 2 3 4 5 | 3", "dijkstra 0 -> 5: 1 4: 2 3 4 5 | 3", "bidir 4 -> 2: 1 9: 5 0 2 | 4",
                   "dijkstra 0 -> 6: 0 -1: | 7", "bidir 6 -> 0: 0 -1: | 7", "bidir 3 -> 3: 1 0: | 7"]
