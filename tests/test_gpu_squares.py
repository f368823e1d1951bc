"""gmx_squares on the device: the counts byte for byte against the one-thread forms (squares_model.py) or a closed form, and
the log line's classes, wedges and batches against what the schedule's D and W give under the knobs in force: every class
forced by knobs, with and without count_host, under the degree and the identity order; the class boundaries; a counter past
2^16 added to by several workgroups; tables with many distinct keys; the batches of the global class; the plan and the adjacency shared
with gmx_ktruss, gmx_clustering and gmx_kclique; unsorted multigraphs uploaded three ways; the driver."""
import os
import subprocess
from math import comb

import numpy as np
import pytest

from conftest import GOLD, ROOT
from squares_sequences import LOG   # (importing it also adds squares' row to the table of interleaved entries)
from squares_model import (LDS_SLOTS, SPLIT, WAVE_MAX, binary_tree, bipartite, bipartite_counts, classes_of, clique, clique_counts, cycle, grid, grid_counts,
                           hypercube, hypercube_counts, knobs_in_force, path, squares_definition, squares_schedule, star)
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_SQUARES_NO_ORDER", "GMX_SQUARES_WAVE_MAX", "GMX_SQUARES_LDS_SLOTS", "GMX_SQUARES_BATCH_BYTES", "GMX_SQUARES_SPLIT", "GMX_SQUARES_PLAIN",
         "GMX_SQUARES_LOG", "GMX_SQUARES_PHASES", "GMX_KCLIQUE_NO_ORDER", "GMX_KTRUSS_NO_ORDER", "GMX_KTRUSS_LOG", "GMX_LCC_NO_ORDER", "GMX_TCD_NO_ORDER")
# the knob sets that force every class on a small graph (the vertices the wave class loses go to the block class, those the
# block class loses -- W > 32 -- to the global class, where SPLIT = 16 cuts them into several workgroups), and PLAIN in each
FORCED = ({}, {"wave_max": 0}, {"wave_max": 0, "lds_slots": 64}, {"wave_max": 0, "lds_slots": 64, "split": 16}, {"plain": 1},
          {"wave_max": 0, "lds_slots": 64, "split": 16, "plain": 1})


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
    def call(g, per_vertex=True, sched=None, **knobs):
        """One call with GMX_SQUARES_LOG and the knobs given (no_order=1, wave_max=0, ...; the others unset): (count, squares,
        stats, the log line's fields), the line checked against the results and, with sched (the schedule model's result
        in the call's order), its classes, wedges and batches too."""
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("GMX_SQUARES_LOG", "1")
        for name, v in knobs.items():
            monkeypatch.setenv("GMX_SQUARES_" + name.upper(), str(v))
        capfd.readouterr()
        cnt, n, st = g.squares(per_vertex=per_vertex)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {key: (v if key in ("order", "counts") else int(v)) for key, v in m.groupdict().items()}
        assert f["V"] == g.V and f["E"] == g.E and f["squares"] == n
        assert f["wave"] + f["block"] + f["glob"] + f["skipped"] == g.V and f["nsplit"] <= f["glob"]
        assert f["order"] == ("identity" if "no_order" in knobs else "degree")
        assert {key: f[key] for key in ("wave_max", "lds_slots", "split", "batch_bytes")} == knobs_in_force(**knobs)
        assert f["counts"] == ("none" if not per_vertex else "global" if "plain" in knobs else "lds")
        assert (f["batches"] > 0) == (f["glob"] > 0) and f["batches"] <= f["glob"]
        assert st["iterations"] == 1 and st["h2d_ms"] == 0 and st["edges_examined"] == f["wedges"] and st["kernel_ms"] > 0
        if per_vertex:
            assert cnt.dtype == np.int64 and len(cnt) == g.V and int(cnt.sum()) == 4 * n and st["vertices_reached"] == int((cnt > 0).sum())
        else:
            assert cnt is None and st["vertices_reached"] == 0
        if sched is not None:
            want = classes_of(sched["D"], sched["W"], **knobs)
            got = {"wave": f["wave"], "block": f["block"], "glob": f["glob"], "split": f["nsplit"], "skipped": f["skipped"], "batches": f["batches"]}
            assert got == want and f["wedges"] == sched["wedges"] and f["up"] == sched["up"]
        return cnt, n, st, f
    return call


def graph_of(gmx, shape):
    V, s, d = shape
    return gmx.Graph.from_edges(V, s, d)


def schedules_of(g, orders=(True, False)):
    """The schedule model of graph g under the degree order and the identity order: {True: ..., False: ...}."""
    begin, idx, _, _ = g.download(reverse=False)
    out = {ordered: squares_schedule(g.V, begin, idx, ordered) for ordered in orders}
    assert out[orders[0]]["count"].tobytes() == out[orders[-1]]["count"].tobytes()
    for s in out.values():
        s["count"].setflags(write=False)
    return out


def agrees(res, count, squares):
    cnt, n, st, f = res
    assert n == squares
    if cnt is not None:
        assert cnt.tobytes() == np.asarray(count, np.int64).tobytes()


def everywhere(run, g, sched, count, squares, forced=FORCED):
    """Every forced class, with and without count_host, under both orders; the classes the runs went through."""
    seen = {"wave": 0, "block": 0, "glob": 0, "nsplit": 0}
    for ordered in (True, False):
        for knobs in forced:
            for per_vertex in (True, False):
                res = run(g, per_vertex, sched[ordered], **knobs, **({} if ordered else {"no_order": 1}))
                agrees(res, count, squares)
                for key in seen:
                    seen[key] += res[3][key]
    return seen


# ---- 1: degenerate shapes
def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    for per_vertex in (True, False):
        cnt, n, st = g.squares(per_vertex=per_vertex)
        assert (cnt is None or len(cnt) == 0) and n == 0 and st["iterations"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, capfd, monkeypatch, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    monkeypatch.setenv("GMX_SQUARES_LOG", "1")
    for again in (False, True):
        capfd.readouterr()
        cnt, n, st = g.squares()
        assert len(cnt) == V and not cnt.any() and n == 0 and (st["vertices_reached"], st["edges_examined"], st["iterations"]) == (0, 0, 1)
        assert g.squares(per_vertex=False)[:2] == (None, 0)
        assert "gmx squares" not in capfd.readouterr().err   # answered without a plan
        g.clustering()                                       # ... and again with the plan another entry built
        g.ktruss()


@pytest.mark.parametrize("name,shape", [("C3", cycle(3)), ("C5", cycle(5)), ("path", path(9)), ("star", star(70)), ("tree", binary_tree(127))])
def test_shapes_without_a_square(gmx, run, name, shape):
    g = graph_of(gmx, shape)
    seen = everywhere(run, g, schedules_of(g), np.zeros(g.V, np.int64), 0)
    assert name != "star" or seen["wave"] + seen["block"] > 0   # the centre has lower neighbours and no wedge: it is launched


def test_one_square(gmx, run):
    g = graph_of(gmx, cycle(4))
    seen = everywhere(run, g, schedules_of(g), [1, 1, 1, 1], 1)
    assert seen["wave"] > 0 and seen["block"] > 0 and seen["glob"] == 0   # two wedges: no knob sends them to the global class


# ---- 2: closed forms, every class forced
SHAPES = {"K4": (clique(4), clique_counts(4)), "K5": (clique(5), clique_counts(5)), "K64": (clique(64), clique_counts(64)), "K65": (clique(65), clique_counts(65)),
          "K257": (clique(257), clique_counts(257)), "K40,40": (bipartite(40, 40), bipartite_counts(40, 40)), "K3,300": (bipartite(3, 300), bipartite_counts(3, 300)),
          "grid5x7": (grid(5, 7), grid_counts(5, 7)), "grid33x65": (grid(33, 65), grid_counts(33, 65))}
SHAPES.update({"Q%d" % d: (hypercube(d), hypercube_counts(d)) for d in range(3, 9)})


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_closed_forms_in_every_class(gmx, run, name):
    shape, (count, squares) = SHAPES[name]
    g = graph_of(gmx, shape)
    seen = everywhere(run, g, schedules_of(g), count, squares)
    assert squares > 0 and seen["wave"] > 0 and seen["block"] > 0
    if name not in ("K4", "K5", "grid5x7", "grid33x65", "Q3", "Q4", "Q5", "Q6"):   # (no vertex of these has more than 32 wedges, the least LDS_SLOTS / 2)
        assert seen["glob"] > 0 and seen["nsplit"] > 0
    if name == "K257":   # the highest vertex walks 256 x 255 wedges: at the defaults the block and the global class are not empty either
        f = run(g, True)[3]
        assert f["block"] > 0 and f["glob"] > 0 and f["nsplit"] > 0


# ---- 3: the class boundaries, on K_{2,n}: under the degree order the higher hub walks one wedge per leaf
def two_hubs(n):
    return np.concatenate([np.full(2, comb(n, 2)), np.full(n, n - 1)]).astype(np.int64), comb(n, 2)


@pytest.mark.parametrize("n,knobs,where", [(40, {"wave_max": 40}, "wave"), (41, {"wave_max": 40}, "block"), (WAVE_MAX, {}, "wave"), (WAVE_MAX + 1, {}, "block"),
                                           (100, {"wave_max": 0, "lds_slots": 200}, "block"), (101, {"wave_max": 0, "lds_slots": 200}, "glob"),
                                           (LDS_SLOTS // 2, {}, "block"), (LDS_SLOTS // 2 + 1, {}, "glob")])
def test_class_boundaries(gmx, run, n, knobs, where):
    g = graph_of(gmx, bipartite(2, n))
    sched = schedules_of(g)
    assert sched[True]["W"].tolist() == [0] * (n + 1) + [n]
    for per_vertex in (True, False):
        res = run(g, per_vertex, sched[True], **knobs)
        agrees(res, *two_hubs(n))
        # the other hub has no wedge: it is in the lowest class there is
        lowest = "wave" if knobs.get("wave_max", WAVE_MAX) > 0 else "block"
        want = {"wave": 0, "block": 0, "glob": 0}
        want[lowest] += 1
        want[where] += 1
        assert {key: res[3][key] for key in want} == want and res[3]["skipped"] == n


def test_a_counter_past_two_to_the_sixteenth(gmx, run):
    n = 65600
    g = graph_of(gmx, bipartite(2, n))
    sched = schedules_of(g, (True,))   # (under the identity order the leaves walk 4 x 10^9 wedges)
    assert int(sched[True]["W"].max()) == n > SPLIT > LDS_SLOTS // 2
    for knobs in ({}, {"split": 1024}, {"split": 1 << 20}):   # 17, 65 and one workgroups add to that one counter
        for per_vertex in (True, False):
            res = run(g, per_vertex, sched[True], **knobs)
            agrees(res, *two_hubs(n))
            assert (res[3]["glob"], res[3]["nsplit"], res[3]["batches"]) == (1, int(knobs.get("split", SPLIT) < n), 1)


# ---- 4: table pressure and the batches
def test_many_distinct_keys_and_the_batches(gmx, run):
    """K_{3,300} under the identity order: leaf k walks 3 k wedges to k distinct leaves, three to each.  With LDS_SLOTS at its
    minimum the block class only holds W <= 32, in tables of 64 slots; a wave's slice takes up to 42 keys in 252 slots; the
    others are the global class, whose vertices need 64 .. 320 counters each."""
    g = graph_of(gmx, bipartite(3, 300))
    sched = schedules_of(g)
    count, squares = bipartite_counts(3, 300)
    W = sched[False]["W"]
    assert W.tolist() == [0, 0, 0] + [3 * k for k in range(300)]
    nglob = int((W > 128).sum())
    for per_vertex in (True, False):
        res = run(g, per_vertex, sched[False], no_order=1, lds_slots=64)
        agrees(res, count, squares)
        assert (res[3]["glob"], res[3]["batches"], res[3]["block"]) == (nglob, 1, 0) and res[3]["wave"] == 300 - nglob
        res = run(g, per_vertex, sched[False], no_order=1, lds_slots=64, wave_max=0)
        agrees(res, count, squares)
        assert res[3]["block"] == int((W[3:] <= 32).sum()) == 11 and res[3]["glob"] == 289 and res[3]["batches"] == 1
        res = run(g, per_vertex, sched[False], no_order=1, lds_slots=64, wave_max=0, batch_bytes=1)   # every global vertex a batch by itself
        agrees(res, count, squares)
        assert res[3]["batches"] == res[3]["glob"] == 289
        res = run(g, per_vertex, sched[False], no_order=1, lds_slots=64, wave_max=0, batch_bytes=3 * 4 * 320, split=100)   # about three vertices a batch
        agrees(res, count, squares)
        assert 289 // 15 <= res[3]["batches"] <= 97 and res[3]["nsplit"] == int((W > 100).sum())   # 64 .. 320 counters a vertex
    agrees(run(g, True, sched[False], no_order=1, lds_slots=64, wave_max=0, batch_bytes=1, plain=1), count, squares)


# ---- 5: RMAT against the model
RMATS = {"rmat10": (10, False, False), "rmat10p": (10, True, False), "rmat10s": (10, False, True), "rmat12": (12, False, False)}


@pytest.fixture(scope="module")
def rmats(gmx):
    out = {}
    for name, (scale, permute, sym) in RMATS.items():
        g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
        g = g.symmetrize() if sym else g
        out[name] = (g, schedules_of(g))
    begin, idx, _, _ = out["rmat10"][0].download(reverse=False)
    d = squares_definition(1 << 10, begin, idx)   # the other form, once
    assert d["count"].tobytes() == out["rmat10"][1][True]["count"].tobytes() and d["squares"] == out["rmat10"][1][True]["squares"]
    return out


@pytest.mark.parametrize("name", sorted(RMATS))
def test_rmat_against_the_model(gmx, run, rmats, name):
    g, sched = rmats[name]
    want = sched[True]
    assert want["squares"] > 0
    a = run(g, True, sched[True])
    agrees(a, want["count"], want["squares"])
    print("%s: %d squares, %d wedges, most wedges at a vertex %d, items %s" % (name, a[1], a[3]["wedges"], int(want["W"].max()),
                                                                              {c: a[3][c] for c in ("wave", "block", "glob", "nsplit", "skipped")}))
    assert a[3]["wave"] > 0 and a[3]["block"] > 0   # both LDS classes at the defaults, at either size
    for per_vertex, knobs in ((False, {}), (True, {"no_order": 1}), (False, {"no_order": 1}), (True, {"wave_max": 0}), (True, {"lds_slots": 256}), (False, {"lds_slots": 256}),
                              (True, {"plain": 1}), (True, {"lds_slots": 256, "split": 2048}), (False, {"lds_slots": 256, "split": 2048}),
                              (True, {"lds_slots": 64, "wave_max": 0, "split": 64, "plain": 1, "batch_bytes": 1 << 16})):
        res = run(g, per_vertex, sched["no_order" not in knobs], **knobs)
        agrees(res, want["count"], want["squares"])
        if "lds_slots" in knobs:
            assert res[3]["glob"] > 0 and ("split" not in knobs or res[3]["nsplit"] > 0)
        if "batch_bytes" in knobs:
            assert res[3]["batches"] > 1


# ---- 6: upload forms
@pytest.mark.parametrize("V,hub_edges", [(64, 200), (3000, 8000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    graphs = (gmx.Graph.upload(begin, idx, rb, ri, flags=0), gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS),
              gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE))
    want = squares_schedule(V, begin, idx)   # on the rows as stored
    assert want["squares"] > 0
    for g in graphs:
        agrees(run(g, True, want), want["count"], want["squares"])
        agrees(run(g, False, want, wave_max=0, lds_slots=64), want["count"], want["squares"])


# ---- 7: one handle
def test_one_handle_shares_the_plan_and_the_adjacency(gmx, run, rmats, capfd, monkeypatch):
    make = lambda: gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    want = rmats["rmat10"][1][True]
    built = lambda r: (r[3]["built"], r[3]["adj_built"], r[3]["classes_built"])
    same = lambda r: r[0].tobytes() == want["count"].tobytes() and r[1] == want["squares"]

    def ktruss_line(g):
        monkeypatch.setenv("GMX_KTRUSS_LOG", "1")
        capfd.readouterr()
        kt = g.ktruss()
        err = capfd.readouterr().err
        monkeypatch.delenv("GMX_KTRUSS_LOG")
        assert " adj_built " in err, err
        return kt, int(err.split(" adj_built ")[1][0])

    fresh = run(make())
    assert built(fresh) == (1, 1, 1) and same(fresh)
    kt0, lc0, kc0 = make().ktruss(), make().clustering(), make().kclique(4)
    g = make()
    a = run(g)
    assert built(a) == (1, 1, 1) and same(a)
    kt, adj = ktruss_line(g)                                                       # ktruss after squares: the adjacency is there
    assert adj == 0 and kt[0].tobytes() == kt0[0].tobytes() and kt[1].tobytes() == kt0[1].tobytes() and kt[2:4] == kt0[2:4]
    assert built(run(g)) == (0, 0, 0)
    lc = g.clustering()
    assert lc[0].tobytes() == lc0[0].tobytes() and lc[2].tobytes() == lc0[2].tobytes() and lc[3:5] == lc0[3:5]
    kc = g.kclique(4)
    assert kc[0].tobytes() == kc0[0].tobytes() and kc[1] == kc0[1]
    b = run(g, True, wave_max=0)
    assert built(b) == (0, 0, 0) and same(b)
    c = run(g, True, no_order=1)                                                   # the other order: rebuilt, and the additions with it
    assert built(c) == (1, 1, 1) and same(c)
    kt, adj = ktruss_line(g)                                                       # ... and back, by ktruss, which builds the adjacency first
    assert adj == 1 and kt[0].tobytes() == kt0[0].tobytes() and kt[1].tobytes() == kt0[1].tobytes()
    d = run(g)
    assert built(d) == (0, 0, 1) and same(d)
    h = make()                                                                     # squares on the plan and adjacency ktruss built
    h.ktruss()
    e = run(h)
    assert built(e) == (0, 0, 1) and same(e)
    assert h.clustering()[0].tobytes() == lc0[0].tobytes() and g.kclique(4)[0].tobytes() == kc0[0].tobytes()
    assert same(run(g)) and same(run(h))


def test_interleaved_with_the_other_entries_of_a_handle(gmx, run, rmats):
    """squares between the entries that hold other state on the handle: every result stays the model's or the first call's,
    and a second pass over the same calls, the global class's counters included, does not grow the workspace."""
    L = gmx.lib()
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    want = rmats["rmat10s"][1][True]
    first, used = {}, None

    def same(name, got):
        got = tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in got)
        assert first.setdefault(name, got) == got, name

    for again in (False, True):
        same("hop_dist", g.hop_dist(0)[:1])
        agrees(run(g), want["count"], want["squares"])
        same("tcd", g.triangle_counting_directed()[:1])
        agrees(run(g, False), want["count"], want["squares"])
        same("kclique", g.kclique(4)[:2])
        res = run(g, True, lds_slots=64, wave_max=0, no_order=1)   # the other order, and counters in the workspace
        agrees(res, want["count"], want["squares"])
        assert res[3]["glob"] > 0
        same("clustering", g.clustering()[:5])
        same("triangle_counting", g.triangle_counting()[:1])
        agrees(run(g, True, plain=1), want["count"], want["squares"])
        same("ktruss", g.ktruss()[:4])
        agrees(run(g, True, lds_slots=64, split=256), want["count"], want["squares"])
        if again:
            assert L.gmx_workspace_bytes() == used
        used = L.gmx_workspace_bytes()
    assert used > 0


# ---- 8: the driver
def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "squares")
    assert os.path.exists(exe), "bin/squares not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    m = squares_definition(256, c["begin"], c["node_idx"])
    assert m["squares"] > 0
    top = int(np.argmax(m["count"]))   # the lowest id with the largest count
    for line in ("squares = %d\n" % m["squares"], "max_count = %d\n" % int(m["count"][top]), "top = %d\n" % top):
        assert line in out.stdout, (line, out.stdout)
