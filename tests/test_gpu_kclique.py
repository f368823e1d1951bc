"""gmx_kclique on the device: the counts byte for byte against the one-thread model (kclique_model.py) or a closed form, and
the log line's classes against the model's orientation: the word boundaries of the bit rows, the recursion's depth for
every k, every size class and every knob that routes vertices between them, the batches of the global class, the plan shared
with gmx_clustering and gmx_ktruss, unsorted multigraphs uploaded three ways, the driver."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from kclique_sequences import LOG   # (importing it also adds kclique's row to the table of interleaved entries)
from kclique_model import (clique, clique_counts, hub_over, hub_over_counts, kclique_model, multipartite, multipartite_counts, orientation)
from test_gpu_scc import _shape
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_KCLIQUE_NO_ORDER", "GMX_KCLIQUE_CAP", "GMX_KCLIQUE_WAVE", "GMX_KCLIQUE_BATCH_BYTES", "GMX_KCLIQUE_PLAIN", "GMX_KCLIQUE_LOG",
         "GMX_KCLIQUE_PHASES", "GMX_KTRUSS_NO_ORDER", "GMX_LCC_NO_ORDER", "GMX_LCC_LOG", "GMX_TCD_NO_ORDER")
SIZES = (64, 65, 33, 1, 40, 70, 17, 30)


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def classes_of(up_len, k, cap=1024, wave=1):
    """The items fields the log line must show for these upper-list lengths."""
    d = np.asarray(up_len)
    live = d >= k - 1
    w = live & (d <= 64) if wave else np.zeros(len(d), bool)
    s = live & ~w & (d <= min(256, cap))
    l = live & ~w & ~s & (d <= cap)
    return {"wave": int(w.sum()), "small": int(s.sum()), "large": int(l.sum()), "glob": int((live & (d > cap)).sum()), "skipped": int((~live).sum())}


@pytest.fixture
def run(capfd, monkeypatch):
    def call(g, k, per_vertex=True, up_len=None, **knobs):
        """One call with GMX_KCLIQUE_LOG and the knobs given (no_order=1, cap=64, ...; the others unset): (count, cliques, stats,
        the log line's fields), the line checked against the results and, with up_len (the model's |UP'(v)| in the call's
        order), its classes too."""
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("GMX_KCLIQUE_LOG", "1")
        for name, v in knobs.items():
            monkeypatch.setenv("GMX_KCLIQUE_" + name.upper(), str(v))
        capfd.readouterr()
        cnt, n, st = g.kclique(k, per_vertex=per_vertex)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {key: (v if key in ("order", "counts") else int(v)) for key, v in m.groupdict().items()}
        assert f["V"] == g.V and f["E"] == g.E and f["k"] == k and f["cliques"] == n
        assert f["wave"] + f["small"] + f["large"] + f["glob"] + f["skipped"] == g.V
        assert f["order"] == ("identity" if "no_order" in knobs else "degree") and f["cap"] == knobs.get("cap", 1024)
        assert f["counts"] == ("none" if not per_vertex else "global" if "plain" in knobs else "lds")
        assert (f["batches"] > 0) == (f["glob"] > 0) and f["batches"] <= f["glob"]
        if knobs.get("wave") == 0:
            assert f["wave"] == 0
        assert st["iterations"] == 1 and st["h2d_ms"] == 0 and st["edges_examined"] == f["up"]
        assert st["kernel_ms"] > 0 or f["skipped"] == g.V   # (nothing is launched when every vertex is skipped)
        if per_vertex:
            assert cnt.dtype == np.int64 and len(cnt) == g.V and int(cnt.sum()) == k * n and st["vertices_reached"] == int((cnt > 0).sum())
        else:
            assert cnt is None and st["vertices_reached"] == 0
        if up_len is not None:
            want = classes_of(up_len, k, knobs.get("cap", 1024), knobs.get("wave", 1))
            assert {key: f[key] for key in want} == want and f["up"] == int(np.sum(up_len))
        return cnt, n, st, f
    return call


def graph_of(gmx, shape):
    V, s, d = shape
    return gmx.Graph.from_edges(V, s, d)


def up_len_of(g, ordered=True):
    begin, idx, _, _ = g.download(reverse=False)
    return np.array([bin(x).count("1") for x in orientation(g.V, begin, idx, ordered)[1]], np.int64)


def agrees(res, count, cliques):
    cnt, n, st, f = res
    assert n == cliques
    if cnt is not None:
        assert cnt.tobytes() == np.asarray(count, np.int64).tobytes()


_MODEL = {}


def model_of(name, g, k):
    """The model's result on graph g, computed once per (name, k) and shared."""
    if (name, k) not in _MODEL:
        begin, idx, _, _ = g.download(reverse=False)
        _MODEL[name, k] = kclique_model(g.V, begin, idx, k)
        _MODEL[name, k]["count"].setflags(write=False)
    return _MODEL[name, k]


# ---- 1: degenerate shapes
def test_empty_graph(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    for per_vertex in (True, False):
        cnt, n, st = g.kclique(4, per_vertex=per_vertex)
        assert (cnt is None or len(cnt) == 0) and n == 0 and st["iterations"] == 0


@pytest.mark.parametrize("name", ["no_edges", "one_vertex", "one_vertex_self_loop", "self_loops_only"])
def test_trivial_shapes_are_all_zero(gmx, capfd, monkeypatch, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    monkeypatch.setenv("GMX_KCLIQUE_LOG", "1")
    for again in (False, True):
        capfd.readouterr()
        for k in (3, 8):
            cnt, n, st = g.kclique(k)
            assert len(cnt) == V and not cnt.any() and n == 0 and (st["vertices_reached"], st["edges_examined"]) == (0, 0)
            assert g.kclique(k, per_vertex=False)[:2] == (None, 0)
        assert "gmx kclique" not in capfd.readouterr().err   # answered without a plan
        g.clustering()                                       # ... and again with the plan another entry built
        g.ktruss()


# ---- 2: cliques at the word boundaries of the bit rows
@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 66, 129, 257])
def test_cliques_at_word_boundaries(gmx, run, n):
    """The lowest vertex of K_n has n - 1 upper neighbours: 63, 64, 65, 128 and 256 are the ends of the rows' 64-bit words and
    of the wave and small classes."""
    g = graph_of(gmx, clique(n))
    up_len = np.arange(n)
    for k in (3, 4):
        want = clique_counts(n, k)
        for per_vertex in (True, False):
            for knobs in ({}, {"no_order": 1}, {"wave": 0}):
                res = run(g, k, per_vertex, up_len, **knobs)
                agrees(res, *want)
        assert res[3]["skipped"] == k - 1 and res[3]["glob"] == 0


def test_every_depth_on_a_clique(gmx, run):
    g = graph_of(gmx, clique(20))
    for k in range(3, 9):
        for per_vertex in (True, False):
            for knobs in ({}, {"wave": 0}, {"cap": 64, "wave": 0}):
                agrees(run(g, k, per_vertex, np.arange(20), **knobs), *clique_counts(20, k))
    g7 = graph_of(gmx, clique(7))
    cnt, n, st, f = run(g7, 8, True, np.arange(7))
    assert n == 0 and not cnt.any() and f["skipped"] == 7   # no vertex has seven upper neighbours


def test_every_depth_in_every_class(gmx, run):
    """Eight parts of ten: under the identity order the first part's vertices have 70 upper neighbours (two words a row), so
    they are in the small class, under CAP=64 in the global class, and every 8-clique starts at one of them."""
    sizes = (10,) * 8
    g = graph_of(gmx, multipartite(sizes))
    ul = up_len_of(g, False)
    assert int(ul.max()) == 70 and int((ul > 64).sum()) == 10
    ud = up_len_of(g, True)
    assert int(ud.max()) == 70   # every order is a tie
    for k in range(3, 9):
        want = multipartite_counts(sizes, k)
        for per_vertex in (True, False):
            res = run(g, k, per_vertex, ud)   # the degree order
            agrees(res, *want)
            assert res[3]["small"] == 10
        for knobs in ({}, {"cap": 64}, {"cap": 64, "batch_bytes": 4096}, {"cap": 64, "plain": 1}, {"wave": 0}):
            for per_vertex in (True, False):
                res = run(g, k, per_vertex, ul, no_order=1, **knobs)
                agrees(res, *want)
                assert (res[3]["glob"], res[3]["small"] > 0) == ((10, False) if "cap" in knobs else (0, True))
                assert "batch_bytes" not in knobs or res[3]["batches"] == 5   # 70 x 2 + 70 words in whole lines: 1792 bytes, two in 4096


# ---- 3: multipartite
@pytest.fixture(scope="module")
def parts(gmx):
    g = graph_of(gmx, multipartite(SIZES))
    return g, {True: up_len_of(g, True), False: up_len_of(g, False)}


@pytest.mark.parametrize("k", [3, 4, 5, 8])
def test_multipartite(gmx, run, parts, k):
    g, up_len = parts
    want = multipartite_counts(SIZES, k)
    assert k != 8 or want[1] == int(np.prod(SIZES, dtype=np.int64))   # one clique per choice of a vertex from every part
    # k = 8 has 2 x 10^11 cliques and a call takes seconds: the total under the degree order and the per-vertex bytes under the
    # identity order, which is the same kernel (small class, rows of four words) on longer lists; the per-vertex bytes of the
    # depth-6 walk under the degree order are test_every_depth_in_every_class's
    a = run(g, k, k != 8, up_len[True])
    agrees(a, *want)
    print("multipartite k = %d: %d cliques, kernel %.3f ms" % (k, a[1], a[2]["kernel_ms"]))
    b = run(g, k, True, up_len[False], no_order=1)
    agrees(b, *want)
    assert b[3]["small"] > 0 and int(up_len[False].max()) == 256 and a[3]["small"] > 0   # rows of more than one word
    if k != 8:
        agrees(run(g, k, False, up_len[False], no_order=1), *want)


def test_three_parts_hold_no_four_clique(gmx, run):
    g = graph_of(gmx, multipartite((4, 4, 4)))
    for knobs in ({}, {"no_order": 1}):
        assert run(g, 3, **knobs)[1] == 64
        cnt, n, st, f = run(g, 4, **knobs)
        assert n == 0 and not cnt.any() and st["vertices_reached"] == 0


# ---- 4: class routing
@pytest.mark.parametrize("k", [3, 4])
def test_knobs_route_the_vertices_and_change_no_byte(gmx, run, parts, k):
    """k = 3 is the thread-per-i_1 form of the workgroup kernels and k = 4 their wave-per-i_1 form; the deeper walks under the
    same knobs are test_every_depth_in_every_class's, on a shape with fewer cliques."""
    g, up_len = parts
    want = multipartite_counts(SIZES, k)
    for ordered in (True, False):
        order = {} if ordered else {"no_order": 1}
        ul = up_len[ordered]
        base = run(g, k, True, ul, **order)
        for knobs in ({"cap": 64}, {"wave": 0}, {"plain": 1}, {"cap": 64, "batch_bytes": 1}, {"cap": 64, "wave": 0, "plain": 1}, {"cap": 128}):
            for per_vertex in (True, False):
                res = run(g, k, per_vertex, ul, **knobs, **order)
                agrees(res, *want)
                f = res[3]
                if knobs.get("cap") == 64:
                    assert f["large"] == 0 and f["glob"] == int((ul > 64).sum()) > 0 and f["small"] == (0 if "wave" not in knobs else base[3]["wave"])
                if "batch_bytes" in knobs:
                    assert f["batches"] == f["glob"] >= 3   # a vertex that alone exceeds the budget is a batch by itself
                elif f["glob"]:
                    assert f["batches"] == 1
                if knobs == {"wave": 0}:
                    assert f["small"] == base[3]["small"] + base[3]["wave"]
                if knobs == {"cap": 128}:
                    assert f["large"] == 0 and f["small"] == int(((ul > 64) & (ul <= 128)).sum()) and f["glob"] == int((ul > 128).sum()) > 0
    # a few vertices per batch: the budget of three of the largest matrices
    words = lambda d: (d * ((d + 63) // 64) + d + 31) // 32 * 32
    res = run(g, k, True, up_len[False], cap=64, no_order=1, batch_bytes=3 * 8 * words(256))
    agrees(res, *want)
    assert 3 <= res[3]["batches"] < res[3]["glob"]


# ---- 5: the global class at the default cap
@pytest.mark.parametrize("k", [3, 4])
def test_hub_over_the_cap(gmx, run, k):
    sizes = (260, 260, 260, 260)
    g = graph_of(gmx, hub_over(multipartite(sizes)))
    want = hub_over_counts(lambda j: multipartite_counts(sizes, j), k)
    ul = up_len_of(g, False)
    assert int(ul[0]) == 1040 and int(ul[1:].max()) == 780
    for per_vertex in (True, False):
        res = run(g, k, per_vertex, ul, no_order=1)
        agrees(res, *want)
        assert res[3]["glob"] == 1 and res[3]["batches"] == 1 and res[3]["large"] == 780
    agrees(run(g, k, True, up_len_of(g, True)), *want)


# ---- 6, 7: RMAT against the model, and k = 3 against clustering()
RMATS = {"rmat10": (10, False, False), "rmat10p": (10, True, False), "rmat10s": (10, False, True), "rmat12": (12, False, False)}
RMAT_CASES = [("rmat10", 3), ("rmat10", 4), ("rmat10", 5), ("rmat10p", 3), ("rmat10p", 4), ("rmat10p", 5), ("rmat10s", 4), ("rmat12", 3), ("rmat12", 4)]


@pytest.fixture(scope="module")
def rmats(gmx):
    out = {}
    for name, (scale, permute, sym) in RMATS.items():
        g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
        g = g.symmetrize() if sym else g
        out[name] = (g, {True: up_len_of(g, True), False: up_len_of(g, False)})
    return out


@pytest.mark.parametrize("name,k", RMAT_CASES)
def test_rmat_against_the_model(gmx, run, rmats, name, k):
    g, up_len = rmats[name]
    want = model_of(name, g, k)
    assert want["cliques"] > 0 and np.array_equal(want["up_len"], up_len[True])
    a = run(g, k, True, up_len[True])
    agrees(a, want["count"], want["cliques"])
    print("%s k = %d: %d cliques, longest upper list %d, items %s" % (name, k, a[1], int(up_len[True].max()), {c: a[3][c] for c in ("wave", "small", "large", "glob", "skipped")}))
    assert a[3]["wave"] > 0 and (name != "rmat12" or a[3]["small"] > 0)   # the two sizes cover the wave and small classes without knobs
    for per_vertex, knobs in ((False, {}), (True, {"no_order": 1}), (True, {"wave": 0}), (True, {"plain": 1}), (True, {"cap": 64}), (False, {"cap": 64, "no_order": 1})):
        res = run(g, k, per_vertex, up_len["no_order" not in knobs], **knobs)
        agrees(res, want["count"], want["cliques"])
        if knobs.get("cap") == 64 and "no_order" in knobs:
            assert res[3]["glob"] > 0


@pytest.mark.parametrize("name", sorted(RMATS))
def test_k3_is_clustering(gmx, run, rmats, name):
    g, up_len = rmats[name]
    cnt, n, st, f = run(g, 3, True, up_len[True])
    tri, _, _, T, _, lst = g.clustering()
    assert cnt.tobytes() == tri.tobytes() and n == T and st["edges_examined"] == lst["edges_examined"] and st["vertices_reached"] == lst["vertices_reached"]
    if name == "rmat10s":   # symmetric and simple
        assert n == g.triangle_counting()[0]


# ---- 8: upload forms
@pytest.mark.parametrize("V,hub_edges", [(64, 200), (3000, 8000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    graphs = (gmx.Graph.upload(begin, idx, rb, ri, flags=0), gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS),
              gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE))
    ul = np.array([bin(x).count("1") for x in orientation(V, begin, idx)[1]], np.int64)
    for k in (3, 4):
        want = kclique_model(V, begin, idx, k)   # on the rows as stored
        assert want["cliques"] > 0
        for g in graphs:
            agrees(run(g, k, True, ul), want["count"], want["cliques"])
            agrees(run(g, k, False, ul, wave=0), want["count"], want["cliques"])


# ---- 9: one handle
def test_one_handle_shares_the_plan_with_ktruss_and_clustering(gmx, run, rmats):
    make = lambda: gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False)
    fresh = {k: run(make(), k) for k in (4, 5)}
    for k in (4, 5):
        assert (fresh[k][3]["built"], fresh[k][3]["classes_built"]) == (1, 1)
        agrees(fresh[k], model_of("rmat10", rmats["rmat10"][0], k)["count"], model_of("rmat10", rmats["rmat10"][0], k)["cliques"])
    kt0, lc0 = make().ktruss(), make().clustering()
    g = make()
    same = lambda a, b: a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    kt = g.ktruss()
    assert kt[0].tobytes() == kt0[0].tobytes() and kt[1].tobytes() == kt0[1].tobytes() and kt[2:4] == kt0[2:4]
    a = run(g, 4)
    assert (a[3]["built"], a[3]["classes_built"]) == (0, 1) and same(a, fresh[4])   # the plan ktruss built, plus the classes
    lc = g.clustering()
    assert lc[0].tobytes() == lc0[0].tobytes() and lc[2].tobytes() == lc0[2].tobytes() and lc[3:5] == lc0[3:5]
    b = run(g, 5)
    assert (b[3]["built"], b[3]["classes_built"]) == (0, 0) and same(b, fresh[5])
    c = run(g, 4)
    assert (c[3]["built"], c[3]["classes_built"]) == (0, 0) and same(c, fresh[4])
    d = run(g, 4, no_order=1)                                                       # the other order: rebuilt, and the classes with it
    assert (d[3]["built"], d[3]["classes_built"]) == (1, 1) and same(d, fresh[4])
    kt = g.ktruss()                                                                 # ... and back, by ktruss
    assert kt[0].tobytes() == kt0[0].tobytes() and kt[1].tobytes() == kt0[1].tobytes()
    e = run(g, 5)
    assert (e[3]["built"], e[3]["classes_built"]) == (0, 1) and same(e, fresh[5])
    assert g.clustering()[0].tobytes() == lc0[0].tobytes()
    assert same(run(g, 4), fresh[4])


def test_interleaved_with_the_other_entries_of_a_handle(gmx, run, rmats):
    """kclique between the entries that hold other state on the handle (the traversal object, the PageRank plans, the oriented
    copy of triangle_counting, the plan's other additions): every result stays the model's or the first call's, and a second
    pass over the same calls, the global class's workspace matrices included, does not grow the workspace."""
    L = gmx.lib()
    g = gmx.Graph.rmat(1 << 10, 16 << 10, 1997, 0.57, 0.19, 0.19, False).symmetrize()
    want = {k: model_of("rmat10s", rmats["rmat10s"][0], k) for k in (3, 4)}
    first, used = {}, None

    def same(name, got):
        got = tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in got)
        assert first.setdefault(name, got) == got, name

    for again in (False, True):
        same("hop_dist", g.hop_dist(0)[:1])
        agrees(run(g, 4), want[4]["count"], want[4]["cliques"])
        same("tcd", g.triangle_counting_directed()[:1])
        agrees(run(g, 3, False), want[3]["count"], want[3]["cliques"])
        rank = g.pagerank(0.001, 0.85, 20, np.float64)[0]
        assert np.allclose(first.setdefault("pagerank", rank), rank, rtol=1e-9, atol=0)
        res = run(g, 4, True, cap=64, no_order=1)   # the other order, and matrices in the workspace
        agrees(res, want[4]["count"], want[4]["cliques"])
        assert res[3]["glob"] > 0
        same("clustering", g.clustering()[:5])
        same("triangle_counting", g.triangle_counting()[:1])
        agrees(run(g, 3, True, plain=1), want[3]["count"], want[3]["cliques"])
        same("ktruss", g.ktruss()[:4])
        same("hop_dist 7", g.hop_dist(7)[:1])
        agrees(run(g, 4, True, wave=0), want[4]["count"], want[4]["cliques"])
        if again:
            assert L.gmx_workspace_bytes() == used
        used = L.gmx_workspace_bytes()
    assert used > 0 and first["clustering"][3] == want[3]["cliques"] == first["triangle_counting"][0]


# ---- 10: the driver
def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "kclique")
    assert os.path.exists(exe), "bin/kclique not built"
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    for args, k in (([], 4), (["4"], 4), (["3"], 3)):
        out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"] + args, stdout=subprocess.PIPE, text=True,
                             timeout=120, cwd=ROOT)
        assert out.returncode == 0, out.stdout
        m = kclique_model(256, c["begin"], c["node_idx"], k)
        assert m["cliques"] > 0
        top = int(np.argmax(m["count"]))   # the lowest id with the largest count
        for line in ("k = %d\n" % k, "cliques = %d\n" % m["cliques"], "max_count = %d\n" % int(m["count"][top]), "top = %d\n" % top):
            assert line in out.stdout, (line, out.stdout)
    bad = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null", "9"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert bad.returncode != 0
