"""gmx_msf on the device: in_forest, count, total, iterations and edges_examined against the host model of the schedule
(test_msf_host.msf_model, itself checked against Kruskal there), against pure-Python Kruskal up to RMAT-12, a certificate
that needs no model, every knob and upload form, and the driver."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_gpu_sssp_path import gm_rand32_lengths
from test_msf_host import ceil_log2, kruskal, msf_model, ruler
from test_upload_forms_host import unsorted_multigraph as _unsorted_multigraph

pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_MSF_TAIL", "GMX_MSF_LOG", "GMX_MSF_PHASES")
LOG = re.compile(r"gmx msf: V (\d+) E (\d+) reverse ([01]) rounds (\d+) grid_rounds (\d+) tail_rounds (\d+) slots (\d+) forest_edges (\d+) "
                 r"weight (-?\d+) comps (\d+)\n")
LOG_FIELDS = ("V", "E", "reverse", "rounds", "grid_rounds", "tail_rounds", "slots", "forest_edges", "weight", "comps")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def ends(g):
    """(src, dst, slot) of every device slot: its ends and the uploaded slot it came from."""
    begin, idx, _, _ = g.download(reverse=False)
    order = g.edge_order()
    return np.repeat(np.arange(g.V), np.diff(begin)), idx.astype(np.int64), np.arange(g.E) if order is None else order.astype(np.int64)


def model_of(g, w):
    src, dst, slot = ends(g)
    return msf_model(g.V, src, dst, w, slot)


def check(g, w, m=None, by_kruskal=False):
    """msf(components=True) equal to the model (m: computed before) in every output and statistic."""
    m = model_of(g, w) if m is None else m
    sel, n, total, comp, nc, st = g.msf(w, components=True)
    assert sel.dtype == bool and sel.shape == (g.E,) and comp.dtype == np.int32
    assert np.array_equal(sel, m["in_forest"])
    assert (n, total, nc) == (m["count"], m["total"], g.V - m["count"])
    assert np.array_equal(comp, m["comp"])
    assert (st["iterations"], st["edges_examined"]) == (m["rounds"], m["slots"])
    assert st["iterations"] <= ceil_log2(g.V)
    assert st["vertices_reached"] == (int(np.bincount(m["comp"]).max()) if g.V else 0)
    sel2, n2, total2, st2 = g.msf(w)   # without the components: the same bytes, no component array
    assert sel2.tobytes() == sel.tobytes() and (n2, total2) == (n, total) and st2["vertices_reached"] == 0
    assert (st2["iterations"], st2["edges_examined"]) == (m["rounds"], m["slots"])
    if by_kruskal:
        src, dst, slot = ends(g)
        up = np.argsort(slot)   # the slots in uploaded order
        ww = np.zeros(g.E, np.int64) if w is None else np.asarray(w)
        assert np.array_equal(sel, kruskal(g.V, src[up], dst[up], ww))
    return sel, n, total, comp, nc, st


def logged(g, w, capfd, monkeypatch):
    monkeypatch.setenv("GMX_MSF_LOG", "1")
    capfd.readouterr()
    out = g.msf(w, components=True)
    err = capfd.readouterr().err
    monkeypatch.delenv("GMX_MSF_LOG")
    mt = LOG.search(err)
    assert mt, err
    f = dict(zip(LOG_FIELDS, map(int, mt.groups())))
    st = out[-1]
    assert f["V"] == g.V and f["E"] == g.E
    assert f["grid_rounds"] + f["tail_rounds"] == f["rounds"] == st["iterations"] and f["slots"] == st["edges_examined"]
    assert (f["forest_edges"], f["weight"], f["comps"]) == (out[1], out[2], out[4])
    return out, f


def test_degenerate_inputs(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    sel, n, total, comp, nc, st = g.msf(components=True)
    assert len(sel) == 0 and len(comp) == 0 and (n, total, nc) == (0, 0, 0) and st["iterations"] == 0 and st["edges_examined"] == 0
    g = gmx.Graph.from_edges(1000, [], [])
    sel, n, total, comp, nc, st = g.msf(components=True)
    assert len(sel) == 0 and (n, total, nc) == (0, 0, 1000) and np.array_equal(comp, np.arange(1000)) and st["iterations"] == 0
    g = gmx.Graph.from_edges(300, np.arange(300), np.arange(300))   # self loops only: read and ignored
    sel, n, total, comp, nc, st = check(g, np.full(300, -5), by_kruskal=True)
    assert not sel.any() and (n, total, nc) == (0, 0, 300) and st["iterations"] == 0 and st["edges_examined"] == 300


def test_one_edge(gmx):
    g = gmx.Graph.from_edges(2, [1], [0])
    sel, n, total, comp, nc, st = check(g, [-7], by_kruskal=True)
    assert sel.tolist() == [True] and (n, total, nc) == (1, -7, 1) and st["iterations"] == 1 and st["edges_examined"] == 2


@pytest.mark.parametrize("w,want", [([5, 5], [True, False]), ([5, 4], [False, True]), ([4, 5], [True, False])])
def test_two_slots_between_one_pair(gmx, w, want):
    g = gmx.Graph.upload([0, 1, 2], [1, 0])   # slot 0: 0 -> 1, slot 1: 1 -> 0
    sel, n, total, comp, nc, st = check(g, w, by_kruskal=True)
    assert sel.tolist() == want and n == 1 and total == min(w)
    h = gmx.Graph.upload([0, 2, 2, 2], [2, 2])   # a repeated slot: the lower one
    assert check(h, [3, 3], by_kruskal=True)[0].tolist() == [True, False]


def test_triangle_with_equal_weights(gmx):
    g = gmx.Graph.upload([0, 1, 2, 3], [1, 2, 0])
    sel, n, total, comp, nc, st = check(g, [1, 1, 1], by_kruskal=True)
    assert sel.tolist() == [True, True, False] and st["iterations"] == 1


def test_grid_with_equal_weights(gmx):
    k = 64
    v = np.arange(k * k).reshape(k, k)
    s = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    d = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    g = gmx.Graph.from_edges(k * k, s, d)
    sel, n, total, comp, nc, st = check(g, np.full(g.E, 9), by_kruskal=True)
    assert n == k * k - 1 and nc == 1 and total == 9 * n
    assert check(g, None)[0].tobytes() == sel.tobytes()


def test_ascending_path_merges_in_one_round(gmx):
    P = 1 << 16
    g = gmx.Graph.from_edges(P, np.arange(P - 1), np.arange(1, P))
    sel, n, total, comp, nc, st = check(g, np.arange(P - 1))
    assert sel.all() and nc == 1 and st["iterations"] == 1 and st["vertices_reached"] == P


def test_ruler_path_takes_log2_rounds(gmx):
    P = 1 << 12
    g = gmx.Graph.from_edges(P, np.arange(P - 1), np.arange(1, P))
    sel, n, total, comp, nc, st = check(g, ruler(P - 1), by_kruskal=True)
    assert sel.all() and st["iterations"] == 12


@pytest.mark.parametrize("name", ["star_out", "star_in"])
def test_star_one_row_across_many_tiles(gmx, name):
    L = 60000
    hub, leaves = np.zeros(L, np.int64), np.arange(1, L + 1)
    g = gmx.Graph.from_edges(L + 1, *((hub, leaves) if name == "star_out" else (leaves, hub)))
    w = np.random.default_rng(4).integers(0, 4, L)
    sel, n, total, comp, nc, st = check(g, w)
    assert sel.all() and nc == 1 and st["iterations"] == 1


def test_extreme_weights(gmx):
    rng = np.random.default_rng(8)
    V, E = 3000, 12000
    g = gmx.Graph.from_edges(V, rng.integers(0, V, E), rng.integers(0, V, E))
    w = rng.choice(np.array([INT32_MIN, -1, 0, INT32_MAX], np.int64), g.E)
    sel, n, total, comp, nc, st = check(g, w, by_kruskal=True)
    assert total == int(w[sel].sum()) and (w[sel] == INT32_MIN).any() and (w[sel] == INT32_MAX).any()


def certificate(gmx_mod, g, sel, n, comp, nc):
    """Model-independent: the selected slots alone are acyclic and span exactly the weak components."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    src, dst, slot = ends(g)
    on = sel[slot]
    parts = connected_components(csr_matrix((np.ones(int(on.sum()), np.int8), (src[on], dst[on])), shape=(g.V, g.V)), directed=True, connection="weak")[0]
    wcomp, wn, _ = g.wcc()
    assert parts == wn == nc and n == g.V - nc     # V - n parts from n slots: no slot closes a cycle
    assert np.array_equal(comp, wcomp)


@pytest.fixture(scope="module")
def rmat_case(gmx):
    cache = {}

    def get(scale, permute):
        if (scale, permute) not in cache:
            cache.clear()   # (one graph at a time)
            cache[(scale, permute)] = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
        return cache[(scale, permute)]
    return get


@pytest.fixture(scope="module")
def driver_weights():
    return gm_rand32_lengths(16 << 14)   # drawn once; a smaller graph takes a prefix, as the driver's stream does


@pytest.mark.parametrize("weights", ["ties", "driver"])
@pytest.mark.parametrize("scale,permute", [(s, p) for s in (8, 10, 12, 14) for p in (False, True)])
def test_rmat(gmx, rmat_case, driver_weights, scale, permute, weights):
    g = rmat_case(scale, permute)
    w = np.random.default_rng(scale).integers(0, 4, g.E) if weights == "ties" else driver_weights[:g.E]
    sel, n, total, comp, nc, st = check(g, w, by_kruskal=scale <= 12)
    assert nc > 1 and st["kernel_ms"] > 0
    certificate(gmx, g, sel, n, comp, nc)


def test_rmat16(gmx, rmat_case):
    g = rmat_case(16, False)
    w = np.random.default_rng(16).integers(1, 101, g.E)
    sel, n, total, comp, nc, st = check(g, w)
    certificate(gmx, g, sel, n, comp, nc)


def test_tail_knob_rmat14(gmx, rmat_case, capfd, monkeypatch):
    g = rmat_case(14, False)
    w = np.random.default_rng(14).integers(0, 4, g.E)
    m = model_of(g, w)
    base, f = logged(g, w, capfd, monkeypatch)
    seen = {}
    for tail in (0, 1024, 1 << 30):
        monkeypatch.setenv("GMX_MSF_TAIL", str(tail))
        check(g, w, m)
        out, f = logged(g, w, capfd, monkeypatch)
        assert out[0].tobytes() == base[0].tobytes() and out[3].tobytes() == base[3].tobytes() and out[1:3] == base[1:3]
        assert (out[-1]["iterations"], out[-1]["edges_examined"]) == (m["rounds"], m["slots"]) and f["reverse"] == 1
        seen[tail] = f
    assert seen[0]["tail_rounds"] == 0 and seen[0]["grid_rounds"] == m["rounds"]
    assert seen[1 << 30]["tail_rounds"] == m["rounds"] and seen[1 << 30]["grid_rounds"] == 0
    # the tail takes over at the first round whose list holds at most 1024 slots
    small = [r for r, s in enumerate(m["per_round"]) if s <= 1024]
    assert seen[1024]["grid_rounds"] == (min(small) if small else m["rounds"])


def test_no_reverse_csr_gives_the_same_bytes(gmx, rmat_case, capfd, monkeypatch):
    g = rmat_case(14, False)
    w = np.random.default_rng(14).integers(0, 4, g.E)
    begin, idx, _, _ = g.download(reverse=False)
    h = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
    want = g.msf(w, components=True)
    out, f = logged(h, w, capfd, monkeypatch)
    assert f["reverse"] == 0
    assert out[0].tobytes() == want[0].tobytes() and out[3].tobytes() == want[3].tobytes() and out[1:3] == want[1:3]
    assert (out[-1]["iterations"], out[-1]["edges_examined"]) == (want[-1]["iterations"], want[-1]["edges_examined"])


@pytest.mark.parametrize("V,hub_edges", [(64, 200), (150000, 400000)])
def test_unsorted_multigraph_verbatim_and_sorted(gmx, V, hub_edges, monkeypatch):
    begin, idx, rb, ri = _unsorted_multigraph(V, hub_edges, V)
    assert np.any(np.diff(idx[begin[5]:begin[6]]) < 0)   # the hub's row really is unsorted
    w = np.random.default_rng(V).integers(-2, 3, len(idx))   # by uploaded slot
    g = gmx.Graph.upload(begin, idx, rb, ri, flags=0)
    assert g.edge_order() is None
    sel, n, total, comp, nc, st = check(g, w, by_kruskal=V == 64)
    sorted_g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS)
    assert sorted_g.edge_order() is not None                 # the gather of the weights and the scatter of the flags
    sel2, n2, total2, comp2, nc2, st2 = check(sorted_g, w)
    assert sel2.tobytes() == sel.tobytes() and (n2, total2, nc2) == (n, total, nc) and np.array_equal(comp2, comp)
    assert (st2["iterations"], st2["edges_examined"]) == (st["iterations"], st["edges_examined"])
    for tail in (0, 1 << 30):
        monkeypatch.setenv("GMX_MSF_TAIL", str(tail))
        assert sorted_g.msf(w)[0].tobytes() == sel.tobytes()


def test_no_weights_equal_zero_weights(gmx, rmat_case):
    g = rmat_case(12, True)
    a = g.msf(None, components=True)
    b = g.msf(np.zeros(g.E, np.int32), components=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1:3] == b[1:3] and a[2] == 0 and a[3].tobytes() == b[3].tobytes()
    assert (a[-1]["iterations"], a[-1]["edges_examined"]) == (b[-1]["iterations"], b[-1]["edges_examined"])
    check(g, None, by_kruskal=True)


def test_repeatable_and_hop_dist_unchanged(gmx, rmat_case):
    g = rmat_case(14, True)
    w = np.random.default_rng(3).integers(1, 101, g.E)
    roots = [0, 1, 777, 12345]
    before = [g.hop_dist(r)[0] for r in roots]
    a = g.msf(w, components=True)
    b = g.msf(w, components=True)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes() and a[1:3] == b[1:3] and a[4] == b[4]
    assert (a[-1]["iterations"], a[-1]["edges_examined"], a[-1]["vertices_reached"]) == (b[-1]["iterations"], b[-1]["edges_examined"], b[-1]["vertices_reached"])
    for x, r in zip(before, roots):
        assert np.array_equal(g.hop_dist(r)[0], x)


def test_dropin_driver(gmx, golden, driver_weights):
    exe = os.path.join(PKG, "bin", "msf")
    assert os.path.exists(exe), "bin/msf not built"

    def report(m, V):
        return ["forest_edges = %d\n" % m["count"], "total_weight = %d\n" % m["total"], "num_components = %d\n" % (V - m["count"]),
                "rounds = %d\n" % m["rounds"]]
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    begin, idx = np.asarray(c["begin"], np.int64), np.asarray(c["node_idx"], np.int64)
    m = msf_model(256, np.repeat(np.arange(256), np.diff(begin)), idx, driver_weights[:len(idx)])
    for line in report(m, 256):
        assert line in out.stdout, (line, out.stdout)
    out = subprocess.run([exe, "RMAT:12", "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    g = gmx.Graph.rmat(1 << 12, 16 << 12, 1997, 0.57, 0.19, 0.19, False)
    for line in report(model_of(g, driver_weights[:g.E]), g.V):
        assert line in out.stdout, (line, out.stdout)
