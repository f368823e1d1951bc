"""gmx_adamic_adar (adamicAdar.gm) on the device against the host restatements of test_adamic_adar_host.py: hand-made
shapes, the staged and the in-memory path on the same inputs, RMAT graphs (every edge up to scale 16, a sample above),
every upload form, the statistics, repeatability, the drop-in driver, and that the graph's cached state is left alone.

Comparison rule per edge with k common-neighbour slots: the same inf positions, exact +0.0 where 0.0 is expected, no NaN,
otherwise |got - want| <= (k + 2) * 2^-52 * want.  (Each term differs between the device and glibc by at most about
4 * 2^-53 -- log within 1 ulp on each side over arguments >= 2, two correctly rounded divisions -- and adding k
non-negative terms in any order adds at most (k - 1) * 2^-53 on each side.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import GOLD, ROOT
from test_adamic_adar_host import aa_by_iterator, aa_vectorised, example_multigraph, golden_graphs, k3
from test_upload_forms_host import sort_rows, ugraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
AA_CAP = 1024   # gmx_tc.hip: row entries a wave stages


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def compare(got, want, k, label=""):
    """The comparison rule; returns the worst |got - want| / bound over the finite non-zero edges (0 when there is none)."""
    assert got.shape == want.shape
    assert not np.isnan(got).any(), label
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), label
    assert (got[inf] > 0).all(), label
    zero = want == 0.0
    assert (got[zero] == 0.0).all() and not np.signbit(got[zero]).any(), label
    m = ~inf & ~zero
    if not m.any():
        return 0.0
    bound = (k[m] + 2) * 2.0 ** -52 * want[m]
    ratio = np.abs(got[m] - want[m]) / bound
    worst = float(ratio.max())
    print("adamic_adar %s: %d edges, %d finite non-zero, %d inf, worst error / bound = %.4f" % (label, len(want), int(m.sum()), int(inf.sum()), worst))
    assert worst <= 1.0, (label, worst)
    return worst


def check_whole(g, label=""):
    """Every edge of a device graph whose slots are the uploaded ones (built on the device, or uploaded in order)."""
    begin, idx, _, _ = g.download(reverse=False)
    want, k = aa_vectorised(begin, idx)
    got = g.adamic_adar()
    st = g.last_stats
    worst = compare(got, want, k, label)
    assert st["edges_examined"] == int(k.sum()), label
    assert st["iterations"] == 1
    if len(idx):
        assert st["kernel_ms"] > 0
    return got, want, k, worst


def from_pyoracle(gmx, og):
    return gmx.Graph.upload(og.begin, og.node_idx, flags=gmx.GMX_GRAPH_NO_REVERSE)


# ---------------------------------------------------------------- hand-made shapes
def hub_graph():
    """Three rows longer than the staged capacity (with repeats), linked to each other and to a random remainder."""
    rng = np.random.default_rng(3)
    V = 6000
    s, d = [], []
    for h, n in ((0, 5000), (1, 3000), (2, 1500)):
        s.append(np.full(n, h))
        d.append(rng.integers(0, V, n))
    s.append(rng.integers(3, V, 30000))
    d.append(rng.integers(0, V, 30000))
    s.append(np.array([0, 0, 1, 1, 2, 2, 0, 7, 8]))
    d.append(np.array([1, 2, 0, 2, 0, 1, 0, 0, 1]))
    return V, np.concatenate(s), np.concatenate(d)


def _shape(name):
    if name == "no_edges":
        return 7, [], []
    if name == "single_edge":
        return 2, [0], [1]
    if name == "self_loops":
        return 4, [0, 0, 0, 1, 1, 2, 3, 3], [0, 0, 1, 1, 0, 2, 3, 0]
    if name == "k3":
        return 3, [0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]
    if name == "clique":
        n = 70
        a, b = np.meshgrid(np.arange(n), np.arange(n))
        m = a != b
        return n, a[m], b[m]
    if name == "star":                 # the centre has 200 out-edges, the leaves none: every value is +0.0
        return 201, np.zeros(200, np.int64), np.arange(1, 201)
    if name == "two_stars":            # 0 -> 1 has 200 common neighbours of out-degree 0: a sum of -0.0 terms, +0.0
        return 202, np.concatenate([[0], np.zeros(200, np.int64), np.ones(200, np.int64)]), np.concatenate([[1], np.arange(2, 202), np.arange(2, 202)])
    if name == "degree_one_common_neighbour":   # 0 -> 1 and 0 -> 3 have the common neighbour 2 of out-degree 1
        return 5, [0, 0, 0, 1, 1, 2, 3, 3], [1, 2, 3, 2, 4, 4, 2, 4]
    if name == "hub":
        return hub_graph()
    raise KeyError(name)


SHAPES = ["no_edges", "single_edge", "self_loops", "k3", "clique", "star", "two_stars", "degree_one_common_neighbour", "hub"]


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(gmx, name):
    V, s, d = _shape(name)
    g = gmx.Graph.from_edges(V, s, d)
    got, want, k, _ = check_whole(g, name)
    if name in ("no_edges", "single_edge", "star"):
        assert not got.any() and not np.signbit(got).any()
    if name == "k3":
        assert got.tolist() == pytest.approx([1.0 / np.log(2.0)] * 6, rel=2.0 ** -50)
    if name == "two_stars":
        assert got[0] == 0.0 and not np.signbit(got[0]) and k[0] == 200
    if name == "degree_one_common_neighbour":
        assert np.isinf(got[0]) and np.isinf(got[2]) and np.isfinite(got[1])
    if name == "hub":
        begin = g.download(reverse=False)[0]
        assert np.diff(begin)[:3].min() > AA_CAP          # these rows are searched in memory
        assert np.isfinite(got).any() and (got > 0).any()


def test_empty_graph_and_null_arguments(gmx):
    g = gmx.Graph.from_edges(0, [], [])
    assert len(g.adamic_adar()) == 0
    assert g.last_stats["iterations"] == 1 and g.last_stats["edges_examined"] == 0
    g = gmx.Graph.from_edges(3, [], [])
    buf = np.full(1, 7.0)
    assert gmx.lib().gmx_adamic_adar(g._h, buf.ctypes.data, None) == 0    # E == 0: nothing is written
    assert buf[0] == 7.0
    g = gmx.Graph.from_edges(3, [0, 0, 1], [1, 2, 2])
    assert gmx.lib().gmx_adamic_adar(None, buf.ctypes.data, None) == -1    # GMX_ERR_ARG
    assert gmx.lib().gmx_adamic_adar(g._h, None, None) == -1
    out = np.zeros(3)
    assert gmx.lib().gmx_adamic_adar(g._h, out.ctypes.data, None) == 0     # stats are optional
    assert out.tolist() == [0.0, 0.0, 0.0]


def test_multigraph_example_both_directions(gmx):
    og = example_multigraph()
    g = from_pyoracle(gmx, og)
    got = g.adamic_adar()
    want, k = aa_by_iterator(og)
    compare(got, want, k, "example")
    b, c = 1.0 / np.log(2.0), 1.0 / np.log(3.0)
    assert got[og.begin[0]] == pytest.approx(2 * b + c, rel=2.0 ** -49)      # s -> t: {b, b, c}
    assert got[og.begin[1]] == pytest.approx(3 * b + c, rel=2.0 ** -49)      # t -> s: {b, b, b, c}
    assert got[og.begin[0] + 2] == got[og.begin[0] + 3]                      # the repeated slot s -> b
    assert g.last_stats["edges_examined"] == int(k.sum())


_GOLDEN_WANT = {}


@pytest.mark.parametrize("env", [{}, {"GMX_AA_CAP": "0"}, {"GMX_AA_CAP": "8"}, {"GMX_AA_ALONE": "0"}, {"GMX_AA_ALONE": "100000"},
                                 {"GMX_AA_CAP": "0", "GMX_AA_ALONE": "100000"}])
def test_golden_graphs_on_every_path(gmx, golden, monkeypatch, env):
    """GMX_AA_CAP lowers the staged capacity (0: every row is searched in memory), GMX_AA_ALONE moves the line between a
    lane walking a slot alone and the whole wave walking it: the same inputs, against the iterator's restatement."""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    graphs = list(golden_graphs(golden)) + [("k3", k3()), ("example", example_multigraph())]
    for name, og in graphs:
        g = from_pyoracle(gmx, og)
        got = g.adamic_adar()
        if name not in _GOLDEN_WANT:
            _GOLDEN_WANT[name] = aa_by_iterator(og)
        want, k = _GOLDEN_WANT[name]
        compare(got, want, k, "%s %s" % (name, env))
        assert g.last_stats["edges_examined"] == int(k.sum()), name


def test_hub_rows_on_both_paths_agree(gmx, monkeypatch):
    """Staged or searched in memory, alone or by the wave: the adds of one edge happen in the same order, so the bits are
    the same."""
    V, s, d = hub_graph()
    g = gmx.Graph.from_edges(V, s, d)
    a = g.adamic_adar().copy()
    monkeypatch.setenv("GMX_AA_CAP", "0")
    b = g.adamic_adar().copy()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------- RMAT
@pytest.mark.parametrize("scale,permute", [(s, False) for s in range(8, 17)] + [(12, True), (16, True)])
def test_rmat_every_edge(gmx, scale, permute):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, permute)
    check_whole(g, "rmat%d%s" % (scale, "p" if permute else ""))


@pytest.mark.parametrize("scale", [20, 22])
def test_rmat_sampled(gmx, scale):
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g.download(reverse=False)
    deg = np.diff(begin)
    slots = [np.random.default_rng(scale).choice(len(idx), 20000, replace=False)]
    longest = np.argsort(-deg, kind="stable")[:3]
    for v in longest:                                   # the first 64 slots of the three longest rows
        slots.append(np.arange(begin[v], begin[v] + min(64, deg[v])))
    slots = np.unique(np.concatenate(slots))
    assert len(slots) >= 20000 and deg[longest].min() > AA_CAP
    got = g.adamic_adar()
    want, k = aa_vectorised(begin, idx, slots)
    assert not np.isnan(got).any()
    compare(got[slots], want, k, "rmat%d sample" % scale)


def test_rmat18_hits_equal_iterator_counts_and_runs_are_identical(gmx):
    g = gmx.Graph.rmat(1 << 18, 16 << 18, 1997, 0.57, 0.19, 0.19, False)
    begin, idx, _, _ = g.download(reverse=False)
    a = g.adamic_adar().copy()
    st = dict(g.last_stats)
    b = g.adamic_adar()
    assert a.tobytes() == b.tobytes()
    assert g.last_stats["edges_examined"] == st["edges_examined"]
    src = np.repeat(np.arange(1 << 18, dtype=np.int32), np.diff(begin))
    counts = g.common_nbr_counts(src, idx)
    assert st["edges_examined"] == int(counts.sum())
    assert not a[counts == 0].any()                      # no item: exactly 0.0
    assert st["d2h_ms"] > 0 and st["kernel_ms"] > 0


# ---------------------------------------------------------------- upload forms
def expected_by_uploaded_slot(begin, idx):
    """aa by the caller's slots of a CSR whose rows may be out of order: computed on the sorted rows and carried back (the
    value of a slot depends on its two ends only)."""
    o = sort_rows(begin, idx)
    want_sorted, k_sorted = aa_vectorised(begin, idx[o])
    want, k = np.zeros_like(want_sorted), np.zeros_like(k_sorted)
    want[o], k[o] = want_sorted, k_sorted
    return want, k


@pytest.mark.parametrize("name", ["multi64", "rmat16_shuffled"])
def test_upload_forms(gmx, name):
    u = ugraph(name)
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    want, k = expected_by_uploaded_slot(u.begin, u.idx)
    forms = {"SORT_ROWS": (True, S), "device-built reverse": (False, 0), "SORT_ROWS|NO_REVERSE": (False, S | N)}
    for label, (rev, flags) in forms.items():
        g = gmx.Graph.upload(u.begin, u.idx, u.rb if rev else None, u.ri if rev else None, flags=flags)
        assert g.edge_order() is not None                # the rows were out of order: the device holds a map
        got = g.adamic_adar()
        compare(got, want, k, "%s %s" % (name, label))
        assert g.last_stats["edges_examined"] == int(k.sum())
    # sorted rows uploaded without a reverse CSR: kept verbatim, slots are the caller's
    o = sort_rows(u.begin, u.idx)
    g = gmx.Graph.upload(u.begin, u.idx[o], flags=N)
    compare(g.adamic_adar(), want[o], k[o], "%s sorted NO_REVERSE" % name)
    # rows kept verbatim out of order: the state error of the common-neighbour entries
    for rev, flags in ((True, 0), (False, N)):
        g = gmx.Graph.upload(u.begin, u.idx, u.rb if rev else None, u.ri if rev else None, flags=flags)
        out = np.zeros(len(u.idx))
        assert gmx.lib().gmx_adamic_adar(g._h, out.ctypes.data, None) == -5   # GMX_ERR_STATE
        assert b"SORT_ROWS" in gmx.lib().gmx_last_error()
        with pytest.raises(gmx.GmxError, match="SORT_ROWS"):
            g.adamic_adar()


# ---------------------------------------------------------------- the rest of the library is left alone
def test_cached_graph_state_is_untouched(gmx):
    g = gmx.Graph.rmat(1 << 14, 16 << 14, 1997, 0.57, 0.19, 0.19, False)
    sym = g.symmetrize()
    rng = np.random.default_rng(9)
    src, dst = rng.integers(0, 1 << 14, 500), rng.integers(0, 1 << 14, 500)
    before = [(x.triangle_counting()[0], x.triangle_counting_cn()[0], x.common_nbr_counts(src, dst).tolist()) for x in (g, sym)]
    for x in (g, sym):
        check_whole(x, "rmat14")
    after = [(x.triangle_counting()[0], x.triangle_counting_cn()[0], x.common_nbr_counts(src, dst).tolist()) for x in (g, sym)]
    assert before == after


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "adamicAdar")
    assert os.path.exists(exe), "bin/adamicAdar not built"
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file, semi-sorted: G's slots after the prologue
    want, _ = aa_vectorised(c["begin"], c["node_idx"])
    nz = np.flatnonzero(want != 0.0)[:101]
    lines = re.findall(r"^(\d+)-> +(\S+)$", out.stdout, re.M)
    assert len(lines) == len(nz) == 101
    assert [int(a) for a, _ in lines] == nz.tolist()
    for (_, text), w in zip(lines, want[nz]):
        if np.isinf(w):
            assert text == "inf"
        else:
            assert text != "inf" and abs(float(text) - w) <= 1e-5, (text, w)
