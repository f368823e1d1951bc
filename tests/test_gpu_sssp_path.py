"""gmx_sssp_path (sssp_path.gm) on the device against the host restatement of test_sssp_path_host.py: dist[] bit for bit
against the oracle and gmx_sssp, prev_node / prev_edge equal to the canonical tree on EVERY vertex when len >= 1, the tree
property (check_tree) and equality on the vertices without a zero-length tight in-edge when lengths may be 0, every upload
form with prev_edge in the caller's slots, both schedules, the statistics and the drop-in driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT
from test_sssp_path_host import INT_MAX, canonical_tree, check_tree, golden_cases, rmat_case, top_hub
from test_upload_forms_host import rows_unsorted, stored, ugraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
SCHEDULES = ["round", "nearfar"]


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def forward_only(gmx, og):
    return gmx.Graph.upload(og.begin, og.node_idx, flags=gmx.GMX_GRAPH_NO_REVERSE)


def check_exact(begin, idx, length, root, want_dist, got, label, only=None):
    """got = (dist, prev_node, prev_edge, stats) of the device: dist exact, the tree property on every vertex, and prev equal
    to the restatement on every vertex (or on the mask `only`)."""
    dist, pn, pe, st = got
    assert np.array_equal(dist, want_dist), label
    check_tree(begin, idx, length, dist, pn, pe, root)
    wn, we, n_tight, allpos = canonical_tree(begin, idx, length, want_dist)
    m = np.ones(len(dist), bool) if only is None else only(allpos)
    assert np.array_equal(pe[m], we[m]), label
    assert np.array_equal(pn[m], wn[m]), label
    return n_tight, allpos


# ---------------------------------------------------------------- hand-made shapes
def _dense_redrop(V=40):
    """Every pair (i, j), i != j: the chain i -> i + 1 costs 1, every other edge out of i costs 2000 - 40 i, so each round
    of the chain lowers every vertex ahead of it again.  With a near / far threshold step of 3 the far pile passes V entries
    in the second round of the first band (38 + 37), which makes the third round compact it first."""
    s, d = np.meshgrid(np.arange(V), np.arange(V), indexing="ij")
    m = s != d
    s, d = s[m], d[m]
    return V, s, d, np.where(d == s + 1, 1, 2000 - 40 * s), 0


def _shape(name):
    """(V, src, dst, len, root) in CSR slot order (sorted by source, then as listed)."""
    if name == "no_edges":
        return 5, [], [], [], 2
    if name == "single_edge":
        return 2, [0], [1], [7], 0
    if name == "root_self_loop":
        return 2, [0, 0], [0, 1], [3, 2], 0
    if name == "root_out_of_range":
        return 3, [0, 1], [1, 2], [1, 1], 3
    if name == "negative_root":
        return 3, [0, 1], [1, 2], [1, 1], -1
    if name == "unreachable_part":
        return 5, [0, 2, 3], [1, 3, 2], [4, 1, 1], 0
    if name == "diamond":
        return 4, [0, 0, 1, 2], [1, 2, 3, 3], [1, 1, 1, 1], 0
    if name == "diamond_late_small":      # the larger predecessor 2 reaches its distance a round before the smaller one 1
        return 5, [0, 0, 1, 2, 4], [2, 4, 3, 3, 1], [2, 1, 1, 1, 1], 0
    if name == "zero_two_cycle":          # 1 <-> 2 with length 0, hanging off 0 -> 1
        return 4, [0, 1, 2, 2], [1, 2, 1, 3], [2, 0, 0, 1], 0
    if name == "zero_into_root":
        return 2, [0, 1], [1, 0], [0, 0], 0
    if name == "all_zero_cycle":
        return 4, [0, 1, 2, 3], [1, 2, 3, 0], [0, 0, 0, 0], 1
    if name == "long_chain_gaps":         # distances far apart: the threshold has to jump
        n = 300
        return n, np.arange(n - 1), np.arange(1, n), np.full(n - 1, 100000), 0
    if name == "dense_redrop":
        return _dense_redrop()
    raise KeyError(name)


SHAPES = ["no_edges", "single_edge", "root_self_loop", "root_out_of_range", "negative_root", "unreachable_part", "diamond",
          "diamond_late_small", "zero_two_cycle", "zero_into_root", "all_zero_cycle", "long_chain_gaps", "dense_redrop"]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SHAPES)
def test_shapes(gmx, monkeypatch, name, schedule):
    monkeypatch.setenv("GMX_SSSP_PATH_SCHEDULE", schedule)
    if name == "dense_redrop":
        monkeypatch.setenv("GMX_SSSP_DELTA", "3")
    if name == "long_chain_gaps":
        monkeypatch.setenv("GMX_SSSP_DELTA", "1000")         # a hundred empty bands between two vertices
    V, s, d, length, root = _shape(name)
    og = po.graph_from_edges(V, np.asarray(s, np.int32), np.asarray(d, np.int32))
    length = np.asarray(length, np.int32)
    assert np.array_equal(np.repeat(np.arange(V), np.diff(og.begin)), s) and np.array_equal(og.node_idx, d)   # slots as listed
    want = po.sssp(og, length, root)[0] if 0 <= root < V else np.full(V, INT_MAX, np.int32)
    g = forward_only(gmx, og)
    got = g.sssp_path(length, root)
    dist, pn, pe, st = got
    zero_ok = name in ("zero_two_cycle", "zero_into_root", "all_zero_cycle")
    check_exact(og.begin, og.node_idx, length, root, want, got, name, only=(lambda allpos: allpos) if zero_ok else None)
    assert np.array_equal(g.sssp(length, root)[0], dist)
    if name == "no_edges":
        assert dist.tolist() == [INT_MAX, INT_MAX, 0, INT_MAX, INT_MAX] and (pn == -1).all() and (pe == -1).all()
    if name == "single_edge":
        assert (dist.tolist(), pn.tolist(), pe.tolist()) == ([0, 7], [-1, 0], [-1, 0])
    if name == "root_self_loop":
        assert (dist.tolist(), pn.tolist(), pe.tolist()) == ([0, 2], [-1, 0], [-1, 1])
    if name in ("root_out_of_range", "negative_root"):
        assert (dist == INT_MAX).all() and (pn == -1).all() and (pe == -1).all() and st["iterations"] == 0
    if name == "unreachable_part":
        assert dist.tolist() == [0, 4, INT_MAX, INT_MAX, INT_MAX] and pn.tolist() == [-1, 0, -1, -1, -1]
    if name == "diamond":
        assert pn.tolist() == [-1, 0, 0, 1] and pe.tolist() == [-1, 0, 1, 2]            # the smaller predecessor of 3
    if name == "diamond_late_small":
        assert dist.tolist() == [0, 2, 2, 3, 1] and pn[3] == 1 and pe[3] == 2
    if name == "zero_two_cycle":
        assert dist.tolist() == [0, 2, 2, 3] and pn.tolist() == [-1, 0, 1, 2] and pe.tolist() == [-1, 0, 1, 3]
    if name == "zero_into_root":
        assert dist.tolist() == [0, 0] and pn.tolist() == [-1, 0] and pe.tolist() == [-1, 0]   # prev[root] stays NIL
    if name == "all_zero_cycle":
        assert dist.tolist() == [0, 0, 0, 0] and pn.tolist() == [3, -1, 1, 2]
    if name == "long_chain_gaps":
        assert st["iterations"] == V and pn.tolist() == [-1] + list(range(V - 1))
    if name == "dense_redrop":
        assert dist.tolist() == list(range(V)) and pn.tolist() == [-1] + list(range(V - 1))


@pytest.mark.parametrize("flags_name", ["verbatim", "sorted_on_device"])
def test_parallel_slots_smallest_tight_uploaded_slot(gmx, flags_name):
    """Row 0 = [1, 2, 1, 1, 2] with lengths [5, 1, 3, 3, 9], row 2 = [1] with length 2: vertex 1 is at distance 3 through the
    uploaded slots 2, 3 (from 0) and 5 (from 2).  Slot 2 must win, kept verbatim or sorted on the device (where it is
    device slot 1)."""
    begin = np.array([0, 5, 5, 6], np.int32)
    idx = np.array([1, 2, 1, 1, 2, 1], np.int32)
    length = np.array([5, 1, 3, 3, 9, 2], np.int32)
    flags = gmx.GMX_GRAPH_NO_REVERSE | (gmx.GMX_GRAPH_SORT_ROWS if flags_name == "sorted_on_device" else 0)
    g = gmx.Graph.upload(begin, idx, flags=flags)
    assert (g.edge_order() is not None) == (flags_name == "sorted_on_device")
    dist, pn, pe, _ = g.sssp_path(length, 0)
    assert dist.tolist() == [0, 3, 1] and pn.tolist() == [-1, 0, 0] and pe.tolist() == [-1, 2, 1]
    check_exact(begin, idx, length, 0, po.sssp(po.Graph(3, begin, idx), length, 0)[0], (dist, pn, pe, None), flags_name)


def test_negative_length_and_null_arguments(gmx):
    og = po.graph_from_edges(3, [0, 1], [1, 2])
    g = forward_only(gmx, og)
    with pytest.raises(gmx.GmxError, match="len"):
        g.sssp_path(np.array([1, -1], np.int32), 0)
    L = gmx.lib()
    length = np.array([1, -5], np.int32)
    out = [np.full(3, 77, np.int32) for _ in range(3)]
    assert L.gmx_sssp_path(g._h, 0, length.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None) == GMX_ERR_ARG
    assert b"len" in L.gmx_last_error()
    assert all((o == 77).all() for o in out)                                    # refused before anything is written
    length = np.array([1, 2], np.int32)
    assert L.gmx_sssp_path(None, 0, length.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, None, None) == GMX_ERR_ARG
    assert L.gmx_sssp_path(g._h, 0, None, out[0].ctypes.data, out[1].ctypes.data, None, None) == GMX_ERR_ARG
    assert L.gmx_sssp_path(g._h, 0, length.ctypes.data, None, out[1].ctypes.data, None, None) == GMX_ERR_ARG
    assert L.gmx_sssp_path(g._h, 0, length.ctypes.data, out[0].ctypes.data, None, None, None) == GMX_ERR_ARG
    # prev_edge and stats are optional
    assert L.gmx_sssp_path(g._h, 0, length.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, None, None) == 0
    assert out[0].tolist() == [0, 1, 3] and out[1].tolist() == [-1, 0, 1] and (out[2] == 77).all()
    # V = 0; E = 0 with len NULL
    e = gmx.Graph.from_edges(0, [], [])
    assert L.gmx_sssp_path(e._h, 0, None, out[0].ctypes.data, out[1].ctypes.data, None, None) == 0
    e = gmx.Graph.from_edges(3, [], [])
    assert L.gmx_sssp_path(e._h, 1, None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None) == 0
    assert out[0].tolist() == [INT_MAX, 0, INT_MAX] and (out[1] == -1).all() and (out[2] == -1).all()


# ---------------------------------------------------------------- golden cases and RMAT, len >= 1: everything is fixed
def test_golden_cases(gmx, golden):
    for name, c, root in golden_cases(golden):
        g = gmx.Graph.upload(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
        got = g.sssp_path(c["sssp_len"], root)
        check_exact(c["begin"], c["node_idx"], c["sssp_len"], root, c["sssp_dist"], got, name)
        again = g.sssp_path(c["sssp_len"], root)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])), name
        assert np.array_equal(g.sssp(c["sssp_len"], root)[0], got[0]), name
        g.free()


def three_roots(og):
    deg = np.diff(og.begin)
    rng = np.random.default_rng(og.N)
    return [top_hub(og), int(np.flatnonzero(deg > 0)[0]), int(rng.choice(np.flatnonzero(deg > 1)))]


@pytest.mark.parametrize("hi", [100, 3])
@pytest.mark.parametrize("scale,permute", [(s, False) for s in range(8, 17)] + [(12, True), (16, True)])
def test_rmat_every_vertex(gmx, scale, permute, hi):
    og = po.rmat_graph(scale, permute=permute)
    length = np.random.default_rng(1).integers(1, hi + 1, og.M).astype(np.int32)
    g = forward_only(gmx, og)
    L = gmx.lib()
    several = 0
    for root in three_roots(og):
        want = po.sssp(og, length, root)[0]
        got = g.sssp_path(length, root)
        n_tight, _ = check_exact(og.begin, og.node_idx, length, root, want, got, (scale, permute, hi, root))
        several += int((n_tight[want != INT_MAX] > 1).sum())
        assert np.array_equal(g.sssp(length, root)[0], got[0])
        again = g.sssp_path(length, root)                                        # a second call: identical arrays
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], again[:3]))
        d2, n2 = np.zeros(og.N, np.int32), np.zeros(og.N, np.int32)               # prev_edge_host = NULL
        assert L.gmx_sssp_path(g._h, root, length.ctypes.data, d2.ctypes.data, n2.ctypes.data, None, None) == 0
        assert np.array_equal(d2, got[0]) and np.array_equal(n2, got[1])
        st = got[3]
        assert st["vertices_reached"] >= int((want != INT_MAX).sum()) and st["edges_examined"] >= 1 and st["d2h_ms"] > 0
    assert several >= 1
    g.free()


# ---------------------------------------------------------------- lengths 0 .. 2: the weak half of the contract
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("scale", [10, 14, 16])
def test_zero_lengths(gmx, monkeypatch, scale, schedule):
    monkeypatch.setenv("GMX_SSSP_PATH_SCHEDULE", schedule)
    og, length, root, want = rmat_case(scale, 0, 2)
    g = forward_only(gmx, og)
    got = g.sssp_path(length, root)
    reached = want != INT_MAX
    _, allpos = check_exact(og.begin, og.node_idx, length, root, want, got, (scale, schedule), only=lambda allpos: allpos & reached)
    inner = reached.copy()
    inner[root] = False
    share = allpos[inner].sum() / reached.sum()
    print("sssp_path rmat%d len 0..2 %s: %d reached, %d compared exactly (%.1f %%)" % (scale, schedule, reached.sum(), allpos[inner].sum(), 100 * share))
    assert share >= 0.10
    assert (~allpos[inner]).any()
    g.free()


# ---------------------------------------------------------------- upload forms: prev_edge in the caller's slots
@pytest.mark.parametrize("hi", [100, 3])
@pytest.mark.parametrize("name", ["multi64", "multi150k", "rmat16_shuffled"])
def test_upload_forms(gmx, name, hi):
    u = ugraph(name)
    assert rows_unsorted(u.begin, u.idx)
    og = stored(u)
    length = np.random.default_rng(7).integers(1, hi + 1, len(u.idx)).astype(np.int32)
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"verbatim both CSRs": (True, 0, False), "SORT_ROWS": (True, S, True), "device-built reverse": (False, 0, True),
             "NO_REVERSE verbatim": (False, N, False), "SORT_ROWS|NO_REVERSE": (False, S | N, True)}
    want = {root: po.sssp(og, length, root)[0] for root in (u.hub, u.loop_root)}
    several = 0
    for label, (rev, flags, mapped) in forms.items():
        g = gmx.Graph.upload(u.begin, u.idx, u.rb if rev else None, u.ri if rev else None, flags=flags)
        assert (g.edge_order() is not None) == mapped, label
        for root, w in want.items():
            got = g.sssp_path(length, root)
            n_tight, _ = check_exact(u.begin, u.idx, length, root, w, got, (name, label, root))
            several += int((n_tight[w != INT_MAX] > 1).sum())
        g.free()
    if hi == 3:
        assert several >= 1                                   # (with 1 .. 100 the 64-vertex graph may have no tie)


# ---------------------------------------------------------------- both schedules, same arrays
@pytest.mark.parametrize("delta", [None, "1", "7"])
def test_schedules_agree(gmx, monkeypatch, delta):
    if delta:
        monkeypatch.setenv("GMX_SSSP_DELTA", delta)
    og, length, root, want = rmat_case(16, 1, 3)
    u = ugraph("multi150k")
    ulen = np.random.default_rng(7).integers(1, 101, len(u.idx)).astype(np.int32)
    uwant = po.sssp(stored(u), ulen, u.hub)[0]
    g = forward_only(gmx, og)
    gu = gmx.Graph.upload(u.begin, u.idx, u.rb, u.ri, flags=gmx.GMX_GRAPH_SORT_ROWS)
    out = {}
    for schedule in SCHEDULES:
        monkeypatch.setenv("GMX_SSSP_PATH_SCHEDULE", schedule)
        a = g.sssp_path(length, root)
        b = gu.sssp_path(ulen, u.hub)
        check_exact(og.begin, og.node_idx, length, root, want, a, schedule)
        check_exact(u.begin, u.idx, ulen, u.hub, uwant, b, schedule)
        out[schedule] = a[:3] + b[:3]
        print("sssp_path %s delta %s: rmat16 %d rounds, %d queue entries, %d edges; multi150k %d rounds, %d queue entries, %d edges" % (
            schedule, delta, a[3]["iterations"], a[3]["vertices_reached"], a[3]["edges_examined"],
            b[3]["iterations"], b[3]["vertices_reached"], b[3]["edges_examined"]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(out["round"], out["nearfar"]))


# ---------------------------------------------------------------- whole arrays at RMAT-22
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_rmat22_whole_arrays(gmx, monkeypatch, schedule):
    monkeypatch.setenv("GMX_SSSP_PATH_SCHEDULE", schedule)
    scale = 22
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, True)
    begin, idx, _, _ = g.download(reverse=False)
    length = np.random.default_rng(1).integers(1, 101, len(idx)).astype(np.int32)
    root = int(np.argmax(np.diff(begin)))
    want, _ = g.sssp(length, root)
    got = g.sssp_path(length, root)
    n_tight, _ = check_exact(begin, idx, length, root, want, got, "rmat22")
    reached = want != INT_MAX
    st = got[3]
    print("sssp_path rmat22 %s: %d reached, %d with a choice, stats %s" % (schedule, reached.sum(), (n_tight[reached] > 1).sum(), st))
    assert st["iterations"] >= 2 and st["vertices_reached"] >= int(reached.sum())
    assert st["kernel_ms"] > 0 and st["edges_examined"] >= int(np.diff(begin)[reached].sum())
    assert (n_tight[reached] > 1).sum() > 1000
    g.free()


# ---------------------------------------------------------------- the driver
def gm_rand32_lengths(n):
    """(rand() % 100) + 1 over gm_rand32's stream from its default seed, as sssp_path_main.cc draws them in slot order."""
    x = np.int32(np.uint32(2463534242).astype(np.int32))
    lens = []
    for _ in range(n):
        x = np.int32(np.uint32(x) ^ np.uint32((int(np.uint32(x)) << 13) & 0xffffffff))
        x = np.int32(x >> 17)
        x = np.int32(np.uint32(x) ^ np.uint32((int(np.uint32(x)) << 5) & 0xffffffff))
        lens.append(int(np.fmod(int(x), 100)) + 1)          # C's % truncates toward zero
    return np.array(lens, np.int32)


def libc_rand_pair():
    libc = C.CDLL("libc.so.6")
    libc.srand(1)                                            # the state of a program that never called srand
    return libc.rand(), libc.rand()


@pytest.mark.parametrize("end_reached", [True, False])
def test_driver(gmx, tmp_path, end_reached):
    exe = os.path.join(PKG, "bin", "sssp_path")
    assert os.path.exists(exe), "bin/sssp_path not built"
    N = 1000
    r0, r1 = libc_rand_pair()
    root, end = r0 % N, r1 % N
    assert root != end
    rng = np.random.default_rng(11)
    s = np.concatenate([np.arange(N), rng.integers(0, N, 6 * N)])
    d = np.concatenate([(np.arange(N) + 1) % N, rng.integers(0, N, 6 * N)])      # a cycle through everything + random edges
    if not end_reached:
        keep = d != end
        s, d = s[keep], d[keep]
    og = po.graph_from_edges(N, s.astype(np.int32), d.astype(np.int32))
    path_bin = str(tmp_path / "g.bin")
    po.store_binary(path_bin, og)
    length = gm_rand32_lengths(og.M)
    want = po.sssp(og, length, root)[0]
    assert (want[end] != INT_MAX) == end_reached
    r = subprocess.run([exe, path_bin, "4", "/dev/null"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "XXXXXXXXXX GM DONE XXXXXXXXXXXXXX" in r.stdout, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    header = "shortest path from %d to %d" % (root, end)
    assert header in lines, r.stdout[-2000:]
    at = lines.index(header)
    path_lines = [l for l in lines if re.fullmatch(r"\d+( -> \d+)*", l)]
    if not end_reached:
        assert not path_lines                                                   # no path line at all
        return
    assert len(path_lines) == 1 and lines[at + 1] == path_lines[0]
    path = [int(x) for x in path_lines[0].split(" -> ")]
    assert path[0] == root and path[-1] == end and len(set(path)) == len(path)
    g = forward_only(gmx, og)
    dist, pn, pe, _ = g.sssp_path(length, root)
    assert np.array_equal(dist, want)
    assert path == gmx.path_from_prev(pn, root, end)
    src = np.repeat(np.arange(N), np.diff(og.begin))
    total = 0
    for a, b in zip(path[:-1], path[1:]):
        e = pe[b]
        assert src[e] == a and og.node_idx[e] == b                             # every hop is an edge: the tree's
        total += int(length[e])
    assert total == want[end]
