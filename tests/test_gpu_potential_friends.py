"""gmx_potential_friends (potential_friends.gm) on the device against the host restatement
(test_potential_friends_host.potential_friends_ref), array for array: every graph, every evaluation regime forced over
every row, the table-full path, both bitmap homes with ragged last words, vertex ranges, the sizing protocol, batches,
every upload form of an unsorted multigraph, the drop-in driver and the hubs of RMAT-14.

There is no reference-compiled fixture for this entry: the reference ships no generated potential_friends.cc.  The literal
triple loop of the .gm in test_potential_friends_host.py stands in for it, and the restatement used here is checked
against that loop there."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_communities_host import csr, named_graph
from test_potential_friends_host import pf_ref_of, potential_friends_ref, report_lines, two_hop_lengths
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_PF_WAVE_MAX", "GMX_PF_BLOCK_MAX", "GMX_PF_LDS_SLOTS", "GMX_PF_LDS_BITS", "GMX_PF_BATCH_BYTES", "GMX_PF_LOG")
HUGE = str(1 << 40)
# the thresholds that send every row through one kernel, and the smallest tables (which fill on rows of a few hundred
# distinct two-hop vertices); "default" is what the others must equal
REGIMES = {
    "default": {},
    "all_wave": {"GMX_PF_WAVE_MAX": HUGE, "GMX_PF_BLOCK_MAX": HUGE},
    "all_block": {"GMX_PF_WAVE_MAX": "0", "GMX_PF_BLOCK_MAX": HUGE},
    "all_lds_bitmap": {"GMX_PF_WAVE_MAX": "0", "GMX_PF_BLOCK_MAX": "0"},
    "all_global_bitmap": {"GMX_PF_WAVE_MAX": "0", "GMX_PF_BLOCK_MAX": "0", "GMX_PF_LDS_BITS": "1"},
    "small_tables": {"GMX_PF_LDS_SLOTS": "512", "GMX_PF_BLOCK_MAX": HUGE},
    "small_tables_global_bitmap": {"GMX_PF_LDS_SLOTS": "512", "GMX_PF_BLOCK_MAX": HUGE, "GMX_PF_LDS_BITS": "1"},
}


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@contextlib.contextmanager
def knobs(**kw):
    """The library reads its thresholds from the environment at every call."""
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


def check(g, name, begin, node_idx):
    """The device against the restatement over all vertices, and the stats as gmx.h defines them."""
    want_b, want_i = pf_ref_of(name, begin, node_idx)
    pb, pi, st = g.potential_friends()
    assert pb.dtype == np.int64 and pi.dtype == np.int32
    assert np.array_equal(pb, want_b), name
    assert np.array_equal(pi, want_i), name
    L, _ = two_hop_lengths(begin, node_idx)
    assert st["edges_examined"] == int(L.sum())
    assert st["vertices_reached"] == int(np.count_nonzero(np.diff(want_b)))
    assert st["iterations"] == (1 if want_b[-1] else 0)        # everything here fits one default batch
    return pb, pi, st


def test_golden_cases(gmx, golden):
    for name, c in sorted(golden["cases"].items()):
        g = gmx.Graph.upload(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
        with knobs():
            check(g, "golden/" + name, c["begin"], c["node_idx"])


@pytest.mark.parametrize("name", ["rmat10", "rmat10p", "rmat12", "rmat12p", "rmat12s", "planted16", "planted64", "uniform", "star33",
                                  "path4096"])
def test_graphs(gmx, name):
    b, i = named_graph(name)
    g = gmx.Graph.upload(b, i)
    with knobs():
        _, _, st = check(g, name, b, i)
    assert st["kernel_ms"] > 0 and st["d2h_ms"] > 0


@pytest.mark.parametrize("regime", [r for r in REGIMES if r != "default"])
@pytest.mark.parametrize("name", ["rmat10", "rmat12s", "uniform", "star33"])
def test_every_regime_takes_every_row(gmx, name, regime):
    b, i = named_graph(name)
    g = gmx.Graph.upload(b, i)
    with knobs(**REGIMES[regime]):
        pb, pi, _ = check(g, name, b, i)
    with knobs():
        db, di, _ = g.potential_friends()
    assert pb.tobytes() == db.tobytes() and pi.tobytes() == di.tobytes()


LINE = re.compile(r"gmx potential_friends (count|fill) rows \[(\d+), (\d+)\): rows (\d+) wave \+ (\d+) block \+ (\d+) bitmap \((\d+) overflowed\), "
                  r"items (\d+) wave \+ (\d+) block \+ (\d+) bitmap")


def test_forced_regimes_are_the_ones_that_run(gmx, capfd):
    """The library's lines (GMX_PF_LOG) show which kernel evaluated the rows: the forced regimes are not vacuous, and with
    the smallest tables RMAT-12's hub rows do take the table-full path, in the counting and in the filling pass."""
    b, i = named_graph("rmat12")
    g = gmx.Graph.upload(b, i)
    L, _ = two_hop_lengths(b, i)
    n_rows = int(np.count_nonzero(L))
    seen = {}
    for regime, env in REGIMES.items():
        capfd.readouterr()
        with knobs(GMX_PF_LOG="1", **env):
            check(g, "rmat12", b, i)
        rows = [(m.group(1),) + tuple(int(x) for x in m.groups()[1:]) for m in LINE.finditer(capfd.readouterr().err)]
        assert [r[0] for r in rows] == ["count", "count", "fill"], regime       # the sizing call, then count + one batch
        for mode, lo, hi, w, k, m_, ovf, iw, ik, im in rows:
            assert (lo, hi) == (0, len(b) - 1) and w + k + m_ == n_rows and iw + ik + im == int(L.sum()), regime
        seen[regime] = rows
    for rows in seen["default"]:
        assert min(rows[3:6]) > 0                                   # the default thresholds use all three kernels
    for rows in seen["all_wave"]:
        assert rows[4:6] == (0, 0) and rows[6] > 0                  # ... and the hubs do not fit a wave's table
    for rows in seen["all_block"]:
        assert rows[3] == 0 and rows[5] == 0
    for regime in ("all_lds_bitmap", "all_global_bitmap"):
        for rows in seen[regime]:
            assert rows[3:5] == (0, 0) and rows[6] == 0
    for regime in ("small_tables", "small_tables_global_bitmap"):
        for rows in seen[regime]:
            assert rows[6] > 0, regime                              # the table-full path ran


def thousand():
    """V = 1000 (31 full words of 32 bits and one of 8; 15 of 64 and one of 40), vertex 999 in many sets."""
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.integers(0, 1000, 6000), rng.integers(0, 1000, 300), np.arange(0, 1000, 3)])
    d = np.concatenate([rng.integers(0, 1000, 6000), np.full(300, 999), np.full(334, 992)])
    return csr(1000, s, d)


@pytest.mark.parametrize("regime", ["all_lds_bitmap", "all_global_bitmap"])
def test_bitmap_tails(gmx, regime):
    b, i = thousand()
    want_b, want_i = pf_ref_of("thousand", b, i)
    assert np.count_nonzero(want_i == 999) > 100 and np.count_nonzero(want_i >= 992) > 500
    for name, (bb, ii) in (("thousand", (b, i)), ("star33", named_graph("star33"))):
        g = gmx.Graph.upload(bb, ii)
        with knobs(**REGIMES[regime]):
            check(g, name, bb, ii)
            for lo, hi in ((len(bb) - 2, len(bb) - 1), (0, 1)):            # the last vertex alone, the first alone
                pb, pi, _ = g.potential_friends(lo, hi)
                rb, ri = potential_friends_ref(bb, ii, lo, hi)
                assert np.array_equal(pb, rb) and np.array_equal(pi, ri)


def test_ranges(gmx):
    b, i = named_graph("rmat10")
    V = len(b) - 1
    g = gmx.Graph.upload(b, i)
    want_b, want_i = pf_ref_of("rmat10", b, i)
    with knobs():
        parts = [g.potential_friends(lo, hi) for lo, hi in ((0, 77), (77, 600), (600, V))]
        assert np.array_equal(np.concatenate([p[1] for p in parts]), want_i)
        assert np.array_equal(np.concatenate([np.diff(p[0]) for p in parts]), np.diff(want_b))
        for (lo, hi), p in zip(((0, 77), (77, 600), (600, V)), parts):
            assert p[0][0] == 0 and len(p[0]) == hi - lo + 1
            assert np.array_equal(p[0], want_b[lo:hi + 1] - want_b[lo])
        for lo in (0, 5, V):                                              # an empty range
            pb, pi, st = g.potential_friends(lo, lo)
            assert pb.tolist() == [0] and len(pi) == 0 and st["iterations"] == 0 and st["edges_examined"] == 0
        assert np.array_equal(g.potential_friend_counts(), np.diff(want_b))
        assert np.array_equal(g.potential_friend_counts(77, 600), np.diff(want_b)[77:600])
        assert g.last_stats["iterations"] == 0
    L = gmx.lib()
    begin = np.zeros(V + 2, np.int64)
    for lo, hi in ((5, 4), (0, V + 1), (-1, 5), (-3, -1), (V + 1, V + 1)):
        assert L.gmx_potential_friends(g._h, lo, hi, begin.ctypes.data, None, 0, None, None) == GMX_ERR_ARG, (lo, hi)
        with pytest.raises(gmx.GmxError):
            g.potential_friends(lo, hi)
    assert L.gmx_potential_friends(g._h, 0, V, None, None, 0, None, None) == GMX_ERR_ARG
    assert L.gmx_potential_friends(g._h, 0, V, begin.ctypes.data, None, -1, None, None) == GMX_ERR_ARG
    assert L.gmx_potential_friends(g._h, 0, V, begin.ctypes.data, None, 0, None, None) == 0      # total and stats may be NULL
    assert np.array_equal(begin[:V + 1], want_b)


def test_sizing_protocol(gmx):
    b, i = named_graph("rmat10")
    V = len(b) - 1
    g = gmx.Graph.upload(b, i)
    want_b, want_i = pf_ref_of("rmat10", b, i)
    total = int(want_b[-1])
    L = gmx.lib()
    with knobs():
        for cap, filled in ((total - 1, False), (0, False), (total, True), (total + 7, True)):
            begin = np.full(V + 1, -1, np.int64)
            idx = np.full(total + 7, -7, np.int32)
            t, st = C.c_int64(-1), gmx.Stats()
            assert L.gmx_potential_friends(g._h, 0, V, begin.ctypes.data, idx.ctypes.data, cap, C.byref(t), C.byref(st)) == 0
            assert t.value == total and np.array_equal(begin, want_b)
            if filled:
                assert np.array_equal(idx[:total], want_i) and np.all(idx[total:] == -7) and st.iterations == 1
            else:
                assert np.all(idx == -7) and st.iterations == 0            # not one element touched
        assert np.array_equal(g.potential_friend_counts(), np.diff(want_b))


def test_batches(gmx):
    b, i = named_graph("rmat12")
    g = gmx.Graph.upload(b, i)
    want_b, want_i = pf_ref_of("rmat12", b, i)
    assert np.diff(want_b).max() * 4 > 4096                             # some sets alone exceed the budget
    with knobs(GMX_PF_BATCH_BYTES="4096"):
        pb, pi, st = g.potential_friends()
    assert np.array_equal(pb, want_b) and np.array_equal(pi, want_i)
    assert 1 < st["iterations"] <= np.count_nonzero(np.diff(want_b))
    with knobs(GMX_PF_BATCH_BYTES="4096", **REGIMES["small_tables_global_bitmap"]):
        pb, pi, _ = g.potential_friends(100, 900)
    assert np.array_equal(pb, want_b[100:901] - want_b[100]) and np.array_equal(pi, want_i[want_b[100]:want_b[900]])


def test_upload_forms_give_identical_arrays(gmx):
    V = 2048
    b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 5000, 2048))
    assert b[6] - b[5] >= 5000
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"F0": (True, S), "F1": (True, 0), "F2": (False, N), "F3": (False, 0), "F4": (False, S | N)}
    want_b, want_i = pf_ref_of("multi", b, i)
    for regime in ("default", "small_tables", "all_global_bitmap"):
        for form, (rev, flags) in forms.items():
            g = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
            with knobs(**REGIMES[regime]):
                pb, pi, _ = g.potential_friends()                          # (a GMX_ERR_STATE would raise)
            assert np.array_equal(pb, want_b) and np.array_equal(pi, want_i), (regime, form)


def test_two_runs_give_identical_bytes(gmx):
    b, i = named_graph("rmat12")
    g = gmx.Graph.upload(b, i)
    with knobs():
        b1, i1, s1 = g.potential_friends()
        b2, i2, s2 = g.potential_friends()
    assert b1.tobytes() == b2.tobytes() and i1.tobytes() == i2.tobytes()
    assert s1["edges_examined"] == s2["edges_examined"] and s1["vertices_reached"] == s2["vertices_reached"]
    dist = g.hop_dist(0)[0]                                              # the graph's other entries are undisturbed
    b3, i3, _ = g.potential_friends()
    assert i3.tobytes() == i1.tobytes() and np.array_equal(g.hop_dist(0)[0], dist)


def test_no_edges_and_no_vertices(gmx):
    g = gmx.Graph.upload(np.zeros(1002, np.int32), np.zeros(0, np.int32))
    pb, pi, st = g.potential_friends()
    assert np.array_equal(pb, np.zeros(1002, np.int64)) and len(pi) == 0
    assert st["iterations"] == 0 and st["edges_examined"] == 0 and st["vertices_reached"] == 0
    assert np.array_equal(g.potential_friend_counts(3, 1001), np.zeros(998, np.int64))
    g = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))
    pb, pi, _ = g.potential_friends()
    assert pb.tolist() == [0] and len(pi) == 0 and len(g.potential_friend_counts()) == 0


def test_hand_graphs_in_every_regime(gmx):
    """The hand cases of the host file: 2-cycle, path, complete graph, lone self loop, neighbour without out-edges, repeats."""
    s7, d7 = np.nonzero(~np.eye(7, dtype=bool))
    cases = [(2, [0, 1], [1, 0]), (6, np.arange(5), np.arange(1, 6)), (7, s7, d7), (3, [0, 1], [0, 2]), (4, [0, 0, 2], [1, 2, 3]),
             (4, [0, 0, 0, 1, 1, 1], [1, 1, 0, 2, 2, 3])]
    for regime, env in REGIMES.items():
        for V, s, d in cases:
            b, i = csr(V, s, d)
            want_b, want_i = potential_friends_ref(b, i)
            with knobs(**env):
                pb, pi, _ = gmx.Graph.upload(b, i).potential_friends()
            assert np.array_equal(pb, want_b) and np.array_equal(pi, want_i), (regime, V)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "potential_friends")
    assert os.path.exists(exe), "bin/potential_friends not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    want_b, want_i = pf_ref_of("golden/rmat8_noperm", c["begin"], c["node_idx"])
    want = report_lines(want_b, want_i, len(c["begin"]) - 1)
    assert want.count("\n") > 5 and "..." in want
    assert want in out.stdout
    assert out.stdout.index(want) > out.stdout.index("running time=")
    assert out.stdout.endswith(want + "XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n")


def test_rmat14_hubs(gmx):
    """RMAT-14: the 64 rows with the most two-hop items, one call each (the hub walks 1.8 M items into a set below V = 16384),
    and 1000 ordinary rows in one range."""
    b, i = named_graph("rmat14")
    V = len(b) - 1
    L, _ = two_hop_lengths(b, i)
    assert V == 16384 and L.max() > 1 << 20
    g = gmx.Graph.upload(b, i)
    with knobs():
        counts = g.potential_friend_counts()
        for v in np.argsort(L)[-64:]:
            want_b, want_i = potential_friends_ref(b, i, int(v), int(v) + 1)
            pb, pi, st = g.potential_friends(int(v), int(v) + 1)
            assert np.array_equal(pb, want_b) and np.array_equal(pi, want_i), v
            assert st["edges_examined"] == L[v] and counts[v] == want_b[1]
        lo, hi = 9000, 10000
        want_b, want_i = potential_friends_ref(b, i, lo, hi)
        pb, pi, st = g.potential_friends(lo, hi)
        assert np.array_equal(pb, want_b) and np.array_equal(pi, want_i)
        assert st["edges_examined"] == int(L[lo:hi].sum()) and np.array_equal(counts[lo:hi], np.diff(want_b))
