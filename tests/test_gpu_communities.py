"""gmx_communities (communities.gm) on the device against the host restatement (test_communities_host.communities_ref):
labels, rounds and converged array for array on every graph, every evaluation regime forced over every row, the
table-full path, the work list against full re-evaluation, every upload form of an unsorted multigraph, the drop-in driver."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_communities_host import communities_ref, csr, is_fixpoint, named_graph, ref_of
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_COMM_WAVE_MIN", "GMX_COMM_BLOCK_MIN", "GMX_COMM_LDS_SLOTS", "GMX_COMM_WORKLIST")
HUGE = str(1 << 30)
# the thresholds that send every row through one kernel, and the smallest tables (the table-full path on rows of a few
# hundred slots); "default" is what the others must equal
REGIMES = {
    "default": {},
    "all_short": {"GMX_COMM_WAVE_MIN": HUGE, "GMX_COMM_BLOCK_MIN": HUGE},
    "all_wave": {"GMX_COMM_WAVE_MIN": "1", "GMX_COMM_BLOCK_MIN": HUGE},
    "all_block": {"GMX_COMM_BLOCK_MIN": "1"},
    "small_tables": {"GMX_COMM_LDS_SLOTS": "512"},
    "all_wave_small_tables": {"GMX_COMM_WAVE_MIN": "1", "GMX_COMM_BLOCK_MIN": HUGE, "GMX_COMM_LDS_SLOTS": "512"},
    "all_block_small_tables": {"GMX_COMM_BLOCK_MIN": "1", "GMX_COMM_LDS_SLOTS": "512"},
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


def check(g, name, begin, node_idx, max_rounds=1000):
    """The device against the restatement: labels, rounds, converged, and the fixpoint property itself."""
    want, rounds, conv = ref_of(name, begin, node_idx, max_rounds)
    comm, r, c, st = g.communities(max_rounds)
    assert np.array_equal(comm, want)
    assert (r, c) == (rounds, conv)
    assert bool(c) == is_fixpoint(begin, node_idx, comm)
    assert st["iterations"] == r
    return comm, r, c, st


def test_golden_cases(gmx, golden):
    for name, c in sorted(golden["cases"].items()):
        g = gmx.Graph.upload(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
        with knobs():
            _, _, conv, _ = check(g, "golden/" + name, c["begin"], c["node_idx"])
        assert conv == 1, name


@pytest.mark.parametrize("name", ["rmat10", "rmat10p", "rmat12", "rmat12p", "rmat14", "rmat14p", "rmat12s", "planted16", "planted64",
                                  "uniform", "star33", "path4096"])
def test_graphs(gmx, name):
    b, i = named_graph(name)
    g = gmx.Graph.upload(b, i)
    with knobs():
        _, r, conv, st = check(g, name, b, i)
    assert conv == 1
    deg = np.diff(b)
    # every vertex with out-edges is evaluated in round 0, and a round that changes something is followed by another
    assert st["vertices_reached"] >= int((deg > 0).sum()) and st["edges_examined"] >= len(i)
    assert st["kernel_ms"] > 0


@pytest.mark.parametrize("max_rounds", [0, 1, 16])
def test_chain_is_cut(gmx, max_rounds):
    b, i = named_graph("chain4096")
    g = gmx.Graph.upload(b, i)
    with knobs():
        comm, r, conv, _ = check(g, "chain4096", b, i, max_rounds)
    assert r == max_rounds and conv == 0
    if max_rounds == 0:
        assert np.array_equal(comm, np.arange(4096))


def test_no_edges_and_no_vertices(gmx):
    g = gmx.Graph.upload(np.zeros(1001, np.int32), np.zeros(0, np.int32))
    for mr in (0, 5):
        comm, r, conv, st = g.communities(mr)
        assert np.array_equal(comm, np.arange(1000)) and (r, conv) == (0, 1) and st["vertices_reached"] == 0
    g = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))
    comm, r, conv, _ = g.communities()
    assert len(comm) == 0 and (r, conv) == (0, 1)
    # max_rounds = 0 on a graph whose identity labels are a fixpoint (self loops only)
    b, i = csr(300, np.arange(300), np.arange(300))
    comm, r, conv, _ = gmx.Graph.upload(b, i).communities(0)
    assert np.array_equal(comm, np.arange(300)) and (r, conv) == (0, 1)


def test_hand_graphs(gmx):
    """The tie rule, the self loop, repeated slots and the vertex without out-edges (test_communities_host's hand graphs)."""
    cases = [(2, [0, 1], [1, 0]), (4, [0, 1], [3, 3]), (4, [0, 0, 0], [2, 2, 1]), (4, [0, 0, 3, 3], [1, 2, 1, 2]),
             (2, [0, 0, 0], [0, 0, 1]), (2, [0, 0, 0], [0, 1, 1])]
    for regime, env in REGIMES.items():
        for V, s, d in cases:
            b, i = csr(V, s, d)
            want, rounds, conv = communities_ref(b, i)
            with knobs(**env):
                comm, r, c, _ = gmx.Graph.upload(b, i).communities()
            assert np.array_equal(comm, want) and (r, c) == (rounds, conv), (regime, V, s, d)


MULTI = {}


def multigraph():
    """An unsorted multigraph whose hub row (vertex 5) holds 5000 slots with repeats, rows in shuffled order."""
    if not MULTI:
        V = 2048
        MULTI["g"] = (V,) + tuple(np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 5000, 2048))
    return MULTI["g"]


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", ["rmat12", "rmat12p", "multi"])
def test_every_regime_takes_every_row(gmx, name, regime):
    """RMAT-12's hubs hold hundreds of distinct labels in round 0, the multigraph's hub thousands: with the smallest tables
    both run the table-full path; a row of thousands of slots through the 16-lane kernel runs its chunk loops."""
    if name == "multi":
        V, b, i, rb, ri = multigraph()
        assert b[6] - b[5] >= 5000
        g = gmx.Graph.upload(b, i, rb, ri)
    else:
        b, i = named_graph(name)
        g = gmx.Graph.upload(b, i)
    with knobs(**REGIMES[regime]):
        comm, r, conv, st = check(g, name, b, i)
    assert conv == 1


ROUND = re.compile(r"gmx communities round (\d+): evals (\d+) short \+ (\d+) wave \+ (\d+) block \((\d+) overflowed\), slots (\d+), changes (\d+)")


@pytest.mark.parametrize("name", ["rmat12", "multi"])
def test_forced_regimes_are_the_ones_that_run(gmx, capfd, name):
    """The library's per-round lines (GMX_COMM_ROUNDS) show which kernel evaluated the rows: the forced regimes are not
    vacuous, and the smallest tables do fill in round 0 (every neighbour still carries its own id)."""
    if name == "multi":
        V, b, i, rb, ri = multigraph()
    else:
        b, i = named_graph(name)
    g = gmx.Graph.upload(b, i)
    n_rows = int((np.diff(b) > 0).sum())
    seen = {}
    for regime, env in REGIMES.items():
        capfd.readouterr()
        with knobs(**env):
            os.environ["GMX_COMM_ROUNDS"] = "1"
            try:
                g.communities()
            finally:
                del os.environ["GMX_COMM_ROUNDS"]
        rows = [tuple(int(x) for x in m.groups()) for m in ROUND.finditer(capfd.readouterr().err)]
        assert rows and rows[0][0] == 0, regime
        _, s, w, k, ovf, slots, changes = rows[0]
        assert s + w + k == n_rows and slots == len(i) and changes > 0, regime     # round 0 evaluates every row once
        seen[regime] = (s, w, k, ovf)
    if name == "rmat12":
        assert min(seen["default"][:3]) > 0                       # the default thresholds use all three kernels
    assert seen["all_short"][1:] == (0, 0, 0)
    assert seen["all_wave"][0] == 0 and seen["all_wave"][2] == 0
    assert seen["all_block"][:2] == (0, 0)
    for regime in ("small_tables", "all_wave_small_tables", "all_block_small_tables"):
        assert seen[regime][3] > 0, regime                       # the table-full path ran


def test_upload_forms_give_identical_labels(gmx):
    V, b, i, rb, ri = multigraph()
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"F0": (True, S), "F1": (True, 0), "F2": (False, N), "F3": (False, 0), "F4": (False, S | N)}
    want, rounds, conv = ref_of("multi", b, i)
    for regime in ("default", "small_tables"):
        for form, (rev, flags) in forms.items():
            g = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
            with knobs(**REGIMES[regime]):
                comm, r, c, _ = g.communities()
            assert np.array_equal(comm, want) and (r, c) == (rounds, conv), (regime, form)


@pytest.mark.parametrize("name", ["rmat14p", "uniform"])
def test_work_list_changes_the_work_only(gmx, name):
    b, i = named_graph(name)
    g = gmx.Graph.upload(b, i)
    with knobs():
        comm, r, conv, st = check(g, name, b, i)
    with knobs(GMX_COMM_WORKLIST="0"):
        comm0, r0, conv0, st0 = check(g, name, b, i)
    assert np.array_equal(comm, comm0) and (r, conv) == (r0, conv0)
    n_rows = int((np.diff(b) > 0).sum())
    assert st0["vertices_reached"] == n_rows * (r0 + 1)       # every row in every round, the last one changing nothing
    assert st0["edges_examined"] == len(i) * (r0 + 1)
    assert st["vertices_reached"] < st0["vertices_reached"]
    assert st["edges_examined"] < st0["edges_examined"]


def test_two_runs_give_identical_bytes(gmx):
    b, i = named_graph("rmat14p")
    g = gmx.Graph.upload(b, i)
    with knobs():
        c1, r1, v1, s1 = g.communities()
        c2, r2, v2, s2 = g.communities()
    assert c1.tobytes() == c2.tobytes() and (r1, v1) == (r2, v2)
    assert s1["vertices_reached"] == s2["vertices_reached"] and s1["edges_examined"] == s2["edges_examined"]
    dist = g.hop_dist(0)[0]                                       # the graph's other entries are undisturbed
    c3, _, _, _ = g.communities()
    assert c3.tobytes() == c1.tobytes() and np.array_equal(g.hop_dist(0)[0], dist)


def test_bad_arguments(gmx):
    import ctypes as C
    b, i = named_graph("star33")
    g = gmx.Graph.upload(b, i)
    out = np.zeros(33, np.int32)
    L = gmx.lib()
    assert L.gmx_communities(g._h, -1, out.ctypes.data, None, None, None) == GMX_ERR_ARG
    assert L.gmx_communities(g._h, 10, None, None, None, None) == GMX_ERR_ARG
    with pytest.raises(gmx.GmxError):
        g.communities(-5)
    # the optional outputs may be NULL
    assert L.gmx_communities(g._h, 10, out.ctypes.data, None, None, None) == 0
    assert np.array_equal(out, ref_of("star33", b, i)[0])
    r = C.c_int32(-1)
    assert L.gmx_communities(g._h, 10, out.ctypes.data, C.byref(r), None, None) == 0 and r.value == ref_of("star33", b, i)[1]


def report_lines(comm):
    sizes = np.bincount(comm)
    shown = np.flatnonzero(sizes)[:10]
    return "Community\t#Nodes\t\t(showing max 10 entries)\n" + "".join("%d\t\t%d\n" % (k, sizes[k]) for k in shown)


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "communities")
    assert os.path.exists(exe), "bin/communities not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS and k != "GMX_COMM_MAX_ROUNDS"}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    want, _, conv = ref_of("golden/rmat8_noperm", c["begin"], c["node_idx"])
    assert conv == 1
    assert report_lines(want) in out.stdout
