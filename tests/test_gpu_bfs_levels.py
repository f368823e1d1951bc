"""hop_dist level by level against tests/bfs_model.py: on every boundary graph of tests/bfs_cases.py and on RMAT graphs the
device's dist[] equals the oracle's queue BFS, its four statistics equal the model's, and every GMX_BFS_DEBUG line -- direction,
form, frontier, frontier edges, entries inspected, next frontier, hint coding -- equals the model's record of that level.  All
comparisons are integer equalities.  test_bfs_model_host.py proves without a device which boundary each case meets."""
import os

import numpy as np
import pytest

import bfs_cases as bc
import bfs_model as bm
import pyoracle as po
from test_gpu_parity import _bfs_ranks_on_graph

pytestmark = pytest.mark.gpu
INT_MAX = bm.INT_MAX


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def upload(gmx, c):
    """the case's arrays verbatim; what the device then holds is what the model was given"""
    if not c.reverse:
        g = gmx.Graph.upload(c.begin, c.node_idx, flags=gmx.GMX_GRAPH_NO_REVERSE)
        b, n, _, _ = g.download(reverse=False)
        assert np.array_equal(b, c.begin) and np.array_equal(n, c.node_idx)
        return g
    g = gmx.Graph.upload(c.begin, c.node_idx, c.r_begin, c.r_node_idx)
    b, n, rb, rn = g.download()
    assert np.array_equal(b, c.begin) and np.array_equal(n, c.node_idx)
    assert np.array_equal(rb, c.r_begin) and np.array_equal(rn, c.r_node_idx)
    return g


class debug_lines:
    """with debug_lines(capfd, GMX_...=...) as d: ...; d.levels = the GMX_BFS_DEBUG lines printed inside, parsed"""

    def __init__(self, capfd, **env):
        self.capfd, self.env = capfd, dict(env, GMX_BFS_DEBUG="1")

    def __enter__(self):
        self.capfd.readouterr()
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        self.levels = bm.parse_debug(self.capfd.readouterr().err)
        return False


def check_run(got_dist, got_stats, got_levels, want, oracle_dist, what):
    assert np.array_equal(got_dist, oracle_dist), what          # the independent reference
    assert np.array_equal(want.dist, oracle_dist), what
    for i, (a, b) in enumerate(zip(got_levels, want.levels)):
        assert a == b, (what, "level %d" % i, "device", tuple(a), "model", tuple(b))
    assert len(got_levels) == len(want.levels), what
    if got_stats is not None:
        for k in ("iterations", "vertices_reached", "edges_reached", "edges_examined"):
            assert got_stats[k] == want.stats[k], (what, k, got_stats[k], want.stats[k])


SEEN = {}   # case -> the forms its levels took on the device


@pytest.mark.parametrize("name", bc.CASES)
def test_boundary_case(gmx, capfd, name):
    c = bc.case(name)
    oracle = po.bfs_queue(po.Graph(len(c.begin) - 1, c.begin, c.node_idx), c.root)
    g = upload(gmx, c)
    try:
        with debug_lines(capfd) as d:
            dist, st = g.hop_dist(c.root)
        check_run(dist, st, d.levels, bc.model(name), oracle, name)
        SEEN[name] = [l.form for l in d.levels]
        lv, n = g.bfs_levels(c.root)
        assert n == bc.model(name).stats["iterations"]
        assert np.array_equal(lv, np.where(oracle == INT_MAX, -2, oracle).astype(np.int16))
    finally:
        g.free()


@pytest.mark.parametrize("scale,permute", [(14, False), (14, True), (16, False), (16, True)])
def test_rmat(gmx, capfd, scale, permute):
    og = po.rmat_graph(scale, permute=permute)
    g = gmx.Graph.upload(og.begin, og.node_idx, og.r_begin, og.r_node_idx)
    try:
        b, n, rb, rn = g.download()
        assert np.array_equal(b, og.begin) and np.array_equal(n, og.node_idx)
        sorted_rows = bm.rows_ascending(b, n)
        rng = np.random.default_rng(100 + scale)
        for root in [0, int(np.argmax(np.diff(b))), og.N - 1] + rng.integers(0, og.N, 2).tolist():
            with debug_lines(capfd) as d:
                dist, st = g.hop_dist(root)
            check_run(dist, st, d.levels, bm.run(b, n, rb, rn, sorted_rows, root), po.bfs_queue(og, root), (scale, permute, root))
    finally:
        g.free()


@pytest.mark.parametrize("name", bc.BOTTOM_UP_CASES)
def test_plain_hints(gmx, capfd, name):
    """GMX_BFS_PLAIN_HINTS: the same levels; the coding has no only-flag, so a vertex with one in-edge whose hint misses walks its
    one entry (test_bfs_model_host.test_plain_hints_walk_the_one_entry_rows: that is the whole difference)"""
    c = bc.case(name)
    oracle = po.bfs_queue(po.Graph(len(c.begin) - 1, c.begin, c.node_idx), c.root)
    with debug_lines(capfd, GMX_BFS_PLAIN_HINTS="1") as d:
        g = upload(gmx, c)          # (the hints are built once per graph: a fresh upload)
        try:
            dist, st = g.hop_dist(c.root)
        finally:
            g.free()
    want = bc.model(name, plain=True)
    assert any(l.encoding == "plain" for l in want.levels)
    check_run(dist, st, d.levels, want, oracle, name)


def test_hub_encodings(gmx, capfd):
    """The padded bottom-up case with GMX_BFS_HUB_MIN_V on both sides of V and with plain hints: per level the same numbers, only
    the coding differs (and, under plain hints, the one-entry walks)."""
    name = bc.HUB_CASE
    c = bc.case(name)
    V = len(c.begin) - 1
    assert bc.HUB_MIN_V <= V < 2 * bc.HUB_MIN_V and V > bm.BFS_HUBS
    oracle = po.bfs_queue(po.Graph(V, c.begin, c.node_idx), c.root)
    runs = {}
    for coding, env, kw in [("hubs-lds", dict(GMX_BFS_HUB_MIN_V=str(bc.HUB_MIN_V)), dict(hub_min_v=bc.HUB_MIN_V)),
                            (None, dict(GMX_BFS_HUB_MIN_V=str(2 * bc.HUB_MIN_V)), dict(hub_min_v=2 * bc.HUB_MIN_V)),
                            ("plain", dict(GMX_BFS_PLAIN_HINTS="1"), dict(plain=True))]:
        g = None
        try:
            with debug_lines(capfd, **env) as d:
                g = upload(gmx, c)     # (the hints are built once per graph: a fresh upload)
                dist, st = g.hop_dist(c.root)
            if coding == "hubs-lds":   # two rank states: ranges shorter than the threshold probe the hubs' bits in memory
                with debug_lines(capfd, **env) as d2:
                    outs, _, exchanges = _bfs_ranks_on_graph(gmx, g, c.root, 2)
        finally:
            if g is not None:
                g.free()
        want = bc.model(name, **kw)
        assert {l.encoding for l in want.levels if l.direction == "bottom-up"} == {coding}
        check_run(dist, st, d.levels, want, oracle, (name, coding))
        runs[coding] = d.levels
    for a, b in zip(runs["hubs-lds"], runs[None]):
        assert a[:7] == b[:7]
    for a, b in zip(runs["hubs-lds"], runs["plain"]):
        assert a[:5] + a[6:7] == b[:5] + b[6:7]
    mem = []
    for rank in range(2):
        want = bc.model(name, rank, 2, False, bc.HUB_MIN_V)
        assert {l.encoding for l in want.levels if l.direction == "bottom-up"} == {"hubs-mem"}
        check_run(outs[rank], None, d2.levels[rank::2], want, oracle, (name, "rank", rank))
        mem.append(want)
    for i, l in enumerate(runs["hubs-lds"]):   # the two ranges' shares are the single range's work
        assert l.inspected == (mem[0].levels[i].inspected + mem[1].levels[i].inspected if l.direction == "bottom-up" else mem[0].levels[i].inspected)
    assert exchanges >= 1


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", bc.RANK_CASES)
def test_rank_states(gmx, capfd, name, nranks):
    """N rank states side by side: every rank's dist[] and every rank's lines (printed rank by rank within a level) equal the
    model of that rank; a rank's edges_examined is the sum of its lines."""
    c = bc.case(name)
    V = len(c.begin) - 1
    oracle = po.bfs_queue(po.Graph(V, c.begin, c.node_idx), c.root)
    g = upload(gmx, c)
    try:
        with debug_lines(capfd) as d:
            outs, _, exchanges = _bfs_ranks_on_graph(gmx, g, c.root, nranks)
    finally:
        g.free()
    assert exchanges >= 1
    for rank in range(nranks):
        want = bc.model(name, rank, nranks)
        lines = d.levels[rank::nranks]
        check_run(outs[rank], None, lines, want, oracle, (name, nranks, rank))
        assert sum(l.inspected for l in lines) == want.stats["edges_examined"]
    slice_vertices = ((V + 63) // 64 + nranks - 1) // nranks * 64
    assert name != "bu_rows" or slice_vertices % 256 != 0          # a slice boundary inside a wave step's 256 vertices


def test_every_form_is_taken_on_the_device(gmx, capfd):
    """Over all cases the device takes every form gmx_bfs_step_begin has (bfs_model.FORMS, which
    test_bfs_model_host.test_model_names_every_form_of_the_library ties to the source) and every origin of a frontier:
    a threshold change that strands a form fails here."""
    for name in bc.CASES:
        if name not in SEEN:   # (run on its own)
            c = bc.case(name)
            g = upload(gmx, c)
            try:
                with debug_lines(capfd) as d:
                    g.hop_dist(c.root)
            finally:
                g.free()
            SEEN[name] = [l.form for l in d.levels]
    forms = {f.split(" ")[0] for fs in SEEN.values() for f in fs}
    assert forms == set(bm.FORMS), set(bm.FORMS) ^ forms
    origins = {f.split(" ")[1] for fs in SEEN.values() for f in fs if " " in f}
    assert origins == set(bm.ORIGINS) | {"from-bitmap"}
