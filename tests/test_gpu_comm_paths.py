"""gmx_communities on the graphs of tests/comm_cases.py, which reach what test_gpu_communities.py's graphs do not: a label class
split again and again, more classes than workgroups, more overflowed rows than a batch, second and later trips of every
grid-stride loop with the staged pending list flushed inside them, the commit's three reverse-row regimes at their boundaries,
and the cut pass through the table-full path.  Labels, rounds, converged and the two work statistics equal the work model
(comm_cases.work_model; pairs23: its closed form), and so does every GMX_COMM_ROUNDS line -- rows per regime, slots, changes --
with the work list and without; `overflowed` lies within the order-free bounds and `splits` says that the split loop ran.
test_comm_cases_host.py proves without a device which path each case takes."""
import os
import re

import numpy as np
import pytest

import comm_cases as cc
from test_communities_host import csr, is_fixpoint, named_graph
from test_gpu_communities import ROUND as ROUND_BEFORE, knobs, multigraph

pytestmark = pytest.mark.gpu
ROUND = re.compile(r"gmx communities round (\d+): evals (\d+) short \+ (\d+) wave \+ (\d+) block \((\d+) overflowed\), slots (\d+), "
                   r"changes (\d+), [0-9.]+ ms, splits (\d+)")
RUN_PARAMS = [pytest.param(name, env, id="%s-%s" % (name, cc.knob_id(env))) for name in cc.CASES for env in cc.RUNS[name]]
NO_LIST = {"GMX_COMM_WORKLIST": "0"}


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(scope="module")
def graphs(gmx):
    """case name -> its graph on the device (the reverse CSR built there), uploaded once and freed with the module"""
    held = {}

    def get(name):
        if name not in held:
            held[name] = gmx.Graph.upload(*cc.case(name))
        return held[name]
    yield get
    for g in held.values():
        g.free()


def logged(g, capfd, env, max_rounds=1000):
    """one call under the knobs: (comm, rounds, converged, stats, the per-round lines as tuples of ints)"""
    capfd.readouterr()
    with knobs(**env):
        os.environ["GMX_COMM_ROUNDS"] = "1"
        try:
            comm, r, c, st = g.communities(max_rounds)
        finally:
            del os.environ["GMX_COMM_ROUNDS"]
    rows = [tuple(int(x) for x in m.groups()) for m in ROUND.finditer(capfd.readouterr().err)]
    return comm, r, c, st, rows


def check_lines(rows, m, what):
    """the device's round lines against the model's rounds: exact but for `overflowed`, which has its two-sided bound"""
    for n, (got, want) in enumerate(zip(rows, m.rounds_log)):
        r, s, w, k, ovf, slots, changes, splits = got
        assert r == n and (s, w, k, slots, changes) == tuple(want[:5]), (what, n, got, tuple(want))
        assert want.ovf_lo <= ovf <= want.ovf_hi, (what, n, got, tuple(want))
        if ovf == 0:
            assert splits == 0, (what, n, got)
    assert len(rows) == len(m.rounds_log), (what, rows, m.rounds_log)


def check_against_model(g, capfd, name, begin, node_idx, env, worklist=True, max_rounds=1000, has_reverse=True):
    """worklist False: by the knob on a graph with a reverse CSR, by itself on one without"""
    m = cc.model_of(name, begin, node_idx, env, worklist, max_rounds)
    what = (name, cc.knob_id(env), worklist, max_rounds)
    comm, r, c, st, rows = logged(g, capfd, env if worklist or not has_reverse else dict(env, **NO_LIST), max_rounds)
    assert np.array_equal(comm, m.comm), what
    assert (r, c) == (m.rounds, m.converged), what
    assert st["iterations"] == r and st["vertices_reached"] == m.evals and st["edges_examined"] == m.slots, (what, st, m.evals, m.slots)
    check_lines(rows, m, what)
    return comm, r, c, st, rows


def test_round_line_keeps_its_form(gmx, capfd):
    """the splits field follows the time: what tools/comm_prof.py and test_gpu_communities.py parse is unchanged"""
    b, i = named_graph("star33")
    g = gmx.Graph.upload(b, i)
    capfd.readouterr()
    with knobs():
        os.environ["GMX_COMM_ROUNDS"] = "1"
        try:
            g.communities()
        finally:
            del os.environ["GMX_COMM_ROUNDS"]
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("gmx communities round")]
    assert lines and all(re.fullmatch(ROUND.pattern, l) for l in lines), err
    assert all(ROUND_BEFORE.match(l) and re.search(r"changes (\d+), ([0-9.]+) ms", l) for l in lines), err
    g.free()


@pytest.mark.parametrize("name,env", RUN_PARAMS)
def test_case(gmx, graphs, capfd, name, env):
    b, i = cc.case(name)
    V = len(b) - 1
    g = graphs(name)
    if name == "pairs23":
        want, rounds, conv = cc.pairs_closed_form(V)
        with knobs(**env):
            c1, r1, v1, s1 = g.communities()
            c2, r2, v2, s2 = g.communities()
        assert np.array_equal(c1, want) and (r1, v1) == (rounds, conv)
        assert (s1["iterations"], s1["vertices_reached"], s1["edges_examined"]) == (1, V // 2, V // 2), s1
        assert c1.tobytes() == c2.tobytes() and (r1, v1) == (r2, v2)
        assert (s2["vertices_reached"], s2["edges_examined"]) == (V // 2, V // 2)
        return
    c1, r1, v1, s1, rows = check_against_model(g, capfd, name, b, i, env)
    assert bool(v1) == is_fixpoint(b, i, c1) and v1 == 1
    with knobs(**env):
        c2, r2, v2, s2 = g.communities()
    assert c1.tobytes() == c2.tobytes() and (r1, v1) == (r2, v2)
    assert s1["vertices_reached"] == s2["vertices_reached"] and s1["edges_examined"] == s2["edges_examined"]
    c0, r0, v0, _, _ = check_against_model(g, capfd, name, b, i, env, worklist=False)
    assert c0.tobytes() == c1.tobytes() and (r0, v0) == (r1, v1)
    # the split loop ran as often as the host test derives: the one class that holds every label fills at levels 3, 4 and 5
    # (the probe case: at level 0), each level given up at its first part, and no other class holds a label
    splits = [row[7] for row in rows]
    if name in cc.SPLIT_COUNT_CASES:
        assert splits[0] >= 3 and splits == [3] + [0] * (len(rows) - 1), rows
    if name == "split_probe":
        assert splits[0] >= 1 and splits == [1] + [0] * (len(rows) - 1), rows
    if name == "many_classes":
        assert splits == [0] * len(rows), rows


def test_pairs23_forward_only(gmx, capfd):
    """without a reverse CSR round 1 evaluates every row again and finds nothing to change"""
    b, i = cc.case("pairs23")
    V = len(b) - 1
    g = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE)
    try:
        comm, r, c, st, rows = logged(g, capfd, {})
        want, rounds, conv = cc.pairs_closed_form(V)
        assert np.array_equal(comm, want) and (r, c) == (rounds, conv)
        assert (st["vertices_reached"], st["edges_examined"]) == (V, V)
        assert [row[:7] for row in rows] == [(0, V // 2, 0, 0, 0, V // 2, V // 2), (1, V // 2, 0, 0, 0, V // 2, 0)]
    finally:
        g.free()


@pytest.mark.parametrize("name", ["rmat12", "rmat14p", "multi"])
def test_named_graphs_round_by_round(gmx, capfd, name):
    """the exact work of every round where test_work_list_changes_the_work_only asserts `less`: a mark that is set needlessly,
    a dirty bit that is not cleared or a row evaluated twice changes a line"""
    if name == "multi":
        V, b, i, rb, ri = multigraph()
        g = gmx.Graph.upload(b, i, rb, ri)
    else:
        b, i = named_graph(name)
        g = gmx.Graph.upload(b, i)
    try:
        for env in ({}, cc.SMALL):
            for worklist in (True, False):
                _, _, _, _, rows = check_against_model(g, capfd, name, b, i, env, worklist)
                if name == "rmat12" and not env:
                    assert [row[7] for row in rows] == [0] * len(rows), rows      # evenly hashed ids: no class fills again
    finally:
        g.free()


@pytest.mark.parametrize("max_rounds", [0, 1])
@pytest.mark.parametrize("name", cc.CUT_CASES)
def test_cut_pass(gmx, graphs, capfd, name, max_rounds):
    """converged from the pass that commits nothing, through comm_overflow_kernel + comm_final_kernel"""
    b, i = cc.case(name)
    env = cc.RUNS[name][0]
    comm, r, c, st, rows = check_against_model(graphs(name), capfd, name, b, i, env, max_rounds=max_rounds)
    assert r == max_rounds and bool(c) == is_fixpoint(b, i, comm)
    if max_rounds == 0:
        assert np.array_equal(comm, np.arange(len(b) - 1)) and c == 0 and not rows
    again = graphs(name).communities()                          # and the cut run leaves nothing behind
    assert np.array_equal(again[0], cc.model(name, {}).comm)


@pytest.mark.parametrize("name", cc.UPLOAD_CASES)
def test_upload_forms(gmx, graphs, capfd, name):
    b, i = cc.case(name)
    V = len(b) - 1
    env = cc.RUNS[name][0]
    rb, ri = csr(V, i, np.repeat(np.arange(V), np.diff(b)))
    given = gmx.Graph.upload(b, i, rb, ri)
    forward = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE)
    try:
        want = cc.model(name, env).comm
        for form, g, worklist in (("both given", given, True), ("reverse built", graphs(name), True), ("no reverse", forward, False)):
            comm, _, _, _, _ = check_against_model(g, capfd, name, b, i, env, worklist, has_reverse=g is not forward)
            assert comm.tobytes() == want.tobytes(), form
    finally:
        given.free()
        forward.free()
