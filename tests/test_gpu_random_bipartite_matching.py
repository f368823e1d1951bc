"""gmx_random_bipartite_matching (random_bipartite_matching.gm) on the device against the program as written
(test_random_bipartite_matching_host.rbm_literal) and, where that loop is too slow, the max / max formulation (rbm_model): every
hand case and named graph, the tail threshold forced to each path (and shown to be the path that ran, from the library's
GMX_RBM_LOG line), the schedule-independent counters and the bound that rules out rescanning matched or dead lefts, every upload
form of an unsorted multigraph, errors, empties, independence of two calls and the driver.

rmat12's hub row has 2376 slots, more than one 2048-item merge-path tile: a row is split across workgroups.  staircase64 matches
one pair per round (64 rounds), fanin4096 sends every proposal to one address.  The reference ships no generated
random_bipartite_matching.cc, so nothing reference-compiled exists for this program and no such fixture is used."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_random_bipartite_matching_host import (HAND, LEFT_TO_LEFT, NAMED, cover, csr_of, literal_of, model_of,
                                                 random_bipartite, rbm_graph, rbm_literal)
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_RBM_TAIL", "GMX_RBM_LOG")
HUGE = "2000000000"
FORCED = {"no_tail": {"GMX_RBM_TAIL": "0"}, "all_tail": {"GMX_RBM_TAIL": HUGE}}
LINE = re.compile(r"gmx random_bipartite_matching: V (\d+) E (\d+) lefts (\d+); tail (\d+); rounds (\d+) grid \+ (\d+) tail; matched (\d+); "
                  r"proposals (\d+) slots (\d+); ms ([0-9.]+) grid \+ ([0-9.]+) tail")
FIELDS = ("V", "E", "lefts", "tail_from", "grid_rounds", "tail_rounds", "matched", "proposals", "slots", "grid_ms", "tail_ms")


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


def logged(g, left, capfd, **env):
    """(match, count, stats, the fields of the library's line) of one call."""
    capfd.readouterr()
    with knobs(GMX_RBM_LOG="1", **env):
        match, cnt, st = g.random_bipartite_matching(left)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    f = {k: (float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, lines[0])}
    return match, cnt, st, f


def check(want, match, cnt, st=None):
    assert cnt == want[0] and match.dtype == np.int32 and np.array_equal(match, want[1])
    if st is not None:
        assert st["vertices_reached"] == cnt and st["iterations"] == want[2] and st["edges_reached"] == want[3]
        assert st["last_diff"] == 0 and st["kernel_ms"] >= 0


def upload(gmx, name, flags=0):
    b, i, left = rbm_graph(name)
    return gmx.Graph.upload(np.ascontiguousarray(b), np.ascontiguousarray(i), flags=flags), left


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(gmx, name):
    g, left = upload(gmx, name)
    for env in ({}, FORCED["no_tail"], FORCED["all_tail"]):
        with knobs(**env):
            check(literal_of(name), *g.random_bipartite_matching(left))


@pytest.mark.parametrize("name", ["rmat8", "rmat10", "rmat10p", "planted16", "star33", "chain4096", "staircase64", "rmat12"])
def test_parity_with_the_literal_loop(gmx, capfd, name):
    g, left = upload(gmx, name)
    match, cnt, st, f = logged(g, left, capfd)
    print("random_bipartite_matching %s: %s" % (name, f))
    check(literal_of(name), match, cnt, st)
    assert f["grid_rounds"] + f["tail_rounds"] == st["iterations"] and f["slots"] == st["edges_examined"]


def test_parity_rmat14_with_the_model(gmx, capfd):
    g, left = upload(gmx, "rmat14")
    match, cnt, st, f = logged(g, left, capfd)
    print("random_bipartite_matching rmat14: %s" % f)
    want = model_of("rmat14")
    check(want, match, cnt, st)
    assert (cnt, st["iterations"], st["edges_reached"]) == (6888, 4, 297857)
    assert f["grid_rounds"] > 0                              # 262144 slots: the grid kernels ran


def test_fanin_all_proposals_hit_one_address(gmx, capfd):
    g, left = upload(gmx, "fanin4096")
    for env in (FORCED["no_tail"], FORCED["all_tail"]):
        match, cnt, st, f = logged(g, left, capfd, **env)
        assert cnt == 1 and match[4096] == 4095 and match[4095] == 4096 and st["iterations"] == 1
        assert np.count_nonzero(match != -1) == 2 and st["edges_reached"] == 4096
        assert f["grid_rounds"] + f["tail_rounds"] == 1


def test_random_multigraphs(gmx):
    for seed in range(40):
        b, i, left = random_bipartite(seed)
        g = gmx.Graph.upload(b, i)
        with knobs(**(FORCED["no_tail"] if seed % 2 else {})):
            check(rbm_literal(b, i, left), *g.random_bipartite_matching(left))
        g.free()


@pytest.mark.parametrize("name", NAMED + ["rmat14"])
def test_counters(gmx, capfd, name):
    """iterations, proposals and the count do not depend on the schedule; the slots read lie between the proposals and the row
    lengths of the live lefts summed over the rounds: reading the row of a matched or dead left once more would break the bound."""
    g, left = upload(gmx, name)
    count, _, rounds, proposals, slots = model_of(name)
    for env in ({}, FORCED["no_tail"], FORCED["all_tail"]):
        _, cnt, st, f = logged(g, left, capfd, **env)
        assert (st["iterations"], st["edges_reached"], st["vertices_reached"]) == (rounds, proposals, count) and cnt == count
        assert proposals <= st["edges_examined"] <= slots
        assert (f["V"], f["E"], f["lefts"]) == (len(left), len(rbm_graph(name)[1]), int(np.count_nonzero(left)))
        assert (f["matched"], f["proposals"], f["slots"]) == (count, proposals, st["edges_examined"])


@pytest.mark.parametrize("forced", sorted(FORCED))
@pytest.mark.parametrize("name", ["staircase64", "planted16"])
def test_forced_paths(gmx, capfd, name, forced):
    """Each forced setting gives the literal loop's bytes, and ran the path it names."""
    g, left = upload(gmx, name)
    match, cnt, st, f = logged(g, left, capfd, **FORCED[forced])
    print(name, forced, f)
    check(literal_of(name), match, cnt, st)
    rounds = model_of(name)[2]
    assert f["grid_rounds"] + f["tail_rounds"] == rounds
    if forced == "no_tail":
        assert f["tail_from"] == 0 and f["tail_rounds"] == 0 and f["grid_rounds"] == rounds and f["tail_ms"] == 0
    else:
        assert f["grid_rounds"] == 0 and f["tail_rounds"] == rounds and f["tail_ms"] > 0


def test_default_planted16_uses_grid_rounds_and_the_tail(gmx, capfd):
    g, left = upload(gmx, "planted16")
    _, _, _, f = logged(g, left, capfd)
    assert f["grid_rounds"] > 0 and f["tail_rounds"] > 0 and f["tail_from"] == 4096


def test_upload_forms_give_one_match(gmx):
    """The result is indexed by vertex: whatever the upload did to the rows, the bytes are the same."""
    V = 300
    b, i, _, _ = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 2000, 3))
    hb, hi, left = cover(b, i)
    want = rbm_literal(hb, hi, left)
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    for regime in ({}, FORCED["no_tail"]):
        for flags in (0, S, N, S | N):
            g = gmx.Graph.upload(hb, hi, flags=flags)
            with knobs(**regime):
                check(want, *g.random_bipartite_matching(left))
            g.free()


def test_left_to_left_edge_is_an_error(gmx):
    V, s, d, left = LEFT_TO_LEFT
    b, i = csr_of(V, s, d)
    g = gmx.Graph.upload(b, i)
    L = gmx.lib()
    left = np.asarray(left, np.uint8)
    for env in (FORCED["no_tail"], FORCED["all_tail"]):
        match = np.full(V, 77, np.int32)
        cnt = C.c_int32(-1)
        with knobs(**env):
            assert L.gmx_random_bipartite_matching(g._h, left.ctypes.data, match.ctypes.data, C.byref(cnt), None) == GMX_ERR_ARG
        assert b"0 -> 1" in L.gmx_last_error() and np.all(match == 77)
    with pytest.raises(Exception):
        g.random_bipartite_matching(left)


def test_errors_and_empties(gmx):
    g, left = upload(gmx, "star33")
    left = np.ascontiguousarray(left)
    L = gmx.lib()
    V = len(left)
    match = np.full(V, 77, np.int32)
    cnt = C.c_int32(-1)
    f = L.gmx_random_bipartite_matching
    assert f(None, left.ctypes.data, match.ctypes.data, C.byref(cnt), None) == GMX_ERR_ARG
    assert f(g._h, left.ctypes.data, match.ctypes.data, None, None) == GMX_ERR_ARG
    assert f(g._h, None, match.ctypes.data, C.byref(cnt), None) == GMX_ERR_ARG
    assert f(g._h, left.ctypes.data, None, C.byref(cnt), None) == GMX_ERR_ARG
    assert np.all(match == 77)
    assert f(g._h, left.ctypes.data, match.ctypes.data, C.byref(cnt), None) == 0 and cnt.value == 2   # stats may be NULL
    assert np.array_equal(match, literal_of("star33")[1])
    e = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))                                # V = 0
    cnt = C.c_int32(-1)
    assert f(e._h, None, None, C.byref(cnt), None) == 0 and cnt.value == 0
    m, c, st = e.random_bipartite_matching(np.zeros(0, np.uint8))
    assert len(m) == 0 and c == 0 and st["iterations"] == 0
    e = gmx.Graph.upload(np.zeros(1002, np.int32), np.zeros(0, np.int32))                             # E = 0
    m, c, st = e.random_bipartite_matching(np.arange(1001) % 2)
    assert len(m) == 1001 and np.all(m == -1) and c == 0 and st["iterations"] == 0 and st["edges_examined"] == 0


def test_two_calls_with_different_sides_are_independent(gmx):
    """Nothing is cached on the graph: the complete bipartite pattern below is matched from either side."""
    V = 6
    s = np.repeat(np.arange(V), V)
    d = np.tile(np.arange(V), V)
    keep = (s < 3) != (d < 3)                                 # edges between {0, 1, 2} and {3, 4, 5}, both directions
    b, i = csr_of(V, s[keep], d[keep])
    g = gmx.Graph.upload(b, i)
    for left in ([1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0]):
        left = np.asarray(left, np.uint8)
        check(rbm_literal(b, i, left), *g.random_bipartite_matching(left))


def test_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "random_bipartite_matching")
    assert os.path.exists(exe), "bin/random_bipartite_matching not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    n = rbm_literal(*cover(c["begin"], c["node_idx"]))[0]
    assert "matching size = %d\n" % n in out.stdout
    assert out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n")
