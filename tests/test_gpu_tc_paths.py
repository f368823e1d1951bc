"""tc_oriented_kernel (gmx_tc.hip) against the oracle on every one of its code paths.

The kernel picks one of six branches per slot from four thresholds, each with a staged (LDS) and an in-memory form.  The
inputs and the knob matrix of tc_paths_common.py reach all eleven (branch, lds/mem) pairs -- test_tc_paths_host.py asserts
that with a restatement of the selection -- among them the three "lane alone, list in memory" arms and the default hub
regime with a real non-hub population (V = 2^17 > 65536 hubs).  Expected counts: the merge oracle, equal to the closed
form where there is one.  GMX_TC_HUBS is read when the oriented copy is built, so every case uploads afresh."""
import pytest

import pyoracle as po
import tc_paths_common as tp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


_CASES = {}


def case(name):
    """(begin, node_idx, T) -- built and counted by the oracle once per module."""
    if name not in _CASES:
        build, closed = {**tp.GRAPHS, **tp.TINY}[name]
        begin, idx = build()
        T = po.triangle_counting_merge(tp.oracle_graph(begin, idx))
        if closed is not None:
            assert closed() == T, name
        _CASES[name] = (begin, idx, T)
    return _CASES[name]


def set_knobs(monkeypatch, knobs):
    for var in tp.KNOB_VARS + ("GMX_TC_NO_LDS", "GMX_TC_NO_ORIENT"):
        monkeypatch.delenv(var, raising=False)
    for var, val in tp.KNOBS[knobs].items():
        monkeypatch.setenv(var, val)


def upload(gmx, begin, idx):
    """Both CSRs given: the symmetric-simple check passes and the oriented copy is built at the first count."""
    return gmx.Graph.upload(begin, idx, begin, idx)


@pytest.mark.parametrize("knobs", list(tp.KNOBS))
@pytest.mark.parametrize("name", list(tp.GRAPHS))
def test_count_on_every_path(gmx, monkeypatch, name, knobs):
    begin, idx, T = case(name)
    set_knobs(monkeypatch, knobs)
    g = upload(gmx, begin, idx)
    try:
        got = g.triangle_counting()[0]
        print("%s under %s: %d (oracle %d)" % (name, knobs, got, T))
        assert got == T
        assert g.triangle_counting()[0] == T          # the claim counter starts from zero on every call
    finally:
        g.free()


@pytest.mark.parametrize("name", list(tp.GRAPHS))
def test_default_knobs_every_form(gmx, monkeypatch, name):
    begin, idx, T = case(name)
    set_knobs(monkeypatch, "default")
    g = upload(gmx, begin, idx)
    try:
        assert g.triangle_counting()[0] == T
        for nparts in (2, 3, 8):
            assert sum(g.triangle_counting(p, nparts)[0] for p in range(nparts)) == T, nparts
        assert g.triangle_counting_cn()[0] == T
        monkeypatch.setenv("GMX_TC_NO_LDS", "1")      # the slot kernels on the same oriented copy
        assert g.triangle_counting()[0] == T
        monkeypatch.delenv("GMX_TC_NO_LDS")
    finally:
        g.free()
    monkeypatch.setenv("GMX_TC_NO_ORIENT", "1")       # emitted order
    g = upload(gmx, begin, idx)
    try:
        assert g.triangle_counting()[0] == T
    finally:
        g.free()
    monkeypatch.delenv("GMX_TC_NO_ORIENT")
    g = gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_NO_REVERSE)   # forward-only form
    try:
        assert g.triangle_counting()[0] == T
    finally:
        g.free()


@pytest.mark.parametrize("knobs", ["default", "hubs0"])
@pytest.mark.parametrize("name", list(tp.TINY))
def test_tiny_cliques_at_the_hub_boundary(gmx, monkeypatch, name, knobs):
    """No hub matrix at all (V < 64), and one of 64 hubs over 1 and over 36 non-hubs."""
    begin, idx, T = case(name)
    set_knobs(monkeypatch, knobs)
    g = upload(gmx, begin, idx)
    try:
        assert g.triangle_counting()[0] == T
        assert g.triangle_counting()[0] == T
        assert sum(g.triangle_counting(p, 3)[0] for p in range(3)) == T
    finally:
        g.free()
