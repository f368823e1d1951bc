"""gmx_louvain on the device, byte for byte against the one-thread model (louvain_model.py): comm, num_comms, num_levels,
intra, the 8 bytes of the modularity, the three stats and the counters of the GMX_LOUVAIN_LOG line -- on the host file's small
graphs, RMAT, rows at every regime boundary, a hub row that overflows the smallest table, every knob at its extremes, weights at
2^31 - 1, every upload form, the refusals, one handle shared with other entries, and the driver."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from louvain_model import louvain_model
from louvain_sequences import LOG, same   # (importing it also adds louvain's row to the table of interleaved entries)
from test_gpu_sssp_path import gm_rand32_lengths
from test_louvain_host import SMALL, hub_and_ring, hubs_of_degrees
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
KNOBS = ("GMX_LOUVAIN_WAVE_MIN", "GMX_LOUVAIN_BLOCK_MIN", "GMX_LOUVAIN_LDS_SLOTS", "GMX_LOUVAIN_PHASES", "GMX_LOUVAIN_LOG")
INT32_MAX = 2 ** 31 - 1
# every knob at both ends of its range (the defaults are 33, 256 and 4096)
SWEEP = [{}, {"wave_min": 1}, {"wave_min": 33, "block_min": 33}, {"block_min": 1}, {"block_min": INT32_MAX}, {"lds_slots": 512}, {"lds_slots": 8192},
         {"wave_min": 1, "block_min": INT32_MAX, "lds_slots": 512}, {"wave_min": 2, "block_min": 2, "lds_slots": 512}]


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def run(capfd, monkeypatch):
    def call(g, weight=None, max_levels=32, max_rounds=64, **knobs):
        """One call with GMX_LOUVAIN_LOG and the knobs given (the others unset): Graph.louvain()'s tuple + the line's fields."""
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("GMX_LOUVAIN_LOG", "1")
        for name, v in knobs.items():
            monkeypatch.setenv("GMX_LOUVAIN_" + name.upper(), str(v))
        capfd.readouterr()
        out = g.louvain(weight, max_levels, max_rounds)
        err = capfd.readouterr().err
        m = LOG.search(err)
        assert m, err
        f = {k: (v if k == "sizes" else int(v)) for k, v in m.groupdict().items()}
        assert (f["V"], f["E"], f["weighted"]) == (g.V, g.E, int(weight is not None))
        assert out[5]["kernel_ms"] > 0 and (out[5]["h2d_ms"] > 0) == (weight is not None)
        return out + (f,)
    return call


@functools.lru_cache(maxsize=None)
def rmat_arrays(scale, symmetrize):
    import gmx
    g = gmx.Graph.rmat(1 << scale, 16 << scale, 1997, 0.57, 0.19, 0.19, False)
    if symmetrize:
        s = g.symmetrize()
        g.free()
        g = s
    begin, idx, _, _ = g.download(reverse=False)
    g.free()
    begin.setflags(write=False)
    idx.setflags(write=False)
    return len(begin) - 1, begin, idx


def rmat_weights(scale, symmetrize, kind):
    V, begin, idx = rmat_arrays(scale, symmetrize)
    if kind == "none":
        return None
    rng = np.random.default_rng(scale)
    return (rng.integers(1, 100, len(idx)) if kind == "small" else rng.integers(1, INT32_MAX, len(idx), endpoint=True)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def rmat_want(scale, symmetrize, kind, max_levels=32, max_rounds=64):
    """The model's result: computed once, shared, left unchanged."""
    V, begin, idx = rmat_arrays(scale, symmetrize)
    return louvain_model(V, begin, idx, rmat_weights(scale, symmetrize, kind), max_levels, max_rounds)


# ---------------------------------------------------------------- the small graphs
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs(gmx, run, name):
    V, begin, idx = SMALL[name]()
    g = gmx.Graph.upload(begin, idx)
    for levels, rounds in ((32, 64), (0, 64), (1, 64), (32, 1), (2, 2)):
        same(louvain_model(V, begin, idx, None, levels, rounds), run(g, None, levels, rounds))
    g.free()


def test_k44_rolls_both_half_rounds_back(gmx, run):
    V, begin, idx = SMALL["k44"]()
    g = gmx.Graph.upload(begin, idx)
    out = run(g)
    assert out[0].tolist() == list(range(8)) and out[2] == 0 and out[3] == -0.125 and (out[6]["rollbacks"], out[6]["rounds"], out[6]["moves"]) == (2, 1, 0)
    g.free()


def test_empty_inputs(gmx, capfd, monkeypatch):
    monkeypatch.setenv("GMX_LOUVAIN_LOG", "1")
    g = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))
    comm, nc, nl, q, intra, st = g.louvain()
    assert len(comm) == 0 and (nc, nl, q, intra) == (0, 0, 0.0, 0) and st["vertices_reached"] == 0
    g.free()
    g = gmx.Graph.upload(np.zeros(6, np.int32), np.zeros(0, np.int32))
    for w in (None, np.zeros(0, np.int32)):
        comm, nc, nl, q, intra, st = g.louvain(w)
        assert comm.tolist() == list(range(5)) and (nc, nl, q, intra) == (5, 0, 0.0, 0)
        assert (st["iterations"], st["vertices_reached"], st["edges_examined"]) == (0, 5, 0)
    g.free()
    assert "gmx louvain" not in capfd.readouterr().err


# ---------------------------------------------------------------- RMAT
@pytest.mark.parametrize("kind", ["none", "small", "int32"])
@pytest.mark.parametrize("scale,symmetrize", [(s, y) for s in (8, 10, 12) for y in (False, True)])
def test_rmat_against_the_model(gmx, run, scale, symmetrize, kind):
    V, begin, idx = rmat_arrays(scale, symmetrize)
    g = gmx.Graph.upload(begin, idx)
    out = run(g, rmat_weights(scale, symmetrize, kind))
    g.free()
    want = rmat_want(scale, symmetrize, kind)
    same(want, out)
    if scale == 12 and kind == "none":
        assert len(want["sizes"]) >= 3 and want["rollbacks"] >= 1


def test_rmat_limits(gmx, run):
    """A level cut by max_rounds, a run cut by max_levels, no level at all."""
    V, begin, idx = rmat_arrays(10, False)
    g = gmx.Graph.upload(begin, idx)
    for levels, rounds in ((32, 1), (1, 64), (2, 3), (0, 5)):
        want = rmat_want(10, False, "none", levels, rounds)
        same(want, run(g, None, levels, rounds))
    assert rmat_want(10, False, "none", 32, 1)["cuts"] >= 1 and rmat_want(10, False, "none", 1, 64)["num_levels"] == 1 < rmat_want(10, False, "none")["num_levels"]
    g.free()


def test_every_weight_at_int32_max(gmx, run):
    """m2 and every e[D] carry the factor 2^31 - 1, so every product is about 2^62 times the unweighted one and exceeds 64
    bits, while every comparison is the unweighted one: the partition must be the unweighted partition.
    An input on which a model that scores in float64 gives another partition was searched for on the CPU and would stand
    here.  The search (RMAT scale 8 and 10, generator seeds 1 .. 16, three weightings each: all 2^31 - 1, uniform
    in [1, 2^31 - 1], 2^31 - 1 minus 0 .. 3: 96 inputs, 20 s) found none: equal integer scores stay equal after rounding and
    unequal ones differ by far more than 2^-53 of their size.  This case stays in its place."""
    V, begin, idx = rmat_arrays(10, True)
    w = np.full(len(idx), INT32_MAX, np.int32)
    g = gmx.Graph.upload(begin, idx)
    out = run(g, w)
    g.free()
    want = louvain_model(V, begin, idx, w)
    same(want, out)
    plain = rmat_want(10, True, "none")
    assert out[0].tobytes() == plain["comm"].tobytes() and out[4] == plain["intra"] * INT32_MAX and want["qnum"] == plain["qnum"] * INT32_MAX ** 2
    assert want["m2"] * want["intra"] > 2 ** 64


# ---------------------------------------------------------------- regimes, the class passes, the knobs
def test_rows_at_the_regime_boundaries(gmx, run):
    """Rows of exactly WAVE_MIN - 1, WAVE_MIN, BLOCK_MIN - 1 and BLOCK_MIN entries, at the defaults and with the thresholds
    moved onto other rows of the same graph."""
    V, begin, idx = hubs_of_degrees((32, 33, 255, 256, 31, 34, 1, 2))
    want = louvain_model(V, begin, idx)
    g = gmx.Graph.upload(begin, idx)
    for knobs in ({}, {"wave_min": 32}, {"wave_min": 31, "block_min": 34}, {"block_min": 255}, {"block_min": 257}, {"wave_min": 2, "block_min": 3}):
        same(want, run(g, **knobs))
    g.free()


@functools.lru_cache(maxsize=None)
def hub_case():
    V, begin, idx = hub_and_ring(1500)
    return V, begin, idx, louvain_model(V, begin, idx)


@pytest.mark.parametrize("knobs", [{"lds_slots": 512}, {"lds_slots": 512, "block_min": INT32_MAX}, {"lds_slots": 512, "block_min": 1, "wave_min": 1}, {}],
                         ids=["block", "wave", "all_block", "default"])
def test_hub_row_with_more_labels_than_table_slots(gmx, run, knobs):
    """A star of 1500 leaves plus a ring among the leaves: at round 0 the hub's row holds 1500 distinct labels, more than the
    512 slots of the smallest workgroup table (64 of a wave's): the row goes to the passes over label classes."""
    V, begin, idx, want = hub_case()
    g = gmx.Graph.upload(begin, idx)
    out = run(g, **knobs)
    g.free()
    same(want, out)
    assert (out[6]["overflowed"] > 0) == ("lds_slots" in knobs)


@pytest.mark.parametrize("case", ["rmat10_sym", "rmat10_int32", "hub"])
def test_knobs_change_no_byte(gmx, run, case):
    if case == "hub":
        V, begin, idx, want = hub_case()
        w = None
    else:
        sym, kind = (True, "none") if case == "rmat10_sym" else (False, "int32")
        (V, begin, idx), w, want = rmat_arrays(10, sym), rmat_weights(10, sym, kind), rmat_want(10, sym, kind)
    g = gmx.Graph.upload(begin, idx)
    for knobs in SWEEP:
        same(want, run(g, w, **knobs))
    g.free()


def test_phases_knob_changes_no_byte(gmx, run):
    V, begin, idx = rmat_arrays(8, False)
    g = gmx.Graph.upload(begin, idx)
    same(rmat_want(8, False, "none"), run(g, phases=1))
    g.free()


# ---------------------------------------------------------------- upload forms
@pytest.mark.parametrize("V,hub_edges", [(64, 200), (3000, 9000)])
def test_upload_forms_give_one_set_of_bytes(gmx, run, V, hub_edges):
    begin, idx, rb, ri = unsorted_multigraph(V, hub_edges, V)
    w = np.random.default_rng(V).integers(1, 1000, len(idx)).astype(np.int32)   # by uploaded slot
    want = louvain_model(V, begin, idx, w)
    for form in ("verbatim", "sorted", "no_reverse"):
        g = (gmx.Graph.upload(begin, idx, rb, ri, flags=0) if form == "verbatim" else
             gmx.Graph.upload(begin, idx, flags=gmx.GMX_GRAPH_SORT_ROWS if form == "sorted" else gmx.GMX_GRAPH_NO_REVERSE))
        assert (g.edge_order() is not None) == (form == "sorted")
        same(want, run(g, w))
        if form == "sorted" and V == 64:
            same(louvain_model(V, begin, idx), run(g))
        g.free()
    # the slots of every row in another order, the weights following their slots: the same graph
    rows = np.repeat(np.arange(V), np.diff(begin))
    order = np.lexsort((np.random.default_rng(7).random(len(idx)), rows))
    assert not np.array_equal(idx[order], idx)
    for flags in (0, gmx.GMX_GRAPH_SORT_ROWS):
        g = gmx.Graph.upload(begin, np.ascontiguousarray(idx[order]), flags=flags)
        same(want, run(g, np.ascontiguousarray(w[order])))
        g.free()


# ---------------------------------------------------------------- refusals, one handle
def test_refusals_leave_the_handle_usable(gmx, run):
    V, begin, idx = rmat_arrays(8, False)
    want = rmat_want(8, False, "none")
    g = gmx.Graph.upload(begin, idx)
    for bad in (0, -1):
        w = np.ones(len(idx), np.int32)
        w[len(idx) // 3] = bad
        with pytest.raises(gmx.GmxError, match=r"gmx status -1:.*weight"):
            g.louvain(w)
        same(want, run(g))
    with pytest.raises(gmx.GmxError, match=r"gmx status -1:.*max_rounds"):
        g.louvain(None, 32, 0)
    with pytest.raises(gmx.GmxError, match=r"gmx status -1:.*max_levels"):
        g.louvain(None, -1, 64)
    same(want, run(g))
    same(louvain_model(V, begin, idx, np.ones(len(idx), np.int32)), run(g, np.ones(len(idx), np.int32)))
    g.free()


def test_repeatable_and_after_other_entries_of_the_handle(gmx, run):
    V, begin, idx = rmat_arrays(10, True)
    want = rmat_want(10, True, "none")
    g = gmx.Graph.upload(begin, idx)
    a, b = run(g), run(g)
    same(want, a)
    same(want, b)
    k4 = g.kclique(4)
    lp = g.communities()
    same(want, run(g))
    w = rmat_weights(10, True, "small")
    same(rmat_want(10, True, "small"), run(g, w))
    again_k4, again_lp = g.kclique(4), g.communities()
    assert again_k4[0].tobytes() == k4[0].tobytes() and again_k4[1] == k4[1] and again_lp[0].tobytes() == lp[0].tobytes()
    g.free()


def test_dropin_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "louvain")
    assert os.path.exists(exe), "bin/louvain not built"
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "16", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    begin, idx = np.asarray(c["begin"], np.int64), np.asarray(c["node_idx"], np.int64)
    m = louvain_model(256, begin, idx, gm_rand32_lengths(len(idx)))
    for line in ("num_communities = %d\n" % m["num_comms"], "num_levels = %d\n" % m["num_levels"], "modularity = %.17g\n" % m["modularity"],
                 "largest_community = %d\n" % int(np.bincount(m["comm"]).max())):
        assert line in out.stdout, (line, out.stdout)
