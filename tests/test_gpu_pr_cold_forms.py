"""The binned PageRank sweep (csrc/gmx_pr_cold.hip) on graphs designed so that every phase-1 form runs every case of its
prefetch loop -- no whole super-step, one, two, an odd and an even number of them -- and every phase-2/3 finish is taken,
in fp32 and fp64, on graphs small enough for the default suite (pr_cold_shapes.py describes them and why).

Each case is a plan build plus two runs of 4 steps.  What is asserted:
  * the ranks against the fp64 oracle within the project's bars, `diff` within the bars the neighbouring tests use.  The
    graphs are built so that every single term of every row is at least 1e-4 of the row's sum (test_pr_cold_shapes.py):
    one lost, doubled or misplaced term shows 100 x above the fp32 bar;
  * PageRankState.cold_shape() equals the host model's prediction for the configuration, and the literal promises of the
    design (which form has how many super-steps, which finish has items): the plan proves which paths ran;
  * bit identity: the downloaded ranks are equal across every GMX_PR_COLD_CHUNK1 (pairs are cut at 512-entry blocks at
    plan time, not by the work items), across every phase-2/3 setting (integer accumulation, one conversion expression
    in all three finishes) and between two runs of one plan.  `diff` is summed per work item in floating point and is
    compared at its bar only.

The knobs are read when the state is created."""
import numpy as np
import pytest

import pr_cold_shapes as S
import pyoracle as po

pytestmark = pytest.mark.gpu
PR_RTOL_F32 = 1e-6      # the bars of test_gpu_parity.py
PR_RTOL_F64 = 1e-12
KNOBS = ("GMX_PR_COLD", "GMX_PR_COLD_CLASS_DENSITY", "GMX_PR_COLD_PAIR_X100", "GMX_PR_COLD_CHUNK1", "GMX_PR_COLD_CHUNK",
         "GMX_PR_COLD_SPLIT_X100", "GMX_PR_SLICES")
_oracle, _runs = {}, {}


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def oracle(name):
    """(host graph, ranks, diff) of the fp64 reference after 4 steps; computed once per graph."""
    if name not in _oracle:
        V, begin, idx = S.csr(name)
        og = po.Graph(V, begin, idx).prepare()
        want, _, want_diff = po.pagerank(og, 1e-300, S.DAMP, S.ITERS)
        want.setflags(write=False)
        _oracle[name] = (og, want, want_diff)
    return _oracle[name]


def run(gmx, monkeypatch, name, elem, density=1, pair_x100=125, chunk1=None, chunk2=None):
    """Plan + 4 steps, twice, under the given knobs: ranks, diff, the plan's shape and whether the second run repeated the
    first bit for bit.  One result per configuration: the bit-identity tests compare what the oracle tests measured."""
    key = (name, elem, density, pair_x100, chunk1, chunk2)
    if key in _runs:
        return _runs[key]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    env = {"GMX_PR_COLD": S.hot_ids(name), "GMX_PR_COLD_CLASS_DENSITY": density, "GMX_PR_COLD_PAIR_X100": pair_x100,
           "GMX_PR_COLD_CHUNK1": chunk1, "GMX_PR_COLD_CHUNK": chunk2}
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))
    og, _, _ = oracle(name)
    g = gmx.Graph.upload(og.begin, og.node_idx, og.r_begin, og.r_node_idx)
    st = gmx.PageRankState(g, elem, 0, 1, gmx.GMX_PR_RELABEL | gmx.GMX_PR_HOT_LDS | gmx.GMX_PR_SLICED | gmx.GMX_PR_COLD_PB)
    info, shape = st.cold_info(), st.cold_shape()
    out = []
    for _ in range(2):
        st.reset(S.DAMP)
        for _ in range(S.ITERS):
            st.step()
        out.append((st.download(), st.diff()))
    st.free()
    g.free()
    out[0][0].setflags(write=False)
    _runs[key] = {"rank": out[0][0], "diff": out[0][1], "info": info, "shape": shape,
                  "repeats": np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]}
    return _runs[key]


def check_against_oracle(name, elem, r):
    _, want, want_diff = oracle(name)
    err = float(np.max(np.abs(r["rank"].astype(np.float64) - want) / want))
    derr = abs(r["diff"] - want_diff) / want_diff
    print(name, elem, "rank rel err %.3g diff rel err %.3g" % (err, derr), r["shape"])
    assert r["info"]["hot_ids"] == S.hot_ids(name) and r["info"]["cold_edges"] > 0
    assert err < (PR_RTOL_F64 if elem == 8 else PR_RTOL_F32)
    assert derr <= (1e-9 if elem == 8 else 1e-3)
    assert r["repeats"]


def check_against_model(r, model):
    assert r["shape"] == {k: model[k] for k in r["shape"]}


@pytest.mark.parametrize("chunk1", [1024, 5120, 32768])
@pytest.mark.parametrize("density", [1, 0])
@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_form_at_every_superstep_case(gmx, name, elem, density, chunk1, monkeypatch):
    r = run(gmx, monkeypatch, name, elem, density, chunk1=chunk1)
    check_against_oracle(name, elem, r)
    check_against_model(r, S.plan_model(name, elem, density, 125, chunk1))
    sh = r["shape"]
    steps, modes = sh["supersteps"], sh["tiles_by_mode"]
    assert sum(modes.values()) == 1 and sh["fused"] and sh["items2_chunk"] == 0
    if name == "A" and density == 1:
        assert modes["classed"] == 1 and all(sh["groups"][f] > 0 for f in ("E1", "E2", "E4", "E8", "H"))
        if chunk1 == 32768:
            assert [steps[f] for f in ("E1", "E2", "E4", "E8", "H")] == [{5}, {4}, {3}, {2}, {1}]
        if chunk1 == 1024:
            assert all(s <= {0, 1} for s in steps.values())
    if name == "A" and density == 0:
        assert modes["pair"] == 1 and sh["groups"]["pair"] > 0
        if chunk1 == 5120:      # the items of five super-steps and the shorter last one
            assert 5 in steps["pair"] and steps["pair"] & {1, 2, 3, 4}
        if chunk1 == 1024:
            assert steps["pair"] == {1}
    if name == "B" and density == 1:
        assert modes["singles"] == 1
        assert 3 in steps["E1"] if chunk1 > 1024 else steps["E1"] == {0, 1}
    if name == "B" and density == 0:
        assert modes["edge"] == 1 and steps["edge"] == {0} and sh["groups"]["edge"] > 0


@pytest.mark.parametrize("density", [1, 0])
@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ranks_do_not_depend_on_the_phase1_items(gmx, name, elem, density, monkeypatch):
    first = run(gmx, monkeypatch, name, elem, density, chunk1=None)      # the default: items of one super-step
    assert first["repeats"]
    for chunk1 in (1024, 5120, 32768):
        r = run(gmx, monkeypatch, name, elem, density, chunk1=chunk1)
        assert r["repeats"] and np.array_equal(r["rank"], first["rank"]), chunk1


@pytest.mark.parametrize("finish", ["sole", "few", "many", "mixed"])
@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("primed", ["", "'"], ids=["fused", "unfused"])
def test_every_finish(gmx, primed, elem, finish, monkeypatch):
    """The sole-chunk flush of the accumulate kernel, the few-slot and the many-slot reduction, each alone and all three in
    one plan, with the fused finish (A: every in-edge binned) and the unfused one (A': the pull sweep has a share).  With
    one tile a bin holds one item per row, so the bins of A differ in size only by their padding: three kinds of bin in
    one plan need the SINGLES storage (an item per edge) of Am, whose rows are dealt their in-degrees by vertex id."""
    name, pair_x100 = ("Am" + primed, 400) if finish == "mixed" else ("A" + primed, 125)
    chunk2 = S.FINISH[finish][elem]
    r = run(gmx, monkeypatch, name, elem, 1, pair_x100, chunk2=chunk2)
    check_against_oracle(name, elem, r)
    check_against_model(r, S.plan_model(name, elem, 1, pair_x100, None, chunk2))
    sh = r["shape"]
    assert sh["fused"] == (primed == "")
    if finish == "sole":
        assert sh["items2_chunk"] == 0 and sh["items2_sole"] > 0 and sh["bins_few"] == sh["bins_many"] == 0
    elif finish == "few":
        assert sh["bins_few"] > 0 and sh["bins_many"] == 0 and 4 * sh["bins_few"] <= sh["items2_chunk"] <= 8 * sh["bins_few"]
    elif finish == "many":
        assert sh["bins_many"] > 0 and sh["items2_chunk"] > 8 * sh["bins_many"]
    else:
        assert sh["tiles_by_mode"]["singles"] == 1
        assert sh["bins_few"] > 0 and sh["bins_many"] > 0 and sh["items2_sole"] > 0
    # the same graph and storage with no bin split: the same bits
    sole = run(gmx, monkeypatch, name, elem, 1, pair_x100, chunk2=S.FINISH["sole"][elem])
    assert sole["shape"]["items2_chunk"] == 0 and np.array_equal(r["rank"], sole["rank"])


@pytest.mark.parametrize("density", [1, 0])
@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("name,pair_x100,modes", [("B", 100, ("pair", "classed")), ("A", 400, ("edge", "singles"))])
def test_pair_threshold_knob(gmx, name, pair_x100, modes, elem, density, monkeypatch):
    """GMX_PR_COLD_PAIR_X100 = edges per pair from which a tile counts as a pair tile: 100 stores B's single edges as pairs
    (in length classes, or in the generic pair form), 400 stores A's rows edge by edge (SINGLES, or the edge form)."""
    r = run(gmx, monkeypatch, name, elem, density, pair_x100)
    check_against_oracle(name, elem, r)
    check_against_model(r, S.plan_model(name, elem, density, pair_x100))
    assert r["shape"]["tiles_by_mode"][modes[density]] == 1 and sum(r["shape"]["tiles_by_mode"].values()) == 1
