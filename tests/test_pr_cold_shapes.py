"""CPU: the designed graphs of pr_cold_shapes.py are what the GPU tests of the binned PageRank sweep take them for.

The construction itself (histograms, who has out-edges), the input condition that makes a single lost, doubled or
misplaced term visible far above the comparison bar, and -- through the host model of the plan -- which phase-1 forms,
super-step counts and phase-2/3 finishes every configuration of test_gpu_pr_cold_forms.py is designed to run."""
import numpy as np
import pytest

import pr_cold_shapes as S
import pyoracle as po

GRAPHS = ("A", "A'", "Am", "Am'", "B")


def in_degrees_from(name, lo, hi):
    """in-degree histogram of the graph counting only the edges whose source has internal id in [lo, hi)"""
    V, src, dst = S.edges(name)
    p = S.relabel(np.bincount(src, minlength=V))[src]
    deg = np.bincount(dst[(p >= lo) & (p < hi)], minlength=V)
    k, n = np.unique(deg[deg > 0], return_counts=True)
    return dict(zip(k.tolist(), n.tolist()))


@pytest.mark.parametrize("name,hist", [("A", S.HIST_A), ("A'", S.HIST_A), ("Am", S.HIST_AM), ("Am'", S.HIST_AM)])
def test_in_degree_histogram(name, hist):
    T = S.hot_ids(name)
    assert in_degrees_from(name, T, T + S.NSRC) == hist           # the binned edges: a row's in-degree is its pair's length
    V, src, dst = S.edges(name)
    assert len(np.unique(dst)) == sum(hist.values())              # the hot edges of the primed graphs add no row
    assert int((S.relabel(np.bincount(src, minlength=V))[src] >= T).sum()) <= 500_000   # the binned edges
    if name.startswith("Am"):
        assert sum(hist.values()) % 16384 == 300 and sum(hist.values()) % 8192 == 300


@pytest.mark.parametrize("name", GRAPHS)
def test_sources_fill_the_first_8192_positions(name):
    V, src, dst = S.edges(name)
    outdeg = np.bincount(src, minlength=V)
    T = S.hot_ids(name)
    assert int((outdeg > 0).sum()) == T + S.NSRC
    perm = S.relabel(outdeg)
    assert sorted(perm[outdeg > 0].tolist()) == list(range(T + S.NSRC))
    if T:       # every hot source is strictly hotter than every original one: GMX_PR_COLD = 8192 cuts between them
        assert outdeg[perm < T].min() > outdeg[(perm >= T) & (outdeg > 0)].max()
    if name == "B":
        assert outdeg[outdeg > 0].min() == 8 and outdeg.max() == 18
    else:       # out-degrees within a factor of about 6
        cold = outdeg[(perm >= T) & (outdeg > 0)]
        assert cold.max() <= 7 * cold.min()


@pytest.mark.parametrize("name", GRAPHS)
def test_no_term_hides_in_its_row(name):
    """Over the 4 iterations every row's smallest term is at least 1e-4 of the row's sum: 100 x the fp32 bar."""
    worst, distinct, rank = S.row_term_ratio(name)
    print(name, "smallest term / row sum", worst, "distinct contributions", distinct)
    assert worst >= S.MIN_TERM
    if name != "B":     # (B's sources differ by out-degree and little else: a term read from the wrong source is caught on
        assert distinct > S.NSRC // 2   # A, which GMX_PR_COLD_PAIR_X100 = 400 sends through B's edge and SINGLES forms too)
    # the numpy iteration is the oracle's (parallel in-edges count once each)
    V, begin, idx = S.csr(name)
    want, _, _ = po.pagerank(po.Graph(V, begin, idx).prepare(), 1e-300, S.DAMP, S.ITERS)
    assert float(np.max(np.abs(rank - want) / want)) < 1e-12


@pytest.mark.parametrize("elem", [4, 8])
def test_designed_phase1_shapes(elem):
    m = S.plan_model("A", elem, 1, 125, 32768)
    assert m["tiles_by_mode"]["classed"] == 1 and m["fused"]
    assert [m["supersteps"][f] for f in ("E1", "E2", "E4", "E8", "H")] == [{5}, {4}, {3}, {2}, {1}]
    for f in ("E1", "E2", "E4", "E8", "H"):     # ... plus a leftover of several blocks, and room to the next super-step
        left = m["groups"][f] % S.SUPER_GROUPS
        assert 4 * S.BLK_GROUPS <= left <= S.SUPER_GROUPS - 4 * S.BLK_GROUPS, (f, left)
    m = S.plan_model("A", elem, 1, 125, 1024)
    assert all(s <= {0, 1} for s in m["supersteps"].values()) and 1 in m["supersteps"]["E1"]
    m = S.plan_model("A", elem, 1, 125, 5120)   # items of five super-steps across the class streams: the odd and even counts
    assert set().union(*m["supersteps"].values()) >= {0, 1, 2, 4, 5}
    m = S.plan_model("A", elem, 0, 125, 5120)
    assert m["tiles_by_mode"]["pair"] == 1 and 5 in m["supersteps"]["pair"] and m["supersteps"]["pair"] & {1, 2, 3, 4}
    assert S.plan_model("A", elem, 0, 125, 32768)["supersteps"]["pair"] == {16}
    for chunk1, want in ((1024, {0, 1}), (5120, {3}), (32768, {3})):
        m = S.plan_model("B", elem, 1, 125, chunk1)
        assert m["tiles_by_mode"]["singles"] == 1 and m["supersteps"]["E1"] == want
    m = S.plan_model("B", elem, 0, 125, 1024)
    assert m["tiles_by_mode"]["edge"] == 1 and m["supersteps"]["edge"] == {0} and m["groups"]["edge"] > 0
    # GMX_PR_COLD_PAIR_X100 moves the tile across the pair / edge border
    assert S.plan_model("B", elem, 1, 100)["tiles_by_mode"]["classed"] == 1 and S.plan_model("B", elem, 0, 100)["tiles_by_mode"]["pair"] == 1
    assert S.plan_model("A", elem, 1, 400)["tiles_by_mode"]["singles"] == 1 and S.plan_model("A", elem, 0, 400)["tiles_by_mode"]["edge"] == 1


@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("primed", ["", "'"])
def test_designed_finishes(elem, primed):
    name = "A" + primed
    m = S.plan_model(name, elem, 1, 125, None, S.FINISH["sole"][elem])
    assert m["items2_chunk"] == 0 and m["items2_sole"] == len(m["bin_groups"]) and m["fused"] == (primed == "")
    m = S.plan_model(name, elem, 1, 125, None, S.FINISH["few"][elem])
    assert m["bins_few"] > 0 and m["bins_many"] == 0
    ch = S.FINISH["few"][elem]
    slots = -(-m["bin_groups"] // ch)
    assert set(slots[m["bin_groups"] > 3 * ch].tolist()) <= set(range(4, 9))
    m = S.plan_model(name, elem, 1, 125, None, S.FINISH["many"][elem])
    assert m["bins_many"] > 0 and m["bins_few"] == 0
    m = S.plan_model("Am" + primed, elem, 1, 400, None, S.FINISH["mixed"][elem])
    assert m["tiles_by_mode"]["singles"] == 1 and m["fused"] == (primed == "")
    assert m["bins_few"] > 0 and m["bins_many"] > 0 and m["items2_sole"] > 0
