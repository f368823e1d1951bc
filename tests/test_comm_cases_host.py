"""tests/comm_cases.py without a device: the work model is communities_ref with the work list's bookkeeping added (labels,
rounds and converged equal on every case and named graph, with and without the list), pairs' closed form is what both give,
and every path of FACTS is met by a named case -- derived from the constants parsed out of gmx_comm.hip, the model's rounds
and the order-free table bounds, never assumed from how a case was built."""
import numpy as np
import pytest

import comm_cases as cc
from test_communities_host import communities_ref, fmix32, is_fixpoint, named_graph, ref_of
from test_upload_forms_host import unsorted_multigraph

FACTS = [
    "split: all labels in one class; it fills by count at levels 3, 4 and 5 and fits at 6 (512 slots)",
    "split: the same at the default table (4096 slots)",
    "split: every label once, the winner is the smallest label",
    "split: the winner is in the part counted last at the deepest level and is not the smallest label",
    "split: the winner is in a middle part at the deepest level and is not the smallest label",
    "split: 70 labels on one start slot fill by the probe limit at level 0, in the hub kernel and in the overflow kernel",
    "split: the probe-limit class fits at level 1",
    "classes: 1024 classes over a grid of 600, the winner's class beyond the grid",
    "classes: without the classes beyond the grid the answer changes",
    "overflows: more than COMM_THREADS rows must overflow in either half-round of round 0",
    "overflows: overflowed rows at positions beyond the grid",
    "wave: more rows in a half-round than one pass takes, tables filling",
    "wave: more rows in a half-round than one pass takes, no table can fill by count",
    "short: a wave stages more than COMM_STAGE - 64 changes in either half-round",
    "wave: a wave stages more than COMM_STAGE - 64 changes in either half-round",
    "block: more rows per workgroup than one trip in either half-round",
    "init: more bitmap words than one pass", "compact: more bitmap words than one pass",
    "commit: more pending entries than one pass",
    "commit: a changed vertex with in-degree 16", "commit: a changed vertex with in-degree 17",
    "commit: a changed vertex with in-degree COMM_REV_BLOCK", "commit: a changed vertex with in-degree COMM_REV_BLOCK + 1",
    "commit: a changed vertex with an in-row of more than two strides of the big kernel and a tail",
    "commit: changed vertices of all three regimes within one stretch of the compaction, leaves between them",
    "work list: a later round evaluates some rows but not all",
    "work list: the rounds' evaluations differ from re-evaluating everything",
    "cut: max_rounds 0 decides converged = 0 through the table-full path",
    "cut: max_rounds 1 ends with nothing dirty",
    "cut: max_rounds 1 ends unconverged with rows that must overflow still dirty",
]


def round0_labels(name):
    b, i = cc.case(name)
    return np.asarray(i[b[0]:b[1]], np.int64)        # vertex 0's row; labels are ids in round 0


def winner(labels):
    lab, cnt = np.unique(labels, return_counts=True)
    return int(lab[cnt == cnt.max()][0])


def facts_of(name):
    out = set()
    b, i = cc.case(name)
    V = len(b) - 1
    deg = np.diff(b)
    if name in cc.SPLIT_COUNT_CASES:
        cap = 4096 if name.endswith("4096") else 512
        env = cc.RUNS[name][0]
        assert int(env.get("GMX_COMM_LDS_SLOTS", cc.COMM_LDS_SLOTS)) == cap
        row = round0_labels(name)
        assert int((deg > 0).sum()) == 1 and deg[0] >= cc.COMM_BLOCK_MIN and not deg[row].any()
        assert len(np.unique(row)) > cc.table_for(len(row), cap)                 # the hub table fills
        lp0 = cc.lp0_of(len(row), cap)
        classes = np.unique(fmix32(row).astype(np.int64) & ((1 << lp0) - 1))
        lv = cc.class_levels(row, lp0, cc.SPLIT_CLASS, cap)
        fates = [(lp, parts[-1][2]) for lp, parts in lv]
        if lp0 == 3 and classes.tolist() == [cc.SPLIT_CLASS] and fates == [(3, "fills"), (4, "fills"), (5, "fills"), (6, "fits")] \
                and all(n > cap for lp, parts in lv[:3] for _, n, f in parts if f == "fills"):
            out.add('split: all labels in one class; it fills by count at levels 3, 4 and 5 and fits at 6 (512 slots)' if cap == 512 else
                    'split: the same at the default table (4096 slots)')
        lp, parts = lv[-1]
        assert len(parts) == 8 and all(f == "fits" for _, _, f in parts)
        w = winner(row)
        part_of_w = int(fmix32([w])[0]) & ((1 << lp) - 1)
        if w == row.min() and len(np.unique(row)) == len(row):
            out.add("split: every label once, the winner is the smallest label")
        if w != row.min() and part_of_w == parts[-1][0]:
            out.add("split: the winner is in the part counted last at the deepest level and is not the smallest label")
        if w != row.min() and part_of_w not in (parts[0][0], parts[-1][0]):
            out.add("split: the winner is in a middle part at the deepest level and is not the smallest label")
        m = cc.model(name, env)
        assert m.comm[0] == w and m.rounds == 1 and m.rounds_log[0].ovf_lo == 1
    if name == "split_probe":
        row = round0_labels(name)
        cap = cc.COMM_LDS_SLOTS_MIN
        assert int((deg > 0).sum()) == 1 and len(row) == cc.COMM_BLOCK_MIN and not deg[row].any()
        lab = np.unique(row)
        starts = fmix32(lab).astype(np.int64) & (cc.table_for(len(row), cap) - 1)
        if len(lab) <= cap and len(np.unique(starts)) == 1 and len(lab) > cc.COMM_PROBES and cc.lp0_of(len(row), cap) == 0 \
                and cc.table_fate(lab, 0, cap) == "fills":
            out.add("split: 70 labels on one start slot fill by the probe limit at level 0, in the hub kernel and in the overflow kernel")
        lv = cc.class_levels(lab, 0, 0, cap)
        if [lp for lp, _ in lv] == [0, 1] and all(f == "fits" for _, _, f in lv[1][1]) and sum(n for _, n, _ in lv[1][1]) == len(lab):
            out.add("split: the probe-limit class fits at level 1")
        m = cc.model(name, cc.SMALL)
        assert m.comm[0] == winner(row) != lab.min()
        # the count alone would let it pass: the lower bound of the per-round check is 0 here, the upper 1
        assert (m.rounds_log[0].ovf_lo, m.rounds_log[0].ovf_hi) == (0, 1)
    if name == "many_classes":
        row = round0_labels(name)
        cap = cc.COMM_LDS_SLOTS_MIN
        grid = cc.block_grid(V)
        lp0 = cc.lp0_of(len(row), cap)
        assert set(row.tolist()) == set(range(1, V)) and not deg[1:].any()
        assert len(np.unique(row)) > cc.table_for(len(row), cap)
        w = winner(row)
        cls = fmix32(row).astype(np.int64) & ((1 << lp0) - 1)
        w_cls = int(fmix32([w])[0]) & ((1 << lp0) - 1)
        if (1 << lp0) == 1024 and grid == 600 and w_cls >= grid:
            out.add("classes: 1024 classes over a grid of 600, the winner's class beyond the grid")
        if winner(row[cls < grid]) != w:
            out.add("classes: without the classes beyond the grid the answer changes")
        # no class fills again: at most a handful of labels each
        assert max(len(np.unique(row[cls == c])) for c in np.unique(cls)) <= cc.COMM_PROBES
        assert cc.model(name, cc.SMALL).comm[0] == w
    if name == "many_overflows":
        small, default = cc.RUNS[name]
        m = cc.model(name, small)
        r0 = m.rounds_log[0]
        n_rows = int((deg > 0).sum())
        a, c = m.half_rows[:2]
        assert a + c == n_rows == r0.wave and r0.short == r0.block == 0
        if r0.ovf_lo == n_rows and min(a, c) > cc.COMM_THREADS:
            out.add("overflows: more than COMM_THREADS rows must overflow in either half-round of round 0")
        if r0.ovf_lo == n_rows and min(a, c) > cc.block_grid(V):
            out.add("overflows: overflowed rows at positions beyond the grid")
        if r0.ovf_lo == n_rows and min(a, c) > cc.WAVE_ROWS_PER_PASS:
            out.add("wave: more rows in a half-round than one pass takes, tables filling")
        d = cc.model(name, default)
        if d.rounds_log[0].wave == n_rows and min(d.half_rows[:2]) > cc.WAVE_ROWS_PER_PASS and d.rounds_log[0].ovf_lo == 0:
            out.add("wave: more rows in a half-round than one pass takes, no table can fill by count")
    if name == "pairs23":
        a, c = cc.pairs_half_rows(V)
        assert a + c == V // 2
        envs = cc.RUNS[name]
        assert envs == [{}, cc.ALL_WAVE, cc.ALL_BLOCK]
        # every selected row changes; a wave of the short kernel takes four rows per trip over the list in order, so it stages
        # (rows / rows per pass) * 4 changes at least
        if min(a, c) // cc.SHORT_ROWS_PER_PASS * 4 > cc.STAGE_FLUSH_AT:
            out.add("short: a wave stages more than COMM_STAGE - 64 changes in either half-round")
        if min(a, c) // cc.WAVE_ROWS_PER_PASS > cc.STAGE_FLUSH_AT:
            out.add("wave: a wave stages more than COMM_STAGE - 64 changes in either half-round")
        if min(a, c) > cc.GRID["block"]:
            out.add("block: more rows per workgroup than one trip in either half-round")
        nwords = (V + 63) // 64
        if nwords > cc.GRID["word"] * cc.WAVES:
            out.add("init: more bitmap words than one pass")
        if nwords > cc.GRID["compact"] * (cc.K["COMM_COMPACT_THREADS"] // 64):
            out.add("compact: more bitmap words than one pass")
        if min(a, c) > cc.GRID["list"] * cc.COMM_THREADS:
            out.add("commit: more pending entries than one pass")
        # one scale less is too few for the short kernel's mid-loop flush
        a2, c2 = cc.pairs_half_rows(V // 2)
        assert max(a2, c2) // cc.SHORT_ROWS_PER_PASS * 4 <= cc.STAGE_FLUSH_AT
    if name == "commit_regimes":
        m = cc.model(name)
        indeg = np.bincount(i, minlength=V)
        ch = np.concatenate(m.changed_indeg[:2])                  # round 0
        centres = np.flatnonzero(indeg >= 16)
        assert len(centres) == len(cc.COMMIT_INDEG) * cc.COMMIT_CENTRES
        assert sorted(ch[ch >= 16].tolist()) == sorted(indeg[centres].tolist())       # every centre changes in round 0
        big_stride = 4 * cc.COMM_THREADS
        for what, d in (("16", 16), ("17", 17), ("COMM_REV_BLOCK", cc.COMM_REV_BLOCK), ("COMM_REV_BLOCK + 1", cc.COMM_REV_BLOCK + 1)):
            if (ch == d).sum() == cc.COMMIT_CENTRES:
                out.add("commit: a changed vertex with in-degree " + what)
        big = ch[ch > cc.COMM_REV_BLOCK + 1]
        if len(big) and (big > 2 * big_stride + 1).all() and (big % big_stride != 0).all():
            out.add("commit: a changed vertex with an in-row of more than two strides of the big kernel and a tail")
        # the order of the pending list is the device's own, so which entries share a wave of the commit cannot be promised;
        # what can: all the centres lie in one 1024-vertex stretch of the compaction, 16 ids apart, leaves between them, so
        # their rows are neighbours in the row list and their changes reach the pending list together
        kinds = np.where(indeg <= 16, 0, np.where(indeg <= cc.COMM_REV_BLOCK, 1, 2))
        stretch = centres // cc.K["COMM_COMPACT_THREADS"]
        if len(np.unique(stretch)) == 1 and set(kinds[centres].tolist()) == {0, 1, 2} and (np.diff(np.sort(centres)) > 1).all():
            out.add("commit: changed vertices of all three regimes within one stretch of the compaction, leaves between them")
        n_rows = int((deg > 0).sum())
        ev = [r.short + r.wave + r.block for r in m.rounds_log]
        if any(0 < e < n_rows for e in ev[1:]):
            out.add("work list: a later round evaluates some rows but not all")
        if ev != [r.short + r.wave + r.block for r in cc.model(name, worklist=False).rounds_log]:
            out.add("work list: the rounds' evaluations differ from re-evaluating everything")
        # the leaves end with their centre's sink
        leaves = np.flatnonzero((deg == 1) & (indeg == 0))
        assert np.array_equal(m.comm[leaves], m.comm[i[b[leaves]]]) and m.converged == 1
        sinks = i[b[centres]]
        assert np.array_equal(m.comm[centres], sinks)
    if name in cc.CUT_CASES:
        env = cc.RUNS[name][0]
        m0, m1 = cc.model(name, env, max_rounds=0), cc.model(name, env, max_rounds=1)
        assert m0.rounds == 0 and np.array_equal(m0.comm, np.arange(V)) and m0.evals == 0
        full = cc.model(name, env)
        if m0.converged == 0 and full.rounds_log[0].ovf_lo > 0:
            out.add("cut: max_rounds 0 decides converged = 0 through the table-full path")
        assert m1.rounds == 1
        if m1.converged == 1 and full.rounds == 1:
            out.add("cut: max_rounds 1 ends with nothing dirty")
        if m1.converged == 0 and full.rounds > 1 and full.rounds_log[1].ovf_lo > 0:
            out.add("cut: max_rounds 1 ends unconverged with rows that must overflow still dirty")
    return out


def test_restated_helpers():
    """comm_table_for and the overflow kernel's first level at the lengths and tables the cases' docstrings use"""
    assert (cc.table_for(100, 64), cc.table_for(100, 512), cc.table_for(256, 512), cc.table_for(1, 512)) == (64, 512, 512, 64)
    assert (cc.lp0_of(2048, 512), cc.lp0_of(2049, 512), cc.lp0_of(16385, 4096), cc.lp0_of(256, 512), cc.lp0_of(1 << 18, 512)) == (3, 3, 3, 0, 10)


def test_clusters_are_order_free():
    """the occupied set of a linear-probing table against brute-force insertion in several orders"""
    rng = np.random.default_rng(3)
    for cap, n in ((16, 5), (16, 16), (64, 40), (64, 63), (128, 100)):
        for _ in range(5):
            starts = rng.integers(0, cap, n) if _ else np.full(n, cap - 2)      # (one case wraps around the end)
            want = None
            for order in range(3):
                occ = np.zeros(cap, bool)
                for s in rng.permutation(starts):
                    while occ[s]:
                        s = (s + 1) % cap
                    occ[s] = True
                runs = sorted(len(r) for r in "".join("x" if o else " " for o in np.roll(occ, -int(np.argmin(occ)))).split()) \
                    if not occ.all() else [cap]
                assert want is None or runs == want
                want = runs
            assert sorted(cc.clusters(starts, cap)) == want


def test_cases_meet_every_path():
    met = {}
    for name in cc.CASES:
        for f in facts_of(name):
            assert f in FACTS, f
            met.setdefault(f, []).append(name)
    for f in FACTS:
        print("%-110s %s" % (f, ", ".join(met.get(f, []))))
    assert not [f for f in FACTS if f not in met]


def _same_as_ref(name, b, i, max_rounds=1000):
    want, rounds, conv = ref_of(name, b, i, max_rounds)
    n_rows = int((np.diff(b) > 0).sum())
    with_list = cc.model_of(name, b, i, max_rounds=max_rounds)
    without = cc.model_of(name, b, i, worklist=False, max_rounds=max_rounds)
    for m in (with_list, without):
        assert np.array_equal(m.comm, want) and (m.rounds, m.converged) == (rounds, conv), name
        assert m.evals == sum(r.short + r.wave + r.block for r in m.rounds_log) and m.slots == sum(r.slots for r in m.rounds_log)
        assert [r.changes > 0 for r in m.rounds_log] == [True] * rounds + [False] * (len(m.rounds_log) - rounds)
    assert all(r.short + r.wave + r.block == n_rows and r.slots == len(i) for r in without.rounds_log)
    assert all(a.short + a.wave + a.block <= n_rows for a in with_list.rounds_log)
    assert [r.changes for r in with_list.rounds_log] == [r.changes for r in without.rounds_log]
    return with_list, without


@pytest.mark.parametrize("name", cc.MODEL_CASES)
def test_model_is_the_restatement_on_cases(name):
    _same_as_ref("case/" + name, *cc.case(name))


@pytest.mark.parametrize("name", ["rmat10", "rmat10p", "rmat12", "rmat12p", "rmat14", "rmat14p", "rmat12s", "planted16", "planted64",
                                  "uniform", "star33", "path4096"])
def test_model_is_the_restatement_on_named_graphs(name):
    with_list, without = _same_as_ref(name, *named_graph(name))
    if name.startswith("rmat1") or name == "uniform":
        assert with_list.evals < without.evals and with_list.slots < without.slots


def test_model_is_the_restatement_on_multigraphs_and_cut_runs():
    rng = np.random.default_rng(1)
    from test_communities_host import csr
    b, i = csr(3000, rng.integers(0, 3000, 30000), rng.integers(0, 3000, 30000))
    with_list, without = _same_as_ref("random3000", b, i)
    ev = [r.short + r.wave + r.block for r in with_list.rounds_log]
    assert ev[0] == int((np.diff(b) > 0).sum()) and ev[-1] < ev[0]
    V, b, i, rb, ri = (2048,) + tuple(np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(2048, 5000, 2048))
    _same_as_ref("multi", b, i)
    b, i = named_graph("chain4096")
    for mr in (0, 1, 16):
        _same_as_ref("chain4096", b, i, mr)
    for name in cc.CUT_CASES:
        for mr in (0, 1):
            m = cc.model(name, cc.RUNS[name][0], max_rounds=mr)
            want, rounds, conv = communities_ref(*cc.case(name), mr)
            assert np.array_equal(m.comm, want) and (m.rounds, m.converged) == (rounds, conv)


def test_pairs_closed_form():
    b, i = cc.pairs(4096)
    want, rounds, conv = communities_ref(b, i)
    comm, r, c = cc.pairs_closed_form(4096)
    assert np.array_equal(comm, want) and (r, c) == (rounds, conv) and is_fixpoint(b, i, comm)
    for env in cc.RUNS["pairs23"]:
        with_list = cc.model_of("pairs4096", b, i, env)
        without = cc.model_of("pairs4096", b, i, env, worklist=False)
        assert np.array_equal(with_list.comm, want) and np.array_equal(without.comm, want)
        # what the device test asserts of pairs23: every row once; without the list, once more in the round that changes nothing
        assert (with_list.evals, with_list.slots) == (2048, 2048) and (without.evals, without.slots) == (4096, 4096)
        assert tuple(with_list.half_rows[:2]) == cc.pairs_half_rows(4096)
    assert sum(cc.pairs_half_rows(cc.PAIRS_V)) == cc.PAIRS_V // 2
