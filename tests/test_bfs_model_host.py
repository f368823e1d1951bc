"""tests/bfs_model.py (hop_dist's level schedule in numpy) and tests/bfs_cases.py (the boundary graphs) without a device:
every boundary of FACTS is met by a named case -- derived from the model's per-level detail and the CSR, never assumed from
how a case was built -- the model's levels are a breadth-first search's, and a rank's share of the work adds up."""
import numpy as np
import pytest

import bfs_cases as bc
import bfs_model as bm
import pyoracle as po

INT_MAX = bm.INT_MAX
BU_LENGTHS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 95, 96, 97]
FACTS = (["bu: looking vertex with an in-row of %d" % n for n in BU_LENGTHS] + [
    "bu: looking vertex with an in-row of at least 161",
    "bu: hint hit",
    "bu: only-flagged vertex whose hint misses (no walk, stays a candidate)",
    "bu: hint misses, own walk finds the parent at 0", "bu: hint misses, own walk finds the parent at 3",
    "bu: hint misses, own walk finds the parent at 4", "bu: hint misses, own walk finds the parent at 31",
    "bu: a second frontier vertex behind the own walk's first hit",
    "bu: wave part finds the parent at its entry 0", "bu: wave part finds the parent at its entry 63",
    "bu: wave part finds the parent at its entry 64", "bu: wave part finds the parent at its last entry",
    "bu: wave part finds the parent in its first step with two more steps behind it",
    "bu: wave part finds the parent in its second step with a step behind it",
    "bu: own walk finds the parent with groups of four behind it, in a row the wave would go on with",
    "bu: no parent in a row of more than 96 entries",
    "bu: aligned block of 256 with more than 64 walkers", "bu: aligned block of 256 without a walker",
    "bu: V % 4 != 0 with looking vertices among the last V % 4", "bu: V % 64 != 0",
    "bu: last step of 1 words", "bu: last step of 2 words", "bu: last step of 3 words",
    "bu: a slice boundary that is no multiple of 256 vertices",
    "bu twice: aligned block of 256 without a candidate in the second level",
    "bu twice: only-flagged vertex misses in the first level and is found in the second",
    "bu twice: a candidate that is never found",
    "bu: a bottom-up run after top-down levels after a bottom-up run",
    "hubs: a looking vertex's hint is a hub slot", "hubs: a looking vertex's hint is a plain id",
    "first: row of 1 slots", "first: row of 2047 slots", "first: row of 2048 slots", "first: row of 2049 slots",
    "first: self-loop", "first: adjacent repeats", "first: every entry is the root (next frontier 0, one iteration)",
    "first: 63 slots, no bitmap", "first: 64 slots, bitmap", "first: at least 64 slots but fewer than V / 1024, no bitmap",
    "first: exactly V / 1024 slots, bitmap",
    "first+bitmap, then a bottom-up level 1 (prewritten)", "first+bitmap, then a top-down level 1 and a bottom-up level later",
    "the rows of a first+bitmap case forward-only", "unsorted root row with repeats apart: a general form at level 0",
    "sparse: one wave with rows of 0, 1, 16, 17, 80 and 81 edges", "sparse: n % 64 != 0 with n > 256",
    "sparse: a vertex reached from every lane and every workgroup, its edges the next level's frontier edges",
    "sparse: one-vertex queue with 1026 edges", "tiles: one-vertex queue with 1027 edges",
    "tiles/small-scan: queue of 16384", "tiles/scan: queue of 16385",
    "from-bitmap with V % 64 != 0, then sparse", "from-bitmap with V % 64 != 0, then tiles"])


def _blocks(v, v_lo, v_hi, weights=None):
    """per aligned block of 256 vertices of [v_lo, v_hi): how many of v[] it holds"""
    return np.bincount((v - v_lo) // 256, weights, minlength=(v_hi - v_lo + 255) // 256)


def facts_of(name):
    c = bc.case(name)
    V = len(c.begin) - 1
    deg = np.diff(c.begin)
    out = set()
    runs = [bc.model(name)]
    if name in bc.RANK_CASES:
        runs += [bc.model(name, r, n) for n in (2, 3) for r in range(n)]
    if name == bc.HUB_CASE:
        runs = [bc.model(name, hub_min_v=bc.HUB_MIN_V)]
    for run_no, r in enumerate(runs):
        lv, det = r.levels, r.detail
        for i, (l, d) in enumerate(zip(lv, det)):
            if l.direction != "bottom-up":
                continue
            if d["nw_last"]:
                out.add("bu: last step of %d words" % d["nw_last"])
            if d["v_lo"] % 256 or (d["v_hi"] % 256 and d["v_hi"] < V):
                out.add("bu: a slice boundary that is no multiple of 256 vertices")
            mine = d["mine"]
            walkers = _blocks(d["v"][mine & d["walks"]], d["v_lo"], min(d["v_hi"], V))
            if (walkers > 64).any():
                out.add("bu: aligned block of 256 with more than 64 walkers")
            if (walkers == 0).any():
                out.add("bu: aligned block of 256 without a walker")
            if run_no:
                continue   # (the facts about single vertices: from the single-rank run, which looks at all of them)
            indeg, pos, has_in = d["indeg"], d["pos"], d["indeg"] > 0
            for n in BU_LENGTHS:
                if (indeg == n).any():
                    out.add("bu: looking vertex with an in-row of %d" % n)
            if (indeg >= 161).any():
                out.add("bu: looking vertex with an in-row of at least 161")
            if d["hint_hit"].any():
                out.add("bu: hint hit")
            if (d["only"] & ~d["hint_hit"]).any():
                out.add("bu: only-flagged vertex whose hint misses (no walk, stays a candidate)")
            for p in (0, 3, 4, 31):
                if (d["own_hit"] & (pos == p)).any():
                    out.add("bu: hint misses, own walk finds the parent at %d" % p)
            for t in np.flatnonzero(d["own_hit"]):
                v = d["v"][t]
                row = c.r_node_idx[c.r_begin[v]:c.r_begin[v + 1]][:bm.BFS_BU_OWN]
                if d["frontier"][row[pos[t] + 1:]].any():
                    out.add("bu: a second frontier vertex behind the own walk's first hit")
            for e in (0, 63, 64):
                if (d["wave_hit"] & (pos - bm.BFS_BU_OWN == e)).any():
                    out.add("bu: wave part finds the parent at its entry %d" % e)
            if (d["wave_hit"] & (pos == indeg - 1)).any():
                out.add("bu: wave part finds the parent at its last entry")
            step, steps = (pos - bm.BFS_BU_OWN) // 64, (indeg - bm.BFS_BU_OWN + 63) // 64
            if (d["wave_hit"] & (step == 0) & (steps >= 3)).any():
                out.add("bu: wave part finds the parent in its first step with two more steps behind it")
            if (d["wave_hit"] & (step == 1) & (steps >= 3)).any():
                out.add("bu: wave part finds the parent in its second step with a step behind it")
            if (d["own_hit"] & (pos // 4 < (bm.BFS_BU_OWN - 1) // 4) & (indeg > bm.BFS_BU_OWN)).any():
                out.add("bu: own walk finds the parent with groups of four behind it, in a row the wave would go on with")
            if (d["walks"] & (pos < 0) & (indeg > 96)).any():
                out.add("bu: no parent in a row of more than 96 entries")
            if V % 4 and (has_in & (d["v"] >= V - V % 4)).any():
                out.add("bu: V % 4 != 0 with looking vertices among the last V % 4")
            if V % 64:
                out.add("bu: V % 64 != 0")
            if d["cand"]:
                prev = det[i - 1]
                assert lv[i - 1].direction == "bottom-up"
                if (_blocks(d["v"][has_in], 0, V) == 0).any():
                    out.add("bu twice: aligned block of 256 without a candidate in the second level")
                missed = prev["v"][prev["only"] & ~prev["hint_hit"]]
                if np.isin(missed, d["v"][d["found"]]).any():
                    out.add("bu twice: only-flagged vertex misses in the first level and is found in the second")
                if (r.dist[d["v"][has_in]] == INT_MAX).any():
                    out.add("bu twice: a candidate that is never found")
            elif any(a.direction == "bottom-up" for a in lv[:i]):
                assert lv[i - 1].direction == "top-down"
                out.add("bu: a bottom-up run after top-down levels after a bottom-up run")
            if name == bc.HUB_CASE:
                assert l.encoding == "hubs-lds"
                thr = bm.hub_threshold(c.begin)
                hd = deg[d["hint"][has_in]]
                if (hd > thr).any():
                    out.add("hubs: a looking vertex's hint is a hub slot")
                if (hd < thr).any():
                    out.add("hubs: a looking vertex's hint is a plain id")
    r = runs[0]
    lv, det = r.levels, r.detail
    l0, d0 = lv[0], det[0]
    forms = [l.form for l in lv]
    if l0.form.startswith("first"):
        if d0["slots"] in (1, 2047, 2048, 2049):
            out.add("first: row of %d slots" % d0["slots"])
        if d0["self_loop"]:
            out.add("first: self-loop")
        if d0["repeats"]:
            out.add("first: adjacent repeats")
        if l0.next_frontier == 0 and l0.frontier_edges > 0 and r.stats["iterations"] == 1:
            out.add("first: every entry is the root (next frontier 0, one iteration)")
        if c.reverse:
            m_f, bitmap = l0.frontier_edges, l0.form == "first+bitmap"
            assert bitmap == (m_f >= 64 and m_f >= V // 1024)
            if m_f == 63 and not bitmap:
                out.add("first: 63 slots, no bitmap")
            if m_f == 64 and bitmap:
                out.add("first: 64 slots, bitmap")
            if 64 <= m_f < V // 1024:
                out.add("first: at least 64 slots but fewer than V / 1024, no bitmap")
            if m_f == V // 1024 and bitmap:
                out.add("first: exactly V / 1024 slots, bitmap")
        if l0.form == "first+bitmap" and len(lv) > 1:
            if forms[1] == "bottom-up/dist prewritten":
                out.add("first+bitmap, then a bottom-up level 1 (prewritten)")
            if lv[1].direction == "top-down" and "bottom-up/dist from-queue" in forms[2:]:
                out.add("first+bitmap, then a top-down level 1 and a bottom-up level later")
        if not c.reverse:
            for other in bc.CASES:
                o = bc.case(other)
                if o.reverse and np.array_equal(o.begin, c.begin) and np.array_equal(o.node_idx, c.node_idx) and \
                        bc.model(other).levels[0].form == "first+bitmap":
                    out.add("the rows of a first+bitmap case forward-only")
    row = c.node_idx[c.begin[c.root]:c.begin[c.root + 1]]
    if not c.rows_sorted and not l0.form.startswith("first") and len(np.unique(row)) < len(row) and \
            (np.sort(row)[1:] == np.sort(row)[:-1]).sum() > (row[1:] == row[:-1]).sum():
        out.add("unsorted root row with repeats apart: a general form at level 0")
    for i, (l, d) in enumerate(zip(lv, det)):
        if l.form.startswith("sparse"):
            if l.frontier <= 64 and {0, 1, 16, 17, 80, 81} <= set(d["row_len"].tolist()):
                assert bm.BFS_SPARSE_OWN == 16
                out.add("sparse: one wave with rows of 0, 1, 16, 17, 80 and 81 edges")
            if l.frontier % 64 and l.frontier > 256:
                out.add("sparse: n % 64 != 0 with n > 256")
                # reached from EVERY queue entry: from two lanes of a wave and from two workgroups whatever the queue's order
                new = np.flatnonzero(r.dist == l.level + 1)
                every = new[np.bincount(d["nbr"], minlength=V)[new] == l.frontier]
                if len(every) and lv[i + 1].frontier_edges == int(deg[new].sum()) > 0:
                    out.add("sparse: a vertex reached from every lane and every workgroup, its edges the next level's frontier edges")
            if l.frontier == 1 and l.frontier_edges == 1026:
                out.add("sparse: one-vertex queue with 1026 edges")
        if l.form.startswith("tiles") and l.frontier == 1 and l.frontier_edges == 1027:
            out.add("tiles: one-vertex queue with 1027 edges")
        if l.form == "tiles/small-scan" and l.frontier == 16384:
            out.add("tiles/small-scan: queue of 16384")
        if l.form == "tiles/scan" and l.frontier == 16385:
            out.add("tiles/scan: queue of 16385")
        if l.form.endswith("from-bitmap") and V % 64 and l.frontier <= V // bm.BOTTOMUP_STAYS_V:
            out.add("from-bitmap with V % 64 != 0, then " + l.form.split("/")[0].split(" ")[0])
    return out


def test_cases_meet_every_boundary():
    met = {}
    for name in bc.CASES:
        for f in facts_of(name):
            assert f in FACTS, f
            met.setdefault(f, []).append(name)
    for f in FACTS:
        print("%-90s %s" % (f, ", ".join(met.get(f, []))))
    assert not [f for f in FACTS if f not in met]


def test_every_form_is_taken():
    seen = {l.form.split(" ")[0] for name in bc.CASES for l in bc.model(name).levels}
    assert seen == set(bm.FORMS)
    origins = {l.form.split(" ")[1] for name in bc.CASES for l in bc.model(name).levels if " " in l.form}
    assert origins == set(bm.ORIGINS) | {"from-bitmap"}


def test_model_names_every_form_of_the_library():
    """the forms gmx_bfs_step_begin can put on the debug line are the model's: one the model does not know fails here"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "green-marl_amd", "csrc", "gmx_bfs.hip")).read()
    body = src[src.index('extern "C" int gmx_bfs_step_begin'):src.index('extern "C" int gmx_bfs_found_bitmap')]
    forms = set()
    for rhs in re.findall(r"b->form = ([^;]+);", body):
        forms |= set(re.findall(r'"([^"]+)"', rhs))
    assert forms == set(bm.FORMS)
    origins = set()
    for rhs in re.findall(r"b->origin = ([^;]+);", body):
        origins |= {s.strip() for s in re.findall(r'"([^"]+)"', rhs)}
    assert origins == set(bm.ORIGINS) | {"from-bitmap"}


def _og(c):
    return po.Graph(len(c.begin) - 1, c.begin, c.node_idx)


@pytest.mark.parametrize("name", bc.CASES)
def test_model_levels_are_bfs_levels(name):
    c = bc.case(name)
    want = po.bfs_queue(_og(c), c.root)
    r = bc.model(name)
    assert np.array_equal(r.dist, want)
    assert r.stats["vertices_reached"] == int((want != INT_MAX).sum())
    assert r.stats["iterations"] == int(want[want != INT_MAX].max()) + 1
    assert bm.rows_ascending(c.begin, c.node_idx) == c.rows_sorted
    if c.reverse:
        assert bm.rows_ascending(c.r_begin, c.r_node_idx)


@pytest.mark.parametrize("scale,permute", [(12, False), (12, True), (14, False), (14, True)])
def test_model_on_rmat(scale, permute):
    og = po.rmat_graph(scale, permute=permute)
    rng = np.random.default_rng(scale)
    for root in [0, int(np.argmax(np.diff(og.begin))), og.N - 1] + rng.integers(0, og.N, 2).tolist():
        want = po.bfs_queue(og, root)
        one = bm.run(og.begin, og.node_idx, og.r_begin, og.r_node_idx, bm.rows_ascending(og.begin, og.node_idx), root)
        assert np.array_equal(one.dist, want), (scale, permute, root)
        fwd = bm.run(og.begin, og.node_idx, None, None, bm.rows_ascending(og.begin, og.node_idx), root)
        assert np.array_equal(fwd.dist, want)
        assert fwd.stats["edges_examined"] == fwd.stats["edges_reached"]   # top-down only: every reached row once
        _check_rank_sums(lambda rank, nranks: bm.run(og.begin, og.node_idx, og.r_begin, og.r_node_idx, True, root, rank, nranks), one)


def test_model_on_golden(golden):
    man = golden["manifest"]
    n = 0
    for name, c in golden["cases"].items():
        if "dist" not in c or "r_begin" not in c:
            continue
        m = man["hand"][name[5:]] if name.startswith("hand_") else man["rmat"][name]
        r = bm.run(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"], bm.rows_ascending(c["begin"], c["node_idx"]), m["root"])
        assert np.array_equal(r.dist, c["dist"]), name
        n += 1
    assert n >= 3


def _check_rank_sums(run, one):
    """edges_examined of one rank == the top-down levels + the sum of the ranks' shares of the bottom-up levels"""
    td = sum(l.inspected for l in one.levels if l.direction == "top-down")
    for nranks in (2, 3):
        parts = [run(r, nranks) for r in range(nranks)]
        for p in parts:
            assert np.array_equal(p.dist, one.dist)
            assert [l[:5] + l[6:7] for l in p.levels] == [l[:5] + l[6:7] for l in one.levels]   # all but `inspected`
            assert sum(l.inspected for l in p.levels if l.direction == "top-down") == td
        bu = sum(l.inspected for p in parts for l in p.levels if l.direction == "bottom-up")
        assert td + bu == one.stats["edges_examined"], nranks


@pytest.mark.parametrize("name", [n for n in bc.CASES if bc.case(n).reverse and n != bc.HUB_CASE])
def test_rank_shares_add_up(name):
    _check_rank_sums(lambda rank, nranks: bc.model(name, rank, nranks), bc.model(name))


def test_plain_hints_walk_the_one_entry_rows():
    """GMX_BFS_PLAIN_HINTS has no only-flag: a vertex with one in-edge whose hint misses walks its row of one entry.  Everything
    else about a level is the same under both codings."""
    for name in bc.BOTTOM_UP_CASES:
        coded, plain = bc.model(name), bc.model(name, plain=True)
        assert np.array_equal(coded.dist, plain.dist)
        for a, b, d in zip(coded.levels, plain.levels, coded.detail):
            assert a[:5] + a[6:7] == b[:5] + b[6:7]
            extra = int((d["only"] & ~d["hint_hit"])[d["mine"]].sum()) if a.direction == "bottom-up" else 0
            assert b.inspected == a.inspected + extra
            assert b.encoding == ("plain" if a.direction == "bottom-up" else None)
