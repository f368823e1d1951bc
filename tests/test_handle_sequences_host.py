"""handle_sequences.py without a device: the table names every algorithm entry of gmx.Graph, its argument sets give different
results, the sequences have the shape they claim, and the runner with the rows' checkers fails where it must -- every
sequence passes on a fake device that returns the model's own result, and for every row a fake that answers with the other
argument set's result (a stale answer) or with one element changed is caught at that step."""
import itertools
import time

import numpy as np
import pytest

import handle_sequences as hs

# what a caller does to a graph besides running an algorithm on it: none of these launches one.  (route only uploads the
# weights; its queries are the route_query steps of held_state.)
HOUSEKEEPING = {"upload", "from_edges", "rmat", "symmetrize", "V", "E", "download", "free", "edge_order", "reverse_edge_map", "route"}


def test_every_entry_of_the_graph_class_is_a_row():
    import gmx
    public = {n for n, v in vars(gmx.Graph).items() if not n.startswith("_") and (callable(v) or isinstance(v, (property, classmethod, staticmethod)))}
    assert not HOUSEKEEPING & set(hs.ROWS)
    assert public == HOUSEKEEPING | set(hs.ROWS), (sorted(public - HOUSEKEEPING - set(hs.ROWS)), sorted((HOUSEKEEPING | set(hs.ROWS)) - public))
    assert set(hs.EXTRA) == {"route_query", "bfs_state", "pr_state"}
    for key, (entry, _, _) in hs.REFUSALS.items():
        assert entry in hs.ROWS and key.startswith(entry + ":")


def differs(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) != len(b) or any(differs(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return sorted(a) != sorted(b) or any(differs(a[k], b[k]) for k in a if not callable(a[k]))
    return a != b


def test_references_complete_and_argument_sets_differ():
    """Every reference of every row on every input it runs on (the time they take together is printed), and at least two
    argument sets per row whose model results differ: a result left over from the call before cannot pass for this one."""
    t0 = time.perf_counter()
    for name, r in itertools.chain(hs.ROWS.items(), hs.EXTRA.items()):
        assert len(r.args) >= 2, name
        for k, (label, _) in enumerate(r.args):
            assert hs.want_of(name, k, label) is not None or name in hs.EXTRA
        assert differs(hs.want_of(name, 0, r.args[0][0]), hs.want_of(name, 1, r.args[1][0])), name
    for e in hs.R_ENTRIES:
        for n in (0, 1):
            hs.want_of(e, hs.first_on(e, "D", n), "R")
    print("handle_sequences: every CPU reference at scale %d in %.1f s" % (hs.SCALE, time.perf_counter() - t0))
    for name in ("common_nbrs", "route_query"):   # the stale-answer test needs something to be stale
        for k in (0, 1):
            inp, a = hs.args_of(hs.Step(name, k, hs.table(name).args[k][0]))
            got = hs.table(name).fake(inp, a, hs.want_of(name, k, inp.label))
            assert len(got if name == "common_nbrs" else got[2]) > 0


def test_the_sequences_have_their_shape():
    names = list(hs.ROWS)
    assert [s.entry for s in hs.forward()] == names and {s.k for s in hs.forward()} == {0}
    assert [s.entry for s in hs.reverse()] == names[::-1] and {s.k for s in hs.reverse()} == {1}
    sh = hs.shuffled()
    n = len(names)
    assert len(sh) == 2 * n and sorted(s.entry for s in sh[:n]) == sorted(names) and [s.entry for s in sh[:n]] == [s.entry for s in sh[n:]]
    assert [s.entry for s in sh[:n]] != names and {s.k for s in sh[:n]} == {0} and {s.k for s in sh[n:]} == {1}
    for s in itertools.chain(hs.forward(), hs.reverse(), sh):
        assert hs.input_of(s.handle).label == hs.home(s.entry, s.k)
    # every group of entries that share state, every ordered pair of it, each pair as a, b, a (the trio: a, b, a, b, a)
    for group, (label, members) in hs.GROUPS.items():
        fam = hs.families(group)
        assert len(fam) == len(members) * (len(members) - 1)
        seen = set()
        for steps in fam:
            ents = [("%s/%d" % (s.entry, s.k)) if group == "pagerank" else s.entry for s in steps]
            assert ents[0] != ents[1] and ents[0::2] == [ents[0]] * len(ents[0::2]) and ents[1::2] == [ents[1]] * len(ents[1::2])
            assert len(steps) == (5 if group == "tcd_plan" else 3) and len({s.handle for s in steps}) == 1
            seen.add((ents[0], ents[1]))
        assert seen == set(itertools.permutations(members, 2))
        assert sorted(map(tuple, sum((hs.families(group, m) for m in members), []))) == sorted(map(tuple, fam))
    assert set(hs.GROUPS["traversal"][1]) >= {"hop_dist", "bfs_levels", "bc", "bc_batch", "bc_all", "scc", "closeness"}
    assert set(hs.GROUPS["counting"][1]) == {"triangle_counting", "triangle_counting_cn", "common_nbrs", "adamic_adar"}
    # the trio flips each entry's own order knob: built, reused, rebuilt for the other order, reused, rebuilt
    for steps in hs.families("tcd_plan"):
        assert hs.plan_builds(steps) == [1, 0, 1, 0, 1]
    # the PageRank group: f32 / f64 x d inside / outside (0, 1] x GMX_PR_RANKS unset / 2
    variants = {(a["dtype"], 0 < a["d"] <= 1, a.get("_env", {}).get("GMX_PR_RANKS")) for _, a in hs.PR_ARGS}
    assert variants == set(itertools.product((np.float32, np.float64), (True, False), (None, "2")))
    dr, ds = hs.two_handles()
    assert [s.handle for s in dr] == ["D", "R"] * (len(dr) // 2) and [s.handle for s in ds] == ["D", "S"] * (len(ds) // 2)
    assert hs.inputs()["R"].flags == hs.GMX_GRAPH_SORT_ROWS and hs.inputs()["R"].idx.tobytes() != hs.inputs()["D"].idx.tobytes()
    routes, bfs, pr = hs.held_state()
    assert {hs.table(s.entry).args[s.k][1]["w"] for s in routes if s.entry == "route_query"} == set(hs.ROUTE_WEIGHTS)
    assert {s.entry for s in routes} == {"route_query", "bidir_dijkstra", "sssp", "sssp_path", "sssp_path_f64"}
    assert {hs.ROWS["sssp_path"].args[s.k][1]["_env"]["GMX_SSSP_PATH_SCHEDULE"] for s in routes if s.entry == "sssp_path"} == {"round", "nearfar"}
    assert {s.entry for s in bfs} == {"bfs_state", "hop_dist", "bc", "scc"} and {s.entry for s in pr} == {"pr_state", "pagerank"}
    ref = hs.refused()
    assert [s.k for s in ref[0::3]] == list(hs.REFUSALS) and all(isinstance(s.k, int) for s in ref[1::3] + ref[2::3])
    assert all(a.entry == b.entry != c.entry and a.handle == b.handle == c.handle for a, b, c in zip(ref[0::3], ref[1::3], ref[2::3]))


def test_every_sequence_passes_on_a_device_that_is_right():
    for name, steps in hs.all_sequences().items():
        assert hs.run(steps, hs.fake_call, hs.check_step) == len(steps), name


def changed(x):
    """(x with one element of its first non-empty array changed, True), or (x, False) when it holds no array."""
    if isinstance(x, np.ndarray) and x.size:
        y = x.copy()
        i = x.size // 2
        if y.dtype == bool:
            y[i] = not y[i]
        elif y.dtype.kind == "f":
            i = next(j for j in itertools.chain(range(i, x.size), range(i)) if np.isfinite(y[j]))
            v = float(y[i])
            y[i] = v / 2 if abs(v) > 1e30 else v * 1.5 + 1
        else:
            y[i] ^= 1
        return y, True
    if isinstance(x, (tuple, list)):
        for n, item in enumerate(x):
            y, ok = changed(item)
            if ok:
                return tuple(x[:n]) + (y,) + tuple(x[n + 1:]), True
    if isinstance(x, dict) and "kernel_ms" not in x:
        for k in x:
            y, ok = changed(x[k])
            if ok:
                return dict(x, **{k: y}), True
    return x, False


def one_element_changed(result):
    y, ok = changed(result)
    if ok:
        return y
    head = result[0] if isinstance(result, tuple) else result   # no array: the count (or the float) itself
    bad = (not head) if isinstance(head, (bool, np.bool_)) else type(head)(head * 1.5 + 1)
    return (bad,) + tuple(result[1:]) if isinstance(result, tuple) else bad


def caught(seq, at, call):
    """run() fails at step `at` of seq and names the steps before it."""
    with pytest.raises(hs.SequenceFailure) as e:
        hs.run(seq, call, hs.check_step)
    return e.value.index == at and e.value.step == seq[at] and e.value.before == seq[:at] and hs.describe(seq[at]) in str(e.value)


ALL_ROWS = list(hs.ROWS) + list(hs.EXTRA)


@pytest.mark.parametrize("name", ALL_ROWS)
def test_a_stale_answer_and_a_changed_element_are_caught(name):
    """Both argument sets of the row, in the middle of a sequence: the steps around it pass, the row's step is the one named."""
    around = [s for s in hs.forward() if s.entry != name]
    for k in (0, 1):
        step, other = hs.Step(name, k, hs.table(name).args[k][0]), hs.Step(name, 1 - k, hs.table(name).args[1 - k][0])
        seq = [around[0], around[1], step, around[2]]
        assert hs.run(seq, hs.fake_call, hs.check_step) == 4
        assert caught(seq, 2, lambda s: hs.fake_call(other) if s is step else hs.fake_call(s)), (name, k, "stale")
        assert caught(seq, 2, lambda s: one_element_changed(hs.fake_call(s)) if s is step else hs.fake_call(s)), (name, k, "changed")


@pytest.mark.parametrize("key", list(hs.REFUSALS))
def test_a_call_that_was_not_refused_is_caught(key):
    entry = hs.REFUSALS[key][0]
    label = "S" if entry == "triangle_counting" else "D"
    seq = [hs.forward()[0], hs.Step(entry, key, label)]
    assert hs.run(seq, hs.fake_call, hs.check_step) == 2
    good = hs.Step(entry, hs.first_on(entry, label), label)
    assert caught(seq, 1, lambda s: hs.fake_call(good) if s is seq[1] else hs.fake_call(s))
    assert caught(seq, 1, lambda s: "gmx status -2: out of memory" if s is seq[1] else hs.fake_call(s))
