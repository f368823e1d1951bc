"""The inputs of test_gpu_tc_paths.py, checked on the host: the two oracles and the closed forms agree on every graph,
and the restated path selection of tc_oriented_kernel (tc_paths_common.census) says that the inputs reach every
(branch, lds/mem) pair of the kernel under the knob sets the device tests run -- coverage is asserted, not assumed."""
import pytest

import pyoracle as po
import tc_paths_common as tp

_CACHE = {}


def graph(name):
    if name not in _CACHE:
        build, _ = {**tp.GRAPHS, **tp.TINY}[name]
        _CACHE[name] = build()
    return _CACHE[name]


def count(name, knobs):
    return tp.census(*graph(name), **tp.census_args(knobs))


@pytest.mark.parametrize("name", list(tp.GRAPHS) + list(tp.TINY))
def test_oracles_and_closed_forms_agree(name):
    begin, idx = graph(name)
    og = tp.oracle_graph(begin, idx)
    merge = po.triangle_counting_merge(og)
    search = po.triangle_counting(og)          # the emitted rule restated: seconds on the large inputs, called once
    assert merge == search
    closed = {**tp.GRAPHS, **tp.TINY}[name][1]
    if closed is not None:
        assert closed() == merge
    print("%s: V %d, %d slots, T %d" % (name, len(begin) - 1, len(idx), merge))


def test_closed_form_values():
    assert tp.crown_triangles(1100) == 1100 * 3294 + 3292 == 3626692
    assert tp.pendants_triangles() == 461685520
    assert len(graph("sparse17")[0]) - 1 == 1 << 17


@pytest.mark.parametrize("name", list(tp.GRAPHS) + list(tp.TINY))
def test_builders_give_symmetric_simple_sorted_csr(name):
    import numpy as np
    begin, idx = graph(name)
    V = len(begin) - 1
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin))
    key = src * V + idx
    assert (np.diff(key) > 0).all()                            # sorted rows, no repeated neighbour
    assert (src != idx).all()
    assert np.array_equal(np.sort(idx.astype(np.int64) * V + src), key)   # symmetric


# (branch, where, graph, knobs, count measured when the inputs were designed or None)
REQUIRED = [
    ("A-walkUpU", "mem", "crown1100", "default", 140800),
    ("A-hubtail", "mem", "clique1100", "aloneBig", 5438),
    ("A-hubtail", "mem", "pendants", "aloneBig", 83072),
    ("A-tailSearch", "mem", "pendants", "hubs0+aloneBig", 512),
    ("W-hub", "mem", "clique1100", "default", 5438),
    ("W-streamTail", "mem", "clique1100", "hubs0", 5504),
    ("W-streamTail", "lds", "clique1100", "hubs0+ratio0", 593461),
    ("W-streamUpU", "lds", "clique1100", "hubs0+ratioBig", 593461),
    ("A-tailSearch", "lds", "sym_rmat12", "hubs0", None),
    ("W-streamTail", "lds", "sym_rmat12", "hubs0", None),
    ("A-walkUpU", "lds", "sym_rmat12", "hubs0", None),
    ("A-hubtail", "lds", "sym_rmat12", "default", None),
    ("W-hub", "lds", "sym_rmat12", "default", None),
    ("W-hub", "mem", "crown1100", "hubtailBig", None),
]


@pytest.mark.parametrize("branch,where,name,knobs,measured", REQUIRED)
def test_input_reaches_branch(branch, where, name, knobs, measured):
    c = count(name, knobs)
    print("%s/%s on %s under %s: %d slots" % (branch, where, name, knobs, c[(branch, where)]))
    assert c[(branch, where)] > 0
    if measured is not None:
        assert c[(branch, where)] == measured


@pytest.mark.parametrize("name", list(tp.GRAPHS) + list(tp.TINY))
def test_no_hub_branch_without_hub_tail(name):
    c = count(name, "hubtail0")
    for where in ("lds", "mem"):
        assert c[("A-hubtail", where)] == 0 and c[("W-hub", where)] == 0


def test_sparse17_has_a_real_non_hub_population():
    c = count("sparse17", "default")
    assert c["hub_base"] == 65536
    for branch in ("A-hubtail", "A-walkUpU", "A-tailSearch", "W-hub", "W-streamUpU"):
        assert c[(branch, "lds")] > 0, branch
    _, idx = graph("sparse17")
    assert 1_800_000 < len(idx) <= 2_400_000


def test_tiny_cliques_sit_on_the_hub_boundary():
    assert [count(n, "default")["hub_base"] for n in ("clique40", "clique65", "clique100")] == [40, 1, 36]
    assert tp.hub_count(40) == 0 and tp.hub_count(65) == 64 and tp.hub_count(100) == 64
    assert tp.hub_count(1 << 17) == 65536 and tp.hub_count((1 << 24) + 1) == 131072 and tp.hub_count(1100, 64) == 64


def test_matrix_covers_every_pair():
    reached = {}
    for name in tp.GRAPHS:
        for knobs in tp.KNOBS:
            c = count(name, knobs)
            for pair in tp.PAIRS:
                if c[pair] and pair not in reached:
                    reached[pair] = (name, knobs, c[pair])
    for pair in tp.PAIRS:
        print("%s/%s: %s" % (pair[0], pair[1], reached.get(pair)))
    assert len(tp.PAIRS) == 11 and set(reached) == set(tp.PAIRS)
