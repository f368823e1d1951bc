"""gmx_triangle_counting_directed (triangle_counting_directed.gm) on the device against the host restatement
(test_tc_directed_host.tcd_ref) and the pinned totals: every golden case and named graph, every path of the count kernel
forced over all slots (and shown to be the one that ran, from the library's GMX_TCD_LOG line), every upload form of an
unsorted multigraph, the 3x identity against gmx_triangle_counting, parts, the plan cache, errors, empties and the driver.

rmat10's longest row has 998 slots (everything is staged in LDS at the default capacity of 1024), rmat12's 2376 (work items
searched in memory occur naturally), rmat14's 5666 (the hub case)."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_tc_directed_host import PINNED, tcd_graph, tcd_ref, tcd_ref_of
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
KNOBS = ("GMX_TCD_NO_ORDER", "GMX_TCD_CAP", "GMX_TCD_ALONE", "GMX_TCD_RATIO", "GMX_TCD_LOG")
CAP = 1024
FORCED = {
    "no_order": {"GMX_TCD_NO_ORDER": "1"},
    "cap64": {"GMX_TCD_CAP": "64"},            # nearly every row is searched in memory
    "no_lane_alone": {"GMX_TCD_ALONE": "0"},   # every slot is a wave's
    "all_alone": {"GMX_TCD_ALONE": "1000000"},  # every slot is a lane's
    "tail_only": {"GMX_TCD_RATIO": "0"},       # the waves only stream the tail
    "list_only": {"GMX_TCD_RATIO": "1000000"},  # the waves only stream the upper list
}
LINE = re.compile(r"gmx triangle_counting_directed: plan V (\d+) out (\d+) up (\d+) order (degree|identity) built (\d) build_ms ([0-9.]+); "
                  r"part (\d+)/(\d+) cap (\d+) alone (\d+) ratio (\d+); items (\d+) staged \+ (\d+) memory; "
                  r"slots (\d+) alone \+ (\d+) list \+ (\d+) tail \+ (\d+) empty")
FIELDS = ("V", "out", "up", "order", "built", "build_ms", "part", "nparts", "cap", "alone_max", "ratio", "staged", "memory", "alone", "list",
          "tail", "empty")


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


def logged(gmx, g, capfd, part=0, nparts=1, **env):
    """(T, stats, the fields of the library's line) of one call."""
    capfd.readouterr()
    with knobs(GMX_TCD_LOG="1", **env):
        T, st = g.triangle_counting_directed(part, nparts)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    f = {k: (v if k == "order" else float(v) if k == "build_ms" else int(v)) for k, v in zip(FIELDS, lines[0])}
    return T, st, f


def work_items(begin, cap):
    """What the kernel's work items are, whatever the numbering: a row of d >= 2 slots has d - 1 slots with something above
    them, in ceil((d - 1) / 64) groups; group k is staged when the row from its first slot on, d - 64 k entries, fits cap."""
    d = np.diff(np.asarray(begin, np.int64))
    d = d[d >= 2]
    groups = (d - 1 + 63) // 64
    first_staged = np.maximum(0, -((cap - d) // 64))         # smallest k with d - 64 k <= cap
    staged = int(np.maximum(0, groups - first_staged).sum())
    return int((d - 1).sum()), int(groups.sum()), staged


def check_stats(st):
    assert st["iterations"] == 1 and st["kernel_ms"] > 0
    assert all(st[k] == 0 for k in ("last_diff", "h2d_ms", "d2h_ms", "edges_examined", "vertices_reached", "edges_reached"))


def test_golden_cases(gmx, golden):
    for name, c in sorted(golden["cases"].items()):
        g = gmx.Graph.upload(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
        with knobs():
            T, _ = g.triangle_counting_directed()
        assert T == tcd_ref(c["begin"], c["node_idx"]), name


@pytest.mark.parametrize("name", sorted(PINNED))
def test_named_graphs(gmx, name):
    b, i = tcd_graph(name)
    g = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE)
    with knobs():
        T, st = g.triangle_counting_directed()
    print("triangle_counting_directed %s: %d, kernel %.3f ms" % (name, T, st["kernel_ms"]))
    assert T == PINNED[name]
    check_stats(st)


@pytest.mark.parametrize("forced", sorted(FORCED))
@pytest.mark.parametrize("name", ["rmat10", "rmat12s", "planted16", "multi300"])
def test_forced_paths(gmx, capfd, name, forced):
    """Every forced setting gives the default's and the reference's count, and moved the slots into the class it names."""
    b, i = tcd_graph(name)
    want = tcd_ref_of(name)
    slots, items, staged = work_items(b, CAP)
    g = gmx.Graph.upload(b, i, flags=gmx.GMX_GRAPH_NO_REVERSE)
    T0, _, d = logged(gmx, g, capfd)
    T1, st, f = logged(gmx, g, capfd, **FORCED[forced])
    print(name, "default", d)
    print(name, forced, f)
    assert T0 == want and T1 == want
    check_stats(st)
    for x in (d, f):
        assert (x["V"], x["out"]) == (len(b) - 1, len(i)) and 2 * x["up"] <= 2 * len(i)
        assert x["staged"] + x["memory"] == items
        assert x["alone"] + x["list"] + x["tail"] + x["empty"] == slots
    assert d["order"] == "degree" and d["built"] == 1 and (d["staged"], d["cap"], d["alone_max"], d["ratio"]) == (staged, CAP, 4, 4)
    busy = d["alone"] + d["list"] + d["tail"]              # slots with two non-empty sides: the same whatever the knobs
    assert busy > 0
    if forced == "no_order":
        assert f["order"] == "identity" and f["built"] == 1 and f["up"] == d["up"]
    else:
        assert f["order"] == "degree" and f["built"] == 0 and f["empty"] == d["empty"]
    if forced == "cap64":
        assert f["cap"] == 64 and f["staged"] == work_items(b, 64)[2]
        assert f["memory"] > 0 or name == "planted16"      # (whose rows all have fewer than 64 slots)
    if forced == "no_lane_alone":
        assert f["alone"] == 0 and f["list"] + f["tail"] == busy
    if forced == "all_alone":
        assert f["alone"] == busy and f["list"] == f["tail"] == 0
    if forced == "tail_only":
        assert f["list"] == 0 and f["alone"] == d["alone"] and f["tail"] == d["list"] + d["tail"] > 0
    if forced == "list_only":
        assert f["tail"] == 0 and f["alone"] == d["alone"] and f["list"] == d["list"] + d["tail"] > 0


def test_default_rmat12_has_staged_and_in_memory_items(gmx, capfd):
    b, i = tcd_graph("rmat12")
    slots, items, staged = work_items(b, CAP)
    assert 0 < staged < items
    g = gmx.Graph.upload(b, i)
    T, _, f = logged(gmx, g, capfd)
    assert T == PINNED["rmat12"]
    assert (f["staged"], f["memory"]) == (staged, items - staged)
    assert min(f["alone"], f["list"], f["tail"]) > 0        # the default thresholds use all three ways to intersect


def test_upload_forms_give_one_number(gmx):
    V = 300
    b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 2000, 3))
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"given reverse, sorted on upload": (True, S), "given reverse, verbatim": (True, 0), "no reverse, verbatim": (False, N),
             "device-built reverse": (False, 0), "no reverse, sorted on upload": (False, S | N)}
    for regime in ({}, FORCED["cap64"], FORCED["no_order"]):
        for form, (rev, flags) in forms.items():
            g = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
            with knobs(**regime):
                T, _ = g.triangle_counting_directed()                      # (a GMX_ERR_STATE would raise)
            assert T == PINNED["multi300"], (regime, form)


def test_three_times_the_undirected_count(gmx):
    g = gmx.Graph.rmat(1 << 12, 16 << 12).symmetrize()
    with knobs():
        Td, _ = g.triangle_counting_directed()
    Tu, _ = g.triangle_counting()
    assert Td == 3 * Tu == PINNED["rmat12s"]


@pytest.mark.parametrize("nparts", [2, 3, 7])
def test_parts_add_up(gmx, nparts):
    b, i = tcd_graph("rmat12")
    g = gmx.Graph.upload(b, i)
    with knobs():
        parts = [g.triangle_counting_directed(p, nparts)[0] for p in range(nparts)]
    assert sum(parts) == PINNED["rmat12"] and min(parts) > 0


def test_plan_is_cached_and_follows_the_order_knob(gmx, capfd):
    b, i = tcd_graph("rmat10")
    g = gmx.Graph.upload(b, i)
    seen = [logged(gmx, g, capfd, **env) for env in ({}, {}, FORCED["no_order"], FORCED["no_order"], {})]
    assert [T for T, _, _ in seen] == [PINNED["rmat10"]] * 5
    assert [(f["order"], f["built"]) for _, _, f in seen] == [("degree", 1), ("degree", 0), ("identity", 1), ("identity", 0), ("degree", 1)]
    assert all((f["build_ms"] > 0) == (f["built"] == 1) for _, _, f in seen)
    dist = g.hop_dist(0)[0]                                              # the graph's other entries are undisturbed
    assert g.triangle_counting_directed()[0] == PINNED["rmat10"] and np.array_equal(g.hop_dist(0)[0], dist)


def test_errors_and_empties(gmx):
    b, i = tcd_graph("star33")
    g = gmx.Graph.upload(b, i)
    L = gmx.lib()
    t = C.c_int64(-1)
    for part, nparts in ((1, 1), (-1, 2), (2, 2), (0, 0), (0, -3)):
        assert L.gmx_triangle_counting_directed_part(g._h, part, nparts, C.byref(t), None) == GMX_ERR_ARG, (part, nparts)
        with pytest.raises(gmx.GmxError):
            g.triangle_counting_directed(part, nparts)
    assert L.gmx_triangle_counting_directed(g._h, None, None) == GMX_ERR_ARG
    assert L.gmx_triangle_counting_directed(None, C.byref(t), None) == GMX_ERR_ARG
    assert L.gmx_triangle_counting_directed(g._h, C.byref(t), None) == 0 and t.value == 0      # stats may be NULL
    for V in (1001, 0):
        e = gmx.Graph.upload(np.zeros(V + 1, np.int32), np.zeros(0, np.int32))
        assert e.triangle_counting_directed()[0] == 0
        assert [e.triangle_counting_directed(p, 3)[0] for p in range(3)] == [0, 0, 0]


def test_driver(gmx, tmp_path):
    exe = os.path.join(PKG, "bin", "triangle_counting_directed")
    assert os.path.exists(exe), "bin/triangle_counting_directed not built"
    path = str(tmp_path / "rmat10.bin")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "make_bin.py"), "10", "0", path], stdout=subprocess.DEVNULL, timeout=120, env=env)
    out = subprocess.run([exe, path, "1", "/dev/null"], stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    assert "number of triangles: 635428\n" in out.stdout
    assert out.stdout.index("number of triangles:") > out.stdout.index("running time=")
    assert out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n")
