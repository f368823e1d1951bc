"""gmx_v_cover (v_cover.gm) on the device against the program as written (test_v_cover_host.v_cover_literal) and, where that
loop is too slow, the cursor formulation (v_cover_ref): every golden case and named graph, the knobs forced to each path (and
shown to be the path that ran, from the library's GMX_VC_LOG line), the schedule-independent counters and the bounds that rule
out rescanning, every upload form of an unsorted multigraph, the plan cache, errors, empties and the driver.

rmat12's longest incident list has more than 2376 entries (wave cursors and several merge-path tiles occur naturally), rmat14
is the hub case (173 rounds), chain4096 runs 2048 rounds, nearly all of them in the tail launch.  The reference ships no
generated v_cover.cc, so nothing reference-compiled exists for this program and no such fixture is used."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_upload_forms_host import unsorted_multigraph
from test_v_cover_host import NAMED, TINY, literal_of, ref_of, v_cover_literal, vc_graph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG, GMX_ERR_STATE = -1, -5
KNOBS = ("GMX_VC_TAIL", "GMX_VC_WAVE", "GMX_VC_LOG")
HUGE = "2000000000"
FORCED = {"no_tail": {"GMX_VC_TAIL": "0"}, "all_tail": {"GMX_VC_TAIL": HUGE}, "always_wave": {"GMX_VC_WAVE": "0"},
          "always_lane": {"GMX_VC_WAVE": HUGE}}
LINE = re.compile(r"gmx v_cover: plan (built|reused) build_ms ([0-9.]+) V (\d+) E (\d+) L (\d+); tail (\d+) wave (\d+); rounds (\d+) grid \+ (\d+) tail; "
                  r"picks (\d+) kept (\d+) covered (\d+); skips (\d+) evals (\d+) walks (\d+); ms ([0-9.]+) grid \+ ([0-9.]+) tail \+ ([0-9.]+) finish")
FIELDS = ("plan", "build_ms", "V", "E", "L", "tail_from", "wave_min", "grid_rounds", "tail_rounds", "picks", "kept", "covered", "skips", "evals",
          "walks", "grid_ms", "tail_ms", "finish_ms")


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


def logged(g, capfd, **env):
    """(select, covered, stats, the fields of the library's line) of one call."""
    capfd.readouterr()
    with knobs(GMX_VC_LOG="1", **env):
        sel, cov, st = g.v_cover()
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    f = {k: (v if k == "plan" else float(v) if k.endswith("ms") else int(v)) for k, v in zip(FIELDS, lines[0])}
    return sel, cov, st, f


def check(want, sel, cov, st=None):
    assert cov == want[0] and sel.dtype == bool and np.array_equal(sel, want[1])
    if st is not None:
        assert st["vertices_reached"] == cov and st["edges_reached"] == int(sel.sum()) and (st["kernel_ms"] > 0) == (len(sel) > 0)
        assert st["last_diff"] == 0 and st["h2d_ms"] == 0


def test_golden_cases(gmx, golden):
    for name, c in sorted(golden["cases"].items()):
        if "begin" not in c:
            continue
        g = gmx.Graph.upload(c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
        with knobs():
            sel, cov, st = g.v_cover()
        check(v_cover_literal(c["begin"], c["node_idx"]), sel, cov, st)


@pytest.mark.parametrize("name", sorted(TINY) + NAMED)
def test_parity_with_the_literal_loop(gmx, capfd, name):
    b, i = vc_graph(name)
    g = gmx.Graph.upload(b, i)
    if len(i) == 0:                                          # nothing runs, nothing is logged
        check(literal_of(name), *g.v_cover())
        return
    sel, cov, st, f = logged(g, capfd)
    print("v_cover %s: %s" % (name, f))
    check(literal_of(name), sel, cov, st)
    if len(i):
        _, _, _, rounds, ctr = ref_of(name)
        assert st["iterations"] == f["grid_rounds"] + f["tail_rounds"] == rounds
        assert st["edges_examined"] == f["skips"] + f["evals"] + f["walks"]


def test_parity_rmat14_with_the_formulation(gmx, capfd):
    b, i = vc_graph("rmat14")
    g = gmx.Graph.upload(b, i)
    sel, cov, st, f = logged(g, capfd)
    print("v_cover rmat14: %s" % f)
    want = ref_of("rmat14")
    check(want, sel, cov, st)
    assert (cov, int(sel.sum())) == (12661, 9716) and st["iterations"] == want[3] == 173


@pytest.mark.parametrize("forced", sorted(FORCED))
@pytest.mark.parametrize("name", ["rmat12", "chain4096", "cut6"])
def test_forced_paths(gmx, capfd, name, forced):
    """Every forced setting gives the literal loop's result, and ran the path it names."""
    b, i = vc_graph(name)
    g = gmx.Graph.upload(b, i)
    sel, cov, st, f = logged(g, capfd, **FORCED[forced])
    print(name, forced, f)
    check(literal_of(name), sel, cov, st)
    _, _, _, rounds, ctr = ref_of(name)
    assert f["grid_rounds"] + f["tail_rounds"] == rounds
    if forced == "no_tail":
        assert f["tail_from"] == 0 and f["tail_rounds"] == 0 and f["tail_ms"] == 0
    if forced == "all_tail":
        assert f["grid_rounds"] == 0 and f["tail_rounds"] == rounds
    if forced == "always_wave":
        assert f["wave_min"] == 0
    if forced == "always_lane":
        assert f["wave_min"] >= 2 * len(i)                   # longer than any list


@pytest.mark.parametrize("name", ["rmat12", "chain4096", "multi300", "cut6", "star33"])
def test_counters(gmx, capfd, name):
    """rounds, picks and kept do not depend on the schedule; the three work counters are bounded by the list entries: a
    fall-back to rescanning rows every round would break the bounds (rmat12: 62 x E)."""
    b, i = vc_graph(name)
    g = gmx.Graph.upload(b, i)
    _, _, _, rounds, ctr = ref_of(name)
    for env in ({}, FORCED["no_tail"], FORCED["all_tail"]):
        _, _, _, f = logged(g, capfd, **env)
        assert (f["V"], f["E"], f["L"]) == (len(b) - 1, len(i), ctr["L"])
        assert (f["grid_rounds"] + f["tail_rounds"], f["picks"], f["kept"]) == (rounds, ctr["picks"], ctr["kept"])
        assert f["skips"] <= f["L"] and f["walks"] <= f["L"] and f["evals"] <= f["L"] + f["V"]
        assert f["evals"] >= np.count_nonzero(np.diff(b)) and f["walks"] > 0
    if name in ("multi300", "cut6"):
        assert ctr["kept"] < ctr["picks"]                    # the cut fired on the device too


def test_default_rmat12_uses_grid_rounds_and_the_tail(gmx, capfd):
    b, i = vc_graph("rmat12")
    g = gmx.Graph.upload(b, i)
    _, _, _, f = logged(g, capfd)
    assert f["grid_rounds"] > 0 and f["tail_rounds"] > 0 and (f["tail_from"], f["wave_min"]) == (2048, 128)


def test_upload_forms_give_one_select(gmx):
    """select is indexed, and ties are decided, by the uploaded slots whatever the device did to the rows."""
    V = 300
    b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 2000, 3))
    want = literal_of("multi300")
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    forms = {"given reverse, sorted on upload": (True, S), "given reverse, verbatim": (True, 0), "device-built reverse": (False, 0)}
    for regime in ({}, FORCED["no_tail"]):
        for form, (rev, flags) in forms.items():
            g = gmx.Graph.upload(b, i, rb if rev else None, ri if rev else None, flags=flags)
            with knobs(**regime):
                sel, cov, _ = g.v_cover()
            check(want, sel, cov)
    L = gmx.lib()
    h = C.c_void_p()
    b64, rb64 = b.astype(np.int64), rb.astype(np.int64)
    for rev in (True, False):
        assert L.gmx_graph_upload_e64(b64.ctypes.data, i.ctypes.data, rb64.ctypes.data if rev else None, ri.ctypes.data if rev else None, V, len(i),
                                      0, C.byref(h)) == 0
        with knobs():
            sel, cov, _ = gmx.Graph(h).v_cover()
        check(want, sel, cov)
    for flags in (N, S | N):
        g = gmx.Graph.upload(b, i, flags=flags)
        sel = np.zeros(len(i), np.uint8)
        cov = C.c_int32(-1)
        assert L.gmx_v_cover(g._h, sel.ctypes.data, C.byref(cov), None) == GMX_ERR_STATE
        assert b"reverse" in L.gmx_last_error() and not sel.any()


def test_plan_is_cached_and_freed_with_the_graph(gmx, capfd):
    b, i = vc_graph("rmat10")
    g = gmx.Graph.upload(b, i)
    want = literal_of("rmat10")
    sel, cov, _, f1 = logged(g, capfd)
    check(want, sel, cov)
    dist = g.hop_dist(0)[0]                                  # the graph's other entries in between
    T = g.triangle_counting_directed()[0]
    sel, cov, _, f2 = logged(g, capfd)
    check(want, sel, cov)
    assert (f1["plan"], f2["plan"]) == ("built", "reused") and f1["build_ms"] > 0 and f2["build_ms"] == 0
    assert np.array_equal(g.hop_dist(0)[0], dist) and g.triangle_counting_directed()[0] == T
    g.free()


def test_errors_and_empties(gmx):
    b, i = vc_graph("star33")
    g = gmx.Graph.upload(b, i)
    L = gmx.lib()
    sel = np.zeros(len(i), np.uint8)
    cov = C.c_int32(-1)
    assert L.gmx_v_cover(None, sel.ctypes.data, C.byref(cov), None) == GMX_ERR_ARG
    assert L.gmx_v_cover(g._h, sel.ctypes.data, None, None) == GMX_ERR_ARG
    assert L.gmx_v_cover(g._h, None, C.byref(cov), None) == GMX_ERR_ARG
    assert L.gmx_v_cover(g._h, sel.ctypes.data, C.byref(cov), None) == 0 and cov.value == 33 and sel.sum() == 32   # stats may be NULL
    for V in (1001, 0):
        e = gmx.Graph.upload(np.zeros(V + 1, np.int32), np.zeros(0, np.int32))
        cov = C.c_int32(-1)
        assert L.gmx_v_cover(e._h, None, C.byref(cov), None) == 0 and cov.value == 0
        s, c, st = e.v_cover()
        assert len(s) == 0 and c == 0 and st["iterations"] == 0


def test_driver(gmx, golden):
    exe = os.path.join(PKG, "bin", "v_cover")
    assert os.path.exists(exe), "bin/v_cover not built"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file
    n = v_cover_literal(c["begin"], c["node_idx"])[0]
    assert "covered (may be non-deterministic) = %d\n" % n in out.stdout
    assert out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n")
