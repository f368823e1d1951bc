"""gmx_random_walk_sampling (parallel_random_walk_jump_sampling.gm) and gmx_node_sampling (random_node_sampling.gm,
random_degree_node_sampling.gm) on the device against the programs as one thread runs them (sampling_common.walk_loop /
node_loop on the downloaded CSR): selected, token, count, rounds and the stream state are compared as bytes, under every
setting of the knobs, and the library's GMX_RW_LOG line shows which path ran.  The draws the line reports are checked too:
the state after is the state before advanced by exactly that many.

Shapes: the pinned table; V = 1; a two-way star with 4097 leaves (tokens = V, and 4000 tokens so that the hub's row holds
thousands of tokens in the rounds that follow and crosses a 2048-item tile); rows without out-edges between others (1-draw
and 2-draw vertices mixed in the scan); repeats and self loops; every upload form; 1 token; V tokens on V = 4096 (the
coupon-collector initial set, several batches); p_jump 0 and 1; N = 0; a closed 2-cycle stopped by max_rounds; RMAT-14."""
import contextlib
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import sampling_common as sc
from conftest import GOLD, ROOT
from test_gpu_sssp_path_adj import _forms
from test_host_cpp import CXX_FLAGS, LINK
from test_upload_forms_host import unsorted_multigraph

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "green-marl_amd")
GMX_ERR_ARG = -1
INT_MAX = 2 ** 31 - 1
KNOBS = ("GMX_RW_TAIL", "GMX_RW_ORDER", "GMX_RW_LOG")
HUGE = "2000000000"
FORCED = {"default": {}, "all_tail": {"GMX_RW_TAIL": HUGE}, "no_tail": {"GMX_RW_TAIL": "0"},
          "sort": {"GMX_RW_TAIL": "0", "GMX_RW_ORDER": "sort"}, "dense": {"GMX_RW_TAIL": "0", "GMX_RW_ORDER": "dense"}}
LINE = re.compile(r"gmx random_walk_sampling: V (\d+) tokens (\d+); tail (\d+); batches (\d+); rounds (\d+) grid \+ (\d+) tail; tail launches (\d+); "
                  r"sort rounds (\d+) dense rounds (\d+); draws (\d+); count (\d+); ms ([0-9.]+)")
FIELDS = ("V", "tokens", "tail_from", "batches", "grid_rounds", "tail_rounds", "tail_launches", "sort_rounds", "dense_rounds", "draws", "count", "ms")


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


def logged(g, capfd, p_size, p_jump, tokens, x, max_rounds=INT_MAX, **env):
    capfd.readouterr()
    with knobs(GMX_RW_LOG="1", **env):
        out = g.random_walk_sampling(p_size, p_jump, tokens, x, max_rounds)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1
    f = {k: (float(v) if k == "ms" else int(v)) for k, v in zip(FIELDS, lines[0])}
    return out, f


def same(got, want):
    """(selected, token, count, rounds, state[, stats]) of the device against the loop's, as bytes"""
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert tuple(got[2:5]) == tuple(want[2:5])


def check_paths(g, capfd, want, p_size, p_jump, tokens, x, max_rounds=INT_MAX, regimes=tuple(FORCED)):
    """every regime gives the loop's bytes and ran the path it names"""
    V, rounds = len(want[0]), want[3]
    for name in regimes:
        got, f = logged(g, capfd, p_size, p_jump, tokens, x, max_rounds, **FORCED[name])
        print(name, f)
        same(got, want)
        st = got[5]
        assert (st["iterations"], st["vertices_reached"], st["edges_examined"]) == (rounds, want[2], rounds * tokens)
        assert (f["V"], f["tokens"], f["count"]) == (V, tokens, want[2]) and f["grid_rounds"] + f["tail_rounds"] == rounds
        assert sc.jump(x, f["draws"]) == want[4]
        if name == "all_tail" or (name == "default" and tokens <= 2048):
            assert f["grid_rounds"] == 0 and f["tail_launches"] == (rounds + 1023) // 1024 and f["sort_rounds"] + f["dense_rounds"] == 0
        else:
            assert f["tail_rounds"] == 0 and f["tail_launches"] == 0 and f["sort_rounds"] + f["dense_rounds"] == rounds
        if name == "sort":
            assert f["dense_rounds"] == 0
        if name == "dense":
            assert f["sort_rounds"] == 0


def upload(gmx, b, i):
    g = gmx.Graph.upload(np.ascontiguousarray(b, np.int32), np.ascontiguousarray(i, np.int32))
    db, di = g.download(reverse=False)[:2]
    return g, db, di


def multigraph(seed, V, E):
    """repeats, self loops, rows in drawn order, a quarter of the vertices (v % 4 == 1) without out-edges, between the others"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, E)
    src = np.sort(src[(src % 4) != 1], kind="stable")
    dst = rng.integers(0, V, len(src))
    dst[::7] = src[::7]                                      # self loops
    dst[1::5] = dst[0:-1:5][:len(dst[1::5])]                 # repeated slots
    b = np.zeros(V + 1, np.int32)
    np.add.at(b, src + 1, 1)
    return np.cumsum(b).astype(np.int32), dst.astype(np.int32)


def star(leaves):
    return sc.csr(leaves + 1, [(0, t) for t in range(1, leaves + 1)] + [(v, 0) for v in range(1, leaves + 1)])


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "v1":
        return np.zeros(2, np.int32), np.zeros(0, np.int32)
    if name == "star4097":
        return star(4097)
    if name == "mixed3000":
        return multigraph(3, 3000, 9000)
    if name == "mixed4096":
        return multigraph(4, 4096, 16000)
    if name == "cycle2":
        return sc.csr(2, [(0, 1), (1, 0)])
    return sc.GRAPHS[name]()


@pytest.mark.parametrize("row", sc.WALK_TABLE, ids=lambda r: "%s-%g-%g-%d" % r[:4])
def test_table(gmx, capfd, row):
    name, p_size, p_jump, tokens, count, rounds, selsum, tokw, state = row
    g, b, i = upload(gmx, *shape(name))
    want = sc.walk_loop(b, i, p_size, p_jump, tokens, INT_MAX, sc.X0)
    assert (want[2], want[3]) + sc.summarize(want[0], want[1]) + (want[4],) == (count, rounds, selsum, tokw, state)
    check_paths(g, capfd, want, p_size, p_jump, tokens, sc.X0)
    g.free()


SHAPES = [("v1", 1.0, 0.15, 1), ("star4097", 1.0, 0.15, 4098), ("star4097", 1.0, 0.15, 4000), ("star4097", 0.9, 0.0, 1),
          ("mixed3000", 0.9, 0.15, 500), ("mixed3000", 0.5, 0.0, 1), ("mixed3000", 0.95, 1.0, 2500), ("mixed4096", 1.0, 0.15, 4096),
          ("mixed4096", 0.0, 0.15, 100), ("ring64", 1.0, 0.0, 3)]


@pytest.mark.parametrize("name,p_size,p_jump,tokens", SHAPES, ids=lambda v: str(v))
def test_shapes(gmx, capfd, name, p_size, p_jump, tokens):
    g, b, i = upload(gmx, *shape(name))
    x = sc.X0 + 12345
    want = sc.walk_loop(b, i, p_size, p_jump, tokens, 300, x)
    print(name, "count", want[2], "rounds", want[3], "max token", int(want[1].max()))
    if p_size == 0.0:
        assert want[3] == 0 and not want[0].any() and int(want[1].sum()) == tokens       # N = 0: the tokens are placed, no round
    check_paths(g, capfd, want, p_size, p_jump, tokens, x, 300)
    g.free()


def test_star_hub_holds_thousands_of_tokens(gmx, capfd):
    """4000 tokens on the star: after the first round the hub's row holds more tokens than one 2048-item tile, round after
    round, and the grid spreads them; the batched initial set took 4000 of 4098 vertices."""
    g, b, i = upload(gmx, *shape("star4097"))
    per_round = []
    for r in (1, 2, 3):
        want = sc.walk_loop(b, i, 1.0, 0.15, 4000, r, sc.X0)
        per_round.append(int(want[1][0]))
        check_paths(g, capfd, want, 1.0, 0.15, 4000, sc.X0, r, regimes=("no_tail", "all_tail"))
    assert max(per_round) > 2048
    g.free()


def test_initial_set_of_every_vertex_takes_batches(gmx, capfd):
    g, b, i = upload(gmx, *shape("mixed4096"))
    want = sc.walk_loop(b, i, 0.0, 0.15, 4096, INT_MAX, sc.X0)
    got, f = logged(g, capfd, 0.0, 0.15, 4096, sc.X0)
    same(got, want)
    assert np.all(got[1] == 1) and f["batches"] >= 2 and f["draws"] > 4096 * 5 and sc.jump(sc.X0, f["draws"]) == want[4]
    g.free()


def test_upload_forms(gmx, capfd):
    V = 300
    b, i, rb, ri = (np.ascontiguousarray(x, np.int32) for x in unsorted_multigraph(V, 2000, 3))
    for label, g in _forms(gmx, b, i, rb, ri):
        db, di = g.download(reverse=False)[:2]
        want = sc.walk_loop(db, di, 0.9, 0.15, 40, 200, sc.X0)
        check_paths(g, capfd, want, 0.9, 0.15, 40, sc.X0, 200, regimes=("default", "sort", "dense"))
        for by_degree, N in ((0, 7), (1, 30)):
            sel, cnt, x, _ = g.node_sampling(by_degree, N, sc.X0)
            w = sc.node_loop(db, by_degree, N, sc.X0)
            assert sel.tobytes() == w[0].tobytes() and (cnt, x) == w[1:], label
        g.free()


def test_closed_cycle_stops_at_max_rounds(gmx, capfd):
    g, b, i = upload(gmx, *shape("cycle2"))
    want = sc.walk_loop(b, i, 1.0, 0.0, 1, 50, sc.X0)
    assert want[3] == 2 and want[2] == 2                      # alone, the cycle is covered after two rounds
    check_paths(g, capfd, want, 1.0, 0.0, 1, sc.X0, 50)
    b3, i3 = sc.csr(3, [(0, 1), (1, 0), (2, 2)])              # the cycle next to a vertex it never reaches: count < N at the stop
    g3, b3, i3 = upload(gmx, b3, i3)
    for x in (sc.X0, sc.X0 + 1, sc.X0 + 2):
        want = sc.walk_loop(b3, i3, 1.0, 0.0, 1, 50, x)
        assert want[3] == 50 and want[2] < 3
        check_paths(g3, capfd, want, 1.0, 0.0, 1, x, 50, regimes=("default", "no_tail"))
    w0 = sc.walk_loop(b, i, 1.0, 0.0, 1, 0, sc.X0)          # max_rounds = 0: the tokens are placed
    same(g.random_walk_sampling(1.0, 0.0, 1, sc.X0, 0), w0)
    g.free()
    g3.free()


def test_more_rounds_than_one_tail_launch(gmx, capfd):
    b3, i3 = sc.csr(3, [(0, 1), (1, 0), (2, 2)])
    g, b3, i3 = upload(gmx, b3, i3)
    x = next(x for x in range(sc.X0, sc.X0 + 50) if sc.walk_loop(b3, i3, 1.0, 0.0, 1, 1, x)[0][2] == 0)
    want = sc.walk_loop(b3, i3, 1.0, 0.0, 1, 2500, x)
    assert want[3] == 2500
    got, f = logged(g, capfd, 1.0, 0.0, 1, x, 2500)
    same(got, want)
    assert f["tail_launches"] == 3 and f["tail_rounds"] == 2500
    g.free()


def test_chained_calls_continue_one_stream(gmx):
    g, b, i = upload(gmx, *shape("mixed3000"))
    for env in (FORCED["default"], FORCED["no_tail"]):
        x = sc.X0
        for call in range(2):
            want = sc.walk_loop(b, i, 0.3, 0.15, 64, INT_MAX, x)
            with knobs(**env):
                got = g.random_walk_sampling(0.3, 0.15, 64, x)
            same(got, want)
            x = got[4]
        sel, cnt, x2, _ = g.node_sampling(1, 100, x)
        w = sc.node_loop(b, 1, 100, x)
        assert sel.tobytes() == w[0].tobytes() and (cnt, x2) == w[1:] and x2 == sc.jump(x, 3000)
    g.free()


def test_rmat14(gmx, capfd):
    g = gmx.Graph.rmat(1 << 14, 16 << 14, 1997, 0.57, 0.19, 0.19, False)
    b, i = g.download(reverse=False)[:2]
    want = sc.walk_loop(b, i, 0.5, 0.15, 2048, INT_MAX, sc.X0)
    print("rmat14: count", want[2], "rounds", want[3])
    assert want[3] >= 3
    check_paths(g, capfd, want, 0.5, 0.15, 2048, sc.X0)
    first = g.random_walk_sampling(0.5, 0.15, 2048, sc.X0)
    for _ in range(3):                                        # run-to-run identity
        same(g.random_walk_sampling(0.5, 0.15, 2048, sc.X0), first)
    for by_degree, N in ((0, 100), (1, 1000)):
        sel, cnt, x, st = g.node_sampling(by_degree, N, sc.X0)
        w = sc.node_loop(b, by_degree, N, sc.X0)
        assert sel.tobytes() == w[0].tobytes() and (cnt, x) == w[1:] and st["vertices_reached"] == cnt and cnt > 0
    g.free()


@pytest.mark.parametrize("row", sc.NODE_TABLE, ids=lambda r: "%s-%d-%d" % r[:3])
def test_node_table(gmx, row):
    name, by_degree, N, count, idsum = row
    g, b, _ = upload(gmx, *shape(name))
    sel, cnt, x, st = g.node_sampling(by_degree, N, sc.X0)
    w = sc.node_loop(b, by_degree, N, sc.X0)
    assert sel.dtype == np.uint8 and sel.tobytes() == w[0].tobytes()
    assert (cnt, sc.summarize(sel, sel)[0], x) == (count, idsum, sc.NODE_STATE) and st["iterations"] == 1
    g.free()


def test_node_sampling_shapes_and_empties(gmx):
    for name in ("v1", "star4097", "mixed3000", "mixed4096"):
        g, b, _ = upload(gmx, *shape(name))
        for by_degree, N in ((0, 3), (1, 50), (0, 0), (0, -2), (1, 0), (1, -5), (1, INT_MAX)):
            sel, cnt, x, _ = g.node_sampling(by_degree, N, sc.X0 + 7)
            w = sc.node_loop(b, by_degree, N, sc.X0 + 7)
            assert sel.tobytes() == w[0].tobytes() and (cnt, x) == w[1:], (name, by_degree, N)
        g.free()
    e = gmx.Graph.upload(np.zeros(1002, np.int32), np.zeros(0, np.int32))                                # E = 0: NaN, the empty set
    sel, cnt, x, _ = e.node_sampling(1, 10, sc.X0)
    assert cnt == 0 and not sel.any() and x == sc.jump(sc.X0, 1001)
    sel, cnt, x, _ = e.node_sampling(0, 2, sc.X0)
    assert sel.tobytes() == sc.node_loop(np.zeros(1002, np.int32), 0, 2, sc.X0)[0].tobytes() and cnt > 0
    z = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))                                   # V = 0
    x, cnt = C.c_uint64(sc.X0), C.c_int64(-1)
    assert gmx.lib().gmx_node_sampling(z._h, 0, 4, C.byref(x), None, C.byref(cnt), None) == 0 and cnt.value == 0 and x.value == sc.X0


def test_errors_write_nothing(gmx):
    g, b, i = upload(gmx, *shape("ring64"))
    z = gmx.Graph.upload(np.zeros(1, np.int32), np.zeros(0, np.int32))
    L = gmx.lib()
    f = L.gmx_random_walk_sampling
    sel, tok = np.full(64, 77, np.uint8), np.full(64, 77, np.int32)
    x, cnt, rounds = C.c_uint64(sc.X0), C.c_int64(-5), C.c_int32(-5)
    st = gmx.Stats()
    st.iterations = 99
    px, pc, pr, ps = C.byref(x), C.byref(cnt), C.byref(rounds), C.byref(st)
    nan = float("nan")
    bad = [(g._h, 0.5, 0.15, 0, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),           # num_tokens < 1
           (g._h, 0.5, 0.15, 65, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),          # > V
           (g._h, nan, 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),
           (g._h, 0.5, nan, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),
           (g._h, 1.5, 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),           # N > V
           (g._h, float("inf"), 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),
           (g._h, 0.5, 0.15, 4, -1, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),           # max_rounds < 0
           (None, 0.5, 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),
           (g._h, 0.5, 0.15, 4, 10, None, sel.ctypes.data, tok.ctypes.data, pc, pr, ps),
           (g._h, 0.5, 0.15, 4, 10, px, None, tok.ctypes.data, pc, pr, ps),
           (g._h, 0.5, 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, None, pr, ps),
           (g._h, 0.5, 0.15, 4, 10, px, sel.ctypes.data, tok.ctypes.data, pc, None, ps),
           (z._h, 0.5, 0.15, 1, 10, px, sel.ctypes.data, tok.ctypes.data, pc, pr, ps)]           # V = 0
    for args in bad:
        assert f(*args) == GMX_ERR_ARG, args[1:5]
        assert L.gmx_last_error()
        assert np.all(sel == 77) and np.all(tok == 77) and (x.value, cnt.value, rounds.value, st.iterations) == (sc.X0, -5, -5, 99)
    # token_host and stats may be NULL
    assert f(g._h, 0.5, 0.15, 4, INT_MAX, px, sel.ctypes.data, None, pc, pr, None) == 0
    want = sc.walk_loop(b, i, 0.5, 0.15, 4, INT_MAX, sc.X0)
    assert sel.tobytes() == want[0].tobytes() and (cnt.value, rounds.value, x.value) == want[2:] and np.all(tok == 77)
    n = L.gmx_node_sampling
    x = C.c_uint64(sc.X0)
    sel[:] = 77
    for args in ((None, 0, 4, C.byref(x), sel.ctypes.data, pc, None), (g._h, 0, 4, None, sel.ctypes.data, pc, None),
                 (g._h, 0, 4, C.byref(x), None, pc, None), (g._h, 0, 4, C.byref(x), sel.ctypes.data, None, None)):
        assert n(*args) == GMX_ERR_ARG
        assert np.all(sel == 77) and x.value == sc.X0
    with pytest.raises(Exception):
        g.random_walk_sampling(0.5, 0.15, 0, sc.X0)


def run_driver(name, *args):
    exe = os.path.join(PKG, "bin", name)
    assert os.path.exists(exe), "bin/%s not built" % name
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([exe, os.path.join(GOLD, "rmat8_ref_store_binary.bin"), "1", "/dev/null"] + [str(a) for a in args], stdout=subprocess.PIPE,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout
    assert out.stdout.endswith("XXXXXXXXXX GM DONE XXXXXXXXXXXXXX\n")
    return out.stdout


def test_drivers(gmx, golden):
    c = golden["cases"]["rmat8_noperm"]   # the graph of that file; one thread: the stream starts at X0
    b, i = c["begin"], c["node_idx"]
    want = sc.walk_loop(b, i, 0.5, 0.15, 16, INT_MAX, sc.X0)
    out = run_driver("parallel_random_walk_jump_sampling", 0.5, 0.15, 16)
    assert "selected = %d, rounds = %d\nset size = %d\n" % (want[2], want[3], int(want[0].sum())) in out
    for name, by_degree in (("random_node_sampling", 0), ("random_degree_node_sampling", 1)):
        n = sc.node_loop(b, by_degree, 8, sc.X0)[1]
        assert "selected = %d, rounds = 1\nset size = %d\n" % (n, n) in run_driver(name, 8)
    members, _ = sc.single_walk_loop(b, i, 200, 0.15, sc.X0)
    assert "selected = %d, rounds = 200\nset size = %d\n" % (len(members), len(members)) in run_driver("random_walk_sampling_with_random_jump", 200, 0.15)


@pytest.mark.parametrize("name", ["ring64", "star64"])
def test_generated_entries_on_a_gm_graph(gmx, tmp_path, name):
    """the three device drop-ins one after the other on the shim's thread-0 stream: each continues where the last stopped"""
    exe = str(tmp_path / "sampling_check")
    subprocess.check_call(["g++"] + CXX_FLAGS + [os.path.join(ROOT, "tests", "cpp", "sampling_check.cc"), "-o", exe] + LINK)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe, "dropin", name, "0.5", "0.15", "4", "6"], stdout=subprocess.PIPE, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout
    out = r.stdout.splitlines()
    b, i = sc.GRAPHS[name]()
    w = sc.walk_loop(b, i, 0.5, 0.15, 4, INT_MAX, sc.X0)
    assert out[0].split()[1:] == [str(v) for v in np.flatnonzero(w[0])] and out[1] == "state %012x" % w[4]
    x = w[4]
    for mode in (0, 1):
        n = sc.node_loop(b, mode, 6, x)
        assert out[2 + 2 * mode].split()[1:] == [str(v) for v in np.flatnonzero(n[0])] and out[3 + 2 * mode] == "state %012x" % n[2]
        x = n[2]
