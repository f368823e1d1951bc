"""The sampling programs, host side (no GPU): the 48-bit stream against libc's erand48, the runtime shim's gm_rt_uniform /
gm_rt_rand / gm_rt_rand_long and gm_graph::pick_random_out_neighbor from a small C++ program, the literal loops (the
arbiter, sampling_common) against the pinned table, a numpy model of the parallel scheme the device follows (offset scan,
jumps by the 2^k table, the initial set in batches) against the literal loop on random multigraphs with isolated vertices,
and the single-walker drop-in.  test_gpu_sampling.py compares the device with the same loops."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sampling_common as sc
from conftest import ROOT
from test_host_cpp import CXX_FLAGS, LINK, PKG, host_built  # noqa: F401  (host_built: a fixture)

NAMES = ["parallel_random_walk_jump_sampling", "random_node_sampling", "random_degree_node_sampling", "random_walk_sampling_with_random_jump"]


def erand48_draws(seed16, n):
    libc = ctypes.CDLL(None)
    libc.erand48.restype = ctypes.c_double
    xs = (ctypes.c_ushort * 3)(*seed16)
    out = [libc.erand48(xs) for _ in range(n)]
    return out, xs[0] | (xs[1] << 16) | (xs[2] << 32)


def random_multigraph(seed, V=40, E=150):
    """repeats, self loops, rows in drawn order, about a quarter of the vertices without out-edges"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, E)
    src = src[(src % 4) != 1]
    return sc.csr(V, [(int(s), int(rng.integers(0, V))) for s in src])


def test_entries_declared_bound_and_exported():
    import gmx
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert re.search(r"\bint gmx_random_walk_sampling\(gmx_graph_t\* g, float p_size, float p_jump, int32_t num_tokens, int32_t max_rounds,\s*"
                     r"uint64_t\* rng_state, uint8_t\* selected_host", hdr)
    assert re.search(r"\bint gmx_node_sampling\(gmx_graph_t\* g, int by_degree, int32_t N, uint64_t\* rng_state,", hdr)
    assert "rand()" in hdr and "gm_graph.h:379-391" in hdr          # what is not reproduced is said
    if not os.path.exists(gmx.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for s in ("gmx_random_walk_sampling", "gmx_node_sampling"):
        assert s in gmx.EXPORTS and hasattr(gmx.lib(), s)
    assert callable(gmx.Graph.random_walk_sampling) and callable(gmx.Graph.node_sampling)


def test_stream_is_erand48():
    want, state = erand48_draws((0x330E, 1, 0), 5)
    s = sc.Stream(0x1330E)
    assert [s.uniform() for _ in range(5)] == want and s.x == state == 0x90C3E9DE8D15
    assert sc.jump(0x1330E, 1) == sc.X0 == 0x0AA849495101
    want, state = erand48_draws((0x330E, 4, 0), 1000)
    s = sc.Stream(0x4330E)
    assert [s.uniform() for _ in range(1000)] == want and s.x == state
    for n in (0, 1, 2, 5, 63, 64, 1000, 123456789):
        t = sc.Stream(sc.X0)
        for _ in range(min(n, 1000)):
            t.uniform()
        if n <= 1000:
            assert sc.jump(sc.X0, n) == t.x
        assert sc.jump(sc.jump(sc.X0, n), 7) == sc.jump(sc.X0, n + 7)


@pytest.mark.parametrize("row", sc.WALK_TABLE, ids=lambda r: "%s-%g-%g-%d" % r[:4])
def test_walk_table(row):
    name, p_size, p_jump, tokens, count, rounds, selsum, tokw, state = row
    b, i = sc.GRAPHS[name]()
    sel, tok, c, r, x = sc.walk_loop(b, i, p_size, p_jump, tokens, 2 ** 31 - 1, sc.X0)
    assert (c, r) + sc.summarize(sel, tok) + (x,) == (count, rounds, selsum, tokw, state)
    assert int(tok.sum()) == tokens and int(sel.sum()) == c
    m = sc.walk_model(b, i, p_size, p_jump, tokens, 2 ** 31 - 1, sc.X0, batch=5)
    assert np.array_equal(m[0], sel) and np.array_equal(m[1], tok) and m[2:] == (c, r, x)


@pytest.mark.parametrize("row", sc.NODE_TABLE, ids=lambda r: "%s-%d-%d" % r[:3])
def test_node_table(row):
    name, by_degree, N, count, idsum = row
    b, _ = sc.GRAPHS[name]()
    sel, c, x = sc.node_loop(b, by_degree, N, sc.X0)
    assert (c, sc.summarize(sel, sel)[0], x) == (count, idsum, sc.NODE_STATE) and x == sc.jump(sc.X0, 64)


def test_node_loop_edge_cases():
    b = np.zeros(11, np.int32)                                   # E = 0: 0 / 0 is NaN, nobody is selected
    assert sc.node_loop(b, 1, 5, sc.X0)[1] == 0
    assert sc.node_loop(b, 0, 0, sc.X0)[1] == 10                 # 1 / 0.0 is +inf: everybody
    assert sc.node_loop(b, 0, -3, sc.X0)[1] == 0


def test_parallel_model_equals_the_literal_loop():
    for seed in range(12):
        b, i = random_multigraph(seed)
        V = len(b) - 1
        assert np.count_nonzero(np.diff(b) == 0) >= 5
        tokens = (1, 3, V, 17)[seed % 4]
        p_jump = (0.15, 0.0, 1.0, 0.5)[(seed // 4) % 4]
        args = (b, i, 0.8, p_jump, tokens, 40, sc.X0 + seed)
        want = sc.walk_loop(*args)
        got = sc.walk_model(*args, batch=(1, 7, 64)[seed % 3])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], seed


def run_check(host_built, tmp_path, *args):
    exe = str(tmp_path / "sampling_check")
    if not os.path.exists(exe):
        subprocess.check_call(["g++"] + CXX_FLAGS + [os.path.join(ROOT, "tests", "cpp", "sampling_check.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


@pytest.mark.parametrize("n", [1, 4])
def test_shim_streams(host_built, tmp_path, n):
    out = run_check(host_built, tmp_path, "streams", n)
    seed = 0x330E | (n << 16)
    start = sc.jump(seed, 1)
    assert out[:n] == ["state %d %012x" % (t, start) for t in range(n)]
    if n == 1:
        assert start == sc.X0
    want, _ = erand48_draws((0x330E, n, 0), 6)
    assert [float.fromhex(l.split()[1]) for l in out[n:n + 5]] == want[1:]
    assert out[n + 5] == "after %012x" % sc.jump(seed, 6)
    if n == 1:
        assert out[n + 5] == "after %012x" % sc.jump(0x90C3E9DE8D15, 1)   # the pinned state is five draws from the seed
    s = sc.Stream(sc.jump(seed, 6))
    a = int(s.uniform() * 10) + 10
    b = int(s.uniform() * 1000000)
    assert out[n + 6] == "rand %d %d" % (a, b) and out[n + 7] == "end %012x" % s.x


@pytest.mark.parametrize("name,N,c", [("ring64", 40, 0.15), ("star64", 100, 0.15), ("star64", 30, 0.0), ("ring64", 25, 1.0)])
def test_single_walker_and_pick_random_out_neighbor(host_built, tmp_path, name, N, c):
    out = run_check(host_built, tmp_path, "walk", name, N, c)
    b, i = sc.GRAPHS[name]()
    s = sc.Stream(sc.X0)
    picks = [int(i[b[0] + int(s.uniform() * float(b[1] - b[0]))]) for _ in range(3)]
    assert out[0].split()[1:] == [str(p) for p in picks]
    members, x = sc.single_walk_loop(b, i, N, c, s.x)
    assert out[1].split()[1:] == [str(m) for m in members] and 1 <= len(members) <= N
    assert out[2] == "state %012x" % x


def test_drop_ins_and_drivers_are_built(host_built):
    for name in NAMES:
        assert os.path.exists(os.path.join(PKG, "generated", name + ".h")) and os.path.exists(os.path.join(PKG, "generated", name + ".cc"))
        exe = os.path.join(PKG, "bin", name)
        assert os.path.exists(exe), "bin/%s not built" % name
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout
    sig = {"parallel_random_walk_jump_sampling": r"\(gm_graph& G, float p_size, float p_jump, int32_t num_tokens, bool\* G_Selected\)",
           "random_node_sampling": r"\(gm_graph& G, int32_t N, gm_node_set& S\)", "random_degree_node_sampling": r"\(gm_graph& G, int32_t N, gm_node_set& S\)",
           "random_walk_sampling_with_random_jump": r"\(gm_graph& G, int32_t N, double c, gm_node_set& S\)"}
    for name, pat in sig.items():
        assert re.search(r"void " + name + pat + ";", open(os.path.join(PKG, "generated", name + ".h")).read())
