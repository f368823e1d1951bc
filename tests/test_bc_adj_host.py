"""bc_adj / gmx_bc_all, host side (no GPU): the entry is declared, bound and exported; gm_graph::load_adjacency_list, the
node keys, GM_Reader and GM_Tokenizer on the reference's two sample files (committed as fixtures) and on a generated file
against the compiled reference loader; the same checker as a stand-alone program under the address and undefined-behaviour
sanitizers; the reference's own bc_adj_main.cc builds against this tree; bin/bc_adj exists; and what comp_BC(G, BC) of
bc_adj.gm is in terms of the oracle -- po.bc over every vertex in node order with the (v != s) filters."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import GOLD, ROOT
from test_bc_random_host import graph, same_f32
from test_host_cpp import CXX_FLAGS, LINK, PKG, REF_APPS, host_built  # noqa: F401  (host_built: a fixture)

CHECKER = os.path.join(ROOT, "tests", "cpp", "adj_loader_check.cc")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libgmref.so")
USAGE = "<input_file> <config_file> <num_threads>"


def test_entry_declared_bound_and_exported():
    import gmx
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert re.search(r"\bint gmx_bc_all\(gmx_graph_t\* g, int skip_root, int32_t width, float\* bc_host[^,]*, gmx_stats_t\* stats\);", hdr)
    assert "gmx_bc_all" in gmx.EXPORTS
    if not os.path.exists(gmx.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(gmx.lib(), "gmx_bc_all")
    assert callable(getattr(gmx.Graph, "bc_all"))


@pytest.fixture(scope="module")
def checker(host_built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adj") / "adj_loader_check")
    subprocess.check_call(["g++"] + CXX_FLAGS + [CHECKER, "-o", exe] + LINK)
    return exe


def load(exe, path, vschema, eschema, tmp_path):
    """The checker's dump of a file: name -> list of numbers."""
    dump = str(tmp_path / "dump.txt")
    r = subprocess.run([exe, path, vschema, eschema, dump], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "adj loader ok" in r.stdout, r.stdout
    out = {}
    for line in open(dump):
        k, *v = line.split()
        out[k] = [float(x) if k[1:5] == "prop" else int(x) for x in v]
    return out


def test_sample_files(checker, golden, tmp_path):
    """The reference's own sample inputs against what ITS loader made of them (golden cases hand_adj_*: CSR and reverse
    CSR), the key table and the property arrays by hand."""
    for fixture, name in (("very_small_sample.adj", "hand_adj_very_small_sample"), ("cpp_be_test.adj", "hand_adj_cpp_be_test")):
        d = load(checker, os.path.join(GOLD, fixture), "d", "d", tmp_path)
        c = golden["cases"][name]
        assert d["N"] == [len(c["begin"]) - 1] and d["M"] == [len(c["node_idx"])]
        for k in ("begin", "node_idx", "r_begin", "r_node_idx"):
            assert d[k] == c[k].tolist(), (name, k)
    # very_small_sample.adj:  128 10.0  1908 27.03 99 8.51  /  99 2.0  333 338.0
    d = load(checker, os.path.join(GOLD, "very_small_sample.adj"), "d", "d", tmp_path)
    assert d["keys"] == [128, 99, 333, 1908]            # sources in order of appearance, then destination-only keys ascending
    assert d["begin"] == [0, 2, 3, 3, 3] and d["node_idx"] == [1, 3, 2]
    assert d["e_idx2idx"] == [1, 0, 2]                  # row 128 was read as (1908, 99) and is stored as (99, 1908)
    assert d["eprop0"] == [8.51, 27.03, 338.0]          # ... and the costs moved with their edges
    assert d["vprop0"] == [10.0, 2.0, 0.0, 0.0]         # destination-only nodes: zero
    # cpp_be_test.adj:  0 0.0 2 20 1 10 3 30  /  1 0.0 3 31 4 41  /  4 0.0 2 24
    d = load(checker, os.path.join(GOLD, "cpp_be_test.adj"), "d", "d", tmp_path)
    assert d["keys"] == [0, 1, 4, 2, 3]
    assert d["node_idx"] == [1, 3, 4, 2, 4, 3] and d["eprop0"] == [10.0, 20.0, 30.0, 41.0, 31.0, 24.0]
    # the same file with other schema types: a long and a float per edge value, an int per vertex
    d = load(checker, os.path.join(GOLD, "cpp_be_test.adj"), "i", "l", tmp_path)
    assert d["eprop0"] == [10, 20, 30, 41, 31, 24] and d["vprop0"] == [0] * 5
    d = load(checker, os.path.join(GOLD, "cpp_be_test.adj"), "b", "f", tmp_path)
    assert d["eprop0"] == [10.0, 20.0, 30.0, 41.0, 31.0, 24.0] and d["vprop0"] == [0] * 5


def test_bad_lines_are_refused(checker, tmp_path):
    for text in ("5 1.0 6 2.0 7\n", "5\n", "5 1.0 6 1.0\n5 2.0\n"):   # ends inside an edge's / a vertex's values; a key twice
        p = tmp_path / "bad.adj"
        p.write_text(text)
        r = subprocess.run([checker, str(p), "d", "d", str(tmp_path / "x.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 3 and "load failed" in r.stdout, (text, r.stdout)


def generated_file(path):
    """About 200 lines: sparse shuffled keys, keys that are only destinations, repeated edges, unsorted rows, blank
    lines, tabs and spaces (runs of them too) as separators."""
    rng = np.random.default_rng(2024)
    keys = rng.choice(np.arange(1, 100000), 260, replace=False)
    sources, extra = keys[:190], keys[190:]
    with open(path, "w") as f:
        for n, k in enumerate(sources):
            deg = int(rng.integers(0, 9)) if n != 7 else 40
            dst = rng.choice(np.concatenate([sources, extra]), deg)
            if deg > 2:
                dst[1] = dst[0]                        # a repeated edge
            seps = [" ", "\t", "  ", " \t"]
            line = "%d%s%.2f" % (k, seps[n % 4], rng.random() * 9)
            for d in dst:
                line += "%s%d%s%.3f" % (seps[(n + 1) % 4], d, seps[(n + 2) % 4], rng.random() * 99)
            f.write(line + "\n")
            if n % 17 == 0:
                f.write("\n" if n % 34 else " \t\n")   # blank lines, one of them of separators only
    return sources, extra


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="oracle/_ref/libgmref.so was not built (needs the reference checkout at build time)")
def test_generated_file_against_reference_loader(checker, tmp_path):
    path = str(tmp_path / "gen.adj")
    sources, extra = generated_file(path)
    R = C.CDLL(REF_LIB)
    n, m = C.c_int32(0), C.c_int32(0)
    rb, ri = np.zeros(4097, np.int32), np.zeros(65536, np.int32)
    R.ref_load_adj.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    assert R.ref_load_adj(path.encode(), C.byref(n), C.byref(m), rb.ctypes.data, ri.ctypes.data, 4096, 65536) == 0
    d = load(checker, path, "d", "d", tmp_path)
    assert d["N"] == [n.value] and d["M"] == [m.value] and n.value > 190 and m.value > 500
    assert d["begin"] == rb[:n.value + 1].tolist() and d["node_idx"] == ri[:m.value].tolist()
    assert d["keys"][:190] == sources.tolist() and d["keys"][190:] == sorted(d["keys"][190:]) and set(d["keys"][190:]) <= set(extra.tolist())
    rows = np.repeat(np.arange(n.value), np.diff(d["begin"]))
    idx = np.array(d["node_idx"])
    assert np.all((np.diff(idx) >= 0) | (np.diff(rows) != 0)) and np.any((np.diff(idx) == 0) & (np.diff(rows) == 0))   # sorted, with repeats
    assert sorted(d["e_idx2idx"]) == list(range(m.value)) and d["e_idx2idx"] != list(range(m.value))


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(host_built, tmp_path):
    """The reference's bc_adj_main.cc and common_main.h, untouched and compiled where they lie, build and link against
    this tree's gm.h / gm_util.h / gm_file_handling.h / generated/bc_adj.h / libraries."""
    exe = str(tmp_path / "bc_adj")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "bc_adj_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)       # no args: usage line, exit(1)
    assert r.returncode == 1 and USAGE in r.stdout


def test_both_comp_bc_headers_in_one_unit(host_built, tmp_path):
    src = tmp_path / "both.cc"
    src.write_text('#include "bc.h"\n#include "bc_adj.h"\n'
                   "int main() { void (*a)(gm_graph&, float*) = comp_BC; void (*b)(gm_graph&, float*, gm_node_seq&) = comp_BC; return a && b ? 0 : 1; }\n")
    subprocess.check_call(["g++"] + CXX_FLAGS + [str(src), "-o", str(tmp_path / "both")] + LINK)


def test_driver_is_built_and_prints_usage(host_built):
    exe = os.path.join(PKG, "bin", "bc_adj")
    assert os.path.exists(exe), "bin/bc_adj not built"
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and USAGE in r.stdout


def test_loader_under_sanitizers(tmp_path):
    """The checker and the host library's sources as ONE stand-alone program built with -fsanitize=address,undefined (the
    device calls gm_graph.cc refers to are stubs in the checker): the fixtures and a generated file, no report."""
    exe = str(tmp_path / "adj_loader_check_san")
    srcs = sorted(os.path.join(PKG, "gm_graph", "src", f) for f in os.listdir(os.path.join(PKG, "gm_graph", "src")) if f.endswith(".cc"))
    subprocess.check_call(["g++", "-g", "-O1", "-fopenmp", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DADJ_CHECK_STUBS",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "gm_graph", "inc"), CHECKER] + srcs + ["-o", exe])
    gen = str(tmp_path / "gen.adj")
    generated_file(gen)
    for path in (os.path.join(GOLD, "very_small_sample.adj"), os.path.join(GOLD, "cpp_be_test.adj"), gen):
        for vs, es in (("d", "d"), ("i", "l"), ("-", "-")):
            r = subprocess.run([exe, path, vs, es, str(tmp_path / "d.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0 and "adj loader ok" in r.stdout and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]


def bc_adj_literal(og):
    """bc_adj.gm:5-29 with one thread, in float32: `For (s: G.Nodes)` in node order; InBFS(v != s) sigma = Sum over UpNbrs
    in reverse-row slot order; InReverse(v != s) delta = Sum over DownNbrs in row slot order, BC += delta."""
    f = np.float32
    N = og.N
    bc = np.zeros(N, f)
    for s in range(N):
        level = np.full(N, -1)
        level[s] = 0
        order = [s]
        for v in order:
            for e in range(og.begin[v], og.begin[v + 1]):
                u = og.node_idx[e]
                if level[u] < 0:
                    level[u] = level[v] + 1
                    order.append(u)
        sigma, delta = np.zeros(N, f), np.zeros(N, f)
        sigma[s] = 1
        for v in order[1:]:
            acc = f(0)
            for e in range(og.r_begin[v], og.r_begin[v + 1]):
                w = og.r_node_idx[e]
                if level[w] == level[v] - 1:
                    acc = f(acc + sigma[w])
            sigma[v] = acc
        for v in order[:0:-1]:
            acc = f(0)
            for e in range(og.begin[v], og.begin[v + 1]):
                w = og.node_idx[e]
                if level[w] == level[v] + 1:
                    acc = f(acc + f(f(sigma[v] / sigma[w]) * f(f(1) + delta[w])))
            delta[v] = acc
            bc[v] = f(bc[v] + acc)
    return bc


def test_oracle_bc_over_every_vertex_is_bc_adj_gm(golden):
    """bc_adj.gm against gm_oracle.c's gmo_bc (oracle/gm_oracle.c:613-665).  .gm:7 `G.BC = 0` is :621; .gm:9
    `For (s: G.Nodes)` is the seed loop :622 over seeds = 0 .. N-1, sequential and in node order; .gm:13-14 are :624-625;
    .gm:17-20 `InBFS (v != s) v.sigma = Sum(w: v.UpNbrs) w.sigma` is :639-649 with skip_root (the filter: :641); .gm:21-26
    `InReverse (v != s) v.delta = Sum(w: v.DownNbrs) v.sigma / w.sigma * (1 + w.delta); v.BC += v.delta` is :651-662 (the
    filter: :653).  So comp_BC(G, BC) = po.bc(g, range(V), skip_root=True): checked here against a literal restatement of
    the .gm, and the order of the sources matters because every `BC +=` is a rounded float add."""
    for name in ("hand_tutorial5", "hand_multi_edge", "hand_self_loop", "hand_adj_cpp_be_test", "hand_star64", "rmat6_perm"):
        c = golden["cases"][name]
        og = po.Graph(len(c["begin"]) - 1, c["begin"].copy(), c["node_idx"].copy(), c["r_begin"].copy(), c["r_node_idx"].copy())
        every = np.arange(og.N, dtype=np.int32)
        assert same_f32(po.bc(og, every, True), bc_adj_literal(og)), name
    og = graph("rmat10")
    every = np.arange(og.N, dtype=np.int32)
    fwd, rev = po.bc(og, every, True), po.bc(og, every[::-1].copy(), True)
    assert not np.isnan(fwd).any() and fwd.any()
    assert int((fwd.view(np.uint32) != rev.view(np.uint32)).sum()) >= 100 and np.allclose(fwd, rev, rtol=1e-4)
