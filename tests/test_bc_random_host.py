"""bc_random / gmx_bc_batch, host side (no GPU): the entry is declared, bound and exported; the reference's own
bc_random_main.cc builds against this tree; bin/bc_random exists; gm_graph::pick_random_node() is libc's rand(); and the
premise of batching -- comp_BC over a seed sequence is the per-seed deltas accumulated into BC in seed order over the
vertices each seed reaches, and the order matters -- pinned on the oracle.  test_gpu_bc_batch.py uses the graphs and seeds."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT
from test_host_cpp import CXX_FLAGS, LINK, PKG, REF_APPS, host_built  # noqa: F401  (host_built: a fixture)

INT_MAX = 2147483647
GRAPHS = {"rmat10": (10, False), "rmat12p": (12, True), "rmat14": (14, False)}
NSEEDS = 70


def same_f32(a, b):
    """float32 arrays equal bit for bit, any NaN counting as NaN (its sign / payload is the platform's)."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


@functools.lru_cache(maxsize=None)
def graph(name):
    scale, permute = GRAPHS[name]
    return po.rmat_graph(scale, permute=permute)


@functools.lru_cache(maxsize=None)
def seeds_of(name):
    """70 seeds: default_rng(scale) draws; 0 and 1 the top-out-degree vertex (a duplicate), 2 a vertex without out-edges."""
    og = graph(name)
    deg = np.diff(og.begin)
    s = np.random.default_rng(GRAPHS[name][0]).integers(0, og.N, NSEEDS).astype(np.int32)
    s[0] = s[1] = int(np.argmax(deg))
    s[2] = int(np.flatnonzero(deg == 0)[0])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def oracle_bc(name, n, skip):
    out = po.bc(graph(name), seeds_of(name)[:n], skip)
    out.setflags(write=False)
    return out


def libc_draws(n, modulo, seed=1):
    libc = ctypes.CDLL(None)
    libc.srand(seed)
    return [libc.rand() % modulo for _ in range(n)]


def test_entry_declared_bound_and_exported():
    import gmx
    hdr = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert re.search(r"\bint gmx_bc_batch\(gmx_graph_t\* g, const gmx_node_t\* seeds, int32_t nseeds, int skip_root,\s*int32_t width,", hdr)
    assert "gmx_bc_batch" in gmx.EXPORTS
    if not os.path.exists(gmx.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(gmx.lib(), "gmx_bc_batch")
    assert callable(getattr(gmx.Graph, "bc_batch"))


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(host_built, tmp_path):
    """The reference's bc_random_main.cc and common_main.h, untouched and compiled where they lie, build and link against
    this tree's gm.h / generated/bc_random.h / libraries (the recipe of test_host_cpp's drop-in check)."""
    exe = str(tmp_path / "bc_random")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "bc_random_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)       # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout


def test_driver_is_built_and_prints_usage(host_built):
    exe = os.path.join(PKG, "bin", "bc_random")
    assert os.path.exists(exe), "bin/bc_random not built"
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout


def test_pick_random_node_is_libc_rand(host_built, tmp_path):
    """Ten pick_random_node() calls on a 256-vertex graph after srand(1) are rand() % 256 (gm_graph.h:389-391); the
    expected draws come from libc here, not from a table."""
    exe = str(tmp_path / "pick_random_check")
    subprocess.check_call(["g++"] + CXX_FLAGS + [os.path.join(ROOT, "tests", "cpp", "pick_random_check.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout
    assert [int(x) for x in r.stdout.split()] == libc_draws(10, 256)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_oracle_bc_is_in_order_accumulation_of_per_seed_deltas(name):
    """po.bc(g, seeds, skip) == BC built one seed at a time: BC[v] = BC[v] + delta_s[v] over the vertices s reaches (with
    skip_root not s itself), in seed order, in float32 -- what a batch's accumulate does column by column.  With the
    seed order reversed the float sums round differently (skip_root form; the literal form holds only 0 and NaN)."""
    og, seeds = graph(name), seeds_of(name)
    assert seeds[0] == seeds[1] and og.begin[seeds[2] + 1] == og.begin[seeds[2]]
    for skip in (False, True):
        acc = np.zeros(og.N, np.float32)
        for s in seeds:
            delta = po.bc(og, np.array([s], np.int32), skip)
            mask = po.bfs_queue(og, int(s)) != INT_MAX
            if skip:
                mask[s] = False
            acc[mask] = acc[mask] + delta[mask]
        assert same_f32(acc, oracle_bc(name, NSEEDS, skip)), skip
    fwd = oracle_bc(name, NSEEDS, True)
    rev = po.bc(og, seeds[::-1].copy(), True)
    assert not np.isnan(fwd).any() and int((fwd.view(np.uint32) != rev.view(np.uint32)).sum()) >= 100
