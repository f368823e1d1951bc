"""sssp_path.gm's result contract restated on the host (no GPU): the canonical shortest-path tree of a given dist[] -- per
vertex the smallest positive-length tight in-edge slot -- and the checker of the tree property that the device tests
(test_gpu_sssp_path.py) apply to what gmx_sssp_path returns.  Both are exercised here on the committed fixtures and on RMAT
graphs with the oracle's sssp as dist[].  Also: the entry is declared, exported, bound and built."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT

INT_MAX = 2147483647
PKG = os.path.join(ROOT, "green-marl_amd")


def sources(begin):
    begin = np.asarray(begin, np.int64)
    return np.repeat(np.arange(len(begin) - 1, dtype=np.int64), np.diff(begin))


def tight_slots(begin, node_idx, length, dist):
    """(positive, zero): masks over the slots e = n -> v with dist[n] != INT_MAX and dist[n] + len[e] == dist[v], split by
    len[e] > 0 / len[e] == 0."""
    src, dst = sources(begin), np.asarray(node_idx, np.int64)
    length, d = np.asarray(length, np.int64), np.asarray(dist, np.int64)
    tight = (d[src] != INT_MAX) & (d[src] + length == d[dst])
    return tight & (length > 0), tight & (length == 0)


def canonical_tree(begin, node_idx, length, dist):
    """(prev_node, prev_edge, n_tight, all_positive): per vertex the smallest tight slot of positive length and its source
    (-1: none), how many such slots it has, and whether it has NO tight in-edge of length 0 (where that holds the device
    must return exactly prev_node / prev_edge)."""
    V = len(begin) - 1
    src, dst = sources(begin), np.asarray(node_idx, np.int64)
    pos, zero = tight_slots(begin, node_idx, length, dist)
    slots = np.flatnonzero(pos)                               # in slot order: the first occurrence of a destination is its smallest
    heads, first = np.unique(dst[slots], return_index=True)
    prev_node, prev_edge = np.full(V, -1, np.int32), np.full(V, -1, np.int32)
    prev_edge[heads] = slots[first]
    prev_node[heads] = src[slots[first]]
    n_tight = np.bincount(dst[slots], minlength=V)
    all_positive = np.ones(V, bool)
    all_positive[dst[zero]] = False
    return prev_node, prev_edge, n_tight, all_positive


def check_tree(begin, node_idx, length, dist, prev_node, prev_edge, root):
    """The tree property: NIL for the root and the unreached; otherwise prev_edge[v] is a tight slot into v whose source is
    prev_node[v]; and prev_node leads from every reached vertex to the root (pointer jumping, ceil(log2 V) + 1 doublings)."""
    V, E = len(begin) - 1, len(node_idx)
    dist, prev_node, prev_edge = (np.asarray(a, np.int64) for a in (dist, prev_node, prev_edge))
    assert len(dist) == len(prev_node) == len(prev_edge) == V
    reached = dist != INT_MAX
    nil = ~reached
    if 0 <= root < V:
        assert dist[root] == 0
        nil[root] = True
    else:
        assert not reached.any()
    assert (prev_node[nil] == -1).all() and (prev_edge[nil] == -1).all()
    v = np.flatnonzero(~nil)
    if len(v) == 0:
        return
    pe, pn = prev_edge[v], prev_node[v]
    assert (pe >= 0).all() and (pe < E).all() and (pn >= 0).all() and (pn < V).all()
    src, dst, length = sources(begin), np.asarray(node_idx, np.int64), np.asarray(length, np.int64)
    assert np.array_equal(dst[pe], v)
    assert np.array_equal(src[pe], pn)
    assert (dist[pn] != INT_MAX).all()
    assert np.array_equal(dist[pn] + length[pe], dist[v])     # tight; dist never increases along prev since len >= 0
    up = np.where(prev_node < 0, np.arange(V), prev_node)
    for _ in range(max(1, math.ceil(math.log2(max(V, 2)))) + 1):
        up = up[up]
    assert (up[reached] == root).all()                        # no cycle, not even through zero-length edges


def golden_cases(golden):
    for name, c in sorted(golden["cases"].items()):
        man = golden["manifest"]["rmat"].get(name) or golden["manifest"]["hand"].get(name[len("hand_"):])
        yield name, c, int(man["root"])


def top_hub(og):
    return int(np.argmax(np.diff(og.begin)))


def rmat_case(scale, lo, hi, permute=False):
    """RMAT-<scale>, lengths lo .. hi from default_rng(1), the top hub and the oracle's dist."""
    og = po.rmat_graph(scale, permute=permute)
    length = np.random.default_rng(1).integers(lo, hi + 1, og.M).astype(np.int32)
    root = top_hub(og)
    return og, length, root, po.sssp(og, length, root)[0]


def describe(label, dist, n_tight, all_positive, root):
    reached = dist != INT_MAX
    inner = reached.copy()
    inner[root] = False
    print("sssp_path %s: %d reached, %d with more than one positive tight in-edge, %d with a positive tight in-edge, "
          "%d without a zero-length tight in-edge" % (label, int(reached.sum()), int((n_tight[reached] > 1).sum()),
                                                        int((n_tight[inner] > 0).sum()), int(all_positive[inner].sum())))


def test_canonical_tree_on_golden_cases(golden):
    several = 0
    for name, c, root in golden_cases(golden):
        pn, pe, n_tight, allpos = canonical_tree(c["begin"], c["node_idx"], c["sssp_len"], c["sssp_dist"])
        assert (c["sssp_len"] >= 1).all(), name               # the reference driver's lengths: the whole output is fixed
        assert allpos.all(), name
        check_tree(c["begin"], c["node_idx"], c["sssp_len"], c["sssp_dist"], pn, pe, root)
        several += int((n_tight[c["sssp_dist"] != INT_MAX] > 1).sum())
    assert several >= 1                                       # some vertex has a choice


@pytest.mark.parametrize("scale,lo,hi", [(8, 1, 100), (12, 1, 100), (16, 1, 100), (16, 1, 3)])
def test_canonical_tree_on_rmat(scale, lo, hi):
    og, length, root, dist = rmat_case(scale, lo, hi)
    pn, pe, n_tight, allpos = canonical_tree(og.begin, og.node_idx, length, dist)
    describe("rmat%d len %d..%d" % (scale, lo, hi), dist, n_tight, allpos, root)
    check_tree(og.begin, og.node_idx, length, dist, pn, pe, root)
    assert allpos.all()
    reached = dist != INT_MAX
    assert (n_tight[reached] > 1).any()                       # not vacuous: the smallest slot is a choice somewhere
    # the smallest slot is in the smallest tight predecessor's row
    pos, _ = tight_slots(og.begin, og.node_idx, length, dist)
    src = sources(og.begin)
    lowest = np.full(og.N, og.N, np.int64)
    np.minimum.at(lowest, og.node_idx[pos], src[pos])
    has = n_tight > 0
    assert np.array_equal(lowest[has], pn[has])


def test_zero_lengths_leave_a_checked_share():
    """Lengths 0 .. 2 on RMAT-16 from the top hub: most reached vertices have a zero-length tight in-edge (the weak half of
    the contract); the share that must equal the restatement exactly is what the device test's 10 % floor rests on."""
    og, length, root, dist = rmat_case(16, 0, 2)
    pn, pe, n_tight, allpos = canonical_tree(og.begin, og.node_idx, length, dist)
    describe("rmat16 len 0..2", dist, n_tight, allpos, root)
    reached = dist != INT_MAX
    inner = reached.copy()
    inner[root] = False
    assert (~allpos[inner]).sum() > 0
    assert allpos[inner].sum() >= 0.10 * reached.sum()
    # a vertex without a zero-length tight in-edge has a positive one: there the restatement is itself a tree edge
    assert (n_tight[inner & allpos] > 0).all()


def test_check_tree_refuses_wrong_trees():
    # 0 -> 1 (1), 0 -> 2 (1), 1 -> 3 (1), 2 -> 3 (1), 3 -> 4 (0), 4 -> 3 (0), 5 isolated
    og = po.graph_from_edges(6, [0, 0, 1, 2, 3, 4], [1, 2, 3, 3, 4, 3])
    length = np.array([1, 1, 1, 1, 0, 0], np.int32)
    dist = po.sssp(og, length, 0)[0]
    assert dist.tolist() == [0, 1, 1, 2, 2, INT_MAX]
    pn, pe, n_tight, allpos = canonical_tree(og.begin, og.node_idx, length, dist)
    assert pn.tolist() == [-1, 0, 0, 1, -1, -1] and pe.tolist() == [-1, 0, 1, 2, -1, -1]
    assert n_tight.tolist() == [0, 1, 1, 2, 0, 0] and allpos.tolist() == [True, True, True, False, False, True]
    good_n, good_e = np.array([-1, 0, 0, 1, 3, -1]), np.array([-1, 0, 1, 2, 4, -1])
    check_tree(og.begin, og.node_idx, length, dist, good_n, good_e, 0)
    check_tree(og.begin, og.node_idx, length, dist, np.array([-1, 0, 0, 2, 3, -1]), np.array([-1, 0, 1, 3, 4, -1]), 0)
    bad = [
        (np.array([-1, 0, 0, 4, 3, -1]), np.array([-1, 0, 1, 5, 4, -1])),    # the zero-length two-cycle 3 <-> 4
        (np.array([-1, 0, 0, 1, 3, 0]), np.array([-1, 0, 1, 2, 4, 0])),      # an unreached vertex with a predecessor
        (np.array([0, 0, 0, 1, 3, -1]), np.array([0, 0, 1, 2, 4, -1])),      # the root with a predecessor
        (np.array([-1, 0, 0, 2, 3, -1]), np.array([-1, 0, 1, 2, 4, -1])),    # prev_node is not the slot's source
        (np.array([-1, 0, 0, 1, 3, -1]), np.array([-1, 0, 1, 2, 5, -1])),    # the slot does not lead to the vertex
        (np.array([-1, 0, 0, -1, 3, -1]), np.array([-1, 0, 1, -1, 4, -1])),  # a reached vertex without a predecessor
    ]
    for n, e in bad:
        with pytest.raises(AssertionError):
            check_tree(og.begin, og.node_idx, length, dist, n, e, 0)


def test_path_from_prev():
    import gmx
    prev = np.array([-1, 0, 1, 2, -1], np.int32)
    assert gmx.path_from_prev(prev, 0, 3) == [0, 1, 2, 3]
    assert gmx.path_from_prev(prev, 1, 3) == [1, 2, 3]
    assert gmx.path_from_prev(prev, 0, 4) == [] and gmx.path_from_prev(prev, 0, 0) == []
    with pytest.raises(gmx.GmxError):
        gmx.path_from_prev(prev, 4, 3)


def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gmx_sssp_path\s*\(", hdr)
    assert "gmx_sssp_path" in gmx.EXPORTS
    assert hasattr(gmx.lib(), "gmx_sssp_path")
    assert hasattr(gmx.Graph, "sssp_path") and hasattr(gmx, "path_from_prev")
    gen = open(os.path.join(PKG, "generated", "sssp_path.h")).read()
    assert re.search(r"\bvoid\s+sssp_path\s*\(\s*gm_graph&", gen) and re.search(r"\bvoid\s+get_path\s*\(\s*gm_graph&", gen)
    exe = os.path.join(PKG, "bin", "sssp_path")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout


REF_APPS = "/root/reference/apps/output_cpp/src"


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(tmp_path):
    """sssp_path_main.cc:44-46 calls both procedures: the reference's own driver builds against this tree's headers."""
    from test_host_cpp import CXX_FLAGS, LINK
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "sssp_path")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "sssp_path_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout
