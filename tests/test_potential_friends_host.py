"""potential_friends.gm's result contract restated on the host (no GPU).

    PF(v) = ( union of row(u) over the slots u of row(v) )  minus  row(v)  minus  {v},   ascending

potential_friends_ref is the numpy restatement of that formula the device tests (test_gpu_potential_friends.py) compare
gmx_potential_friends with, array for array; potential_friends_literal is the triple loop of the .gm with all three
filters, and the two agree on small graphs with self loops, repeated slots and unsorted rows.  The reference ships no
generated potential_friends.cc, so there is no reference-compiled fixture for this entry: the literal loop stands in for
it.  Also: the entry is declared, exported, bound and built, and the new host headers compile and behave."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_communities_host import csr, named_graph
from test_upload_forms_host import unsorted_multigraph

PKG = os.path.join(ROOT, "green-marl_amd")


def two_hop_lengths(begin, node_idx):
    """L(v) = sum of outdeg(u) over the slots u of row(v), int64[V], and its running sum over the slots."""
    begin = np.asarray(begin, np.int64)
    deg = np.diff(begin)
    run = np.concatenate([[0], np.cumsum(deg[np.asarray(node_idx, np.int64)])]).astype(np.int64)
    return run[begin[1:]] - run[begin[:-1]], run


def potential_friends_ref(begin, node_idx, lo=0, hi=None):
    """(pf_begin[int64], pf_idx[int32]) for the vertices lo <= v < hi: the set formula, rows ascending.  Vertex chunks whose
    two-hop items are gathered at once; a chunk becomes a rows x V boolean matrix when that is smaller than sorting its
    items, and a sorted list of distinct (row, vertex) keys otherwise."""
    begin = np.asarray(begin, np.int64)
    idx = np.asarray(node_idx, np.int64)
    V = len(begin) - 1
    hi = V if hi is None else hi
    deg = np.diff(begin)
    _, run = two_hop_lengths(begin, idx)
    at_row = run[begin]
    counts, parts = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    v = lo
    while v < hi:
        e = int(min(hi, max(v + 1, np.searchsorted(at_row, at_row[v] + (1 << 22), side="right") - 1)))
        n = e - v
        s0, s1 = begin[v], begin[e]
        u = idx[s0:s1]
        src = np.repeat(np.arange(n, dtype=np.int64), deg[v:e])
        d = deg[u]
        T = int(d.sum())
        w = idx[np.repeat(begin[u], d) + (np.arange(T, dtype=np.int64) - np.repeat(np.cumsum(d) - d, d))]
        r = np.repeat(src, d)
        if n * V <= 4 * T + (1 << 20):
            mat = np.zeros((n, V), bool)
            mat[r, w] = True
            mat[src, u] = False
            mat[np.arange(n), np.arange(v, e)] = False
            counts.append(mat.sum(1).astype(np.int64))
            parts.append(np.nonzero(mat)[1])
        else:
            key = np.unique(r * V + w)
            drop = np.concatenate([src * V + u, np.arange(n, dtype=np.int64) * V + np.arange(v, e)])
            key = key[~np.isin(key, drop)]
            counts.append(np.bincount(key // V, minlength=n).astype(np.int64))
            parts.append(key % V)
        v = e
    pf_begin = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    return pf_begin, np.concatenate(parts).astype(np.int32)


def potential_friends_literal(begin, node_idx, lo=0, hi=None):
    """The .gm as written: Foreach(v) Foreach(u: v.Nbrs)(u != v) Foreach(w: u.Nbrs)(w != u && w != v)
    If (!v.HasEdgeTo(w)) v.potFriend.Add(w); every set iterated in ascending order, as gm_node_set does."""
    begin = [int(x) for x in begin]
    idx = [int(x) for x in node_idx]
    V = len(begin) - 1
    hi = V if hi is None else hi
    pf_begin, pf_idx = [0], []
    for v in range(lo, hi):
        row = idx[begin[v]:begin[v + 1]]
        has_edge_to = set(row)
        pot = set()
        for u in row:
            if u != v:
                for w in idx[begin[u]:begin[u + 1]]:
                    if w != u and w != v:
                        if w not in has_edge_to:
                            pot.add(w)
        pf_idx.extend(sorted(pot))
        pf_begin.append(len(pf_idx))
    return np.array(pf_begin, np.int64), np.array(pf_idx, np.int32)


_REF = {}


def pf_ref_of(name, begin, node_idx):
    """potential_friends_ref over all vertices, computed once per named graph and shared between the tests (read-only)."""
    if name not in _REF:
        b, i = potential_friends_ref(begin, node_idx)
        b.setflags(write=False)
        i.setflags(write=False)
        _REF[name] = (b, i)
    return _REF[name]


def report_lines(pf_begin, pf_idx, V):
    """What the driver prints after its timing lines."""
    out = "potential friends for the first 10 nodes (max. 10 entries per node shown):\n"
    for v in range(min(10, V)):
        row = pf_idx[pf_begin[v]:pf_begin[v + 1]]
        if len(row) == 0:
            continue
        out += "node #%d: {%s%s}\n" % (v, ", ".join(str(int(x)) for x in row[:10]), "..." if len(row) >= 10 else "")
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype == np.int32


# ------------------------------------------------------------------ the restatement against the literal loop

@pytest.mark.parametrize("name", ["star33", "rmat10", "planted16"])
def test_formula_is_the_literal_loop_on_named_graphs(name):
    b, i = named_graph(name)
    assert same(pf_ref_of(name, b, i), potential_friends_literal(b, i))


def test_formula_is_the_literal_loop_on_an_unsorted_multigraph():
    b, i, _, _ = unsorted_multigraph(300, 700, 11)
    ref = potential_friends_ref(b, i)
    assert same(ref, potential_friends_literal(b, i))
    o = np.lexsort((i, np.repeat(np.arange(300), np.diff(b))))      # the same graph with sorted rows: the same sets
    assert same(ref, potential_friends_ref(b, np.asarray(i)[o]))
    assert same(potential_friends_ref(b, i, 17, 203), potential_friends_literal(b, i, 17, 203))


def test_hand_cases():
    def both(V, s, d):
        b, i = csr(V, s, d)
        ref = potential_friends_ref(b, i)
        assert same(ref, potential_friends_literal(b, i))
        return [ref[1][ref[0][v]:ref[0][v + 1]].tolist() for v in range(V)]
    assert both(2, [0, 1], [1, 0]) == [[], []]                                 # directed 2-cycle: 0 -> 1 -> 0 is v itself
    assert both(6, np.arange(5), np.arange(1, 6)) == [[2], [3], [4], [5], [], []]   # directed path
    s, d = np.nonzero(~np.eye(7, dtype=bool))
    assert both(7, s, d) == [[]] * 7                                           # complete graph
    assert both(3, [0, 1], [0, 2]) == [[], [], []]                             # 0's only slot is a self loop
    assert both(4, [0, 0, 2], [1, 2, 3]) == [[3], [], [], []]                  # neighbour 1 has no out-edges
    assert both(4, [0, 0, 0, 1, 1, 1], [1, 1, 0, 2, 2, 3]) == [[2, 3], [], [], []]   # repeats and a self loop add nothing


PINNED = {"star33": (992, 31), "rmat10": (259832, 634), "rmat12": (2355051, 2350), "rmat12s": (4350494, 2800),
          "planted16": (55758, 150), "uniform": (2160708, 96)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_totals(name):
    b, i = named_graph(name)
    pb, pi = pf_ref_of(name, b, i)
    print("potential_friends %s: total %d, largest set %d" % (name, pb[-1], np.diff(pb).max()))
    assert (int(pb[-1]), int(np.diff(pb).max())) == PINNED[name]
    assert len(pi) == pb[-1]
    rows = np.repeat(np.arange(len(pb) - 1), np.diff(pb))
    assert np.all((np.diff(pi) > 0) | (np.diff(rows) > 0))                      # ascending and distinct inside every row


# ------------------------------------------------------------------ plumbing

def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gmx_potential_friends\s*\(", hdr)
    assert "gmx_potential_friends" in gmx.EXPORTS
    assert hasattr(gmx.lib(), "gmx_potential_friends")
    assert hasattr(gmx.Graph, "potential_friends") and hasattr(gmx.Graph, "potential_friend_counts")
    gen = open(os.path.join(PKG, "generated", "potential_friends.h")).read()
    assert re.search(r"\bvoid\s+potential_friends\s*\(\s*gm_graph&\s*G\s*,\s*gm_property_of_collection<gm_node_set>&", gen)
    exe = os.path.join(PKG, "bin", "potential_friends")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout


def test_driver_is_built_by_build():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.exists(os.path.join(PKG, "bin", "potential_friends"))


HEADER_PROGRAM = r"""
#include <stdio.h>
#include "gm.h"
int main() {
    const int V = 50;
    gm_property_of_collection_impl<gm_node_set, false> sets(V);
    gm_property_of_collection_impl<gm_node_set, true> lazy(V);
    gm_property_of_collection<gm_node_set>& prop = sets;
    for (int v = 0; v < V; v++)
        for (int k = 3; k >= 0; k--) {
            prop[v].add((node_t) ((v * 7 + k * 11) % V));
            prop[v].add((node_t) ((v * 7 + k * 11) % V));      // a second add changes nothing
        }
    const node_t sorted[3] = {4, 9, 40};
    prop[5].assign_sorted(sorted, 3);
    lazy[7].assign_sorted(sorted, 2);
    long sum = 0;
    for (int v = 0; v < V; v++) {
        gm_node_set copy = prop[v];                            // the driver iterates a copy
        gm_node_set::seq_iter it = copy.prepare_seq_iteration();
        node_t last = -1;
        int n = 0;
        while (it.has_next()) {
            const node_t x = it.get_next();
            if (x <= last || !prop[v].is_in(x)) return 1;      // ascending, distinct, members
            last = x;
            n++;
            sum += x;
        }
        if (n != (int) prop[v].get_size()) return 2;
    }
    if (prop[5].get_size() != 3 || prop[5].is_in(5) || !prop[5].is_in(40)) return 3;
    if (lazy[7].get_size() != 2 || lazy[8].get_size() != 0) return 4;
    prop[5].clear();
    if (prop[5].get_size() != 0 || prop[5].prepare_seq_iteration().has_next()) return 5;
    printf("sum %ld\n", sum);
    return 0;
}
"""


def test_host_headers_compile_and_iterate_in_order(tmp_path):
    """gm_set.h and gm_property_of_collection.h through gm.h, in a plain program with its own main under the host
    sanitizers."""
    src = tmp_path / "sets.cc"
    src.write_text(HEADER_PROGRAM)
    exe = str(tmp_path / "sets")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "gm_graph", "inc"), "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    want = 0
    for v in range(50):
        s = {(v * 7 + k * 11) % 50 for k in range(4)}
        want += sum((4, 9, 40) if v == 5 else s)
    assert r.returncode == 0 and r.stdout.strip() == "sum %d" % want, r.stdout


REF_APPS = "/root/reference/apps/output_cpp/src"


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(tmp_path):
    """The reference's own potential_friends_main.cc builds and links against this tree's headers and libraries."""
    from test_host_cpp import CXX_FLAGS, LINK
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "potential_friends")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "potential_friends_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout
