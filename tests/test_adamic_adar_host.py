"""adamicAdar.gm restated on the host, twice: over the oracle's common-neighbour iterator (pinned on the reference's class),
slot by slot in Python, and vectorised in numpy for the larger graphs the device tests use.  The two must agree bit for
bit.  Also: the reference's own adamicAdar_main.cc builds unchanged against this tree, and the entry is exported."""
import math
import os
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT

PKG = os.path.join(ROOT, "green-marl_amd")
REF_APPS = "/root/reference/apps/output_cpp/src"


def term(deg):
    """1.0 / log((double) deg) as IEEE double gives it: -0.0 for deg 0 (1 / -inf), +inf for deg 1 (1 / +0.0)."""
    if deg == 0:
        return -0.0
    if deg == 1:
        return math.inf
    return 1.0 / math.log(float(deg))


def term_table(begin):
    """term() of every out-degree that occurs, indexed by degree (math.log, not numpy's: one libm for both restatements)."""
    deg = np.diff(np.asarray(begin, np.int64))
    t = np.zeros(int(deg.max(initial=0)) + 1, np.float64)
    for d in np.unique(deg):
        t[d] = term(int(d))
    return deg, t


def aa_by_iterator(g, slots=None):
    """(aa, k) per forward slot (all, or the given ones): the terms of the iterator's items added in its order, from +0.0."""
    deg = np.diff(g.begin.astype(np.int64))
    src = np.repeat(np.arange(g.N), deg)
    slots = np.arange(g.M) if slots is None else np.asarray(slots)
    aa, k = np.zeros(len(slots), np.float64), np.zeros(len(slots), np.int64)
    for i, e in enumerate(slots):
        items = po.common_nbrs(g, int(src[e]), int(g.node_idx[e]))
        acc = 0.0
        for n in items:
            acc += term(int(deg[n]))
        aa[i], k[i] = acc, len(items)
    return aa, k


def _expand(counts):
    """For counts c: (which entry, position inside it) of sum(c) items, entry by entry."""
    counts = np.asarray(counts, np.int64)
    which = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return which, np.arange(int(counts.sum())) - first[which]


def aa_vectorised(begin, node_idx, slots=None, chunk=1 << 24):
    """The same numbers without a Python loop per item.  Rows must be sorted.  For a slot (from -> to) the shorter of the
    two rows is walked: row(from)'s slots are looked up in row(to), or row(to)'s distinct values are located in row(from)
    and every slot of their run counts.  The hits (slot e, slot j of row(from)) are then ordered by (e, j) and added one
    after the other (np.bincount adds in array order), so the sum runs in row(from)'s slot order like the iterator's."""
    begin = np.asarray(begin, np.int64)
    node_idx = np.asarray(node_idx, np.int64)
    V, E = len(begin) - 1, len(node_idx)
    deg, table = term_table(begin)
    src = np.repeat(np.arange(V, dtype=np.int64), deg)
    key = src * V + node_idx                      # sorted, because the rows are: (row, value) of every slot
    slots = np.arange(E, dtype=np.int64) if slots is None else np.asarray(slots, np.int64)
    aa, k = np.zeros(len(slots), np.float64), np.zeros(len(slots), np.int64)
    frm, to = src[slots], node_idx[slots]
    da, db = deg[frm], deg[to]
    work = np.minimum(da, db)
    if len(slots) == 0:
        return aa, k
    part = (np.cumsum(work) - work) // chunk       # pieces of about `chunk` candidates (a slot is never split)
    bounds = [0] + (np.flatnonzero(np.diff(part)) + 1).tolist() + [len(slots)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sel = np.arange(lo, hi)
        walk_from = da[sel] <= db[sel]
        he, hj = [], []
        a = sel[walk_from]                         # every slot j of row(from): is (to, value) a slot of the graph?
        which, pos = _expand(da[a])
        j = begin[frm[a]][which] + pos
        probe = to[a][which] * V + node_idx[j]
        at = np.searchsorted(key, probe)
        hit = (at < E) & (key[np.minimum(at, E - 1)] == probe)
        he.append(a[which][hit])
        hj.append(j[hit])
        b = sel[~walk_from]                        # every distinct value of row(to): its run in row(from)
        which, pos = _expand(db[b])
        p = begin[to[b]][which] + pos
        x = node_idx[p]
        distinct = (pos == 0) | (node_idx[np.maximum(p - 1, 0)] != x)
        which, x = which[distinct], x[distinct]
        probe = frm[b][which] * V + x
        r_lo, r_hi = np.searchsorted(key, probe, "left"), np.searchsorted(key, probe, "right")
        w2, pos2 = _expand(r_hi - r_lo)
        he.append(b[which][w2])
        hj.append(r_lo[w2] + pos2)
        he, hj = np.concatenate(he), np.concatenate(hj)
        order = np.lexsort((hj, he))
        he, hj = he[order], hj[order]
        aa[lo:hi] = np.bincount(he - lo, weights=table[deg[node_idx[hj]]], minlength=hi - lo)
        k[lo:hi] = np.bincount(he - lo, minlength=hi - lo)
    return aa, k


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def example_multigraph():
    """The example of the reference's gm_common_neighbor_iter.h:11-14 with s = 0, t = 1, a .. d = 2 .. 5, the edges s -> t
    and t -> s added, and out-degrees a: 1, b: 2, c: 3, d: 0."""
    s, t, a, b, c, d = range(6)
    src = [s, s, s, s, s, t, t, t, t, t, t, a, b, b, c, c, c]
    dst = [t, a, b, b, c, s, b, b, b, c, d, s, s, t, s, t, a]
    return po.graph_from_edges(6, src, dst)


def k3():
    return po.graph_from_edges(3, [0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1])


def golden_graphs(golden):
    for name, c in sorted(golden["cases"].items()):
        yield name, po.Graph(len(c["begin"]) - 1, c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])


def test_restatements_agree_on_golden_graphs(golden):
    for name, g in golden_graphs(golden):
        want, wk = aa_by_iterator(g)
        for chunk in (1 << 24, 64):
            got, gk = aa_vectorised(g.begin, g.node_idx, chunk=chunk)
            assert same_bits(got, want), name
            assert np.array_equal(gk, wk), name
        assert not np.isnan(want).any()


def test_restatements_agree_on_a_sample_of_slots(golden):
    c = golden["cases"]["rmat10_noperm"]
    g = po.Graph(1024, c["begin"], c["node_idx"], c["r_begin"], c["r_node_idx"])
    slots = np.random.default_rng(5).choice(g.M, 700, replace=False)
    want, wk = aa_by_iterator(g, slots)
    got, gk = aa_vectorised(g.begin, g.node_idx, slots)
    assert same_bits(got, want) and np.array_equal(gk, wk)


def test_multigraph_example_both_directions():
    g = example_multigraph()
    assert g.node_idx[g.begin[0]:g.begin[1]].tolist() == [1, 2, 3, 3, 4]
    assert g.node_idx[g.begin[1]:g.begin[2]].tolist() == [0, 3, 3, 3, 4, 5]
    assert po.common_nbrs(g, 0, 1).tolist() == [3, 3, 4]
    assert po.common_nbrs(g, 1, 0).tolist() == [3, 3, 3, 4]
    want, wk = aa_by_iterator(g)
    got, gk = aa_vectorised(g.begin, g.node_idx)
    assert same_bits(got, want) and np.array_equal(gk, wk)
    b, c = 1.0 / math.log(2.0), 1.0 / math.log(3.0)
    assert want[g.begin[0]] == (0.0 + b + b) + c and wk[g.begin[0]] == 3          # s -> t
    assert want[g.begin[1]] == ((0.0 + b) + b + b) + c and wk[g.begin[1]] == 4    # t -> s
    assert want[g.begin[0] + 2] == want[g.begin[0] + 3]                            # the two slots s -> b


def test_k3_every_edge_is_one_over_ln2():
    g = k3()
    want, wk = aa_by_iterator(g)
    got, _ = aa_vectorised(g.begin, g.node_idx)
    assert same_bits(got, want)
    assert wk.tolist() == [1] * 6
    assert want.tolist() == [1.0 / math.log(2.0)] * 6


def test_special_values():
    # 0 -> 1, 0 -> 2, 1 -> 2, 2 -> 3: the edge 0 -> 1 has the common neighbour 2 of out-degree 1
    g = po.graph_from_edges(4, [0, 0, 1, 2], [1, 2, 2, 3])
    for aa, k in (aa_by_iterator(g), aa_vectorised(g.begin, g.node_idx)):
        assert aa[0] == math.inf and k[0] == 1
        assert aa[1:].tolist() == [0.0, 0.0, 0.0] and not np.signbit(aa[1:]).any() and k[1:].tolist() == [0, 0, 0]
    # 0 -> 1, 0 -> 2, 1 -> 2: the common neighbour 2 has out-degree 0 and contributes -0.0; the sum stays +0.0
    g = po.graph_from_edges(3, [0, 0, 1], [1, 2, 2])
    for aa, k in (aa_by_iterator(g), aa_vectorised(g.begin, g.node_idx)):
        assert aa.tolist() == [0.0, 0.0, 0.0] and not np.signbit(aa).any() and k.tolist() == [1, 0, 0]
    assert term(0) == 0.0 and math.copysign(1.0, term(0)) == -1.0 and term(1) == math.inf


def test_exported():
    import gmx
    assert "gmx_adamic_adar" in gmx.EXPORTS
    assert "gmx_adamic_adar" in open(os.path.join(ROOT, "include", "gmx.h")).read()


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(tmp_path):
    """The recipe of test_host_cpp.test_reference_drivers_compile_unchanged for adamicAdar_main.cc."""
    from test_host_cpp import CXX_FLAGS, LINK
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "adamicAdar")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    cmd = ["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "adamicAdar_main.cc"), "-o", exe] + LINK
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)       # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout


def test_own_driver_is_built():
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = os.path.join(PKG, "bin", "adamicAdar")
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads> <nfspath>" in r.stdout
