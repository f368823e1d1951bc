"""communities.gm's result contract restated on the host (no GPU): label propagation with the canonical tie rule (the
smallest label among the most frequent, taken only when the vertex's own label is not among them), the canonical
schedule (two half-rounds per round, halves drawn by a murmur3 finaliser of vertex and round) and the fixpoint checker.
The device tests (test_gpu_communities.py) compare gmx_communities with communities_ref array for array.  Also: the
entry is declared, exported, bound and built."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
from conftest import GOLD, ROOT

PKG = os.path.join(ROOT, "green-marl_amd")
M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3's 32-bit finaliser on an array (uint64 arithmetic masked to 32 bits)."""
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def half_of(V, r):
    """h(v, r) for v = 0 .. V-1."""
    salt = np.uint64((r * 0x9E3779B9) & 0xFFFFFFFF)
    return (fmix32(np.arange(V, dtype=np.uint64) ^ salt) & np.uint64(1)).astype(np.int64)


def row_votes(begin, node_idx, comm, rows=None):
    """Per vertex of `rows` (a mask; None: all): (max count over its row, smallest label with that count, count of the
    vertex's own label).  Rows without slots get (0, -1, 0)."""
    V = len(begin) - 1
    begin = np.asarray(begin, np.int64)
    deg = np.diff(begin)
    src = np.repeat(np.arange(V, dtype=np.int64), deg)
    lab = np.asarray(comm, np.int64)[np.asarray(node_idx, np.int64)]
    if rows is not None:
        keep = rows[src]
        src, lab = src[keep], lab[keep]
    key, cnt = np.unique(src * V + lab, return_counts=True)
    ks, kl = key // V, key % V
    mx = np.zeros(V, np.int64)
    np.maximum.at(mx, ks, cnt)
    best = np.full(V, -1, np.int64)
    top = cnt == mx[ks]
    # keys ascend by (vertex, label): the first top entry of a vertex is its smallest label
    v_first, first = np.unique(ks[top], return_index=True)
    best[v_first] = kl[top][first]
    own = np.zeros(V, np.int64)
    me = np.arange(V, dtype=np.int64) * V + np.asarray(comm, np.int64)
    at = np.searchsorted(key, me)
    hit = (at < len(key))
    hit[hit] = key[at[hit]] == me[hit]
    own[hit] = cnt[at[hit]]
    return mx, best, own


def is_fixpoint(begin, node_idx, comm):
    """Every vertex with out-neighbours holds a label whose count over its row is the row's maximum."""
    mx, _, own = row_votes(begin, node_idx, comm)
    return bool(np.all(own == mx))


def communities_ref(begin, node_idx, max_rounds=1000):
    """(comm[int32], rounds, converged) under the canonical schedule."""
    V = len(begin) - 1
    comm = np.arange(V, dtype=np.int32)
    deg = np.diff(np.asarray(begin, np.int64))
    rounds = 0
    for r in range(max_rounds):
        h = half_of(V, r)
        changed = 0
        for half in (0, 1):
            rows = (h == half) & (deg > 0)
            mx, best, own = row_votes(begin, node_idx, comm, rows)
            move = rows & (own != mx)
            changed += int(move.sum())
            comm[move] = best[move]            # one snapshot: all of the half-round's labels are committed together
        if changed == 0:
            break
        rounds += 1
    return comm, rounds, int(is_fixpoint(begin, node_idx, comm))


# ------------------------------------------------------------------ graphs (shared with the device tests)

def csr(V, src, dst):
    """Forward CSR of an edge list, rows in input order."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    o = np.argsort(src, kind="stable")
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), dst[o].astype(np.int32)


def star(n):
    c = np.arange(1, n)
    return n, np.concatenate([np.zeros(n - 1, np.int64), c]), np.concatenate([c, np.zeros(n - 1, np.int64)])


def chain(n):
    return n, np.arange(n - 1), np.arange(1, n)


def undirected_path(n):
    a = np.arange(n - 1)
    return n, np.concatenate([a, a + 1]), np.concatenate([a + 1, a])


def uniform_symmetric(V=65536, draws=3, seed=7):
    rng = np.random.default_rng(seed)
    s = np.repeat(np.arange(V), draws)
    d = rng.integers(0, V, V * draws)
    return V, np.concatenate([s, d]), np.concatenate([d, s])


def planted(k=16, size=64, density=0.3, cross=200, seed=5):
    """k dense blocks (each ordered pair inside a block drawn with `density`) plus `cross` random edges, symmetrised and
    without repeats or self loops."""
    rng = np.random.default_rng(seed)
    V = k * size
    s, d = [], []
    for b in range(k):
        m = rng.random((size, size)) < density
        i, j = np.nonzero(m)
        s.append(b * size + i)
        d.append(b * size + j)
    s.append(rng.integers(0, V, cross))
    d.append(rng.integers(0, V, cross))
    s, d = np.concatenate(s), np.concatenate(d)
    a, b = np.concatenate([s, d]), np.concatenate([d, s])
    keep = a != b
    key = np.unique(a[keep] * V + b[keep])
    return V, key // V, key % V


_REF = {}


def ref_of(name, begin, node_idx, max_rounds=1000):
    """communities_ref, computed once per named graph and bound and shared between the tests."""
    k = (name, max_rounds)
    if k not in _REF:
        c, r, cv = communities_ref(begin, node_idx, max_rounds)
        c.setflags(write=False)
        _REF[k] = (c, r, cv)
    return _REF[k]


_GRAPHS = {}


def named_graph(name):
    """(begin, node_idx) of the graphs both test files use."""
    if name not in _GRAPHS:
        if name.startswith("rmat"):          # rmat<scale>[p][s]: permuted / symmetrised
            m = re.match(r"rmat(\d+)(p?)(s?)$", name)
            og = po.rmat_graph(int(m.group(1)), permute=bool(m.group(2)))
            if m.group(3):
                og = po.symmetrize(og)
            _GRAPHS[name] = (og.begin, og.node_idx)
        else:
            V, s, d = {"star33": lambda: star(33), "chain4096": lambda: chain(4096), "path4096": lambda: undirected_path(4096),
                       "uniform": uniform_symmetric, "planted16": planted,
                       "planted64": lambda: planted(64, 128, 0.15, 3000, 9)}[name]()
            _GRAPHS[name] = csr(V, s, d)
    return _GRAPHS[name]


def check_labels(begin, node_idx, comm):
    V = len(begin) - 1
    assert len(comm) == V
    if V:
        assert comm.min() >= 0 and comm.max() < V            # labels are always vertex ids


# ------------------------------------------------------------------ hand graphs

def run(V, src, dst, max_rounds=1000):
    b, i = csr(V, src, dst)
    return communities_ref(b, i, max_rounds) + (b, i)


def test_star_ends_with_one_label():
    comm, rounds, conv, b, i = run(*star(33))
    assert len(set(comm.tolist())) == 1 and conv == 1 and is_fixpoint(b, i, comm)
    assert rounds <= 4


def test_two_cycle():
    """Synchronous rounds swap the two labels for ever; the half-rounds end with one label after one round.  Which one
    follows from the schedule: fmix32(0) = 0, so vertex 0 is in half 0 of round 0, moves first and adopts 1 (fmix32(1) is
    odd: vertex 1 is evaluated after that commit and keeps its label)."""
    assert half_of(2, 0).tolist() == [0, 1]
    comm, rounds, conv, b, i = run(2, [0, 1], [1, 0])
    assert comm.tolist() == [1, 1] and conv == 1 and rounds == 1 and is_fixpoint(b, i, comm)


def test_vertex_without_out_edges_keeps_its_id():
    comm, _, conv, _, _ = run(4, [0, 1], [3, 3])
    assert comm[3] == 3 and comm[2] == 2 and comm[0] == 3 and comm[1] == 3 and conv == 1


def test_most_frequent_label_wins():
    # 0 -> [2, 2, 1]; 1, 2, 3 have no out-edges and keep their ids
    comm, _, conv, _, _ = run(4, [0, 0, 0], [2, 2, 1])
    assert comm.tolist() == [2, 1, 2, 3] and conv == 1


def test_tie_takes_the_smallest_unless_own_label_is_among_them():
    # 0 -> [1, 2]: tied, takes 1.  3 -> [1, 2] too; a vertex that already holds 2 keeps it
    b, i = csr(4, [0, 0, 3, 3], [1, 2, 1, 2])
    mx, best, own = row_votes(b, i, np.array([0, 1, 2, 2]))
    assert mx[0] == 1 and best[0] == 1 and own[0] == 0
    assert mx[3] == 1 and best[3] == 1 and own[3] == 1       # own label 2 is among the most frequent: no move
    comm, _, conv = communities_ref(b, i)
    assert comm[0] == 1 and comm[3] == 1 and conv == 1
    assert is_fixpoint(b, i, np.array([1, 1, 2, 2])) and not is_fixpoint(b, i, np.array([0, 1, 2, 2]))


def test_self_loop_counts():
    # 0 -> [0, 0, 1]: its own label has the highest count through the self loops
    comm, rounds, conv, _, _ = run(2, [0, 0, 0], [0, 0, 1])
    assert comm.tolist() == [0, 1] and rounds == 0 and conv == 1
    # 0 -> [0, 1, 1]: the self loop counts once, 1 twice
    comm, _, conv, _, _ = run(2, [0, 0, 0], [0, 1, 1])
    assert comm.tolist() == [1, 1] and conv == 1


def test_halves_follow_the_formula():
    def scalar(v, r):
        h = (v ^ ((r * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        return h & 1
    for r in (0, 1, 7, 1000):
        assert half_of(64, r).tolist() == [scalar(v, r) for v in range(64)]
    assert 0 < half_of(4096, 0).sum() < 4096


# ------------------------------------------------------------------ larger graphs

@pytest.mark.parametrize("name,k,size", [("planted16", 16, 64), ("planted64", 64, 128)])
def test_planted_partition_is_recovered(name, k, size):
    b, i = named_graph(name)
    comm, rounds, conv = ref_of(name, b, i)
    print("communities %s: %d rounds" % (name, rounds))
    assert conv == 1 and rounds <= 12
    blocks = comm.reshape(k, size)
    assert (blocks == blocks[:, :1]).all()                    # one label per block
    assert len(np.unique(blocks[:, 0])) == k                  # and k different ones
    assert (blocks[:, 0] // size == np.arange(k)).all()       # each the id of a member


def test_schedule_converges_where_synchronous_rounds_do_not():
    b, i = named_graph("uniform")
    comm, rounds, conv = ref_of("uniform", b, i)
    print("communities uniform: %d rounds" % rounds)
    assert conv == 1 and rounds <= 32 and is_fixpoint(b, i, comm)
    b, i = named_graph("path4096")
    comm, rounds, conv = ref_of("path4096", b, i)
    assert conv == 1 and rounds <= 32


def test_chain_is_cut_by_max_rounds():
    b, i = named_graph("chain4096")
    comm, rounds, conv = ref_of("chain4096", b, i, 16)
    assert conv == 0 and rounds == 16 and not is_fixpoint(b, i, comm)
    comm0, rounds0, conv0 = communities_ref(b, i, 0)
    assert np.array_equal(comm0, np.arange(4096)) and rounds0 == 0 and conv0 == 0


def test_golden_cases_reach_a_fixpoint(golden):
    for name, c in sorted(golden["cases"].items()):
        comm, rounds, conv = ref_of("golden/" + name, c["begin"], c["node_idx"])
        assert conv == 1 and is_fixpoint(c["begin"], c["node_idx"], comm), name
        check_labels(c["begin"], c["node_idx"], comm)


@pytest.mark.parametrize("name", ["rmat8", "rmat8p", "rmat10", "rmat10p", "rmat12", "rmat12p"])
def test_rmat_reaches_a_fixpoint(name):
    b, i = named_graph(name)
    comm, rounds, conv = ref_of(name, b, i)
    print("communities %s: %d rounds, %d labels" % (name, rounds, len(np.unique(comm))))
    assert conv == 1 and rounds <= 32 and is_fixpoint(b, i, comm)
    check_labels(b, i, comm)


# ------------------------------------------------------------------ plumbing

def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gmx_communities\s*\(", hdr)
    assert "gmx_communities" in gmx.EXPORTS
    assert hasattr(gmx.lib(), "gmx_communities")
    assert hasattr(gmx.Graph, "communities")
    gen = open(os.path.join(PKG, "generated", "communities.h")).read()
    assert re.search(r"\bvoid\s+communities\s*\(\s*gm_graph&\s*G\s*,\s*node_t\s*\*", gen)
    exe = os.path.join(PKG, "bin", "communities")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout


REF_APPS = "/root/reference/apps/output_cpp/src"


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(tmp_path):
    """The reference's own communities_main.cc builds and links against this tree's headers and libraries."""
    from test_host_cpp import CXX_FLAGS, LINK
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "communities")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "communities_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout
