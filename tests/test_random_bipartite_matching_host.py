"""random_bipartite_matching (apps/src/random_bipartite_matching.gm) on the host: the program as written, run as one thread runs
it (rbm_literal: the arbiter), and the max / max formulation with the live list that the device implements (rbm_model,
gmx_match.hip), shown equal on hand-made cases, seeded random bipartite multigraphs and the named graphs; independent properties
of the result (involution, left-to-right pairs, maximality), pinned totals, and the plumbing of the entry (header, library,
binding, drop-in header, driver).

The reference ships no generated random_bipartite_matching.cc and no driver, so nothing reference-compiled exists for this
program and no such fixture is used: the literal loop below is the statement-by-statement transcription of the .gm, and where
it disagrees with anything else here, it wins."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_communities_host import named_graph

PKG = os.path.join(ROOT, "green-marl_amd")
NIL = -1


# ------------------------------------------------------------------ the program as written
def rbm_literal(begin, node_idx, is_left):
    """(count, Match[V], rounds, proposals) of the .gm's loop as one thread runs it: Foreach visits vertices in ascending id and
    a row in slot order, so the last writer of t.Suitor wins.  rounds (iterations that made a proposal) and proposals (executions
    of `t.Suitor = n`) are counted on the side; everything else is the program's own statements, three loops per round."""
    begin, node_idx = np.asarray(begin).tolist(), np.asarray(node_idx).tolist()
    is_left = [bool(x) for x in np.asarray(is_left).tolist()]
    V = len(begin) - 1
    count = 0
    finished = False
    match = [NIL] * V                                        # G.Match = NIL;
    suitor = [NIL] * V                                       # G.Suitor = NIL;
    rounds = proposals = 0
    while not finished:                                      # While (!finished) {
        finished = True
        for n in range(V):                                   # Foreach(n: G.Nodes)(n.isLeft && n.Match == NIL)
            if is_left[n] and match[n] == NIL:
                for s in range(begin[n], begin[n + 1]):      # Foreach(t: n.Nbrs)(t.Match == NIL)
                    t = node_idx[s]
                    if match[t] == NIL:
                        suitor[t] = n                        # intended write-write conflict
                        finished &= False
                        proposals += 1
        for t in range(V):                                   # Foreach(t: G.Nodes)(!t.isLeft && t.Match == NIL)
            if not is_left[t] and match[t] == NIL:
                if suitor[t] != NIL:
                    n = suitor[t]
                    suitor[n] = t
                    suitor[t] = NIL
        for n in range(V):                                   # Foreach(n: G.Nodes)(n.isLeft && n.Match == NIL)
            if is_left[n] and match[n] == NIL:
                if suitor[n] != NIL:
                    t = suitor[n]
                    match[n] = t
                    match[t] = n
                    count += 1
        rounds += 0 if finished else 1
    return count, np.asarray(match, np.int32).reshape(V), rounds, proposals


# ------------------------------------------------------------------ the max / max formulation (what the device runs)
def rbm_model(begin, node_idx, is_left):
    """(count, Match[V], rounds, proposals, slots): per round every unmatched right takes the LARGEST unmatched left with an edge to
    it, every left the LARGEST right that took it.  The live list holds the lefts with a non-empty row, then the unmatched lefts
    that proposed in the round before; slots sums the row lengths of the live lefts over all rounds, the last one (which proposes
    nothing) included.  A left -> left edge raises ValueError."""
    begin = np.asarray(begin, np.int64)
    node_idx = np.asarray(node_idx, np.int64)
    left = np.asarray(is_left) != 0
    V = len(begin) - 1
    deg = np.diff(begin)
    src = np.repeat(np.arange(V, dtype=np.int64), deg)
    bad = left[src] & left[node_idx] if len(node_idx) else np.zeros(0, bool)
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        raise ValueError("edge %d -> %d joins two left vertices" % (src[e], node_idx[e]))
    match = np.full(V, NIL, np.int64)
    live = np.flatnonzero(left & (deg > 0))
    count = rounds = proposals = slots = 0
    while len(live):
        d = deg[live]
        idx = np.repeat(begin[live] - np.concatenate([[0], np.cumsum(d)[:-1]]), d) + np.arange(int(d.sum()))
        slots += len(idx)
        n, t = src[idx], node_idx[idx]
        ok = match[t] == NIL
        if not ok.any():
            break
        rounds += 1
        proposals += int(ok.sum())
        n, t = n[ok], t[ok]
        suitor = np.full(V, NIL, np.int64)
        np.maximum.at(suitor, t, n)
        tt = np.flatnonzero(suitor != NIL)
        reply = np.full(V, NIL, np.int64)
        np.maximum.at(reply, suitor[tt], tt)
        nn = np.flatnonzero(reply != NIL)
        match[nn] = reply[nn]
        match[reply[nn]] = nn
        count += len(nn)
        proposed = np.zeros(V, bool)
        proposed[n] = True
        live = live[(match[live] == NIL) & proposed[live]]
    return count, match.astype(np.int32), rounds, proposals, slots


# ------------------------------------------------------------------ graphs (shared with the device tests)
def csr_of(V, src, dst):
    """Forward CSR with the edges in the order given (src non-decreasing): slot i is edge i."""
    src = np.asarray(src, np.int64)
    assert np.all(np.diff(src) >= 0)
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), np.asarray(dst, np.int32)


def cover(begin, node_idx):
    """The bipartite double cover H of G: 2 V vertices, v < V is left and keeps G's row v with every target shifted by + V,
    V .. 2 V - 1 are right with empty rows.  Returns (begin, node_idx, is_left) of H."""
    begin = np.asarray(begin, np.int32)
    V = len(begin) - 1
    b = np.concatenate([begin, np.full(V, begin[V], np.int32)]).astype(np.int32)
    left = np.zeros(2 * V, np.uint8)
    left[:V] = 1
    return b, (np.asarray(node_idx, np.int64) + V).astype(np.int32), left


def staircase(k):
    """lefts 0 .. k-1, left i has an edge to the rights k .. k+i: every round matches one pair, (k-1, 2k-1) first."""
    s = np.repeat(np.arange(k), np.arange(1, k + 1))
    d = np.concatenate([k + np.arange(i + 1) for i in range(k)])
    left = np.zeros(2 * k, np.uint8)
    left[:k] = 1
    return csr_of(2 * k, s, d) + (left,)


def fanin(k):
    """k lefts, one right (vertex k): every proposal hits one address."""
    left = np.ones(k + 1, np.uint8)
    left[k] = 0
    return csr_of(k + 1, np.arange(k), np.full(k, k)) + (left,)


# name: (V, src, dst, is_left)
HAND = {
    "empty": (5, [], [], [1, 0, 1, 0, 0]),
    "one_edge": (3, [0], [2], [1, 0, 0]),
    "duplicates": (4, [0, 0, 0, 2, 2], [1, 1, 3, 3, 3], [1, 0, 1, 0]),
    "two_rights_one_left": (4, [0, 1, 1], [2, 2, 3], [1, 1, 0, 0]),
    "neighbours_taken": (7, [0, 1, 2, 2, 3, 3, 3], [6, 4, 4, 5, 4, 5, 6], [1, 1, 1, 1, 0, 0, 0]),
    "right_rows_ignored": (5, [0, 2, 2, 3, 4, 4], [3, 0, 4, 3, 1, 2], [1, 1, 0, 0, 0]),
    "interleaved": (8, [0, 0, 2, 2, 4, 6, 6, 6], [1, 3, 3, 5, 5, 1, 5, 7], [1, 0, 1, 0, 1, 0, 1, 0]),
}
LEFT_TO_LEFT = (4, [0, 0, 1], [2, 1, 3], [1, 1, 0, 0])      # slot 1 is 0 -> 1
COVERS = ["star33", "chain4096", "path4096", "planted16", "rmat8", "rmat10", "rmat10p", "rmat12"]
NAMED = COVERS + ["staircase64"]
_GRAPHS, _LIT, _MODEL = {}, {}, {}


def rbm_graph(name):
    """(begin, node_idx, is_left) of a hand case, `staircase<k>`, `fanin<k>` or the cover of a named graph."""
    if name not in _GRAPHS:
        if name in HAND:
            V, s, d, left = HAND[name]
            g = csr_of(V, s, d) + (np.asarray(left, np.uint8),)
        elif name.startswith("staircase"):
            g = staircase(int(name[9:]))
        elif name.startswith("fanin"):
            g = fanin(int(name[5:]))
        else:
            g = cover(*named_graph(name))
        for a in g:
            a.setflags(write=False)
        _GRAPHS[name] = g
    return _GRAPHS[name]


def literal_of(name):
    """rbm_literal, computed once per graph and shared between the tests (this file's and the device's)."""
    if name not in _LIT:
        _LIT[name] = rbm_literal(*rbm_graph(name))
        _LIT[name][1].setflags(write=False)
    return _LIT[name]


def model_of(name):
    if name not in _MODEL:
        _MODEL[name] = rbm_model(*rbm_graph(name))
        _MODEL[name][1].setflags(write=False)
    return _MODEL[name]


def random_bipartite(seed):
    """Up to 40 vertices, the sides interleaved at random, left -> right edges with repeats; every other seed adds rows to right
    vertices (to either side, self loops included), which the program never reads."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(2, 41))
    left = (rng.random(V) < rng.uniform(0.2, 0.8)).astype(np.uint8)
    L, R = np.flatnonzero(left), np.flatnonzero(left == 0)
    s, d = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if len(L) and len(R):
        E = int(rng.integers(0, 4 * V + 1))
        s, d = rng.choice(L, E), rng.choice(R, E)
        if seed % 2:
            k = int(rng.integers(0, V + 1))
            rs = rng.choice(R, k)
            rd = np.where(rng.random(k) < 0.3, rs, rng.integers(0, V, k))
            s, d = np.concatenate([s, rs]), np.concatenate([d, rd])
    o = np.argsort(s, kind="stable")
    return csr_of(V, s[o], d[o]) + (left,)


def same(lit, model):
    return lit[0] == model[0] and np.array_equal(lit[1], model[1]) and lit[2:4] == model[2:4]


# ------------------------------------------------------------------ the definition on hand-made cases
def run(name):
    lit, model = literal_of(name), model_of(name)
    assert same(lit, model), name
    return lit[0], lit[1].tolist(), lit[2], lit[3], model[4]


def test_empty_and_one_edge():
    assert run("empty") == (0, [-1] * 5, 0, 0, 0)
    assert run("one_edge") == (1, [2, -1, 0], 1, 1, 1)
    assert rbm_model([0], [], [])[:1] + rbm_model([0], [], [])[2:] == (0, 0, 0, 0)   # V = 0
    assert rbm_literal([0], [], [])[0] == 0


def test_duplicate_slots_are_harmless():
    # round 1: 1 <- {0, 0}, 3 <- {0, 2, 2} = 2; left 0 takes 1, left 2 takes 3
    assert run("duplicates") == (2, [1, 0, 3, 2], 1, 5, 5)


def test_two_rights_choose_one_left():
    # rights 2 and 3 both take left 1; it keeps the higher right, 2 stays for round 2 and goes to left 0
    assert run("two_rights_one_left") == (2, [2, 3, 0, 1], 2, 4, 4)


def test_left_whose_neighbours_are_taken_leaves_the_live_list():
    # rounds match (3, 6), (2, 5), (1, 4).  Left 0 has only right 6: it proposes in round 1, is read in round 2 (no proposal) and
    # is gone in round 3: slots 7 + 4 + 1 (with left 0 still live it would be 13)
    assert run("neighbours_taken") == (3, [-1, 4, 5, 6, 1, 2, 3], 3, 11, 12)


def test_rows_of_right_vertices_are_ignored():
    # rights 2, 3, 4 have rows (to lefts, to a right, a self loop 3 -> 3): only 0 -> 3 is read; left 1 has no row
    assert run("right_rows_ignored") == (1, [3, -1, -1, 0, -1], 1, 1, 1)


def test_interleaved_sides():
    # lefts 0 2 4 6, rights 1 3 5 7.  Round 1: 1 <- 6, 3 <- 2, 5 <- 6, 7 <- 6: left 6 takes 7, left 2 takes 3.  Round 2: left 0
    # proposes to 1, left 4 to 5
    assert run("interleaved") == (4, [1, 0, 3, 2, 5, 4, 7, 6], 2, 10, 11)


def test_left_to_left_edge_raises():
    V, s, d, left = LEFT_TO_LEFT
    with pytest.raises(ValueError, match="0 -> 1"):
        rbm_model(*csr_of(V, s, d), left)


# ------------------------------------------------------------------ model = literal
@pytest.mark.parametrize("block", range(5))
def test_model_is_the_literal_loop_on_random_multigraphs(block):
    for seed in range(block * 60, block * 60 + 60):          # 300 graphs
        g = random_bipartite(seed)
        assert same(rbm_literal(*g), rbm_model(*g)), seed


@pytest.mark.parametrize("name", NAMED)
def test_model_is_the_literal_loop(name):
    lit, model = literal_of(name), model_of(name)
    print("random_bipartite_matching %s: count %d rounds %d proposals %d slots %d" % ((name,) + lit[:1] + lit[2:] + model[4:]))
    assert same(lit, model)
    assert model[3] <= model[4]


@pytest.mark.parametrize("name", NAMED)
def test_properties(name):
    begin, node_idx, left = rbm_graph(name)
    count, match, _, _ = literal_of(name)
    V = len(begin) - 1
    m = np.flatnonzero(match != NIL)
    assert np.array_equal(match[match[m]], m)                # an involution on the matched
    assert len(m) == 2 * count
    src = np.repeat(np.arange(V), np.diff(begin))
    lr = left[src] != 0
    src, dst = src[lr], np.asarray(node_idx)[lr]
    assert not left[dst].any()                               # the precondition
    edges = set(zip(src.tolist(), dst.tolist()))
    ml = m[left[m] != 0]
    assert len(ml) == count and all((int(n), int(match[n])) in edges for n in ml)   # every pair is a left -> right edge
    assert not np.any((match[src] == NIL) & (match[dst] == NIL))                     # maximal


# count / rounds / proposals
PINNED = {"rmat8": (163, 3, 4635), "rmat10": (572, 4, 18741), "rmat10p": (555, 4, 21643), "rmat12": (1989, 4, 76086),
          "planted16": (955, 13, 99183), "chain4096": (4095, 1, 4095), "path4096": (4095, 1, 8190), "star33": (2, 1, 64),
          "staircase64": (64, 64, 45760)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_totals(name):
    lit = literal_of(name)
    assert (lit[0], lit[2], lit[3]) == PINNED[name]


def test_pinned_rmat14_by_the_model():
    count, _, rounds, proposals, slots = model_of("rmat14")
    print("random_bipartite_matching rmat14: slots %d" % slots)
    assert (count, rounds, proposals) == (6888, 4, 297857)


def test_rmat12_has_a_row_longer_than_a_tile():
    assert int(np.diff(rbm_graph("rmat12")[0]).max()) == 2376


# ------------------------------------------------------------------ plumbing
def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gmx_random_bipartite_matching\s*\(\s*gmx_graph_t\s*\*\s*g\s*,\s*const\s+uint8_t\s*\*\s*is_left_host\s*,"
                     r"\s*gmx_node_t\s*\*\s*match_host\s*,\s*int32_t\s*\*\s*count\s*,\s*gmx_stats_t\s*\*\s*stats\s*\)", hdr)
    assert "gmx_random_bipartite_matching" in gmx.EXPORTS
    assert hasattr(gmx.lib(), "gmx_random_bipartite_matching")
    assert hasattr(gmx.Graph, "random_bipartite_matching")
    gen = open(os.path.join(PKG, "generated", "random_bipartite_matching.h")).read()
    assert "#ifndef GM_GENERATED_CPP_RANDOM_BIPARTITE_MATCHING_H" in gen
    assert re.search(r"\bint32_t\s+random_bipartite_matching\s*\(\s*gm_graph&\s*G\s*,\s*bool\s*\*\s*G_isLeft\s*,\s*node_t\s*\*\s*G_Match\s*\)", gen)
    exe = os.path.join(PKG, "bin", "random_bipartite_matching")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout
