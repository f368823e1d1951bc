"""v_cover (apps/src/v_cover.gm) on the host: the program as written, run as one thread runs it (v_cover_literal: the arbiter),
and the cursor formulation the device implements (v_cover_ref, gmx_vcover.hip), shown equal on hand-made cases, seeded random
multigraphs and the named graphs; independent properties of the result, pinned totals, the counter bounds that make the work
O(E), and the plumbing of the entry (header, library, binding, drop-in header, driver).

Measured here with v_cover_ref: rounds chain4096 2048, star33 2; the cut (remain <= 0 with picks left) fires on cut6 and on
both unsorted multigraphs, which carry self loops."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tc_directed_host import MULTI, tcd_graph

PKG = os.path.join(ROOT, "green-marl_amd")
INF = (1 << 31) - 1


# ------------------------------------------------------------------ the program as written
def edges_of(begin, node_idx):
    begin = np.asarray(begin, np.int64)
    V = len(begin) - 1
    return V, np.repeat(np.arange(V, dtype=np.int64), np.diff(begin)), np.asarray(node_idx, np.int64)


def v_cover_literal(begin, node_idx):
    """(covered, select[E], [(max_val, slot) ...]) of the .gm's loop with the one-thread tie rule: s ascending, slots ascending,
    update on strict > only, i.e. the first maximum -- which is what np.argmax returns."""
    V, src, dst = edges_of(begin, node_idx)
    E = len(dst)
    deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
    cov = np.zeros(V, bool)
    select = np.zeros(E, bool)
    picks = []
    remain = 2 * E
    while remain > 0:
        key = deg[src] + deg[dst]
        key[cov[src] & cov[dst]] = 0          # filtered out: max_val starts at 0 and only a strictly larger key replaces it
        e = int(np.argmax(key))
        max_val = int(key[e])
        assert max_val > 0                    # remain <= the degree sum left: some edge still has an uncovered end
        remain -= max_val
        s, t = int(src[e]), int(dst[e])
        deg[s] = deg[t] = 0
        select[e] = True
        cov[s] = cov[t] = True
        picks.append((max_val, e))
    return int(cov.sum()), select, picks


# ------------------------------------------------------------------ the cursor formulation (what the device runs)
def v_cover_ref(begin, node_idx):
    """(covered, select[E], kept picks [(key, slot) ...] in the loop's order, rounds, counters) of the parallel schedule:
    every round picks the edges that are the best edge of each of their uncovered ends; the best edge of a vertex is found
    with a forward-only cursor into its incident list sorted by (Deg0 of the other end descending, slot ascending); a vertex
    is evaluated again only when the other end of its best edge was covered by another edge."""
    V, src, dst = edges_of(begin, node_idx)
    E = len(dst)
    deg0 = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
    slots = np.arange(E, dtype=np.int64)
    owner = np.concatenate([src, dst])
    other = np.concatenate([dst, src])
    slot = np.concatenate([slots, slots])
    o = np.lexsort((slot, -deg0[other], owner))
    L = 2 * E
    off = np.concatenate([[0], np.cumsum(deg0)]).tolist()
    ent_x, ent_s = other[o].tolist(), slot[o].tolist()
    low = [min(range(off[v], off[v + 1]), key=lambda i: (ent_s[i], i)) if off[v + 1] > off[v] else -1 for v in range(V)]
    deg0 = deg0.tolist()
    cov = [INF] * V
    cur = off[:V]
    bent, bkey, bslot = [-1] * V, [0] * V, [-1] * V
    stamp = [1] * V
    active = [v for v in range(V) if deg0[v] > 0]
    picks = []                                 # (key, slot, u, x)
    skips = evals = walks = rounds = 0
    r = 1
    while active:
        rounds += 1
        for u in active:                       # evaluate
            c, end = cur[u], off[u + 1]
            while c < end and cov[ent_x[c]] != INF:
                c += 1
            skips += c - cur[u]
            evals += 1
            cur[u] = c
            b = c if c < end else low[u]
            bent[u], bslot[u] = b, ent_s[b]
            bkey[u] = deg0[u] + (deg0[ent_x[b]] if c < end else 0)
        newly = []
        for u in active:                       # pick (reads the cover of the rounds before: cov < r)
            x = ent_x[bent[u]]
            if x == u or cov[x] < r:
                rec, addx = True, False
            elif (bkey[x], bslot[x]) == (bkey[u], bslot[u]):
                rec = addx = not (stamp[x] == r and x < u)
            else:
                rec = addx = False
            if rec:
                picks.append((bkey[u], bslot[u], u, x))
                cov[u] = r
                newly.append(u)
                if addx:
                    cov[x] = r
                    newly.append(x)
        r += 1
        active = []
        for v in newly:                        # activate
            for i in range(off[v], off[v + 1]):
                walks += 1
                w = ent_x[i]
                if cov[w] == INF and bslot[w] == ent_s[i] and stamp[w] != r:
                    stamp[w] = r
                    active.append(w)
    picks.sort(key=lambda p: (-p[0], p[1]))    # the loop's order; replay remain and cut
    remain = 2 * E
    kept = []
    for p in picks:
        if remain <= 0:
            break
        remain -= p[0]
        kept.append(p)
    select = np.zeros(E, bool)
    done = set()
    for _, s, u, x in kept:
        select[s] = True
        done.update((u, x))
    ctr = {"skips": skips, "evals": evals, "walks": walks, "picks": len(picks), "kept": len(kept), "L": L, "V": V}
    return len(done), select, [(k, s) for k, s, _, _ in kept], rounds, ctr


# ------------------------------------------------------------------ graphs (shared with the device tests)
def csr_of(V, src, dst):
    """Forward CSR with the edges in the order given (src non-decreasing): slot i is edge i."""
    src = np.asarray(src, np.int64)
    assert np.all(np.diff(src) >= 0)
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), np.asarray(dst, np.int32)


TINY = {
    "empty": (5, [], []),
    "one_edge": (3, [0], [2]),
    "self_loop": (2, [1], [1]),
    "two_cycle": (2, [0, 1], [1, 0]),
    "duplicates": (3, [0, 0, 0, 1], [1, 1, 2, 2]),
    "cut6": (6, [1, 3, 4, 4, 5, 5], [1, 3, 1, 4, 1, 4]),
}
NAMED = ["star33", "chain4096", "path4096", "planted16", "rmat8", "rmat10", "rmat12", "rmat10p"] + sorted(MULTI)
_REF, _LIT = {}, {}


def vc_graph(name):
    if name in TINY:
        return csr_of(*TINY[name])
    return tcd_graph(name)


def ref_of(name):
    """v_cover_ref, computed once per named graph and shared between the tests (this file's and the device's)."""
    if name not in _REF:
        _REF[name] = v_cover_ref(*vc_graph(name))
        _REF[name][1].setflags(write=False)
    return _REF[name]


def literal_of(name):
    if name not in _LIT:
        _LIT[name] = v_cover_literal(*vc_graph(name))
        _LIT[name][1].setflags(write=False)
    return _LIT[name]


def random_multigraph(seed):
    """Up to 40 vertices; every other seed is self-loop heavy (30-40 % of the edges)."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 41))
    E = int(rng.integers(0, 4 * V + 1))
    s = np.sort(rng.integers(0, V, E))
    d = rng.integers(0, V, E)
    if seed % 2:
        loops = rng.random(E) < rng.uniform(0.3, 0.4)
        d = np.where(loops, s, d)
    return csr_of(V, s, d)


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ------------------------------------------------------------------ the definition on tiny graphs
def test_tiny_cases():
    def run(name):
        lit, ref = literal_of(name), ref_of(name)
        assert same(lit, ref), name
        return lit[0], np.flatnonzero(lit[1]).tolist()
    assert run("empty") == (0, [])
    assert run("one_edge") == (2, [0])
    assert run("self_loop") == (1, [0])
    assert run("two_cycle") == (2, [0])                      # slot 0 wins the tie, the other edge stays unselected
    assert run("duplicates") == (3, [0, 2])                  # of the repeated edge 0 -> 1 the lower slot; then 0 -> 2 before 1 -> 2
    cov, sel = run("star33")
    assert (cov, len(sel)) == (33, 32) and ref_of("star33")[3] == 2
    assert run("cut6") == (2, [0, 3])                        # vertices 3 and 5 stay uncovered: remain ran out first
    assert ref_of("cut6")[4]["picks"] == 4 and ref_of("cut6")[4]["kept"] == 2


def test_duplicates_are_separate_slots():
    b, i = vc_graph("duplicates")
    _, sel, picks = v_cover_literal(b, i)
    assert picks[0] == (6, 0) and not sel[1]                 # Deg = (3, 3, 2): slots 0 and 1 tie at 6


@pytest.mark.parametrize("block", range(6))
def test_formulation_is_the_literal_loop_on_random_multigraphs(block):
    for seed in range(block * 60, block * 60 + 60):          # 360 graphs, half of them self-loop heavy
        b, i = random_multigraph(seed)
        assert same(v_cover_literal(b, i), v_cover_ref(b, i)[:3]), seed


@pytest.mark.parametrize("name", NAMED)
def test_formulation_is_the_literal_loop(name):
    lit, ref = literal_of(name), ref_of(name)
    print("v_cover %s: covered %d selected %d rounds %d %s" % (name, lit[0], int(lit[1].sum()), ref[3], ref[4]))
    assert same(lit, ref)


def test_the_cut_fires():
    fired = [n for n in list(TINY) + NAMED if ref_of(n)[4]["kept"] < ref_of(n)[4]["picks"]]
    print("cut fires on", fired)
    assert "cut6" in fired and any(n in fired for n in NAMED)
    for n in fired:                                          # ... and only where there are self loops
        V, s, d = edges_of(*vc_graph(n))
        assert np.any(s == d)


@pytest.mark.parametrize("name", NAMED)
def test_properties(name):
    b, i = vc_graph(name)
    V, src, dst = edges_of(b, i)
    covered, select, picks = literal_of(name)
    seen = np.zeros(V, bool)
    for _, e in picks:                                       # every selected edge had an uncovered end when it was picked
        assert not (seen[src[e]] and seen[dst[e]])
        seen[src[e]] = seen[dst[e]] = True
    assert int(select.sum()) == len(picks) <= covered
    assert covered == len(np.union1d(src[select], dst[select])) == int(seen.sum())
    if not np.any(src == dst):                               # without self loops the loop runs until every edge is covered
        touched = np.zeros(V, bool)
        touched[src] = touched[dst] = True
        assert np.array_equal(seen, touched)
    assert [k for k, _ in picks] == sorted((k for k, _ in picks), reverse=True)   # max_val never rises


PINNED = {"rmat8": (232, 170), "rmat10": (884, 648), "rmat12": (3365, 2534), "chain4096": (4096, 2049), "star33": (33, 32)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_totals(name):
    covered, select, _ = literal_of(name)
    assert (covered, int(select.sum())) == PINNED[name]


def test_pinned_rmat14_by_the_formulation():
    covered, select, _, rounds, ctr = ref_of("rmat14")
    print("v_cover rmat14: rounds %d %s" % (rounds, ctr))
    assert (covered, int(select.sum())) == (12661, 9716)


@pytest.mark.parametrize("name", NAMED + ["rmat14"])
def test_counter_bounds(name):
    """The cursor only moves forward, every list is walked once, and every evaluation after the first is caused by one walked
    entry: the work is O(L + V) whatever the number of rounds."""
    c = ref_of(name)[4]
    assert c["L"] == 2 * len(vc_graph(name)[1])
    assert c["skips"] <= c["L"] and c["walks"] <= c["L"] and c["evals"] <= c["L"] + c["V"]


# ------------------------------------------------------------------ plumbing
def test_entry_is_declared_exported_bound_and_built():
    """Fails without the feature, on any box: the header, the library, the binding, the drop-in header and the driver."""
    import gmx
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gmx_v_cover\s*\(\s*gmx_graph_t\s*\*\s*g\s*,\s*uint8_t\s*\*\s*select_host\s*,\s*int32_t\s*\*\s*covered\s*,", hdr)
    assert "gmx_v_cover" in gmx.EXPORTS
    assert hasattr(gmx.lib(), "gmx_v_cover")
    assert hasattr(gmx.Graph, "v_cover")
    gen = open(os.path.join(PKG, "generated", "v_cover.h")).read()
    assert "#ifndef GM_GENERATED_CPP_V_COVER_H" in gen
    assert re.search(r"\bint32_t\s+v_cover\s*\(\s*gm_graph&\s*G\s*,\s*bool\s*\*\s*G_select\s*\)", gen)
    exe = os.path.join(PKG, "bin", "v_cover")
    assert os.path.exists(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)          # no args: usage line, exit(EXIT_FAILURE)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout


REF_APPS = "/root/reference/apps/output_cpp/src"


@pytest.mark.skipif(not os.path.isdir(REF_APPS), reason="reference tree not present (GPU box)")
def test_reference_driver_compiles_unchanged(tmp_path):
    """The reference's own v_cover_main.cc builds and links against this tree's headers and libraries."""
    from test_host_cpp import CXX_FLAGS, LINK
    subprocess.check_call(["make", "-C", PKG, "-j4", "lib", "host"], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "v_cover")
    flags = [f for f in CXX_FLAGS if "apps" not in f]   # the reference's common_main.h, not ours
    subprocess.check_call(["g++"] + flags + ["-I" + REF_APPS, "-w", os.path.join(REF_APPS, "v_cover_main.cc"), "-o", exe] + LINK)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "<graph_name> <num_threads>" in r.stdout
