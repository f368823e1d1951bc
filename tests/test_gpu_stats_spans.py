"""The h2d_ms / kernel_ms / d2h_ms fields of gmx_stats_t, for every whole-algorithm entry point at once: which of the
three an entry fills (> 0) and which it leaves at the zero of its memset (== 0).

One tiny graph -- a directed ring on 96 vertices plus about 300 random chords, its symmetrised and its bipartite form where
an entry needs one -- goes through every entry once.  EXPECT was taken from the library before the entries shared one span
timer (two runs of collect() on the device; a field is listed only where both runs agreed), so it pins what each field
covered then: a span that is lost, or a field that is written without its span having been begun, shows here.  The
results themselves are checked in each entry's own test file."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 96
POS, ZERO = "> 0", "== 0"
FIELDS = ("h2d_ms", "kernel_ms", "d2h_ms")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def sorted_csr(n, src, dst):
    """Forward CSR of the distinct edges without self loops, rows and targets ascending."""
    keep = src != dst
    e = np.unique(np.stack([src[keep], dst[keep]], 1), axis=0)
    begin = np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]).astype(np.int32)
    return begin, e[:, 1].astype(np.int32)


def ring_with_chords():
    rng = np.random.default_rng(96)
    ring = np.arange(V)
    return (np.concatenate([ring, rng.integers(0, V, 300)]), np.concatenate([(ring + 1) % V, rng.integers(0, V, 300)]))


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def pf_counts(g):
    g.potential_friend_counts()
    return g.last_stats


def adamic_adar(g):
    g.adamic_adar()
    return g.last_stats


def route_query(g, w):
    r = g.route(w)
    try:
        return r.query(0, V // 2)[-1]
    finally:
        r.free()


def pagerank(g, dtype, ranks):
    if ranks == 1:
        return g.pagerank(0.001, 0.85, 100, dtype)[1]
    with env(GMX_PR_RANKS=str(ranks)):
        return g.pagerank(0.001, 0.85, 100, dtype)[1]


def collect(gmx):
    """name -> stats of one call of every entry.  Every graph is uploaded afresh: no entry finds another's cached plan."""
    src, dst = ring_with_chords()
    b, i = sorted_csr(V, src, dst)
    sb, si = sorted_csr(V, np.concatenate([src, dst]), np.concatenate([dst, src]))
    left = np.arange(V) % 2 == 0
    lr = left[src] & ~left[dst]
    bb, bi = sorted_csr(V, src[lr], dst[lr])
    rng = np.random.default_rng(7)
    E = len(i)
    w = rng.integers(1, 10, E).astype(np.int32)
    cost = rng.random(E) + 0.5
    age = rng.integers(5, 40, V).astype(np.int32)
    member = rng.integers(0, 2, V).astype(np.int32)
    sw = rng.integers(1, 10, len(si)).astype(np.int32)
    seeds = np.array([0, 17, 50], np.int32)
    fresh = lambda: gmx.Graph.upload(b, i)
    sym = lambda: gmx.Graph.upload(sb, si)
    out = {}
    calls = [
        ("triangle_counting", lambda: sym().triangle_counting()[1]),
        ("triangle_counting_cn", lambda: sym().triangle_counting_cn()[1]),
        ("adamic_adar", lambda: adamic_adar(fresh())),
        ("avg_teen_cnt", lambda: fresh().avg_teen_cnt(age, 10)[2]),
        ("conduct", lambda: fresh().conduct(member, 1)[1]),
        ("hop_dist", lambda: fresh().hop_dist(0)[1]),
        ("bc", lambda: fresh().bc(seeds)[1]),
        ("bc_batch", lambda: fresh().bc_batch(seeds)[1]),
        ("bc_all", lambda: fresh().bc_all()[1]),
        ("sssp", lambda: fresh().sssp(w, 0)[1]),
        ("sssp_path", lambda: fresh().sssp_path(w, 0)[3]),
        ("sssp_path_f64", lambda: fresh().sssp_path_f64(cost, 0)[3]),
        ("bidir_dijkstra", lambda: fresh().bidir_dijkstra(w, 0, V // 2)[3]),
        ("route_query", lambda: route_query(fresh(), w)),
        ("scc", lambda: fresh().scc()[2]),
        ("wcc", lambda: fresh().wcc()[2]),
        ("communities", lambda: sym().communities()[3]),
        ("kcore", lambda: sym().kcore("in")[2]),
        ("msf", lambda: sym().msf(sw)[3]),
        ("coloring", lambda: sym().coloring()[2]),
        ("closeness", lambda: fresh().closeness("out")[4]),
        ("random_bipartite_matching", lambda: gmx.Graph.upload(bb, bi).random_bipartite_matching(left)[2]),
        ("v_cover", lambda: fresh().v_cover()[2]),
        ("potential_friends", lambda: fresh().potential_friends()[2]),
        ("potential_friends_sizing", lambda: pf_counts(fresh())),
        ("triangle_counting_directed", lambda: fresh().triangle_counting_directed()[1]),
        ("clustering", lambda: fresh().clustering()[5]),
        ("random_walk_sampling", lambda: fresh().random_walk_sampling(0.3, 0.15, 16, 12345)[5]),
        ("node_sampling", lambda: fresh().node_sampling(0, 20, 12345)[3]),
        ("degree_node_sampling", lambda: fresh().node_sampling(1, 20, 12345)[3]),
        ("pagerank_f32", lambda: pagerank(fresh(), np.float32, 1)),
        ("pagerank_f64", lambda: pagerank(fresh(), np.float64, 1)),
        ("pagerank_f32_2ranks", lambda: pagerank(fresh(), np.float32, 2)),
        ("pagerank_f64_2ranks", lambda: pagerank(fresh(), np.float64, 2)),
    ]
    for name, call in calls:
        out[name] = call()
    return out


# entry -> (h2d_ms, kernel_ms, d2h_ms).  The two runs agreed on every field of every entry: none is left out.  (coloring's
# h2d_ms is positive without priorities too: its span then encloses nothing, and two events still lie a few microseconds apart.)
EXPECT = {
    "triangle_counting": (ZERO, POS, ZERO),
    "triangle_counting_cn": (ZERO, POS, ZERO),
    "adamic_adar": (ZERO, POS, POS),
    "avg_teen_cnt": (ZERO, POS, ZERO),
    "conduct": (ZERO, POS, ZERO),
    "hop_dist": (ZERO, POS, POS),
    "bc": (ZERO, POS, ZERO),
    "bc_batch": (ZERO, POS, ZERO),
    "bc_all": (ZERO, POS, ZERO),
    "sssp": (POS, POS, ZERO),
    "sssp_path": (POS, POS, POS),
    "sssp_path_f64": (POS, POS, POS),
    "bidir_dijkstra": (POS, POS, POS),
    "route_query": (ZERO, POS, POS),
    "scc": (ZERO, POS, POS),
    "wcc": (ZERO, POS, POS),
    "communities": (ZERO, POS, POS),
    "kcore": (ZERO, POS, POS),
    "msf": (POS, POS, POS),
    "coloring": (POS, POS, POS),
    "closeness": (POS, POS, POS),
    "random_bipartite_matching": (POS, POS, POS),
    "v_cover": (ZERO, POS, POS),
    "potential_friends": (ZERO, POS, POS),
    "potential_friends_sizing": (ZERO, POS, POS),
    "triangle_counting_directed": (ZERO, POS, ZERO),
    "clustering": (ZERO, POS, POS),
    "random_walk_sampling": (ZERO, POS, POS),
    "node_sampling": (ZERO, POS, POS),
    "degree_node_sampling": (ZERO, POS, POS),
    "pagerank_f32": (ZERO, POS, POS),
    "pagerank_f64": (ZERO, POS, POS),
    "pagerank_f32_2ranks": (ZERO, POS, POS),
    "pagerank_f64_2ranks": (ZERO, POS, POS),
}


@pytest.fixture(scope="module")
def stats(gmx):
    return collect(gmx)


def test_every_entry_is_in_the_table(stats):
    assert sorted(stats) == sorted(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_spans(stats, name):
    st = stats[name]
    print(name, {f: st[f] for f in FIELDS})
    for f, want in zip(FIELDS, EXPECT[name]):
        if want == POS:
            assert st[f] > 0, (name, f, st)
        else:
            assert want == ZERO and st[f] == 0, (name, f, st)


def test_potential_friends_batches_accumulate(gmx):
    """Three or more batches: kernel_ms and d2h_ms are the sizing pass plus one lap per batch, each added to the sum."""
    src, dst = ring_with_chords()
    g = gmx.Graph.upload(*sorted_csr(V, src, dst))
    with env(GMX_PF_BATCH_BYTES="512"):
        pb, pi, st = g.potential_friends()
    _, pi1, _ = g.potential_friends()
    assert np.array_equal(pi, pi1)
    print("batches", st)
    assert st["iterations"] >= 3
    assert st["kernel_ms"] > 0 and st["d2h_ms"] > 0 and st["h2d_ms"] == 0


def test_copy_bandwidth(gmx):
    assert gmx.copy_bandwidth(1 << 22, 2) > 0
