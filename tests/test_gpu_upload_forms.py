"""Uploaded CSRs whose rows are out of order, on the device: every entry on every upload form, against the oracle run on
the caller's CSR as stored (test_upload_forms_host.py checks that premise), and the upload's validation of the arrays it
keeps.

Forms (gmx.h): F0 GMX_GRAPH_SORT_ROWS; F1 flags 0 with both CSRs (kept verbatim); F2 GMX_GRAPH_NO_REVERSE (the forward
CSR verbatim); F3 flags 0 without a reverse CSR (sorted on the device, with an e_idx2idx map); F4 SORT_ROWS | NO_REVERSE.
Edge properties are indexed by the caller's slots on every form."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle as po
from test_gpu_parity import INT_MAX, PR_RTOL_F32, PR_RTOL_F64, _bfs_ranks_on_graph, rel_err, same_f32
from test_scc_host import canonical, kosaraju_check, scipy_scc
from test_upload_forms_host import BUILDERS, roots, rows_unsorted, sort_rows, stored, tc_reference, ugraph

pytestmark = pytest.mark.gpu
GRAPHS = list(BUILDERS)
FORMS = ["F0", "F1", "F2", "F3", "F4"]
WITH_REVERSE = ("F0", "F1", "F3")     # the device graph has a reverse CSR
SORTED = ("F0", "F3", "F4")           # the device graph has sorted rows (every builder's rows are unsorted)
GMX_ERR_ARG = -1


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


def form_args(gmx, form):
    """(pass the reverse CSR, flags) of an upload form."""
    S, N = gmx.GMX_GRAPH_SORT_ROWS, gmx.GMX_GRAPH_NO_REVERSE
    return {"F0": (True, S), "F1": (True, 0), "F2": (False, N), "F3": (False, 0), "F4": (False, S | N)}[form]


def upload(gmx, g, form):
    rev, flags = form_args(gmx, form)
    return gmx.Graph.upload(g.begin, g.idx, g.rb if rev else None, g.ri if rev else None, flags=flags)


@pytest.fixture(scope="module")
def dev(gmx):
    """(graph, form) -> its device graph, uploaded once for the module."""
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            cache[(name, form)] = upload(gmx, ugraph(name), form)
        return cache[(name, form)]
    yield get
    for d in cache.values():
        d.free()


def held(d, form):
    """The oracle's graph of the CSR the device holds."""
    b, i, rb, ri = d.download(reverse=form in WITH_REVERSE)
    return po.Graph(len(b) - 1, b, i, rb, ri)


@functools.lru_cache(maxsize=None)
def scc_expected(name):
    g = ugraph(name)
    if g.V <= (1 << 16):
        n, mem = kosaraju_check(g.V, g.begin, g.idx, g.rb, g.ri)
        return n, canonical(mem)
    return scipy_scc(g.V, g.begin, g.idx)


@functools.lru_cache(maxsize=None)
def sym_expected(name):
    ws = po.symmetrize(stored(ugraph(name)))
    return ws, tc_reference(ws.N, ws.begin, ws.node_idx)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_download_and_edge_order(gmx, dev, name, form):
    """F1 / F2 hold the uploaded arrays; the other forms hold sorted rows and the map back to the uploaded slots (F3: the
    map that flags 0 without a reverse CSR did not record before)."""
    g, d = ugraph(name), dev(name, form)
    b, i, rb, ri = d.download(reverse=form in WITH_REVERSE)
    assert np.array_equal(b, g.begin)
    if form in ("F1", "F2"):
        assert np.array_equal(i, g.idx)
        if form == "F1":
            assert np.array_equal(rb, g.rb) and np.array_equal(ri, g.ri)
        assert d.edge_order() is None
        return
    assert not rows_unsorted(b, i)
    emap = d.edge_order()
    assert emap is not None and np.array_equal(np.sort(emap), np.arange(len(i)))
    assert np.array_equal(i, g.idx[emap])
    assert np.array_equal(emap, sort_rows(g.begin, g.idx))          # equal destinations keep their uploaded order
    if form in WITH_REVERSE:
        assert np.array_equal(rb, g.rb) and not rows_unsorted(rb, ri)
        assert np.array_equal(ri, g.ri[sort_rows(g.rb, g.ri)])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_hop_dist_and_bfs_levels(gmx, dev, name, form):
    """From the hub (on multi150k its row has more distinct-from-the-previous slots than the queue has entries), 0, V-1 and
    the self-loop root: dist[], the reached count and the BFS object's levels; one BfsState rank."""
    g, d = ugraph(name), dev(name, form)
    og = stored(g)
    for r in roots(g):
        want = po.bfs_queue(og, r)
        dist, st = d.hop_dist(r)
        assert np.array_equal(dist, want), r
        assert st["vertices_reached"] == int((want != INT_MAX).sum()), r
        lv, n = d.bfs_levels(r)
        want_lv = np.where(want == INT_MAX, -2, want).astype(np.int16)
        assert np.array_equal(lv, want_lv) and n == int(want_lv.max()) + 1, r
    outs, _, _ = _bfs_ranks_on_graph(gmx, d, g.hub, 1)
    assert np.array_equal(outs[0], po.bfs_queue(og, g.hub))


@pytest.mark.parametrize("mode", ["plain", "hubs_lds", "hubs_memory"])
def test_hop_dist_hint_encodings_on_verbatim_multigraph(gmx, mode, monkeypatch):
    """test_hop_dist_hint_encodings' three bottom-up hint encodings on multi150k uploaded verbatim (F1)."""
    if mode == "plain":
        monkeypatch.setenv("GMX_BFS_PLAIN_HINTS", "1")
    else:
        monkeypatch.setenv("GMX_BFS_HUB_MIN_V", str(1 << 17) if mode == "hubs_lds" else str(1 << 18))
    g = ugraph("multi150k")
    og = stored(g)
    d = upload(gmx, g, "F1")     # (fresh: the options are read when the graph's hints are built)
    for r in roots(g):
        want = po.bfs_queue(og, r)
        dist, st = d.hop_dist(r)
        assert np.array_equal(dist, want), (mode, r)
        assert st["vertices_reached"] == int((want != INT_MAX).sum())
    want = po.bfs_queue(og, g.hub)
    for nranks in (2, 3):
        outs, _, _ = _bfs_ranks_on_graph(gmx, d, g.hub, nranks)
        assert all(np.array_equal(o, want) for o in outs), (mode, nranks)
    d.free()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_partitioned_bfs_ranks(gmx, dev, name, form):
    g, d = ugraph(name), dev(name, form)
    if form not in WITH_REVERSE:
        with pytest.raises(gmx.GmxError, match="reverse"):
            gmx.BfsState(d, 0, 2)
        return
    og = stored(g)
    for root in (g.hub, g.loop_root):
        want = po.bfs_queue(og, root)
        for nranks in (2, 3):
            outs, _, _ = _bfs_ranks_on_graph(gmx, d, root, nranks)
            assert all(np.array_equal(o, want) for o in outs), (root, nranks)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_bc(gmx, dev, name, form):
    """comp_BC bit for bit against the oracle on the CSR the device holds (its float sums follow the slot order)."""
    g, d = ugraph(name), dev(name, form)
    rng = np.random.default_rng(len(name))
    seeds = np.concatenate([[g.hub], rng.integers(0, g.V, 4)]).astype(np.int32)
    if form not in WITH_REVERSE:
        with pytest.raises(gmx.GmxError, match="reverse"):
            d.bc(seeds)
        return
    dg = held(d, form)
    for skip in (False, True):
        got, st = d.bc(seeds, skip)
        assert same_f32(got, po.bc(dg, seeds, skip)), skip
        assert st["iterations"] == len(seeds)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_sssp_lengths_by_caller_slot(gmx, dev, name, form):
    g, d = ugraph(name), dev(name, form)
    og = stored(g)
    rng = np.random.default_rng(7)
    for length in (rng.integers(1, 101, len(g.idx)).astype(np.int32), np.ones(len(g.idx), np.int32)):
        for root in (g.hub, g.loop_root):
            dist, _ = d.sssp(length, root)
            assert np.array_equal(dist, po.sssp(og, length, root)[0]), root


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_avg_teen_cnt_and_conduct(gmx, dev, name, form):
    g, d = ugraph(name), dev(name, form)
    og = stored(g)
    rng = np.random.default_rng(9)
    age = rng.integers(0, 40, g.V).astype(np.int32)
    for K in (5, 30):
        avg, cnt, _ = d.avg_teen_cnt(age, K)
        want_avg, want_cnt = po.avg_teen_cnt(og, age, K)
        assert np.array_equal(cnt, want_cnt)
        assert np.float32(avg).tobytes() == np.float32(want_avg).tobytes()
    member = rng.integers(0, 4, g.V).astype(np.int32)
    for num in (0, 1, 3):
        assert np.float32(d.conduct(member, num)[0]).tobytes() == np.float32(po.conduct(og, member, num)).tobytes()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_pagerank_converged(gmx, dev, name, form):
    g, d = ugraph(name), dev(name, form)
    if form not in WITH_REVERSE:
        with pytest.raises(gmx.GmxError, match="reverse"):
            d.pagerank()
        return
    want, it, _ = po.pagerank(stored(g), 0.001, 0.85, 100)
    r64, st64 = d.pagerank(0.001, 0.85, 100, np.float64)
    r32, st32 = d.pagerank(0.001, 0.85, 100, np.float32)
    assert st64["iterations"] == it and st32["iterations"] == it
    assert rel_err(r64, want) < PR_RTOL_F64
    assert rel_err(r32, want) < PR_RTOL_F32


@pytest.mark.parametrize("options", [0, 1, 3, 5, 7])
@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("name", GRAPHS)
def test_pagerank_stepping_variants_verbatim(gmx, dev, name, elem, options):
    g, d = ugraph(name), dev(name, "F1")
    want, _, _ = po.pagerank(stored(g), 1e-300, 0.85, 20)
    st = gmx.PageRankState(d, elem, 0, 1, options)
    st.reset(0.85)
    for _ in range(20):
        st.step()
    got = st.download()
    st.free()
    assert rel_err(got, want) < (PR_RTOL_F32 if elem == 4 else PR_RTOL_F64)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_scc(gmx, dev, name, form):
    d = dev(name, form)
    if form not in WITH_REVERSE:
        with pytest.raises(gmx.GmxError, match="reverse"):
            d.scc()
        return
    comp, n, st = d.scc()
    en, ecomp = scc_expected(name)
    assert n == en and np.array_equal(comp, ecomp)


@pytest.mark.parametrize("form", ["F1", "F2"])
@pytest.mark.parametrize("name", GRAPHS)
def test_symmetrize_verbatim_and_count(gmx, dev, name, form, monkeypatch):
    """gmx_graph_symmetrize of a verbatim upload, and triangle counting of the result (default hubs and 64 hubs)."""
    d = dev(name, form)
    ws, want = sym_expected(name)
    for hubs in (None, "64"):
        if hubs:
            monkeypatch.setenv("GMX_TC_HUBS", hubs)     # (read when the symmetric graph's oriented copy is built)
        gs = d.symmetrize()
        b, i, rb, ri = gs.download()
        assert np.array_equal(b, ws.begin) and np.array_equal(i, ws.node_idx)
        assert np.array_equal(rb, ws.begin) and np.array_equal(ri, ws.node_idx)
        assert gs.triangle_counting()[0] == want, hubs
        gs.free()


def _pairs(g, rng):
    src = np.concatenate([[g.hub, g.loop_root, g.loop_root, g.hub], rng.integers(0, g.V, 60)]).astype(np.int32)
    dst = np.concatenate([[g.loop_root, g.hub, g.loop_root, g.hub], rng.integers(0, g.V, 60)]).astype(np.int32)
    return src, dst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_triangle_counting_and_common_neighbours(gmx, dev, name, form):
    """On sorted rows: the counts of the rows the device holds, whole and in three parts, and the common-neighbour
    entries.  On rows kept verbatim out of order: GMX_ERR_STATE that names GMX_GRAPH_SORT_ROWS, from every one of them."""
    g, d = ugraph(name), dev(name, form)
    src, dst = _pairs(g, np.random.default_rng(2))
    if form not in SORTED:
        calls = [lambda: d.triangle_counting(), lambda: d.triangle_counting(1, 3), lambda: d.triangle_counting_cn(),
                 lambda: d.common_nbrs(g.hub, g.loop_root), lambda: d.common_nbr_counts(src, dst)]
        for call in calls:
            with pytest.raises(gmx.GmxError, match="SORT_ROWS") as e:
                call()
            assert "status -5" in str(e.value)
            assert b"SORT_ROWS" in gmx.lib().gmx_last_error()
        return
    dg = held(d, form)
    # (F4 has no reverse CSR: the emitted forward-only form, quadratic in multi150k's hub row -- counted on F0 / F3)
    if not (name == "multi150k" and form == "F4"):
        want = tc_reference(g.V, dg.begin, dg.node_idx)
        assert d.triangle_counting()[0] == want
        assert sum(d.triangle_counting(p, 3)[0] for p in range(3)) == want
    assert d.triangle_counting_cn()[0] == tc_reference(g.V, dg.begin, dg.node_idx, cn=True)
    want_n = [len(po.common_nbrs(dg, s, t)) for s, t in zip(src, dst)]
    assert d.common_nbr_counts(src, dst).tolist() == want_n
    for s, t in list(zip(src, dst))[:12]:
        assert np.array_equal(d.common_nbrs(s, t), po.common_nbrs(dg, s, t)), (s, t)


@pytest.mark.parametrize("name", ["multi64", "rmat16_shuffled", "sym14_shuffled"])
def test_triangle_counting_sorted_forward_unsorted_reverse(gmx, name):
    """Sorted forward rows with a reverse CSR whose rows are out of order: counted in the forward-only form, not
    searched in the reverse rows."""
    g = ugraph(name)
    o = sort_rows(g.begin, g.idx)
    fwd = np.ascontiguousarray(g.idx[o])
    assert rows_unsorted(g.rb, g.ri)
    d = gmx.Graph.upload(g.begin, fwd, g.rb, g.ri, flags=0)
    want = tc_reference(g.V, g.begin, fwd)
    assert d.triangle_counting()[0] == want
    assert sum(d.triangle_counting(p, 3)[0] for p in range(3)) == want
    assert d.triangle_counting_cn()[0] == tc_reference(g.V, g.begin, fwd, cn=True)
    d.free()


# ------------------------------------------------------------------ invalid CSRs: upload only, never an entry
def _raw_upload(gmx, e64, begin, idx, rb, ri, flags):
    """gmx_graph_upload / gmx_graph_upload_e64 through ctypes: (status, handle)."""
    bt = np.int64 if e64 else np.int32
    arrs = [np.ascontiguousarray(begin, bt), np.ascontiguousarray(idx, np.int32),
            None if rb is None else np.ascontiguousarray(rb, bt), None if ri is None else np.ascontiguousarray(ri, np.int32)]
    L = gmx.lib()
    h = C.c_void_p()
    f = L.gmx_graph_upload_e64 if e64 else L.gmx_graph_upload
    st = f(*[a.ctypes.data if a is not None else None for a in arrs], len(begin) - 1, len(idx), flags, C.byref(h))
    return st, h


def _invalid(case):
    g = ugraph("multi64")
    b, i, rb, ri = g.begin.copy(), g.idx.copy(), g.rb.copy(), g.ri.copy()
    V, E = g.V, len(g.idx)
    if case == "node_idx_V":
        i[E // 2] = V
    elif case == "node_idx_negative":
        i[E - 1] = -1
    elif case == "begin_decreases":
        r = int(np.flatnonzero(np.diff(b) >= 2)[0])
        b[r + 1] = b[r] - 1 if b[r] > 0 else b[r + 2] + 1      # (begin[0] and begin[V] stay right)
        assert np.any(np.diff(b) < 0) and b[0] == 0 and b[V] == E
    elif case == "r_node_idx_V":
        ri[3] = V
    elif case == "r_begin_V_not_E":
        rb[V] = E - 1
    return b, i, rb, ri


# the forward cases on every form; the reverse ones where the upload keeps a caller-given reverse CSR (F1: the other forms
# build their own or none)
INVALID = [(c, f) for c in ("node_idx_V", "node_idx_negative", "begin_decreases") for f in FORMS] + \
          [(c, "F1") for c in ("r_node_idx_V", "r_begin_V_not_E")]


@pytest.mark.parametrize("e64", [False, True])
@pytest.mark.parametrize("case,form", INVALID)
def test_invalid_csr_is_refused(gmx, case, form, e64):
    """GMX_ERR_ARG with a message that says what failed; afterwards a valid upload works as if nothing had happened."""
    rev, flags = form_args(gmx, form)
    b, i, rb, ri = _invalid(case)
    st, h = _raw_upload(gmx, e64, b, i, rb if rev else None, ri if rev else None, flags)
    if h.value:
        gmx.lib().gmx_graph_free(h)                      # (never used: an entry on it would index outside its arrays)
    assert st == GMX_ERR_ARG and not h.value, (case, form, st)
    msg = gmx.lib().gmx_last_error().decode()
    assert ("node_idx" in msg) if "node_idx" in case else ("begin" in msg), msg
    g = ugraph("multi64")
    st, h = _raw_upload(gmx, e64, g.begin, g.idx, g.rb if rev else None, g.ri if rev else None, flags)
    assert st == 0 and h.value
    d = gmx.Graph(h)
    assert np.array_equal(d.hop_dist(g.hub)[0], po.bfs_queue(stored(g), g.hub))
    assert np.array_equal(d.download(reverse=False)[0], g.begin)
    d.free()
