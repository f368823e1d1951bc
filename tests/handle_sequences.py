"""One graph handle, many entries: the scenario table, the named sequences and their runner (no device code).

Every algorithm entry of gmx.Graph is a row of ROWS: the inputs it runs on, argument sets that give different results, the
CPU model and the compare function of the entry's own test file (imported, none copied; a checker that makes the call
itself is handed a Replay of the result already obtained).  A step is (entry, argument set, handle label); run() walks a
list of steps with call(step) and check(step, result) and names the step that failed and the steps before it.  The device
tests give run() a call that drives the library (test_gpu_handle_sequences.py); the host tests give it a fake that returns
the model's own result, a stale one or one with an element changed (test_handle_sequences_host.py).

Inputs, built once: D = rmat_graph(12, permute=True) with both CSRs (repeats and loops kept), S = its symmetrised simple
form, B = the left -> right edges of D for left = the even ids, R = D with the slots of every row shuffled, uploaded with
GMX_GRAPH_SORT_ROWS (the device holds D's arrays and e_idx2idx; edge properties stay in the shuffled slots).  No entry
needs a smaller scale: every reference is computed at scale 12 (closeness over a list of pivots, as its own RMAT tests do).

An entry without arguments (scc, wcc, v_cover, triangle_counting_cn, adamic_adar) has its second argument set on another
input; it meets its own cached state where a sequence repeats a step on the same handle (workspace, families)."""
import collections
import functools
import heapq
import itertools

import numpy as np

import pyoracle as po
import sampling_common as sc
import test_gpu_adamic_adar as taa
import test_gpu_bicc as tbi
import test_gpu_closeness as tcl
import test_gpu_clustering as tlc
import test_gpu_coloring as tco
import test_gpu_communities as tcm
import test_gpu_kcore as tkc
import test_gpu_ktruss as tkt
import test_gpu_msf as tms
import test_gpu_potential_friends as tpf
import test_gpu_random_bipartite_matching as rbm
import test_gpu_route as rt
import test_gpu_sampling as tsa
import test_gpu_scc as tsc
import test_gpu_sssp_path_adj as spf
import test_gpu_tc_directed as ttd
import test_gpu_v_cover as tvc
import test_gpu_wcc as twc
from bicc_model import forest_model, hopcroft_tarjan
from ktruss_model import ktruss_model
from test_adamic_adar_host import aa_vectorised
from test_clustering_host import clustering_model
from test_closeness_host import closeness_model
from test_coloring_host import greedy_model
from test_gpu_parity import INT_MAX, PR_RTOL_F32, PR_RTOL_F64, rel_err, same_f32
from test_gpu_sssp_path import check_exact
from test_kcore_host import kcore_model
from test_msf_host import msf_model
from test_potential_friends_host import potential_friends_ref
from test_random_bipartite_matching_host import rbm_model
from test_route_host import dijkstra_cost, route_of_parents, valid_route
from test_sssp_path_adj_host import spf_model
from test_sssp_path_host import canonical_tree
from test_tc_directed_host import tcd_ref
from test_v_cover_host import v_cover_ref
from test_wcc_host import scipy_wcc

SCALE = 12
GMX_GRAPH_SORT_ROWS = 0x1   # gmx.GMX_GRAPH_SORT_ROWS (this module does not load the library)
GMX_ERR_ARG = -1

Input = collections.namedtuple("Input", "label V E begin idx rb ri og flags stored")
Step = collections.namedtuple("Step", "entry k handle")
Row = collections.namedtuple("Row", "name args call model fake check log")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs():
    """label -> Input.  begin / idx are the arrays as uploaded (edge properties are indexed by their slots), stored the
    four arrays the device holds afterwards."""
    d = po.rmat_graph(SCALE, permute=True)
    s = po.symmetrize(d)
    rows = np.repeat(np.arange(d.N), np.diff(d.begin))
    left = np.arange(d.N) % 2 == 0
    lr = left[rows] & ~left[d.node_idx]
    b = po.graph_from_edges(d.N, rows[lr].astype(np.int32), d.node_idx[lr])
    out = {}
    for label, og in (("D", d), ("S", s), ("B", b)):
        _frozen(og.begin, og.node_idx, og.r_begin, og.r_node_idx)
        out[label] = Input(label, og.N, og.M, og.begin, og.node_idx, og.r_begin, og.r_node_idx, og, 0,
                           (og.begin, og.node_idx, og.r_begin, og.r_node_idx))
    # R: a random order inside every row; sorting it back (stable by destination) gives D's arrays
    key = np.random.default_rng(SCALE).random(d.M)
    shuffled = np.ascontiguousarray(d.node_idx[np.lexsort((key, rows))])
    assert (np.diff(shuffled) < 0)[np.diff(rows) == 0].any()
    _frozen(shuffled)
    out["R"] = Input("R", d.N, d.M, d.begin, shuffled, None, None, po.Graph(d.N, d.begin, shuffled, d.r_begin, d.r_node_idx), GMX_GRAPH_SORT_ROWS, out["D"].stored)
    return out


def input_of(handle):
    """The input a handle label stands for: "D", "D#2" (another upload of D), "S#fresh" ..."""
    return inputs()[handle.split("#")[0]]


def upload(gmx, inp):
    return gmx.Graph.upload(inp.begin, inp.idx, inp.rb, inp.ri, flags=inp.flags)


# ---------------------------------------------------------------- the data the argument sets name
@functools.lru_cache(maxsize=None)
def lengths(label, seed, hi=100):
    return _frozen(np.random.default_rng(seed).integers(1, hi, inputs()[label].E).astype(np.int32))[0]


@functools.lru_cache(maxsize=None)
def costs(label, seed):
    return _frozen(np.random.default_rng(seed).random(inputs()[label].E) + 0.5)[0]


@functools.lru_cache(maxsize=None)
def vertex_ints(label, seed, lo, hi):
    return _frozen(np.random.default_rng(seed).integers(lo, hi, inputs()[label].V).astype(np.int32))[0]


@functools.lru_cache(maxsize=None)
def by_out_degree(label):
    """The vertices, largest out-degree first."""
    return np.argsort(-np.diff(inputs()[label].begin), kind="stable")


def hub(label, n=0):
    return int(by_out_degree(label)[n])


@functools.lru_cache(maxsize=None)
def pivots(label, seed, n):
    return _frozen(np.concatenate([[hub(label)], np.random.default_rng(seed).integers(0, inputs()[label].V, n - 1)]).astype(np.int32))[0]


def lefts(label, step):
    return (np.arange(inputs()[label].V) % step == 0).astype(np.uint8)


def stats(**kw):
    """What a call's statistics look like when nothing else is known of them (the fake device's)."""
    st = dict(iterations=0, last_diff=0.0, kernel_ms=1.0, h2d_ms=0.0, d2h_ms=0.0, edges_examined=0, vertices_reached=0, edges_reached=0)
    st.update(kw)
    return st


class Replay:
    """Stands for the handle inside a checker that makes the call itself: the entry returns the result already obtained,
    the accessors the input's arrays as the device holds them."""

    def __init__(self, inp, **entries):
        self._inp, self._entries = inp, entries
        self.V, self.E = inp.V, inp.E

    def download(self, reverse=True):
        b, i, rb, ri = self._inp.stored
        return (b, i, rb, ri) if reverse else (b, i, None, None)

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._entries:
            raise AttributeError(name)
        return self._entries[name]


def shortest_route(begin, idx, w, src, dst):
    """(cost, nodes after src, slots into them) of one shortest route, or None: what the fake device answers a query with."""
    begin, idx, w = begin.tolist(), idx.tolist(), w.tolist()
    dist, via = {src: 0}, {}
    heap = [(0, src)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        if u == dst:
            nodes, edges = [], []
            while u != src:
                nodes.insert(0, u)
                edges.insert(0, via[u][1])
                u = via[u][0]
            return d, nodes, edges
        for e in range(begin[u], begin[u + 1]):
            if d + w[e] < dist.get(idx[e], INT_MAX):
                dist[idx[e]] = d + w[e]
                via[idx[e]] = (u, e)
                heapq.heappush(heap, (d + w[e], idx[e]))
    return None


# ---------------------------------------------------------------- the rows
ROWS = collections.OrderedDict()
EXTRA = collections.OrderedDict()   # what a caller holds on a graph besides the entries: Route, BfsState, PageRankState


def row(name, args, call, model, fake, check, log=None, table=None):
    (ROWS if table is None else table)[name] = Row(name, args, call, model, fake, check, log)


def _ints(m, fields, keep=()):
    return {k: (v if k in keep else int(v)) for k, v in zip(fields, m)}


def last_line(pattern, fields, keep=()):
    """err -> the fields of the last line of a findall-style pattern (tuples of groups)."""
    def parse(err):
        lines = pattern.findall(err)
        assert lines, err
        return _ints(lines[-1], fields, keep)
    return parse


def named_line(pattern, keep=()):
    def parse(err):
        m = pattern.search(err)
        assert m, err
        return {k: (v if k in keep else int(v)) for k, v in m.groupdict().items()}
    return parse


# pagerank: the tolerances of test_gpu_parity (d in (0, 1]: relative; outside: against the largest |rank|)
def _pr_model(inp, a):
    want, it, _ = po.pagerank(inp.og, a["e"], a["d"], a["max_iter"])
    return _frozen(want)[0], it


def _pr_check(inp, a, want, got):
    rank, st = got
    assert rank.dtype == a["dtype"] and st["iterations"] == want[1], st
    if 0 < a["d"] <= 1:
        assert rel_err(rank, want[0]) < (PR_RTOL_F32 if a["dtype"] == np.float32 else PR_RTOL_F64), rel_err(rank, want[0])
    else:
        tol = 2e-6 if a["dtype"] == np.float32 else 1e-11
        assert float(np.max(np.abs(rank.astype(np.float64) - want[0]))) < tol * float(np.max(np.abs(want[0])))


def _pr(d, dtype, ranks=None):
    a = {"e": 0.001, "d": 0.85, "max_iter": 100, "dtype": dtype} if d == 0.85 else {"e": 1e-300, "d": d, "max_iter": 6, "dtype": dtype}
    if ranks:
        a["_env"] = {"GMX_PR_RANKS": str(ranks)}
    return ("D", a)


PR_ARGS = [_pr(d, t, r) for r in (None, 2) for d, t in ((0.85, np.float64), (1.5, np.float32), (0.85, np.float32), (1.5, np.float64))]
row("pagerank", PR_ARGS,
    lambda g, inp, a: g.pagerank(a["e"], a["d"], a["max_iter"], a["dtype"]),
    _pr_model, lambda inp, a, w: (w[0].astype(a["dtype"]), stats(iterations=w[1])), _pr_check)


# the traversal object: hop_dist, bfs_levels, bc, bc_batch, bc_all (scc and closeness further down)
def _dist_check(inp, a, want, got):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want)


row("hop_dist", [("D", {"root": hub("D")}), ("D", {"root": hub("D", 40)})],
    lambda g, inp, a: g.hop_dist(a["root"]),
    lambda inp, a: po.bfs_queue(inp.og, a["root"]), lambda inp, a, w: (w.copy(), stats()), _dist_check)


def _levels_model(inp, a):
    dist = po.bfs_queue(inp.og, a["root"])
    lv = np.where(dist == INT_MAX, -2, dist).astype(np.int16)
    return lv, int(lv.max()) + 1


def _levels_check(inp, a, want, got):
    assert got[0].dtype == np.int16 and np.array_equal(got[0], want[0]) and got[1] == want[1]


row("bfs_levels", [("D", {"root": hub("D", 3)}), ("D", {"root": hub("D", 77)})],
    lambda g, inp, a: g.bfs_levels(a["root"]), _levels_model, lambda inp, a, w: (w[0].copy(), w[1]), _levels_check)


def _bc_model(inp, a):
    seeds = np.arange(inp.V, dtype=np.int32) if a.get("all") else pivots(inp.label, a["seeds"], a["n"])
    return po.bc(inp.og, seeds, a["skip"]).copy(), len(seeds)


def _bc_check(inp, a, want, got):
    bc, st = got
    assert bc.dtype == np.float32 and same_f32(bc, want[0])
    assert st["iterations"] == want[1]


def _bc_fake(inp, a, w):
    return w[0].copy(), stats(iterations=w[1])


row("bc", [("D", {"seeds": 1, "n": 5, "skip": False}), ("D", {"seeds": 2, "n": 3, "skip": True})],
    lambda g, inp, a: g.bc(pivots(inp.label, a["seeds"], a["n"]), a["skip"]), _bc_model, _bc_fake, _bc_check)
row("bc_batch", [("D", {"seeds": 3, "n": 20, "skip": True, "width": 16}), ("D", {"seeds": 4, "n": 33, "skip": False, "width": 0})],
    lambda g, inp, a: g.bc_batch(pivots(inp.label, a["seeds"], a["n"]), a["skip"], a["width"]), _bc_model, _bc_fake, _bc_check)
row("bc_all", [("D", {"all": True, "skip": True}), ("D", {"all": True, "skip": False})],
    lambda g, inp, a: g.bc_all(a["skip"]), _bc_model, _bc_fake, _bc_check)

# sssp, sssp_path (both schedules), sssp_path_f64
row("sssp", [("D", {"len": 11, "root": hub("D")}), ("D", {"len": 12, "root": hub("D", 9)})],
    lambda g, inp, a: g.sssp(lengths(inp.label, a["len"]), a["root"]),
    lambda inp, a: po.sssp(inp.og, lengths(inp.label, a["len"]), a["root"])[0], lambda inp, a, w: (w.copy(), stats(iterations=1)), _dist_check)


def _tree_fake(inp, a, w):
    pn, pe, _, _ = canonical_tree(inp.begin, inp.idx, lengths(inp.label, a["len"]), w)
    return w.copy(), pn, pe, stats(iterations=1)


row("sssp_path", [("D", {"len": 13, "root": hub("D", 1), "_env": {"GMX_SSSP_PATH_SCHEDULE": "round"}}),
                  ("D", {"len": 14, "root": hub("D", 5), "_env": {"GMX_SSSP_PATH_SCHEDULE": "nearfar"}})],
    lambda g, inp, a: g.sssp_path(lengths(inp.label, a["len"]), a["root"]),
    lambda inp, a: po.sssp(inp.og, lengths(inp.label, a["len"]), a["root"])[0], _tree_fake,
    lambda inp, a, want, got: check_exact(inp.begin, inp.idx, lengths(inp.label, a["len"]), a["root"], want, got, a))


def _spf_model(inp, a):
    want = spf_model(inp.begin, inp.idx, costs(inp.label, a["cost"]), a["root"], a["end"])
    _frozen(*want[:3])
    return want


row("sssp_path_f64", [("D", {"cost": 15, "root": hub("D"), "end": -1}), ("D", {"cost": 16, "root": hub("D", 2), "end": hub("D", 300)})],
    lambda g, inp, a: g.sssp_path_f64(costs(inp.label, a["cost"]), a["root"], a["end"]), _spf_model,
    lambda inp, a, w: (w[0].copy(), w[1].copy(), w[2].copy(), stats(iterations=w[3], edges_examined=w[4], vertices_reached=w[5])),
    lambda inp, a, want, got: spf.check(want, got, a))


# route queries: flag and cost are dijkstra_cost's, the route passes valid_route (test_gpu_route)
def _route_model(inp, a):
    return dijkstra_cost(inp.begin, inp.idx, lengths(inp.label, a["w"]), a["src"], a["dst"])


def _bidir_fake(inp, a, w):
    parent, edge = np.full(inp.V, -1, np.int32), np.full(inp.V, -1, np.int32)
    if w is not None:
        _, nodes, edges = shortest_route(inp.begin, inp.idx, lengths(inp.label, a["w"]), a["src"], a["dst"])
        parent[nodes], edge[nodes] = [a["src"]] + nodes[:-1], edges
    return w is not None, parent, edge, stats(h2d_ms=1.0)


def _bidir_check(inp, a, want, got):
    hit, parent, parent_edge, st = got
    src, dst = a["src"], a["dst"]
    assert parent.dtype == np.int32 and parent_edge.dtype == np.int32
    assert hit == (want is not None) and st["h2d_ms"] > 0
    nodes, edges = route_of_parents(parent, parent_edge, src, dst)
    if hit:
        assert valid_route(inp.begin, inp.idx, lengths(inp.label, a["w"]), src, dst, nodes, edges, want) is None
    on = np.zeros(inp.V, bool)
    on[nodes] = True
    assert (parent[~on] == -1).all() and (parent_edge[~on] == -1).all() and (parent[on] != -1).all() and not on[src]


row("bidir_dijkstra", [("D", {"w": 17, "src": hub("D"), "dst": hub("D", 500)}), ("D", {"w": 18, "src": hub("D", 7), "dst": hub("D", 900)})],
    lambda g, inp, a: g.bidir_dijkstra(lengths(inp.label, a["w"]), a["src"], a["dst"]), _route_model, _bidir_fake, _bidir_check)


def _query_fake(inp, a, w):
    if w is None:
        return False, None, np.zeros(0, np.int32), np.zeros(0, np.int32), 0, stats()
    _, nodes, edges = shortest_route(inp.begin, inp.idx, lengths(inp.label, a["w"]), a["src"], a["dst"])
    return True, w, np.array(nodes, np.int32), np.array(edges, np.int32), len(nodes), stats()


ROUTE_WEIGHTS = (21, 22)   # the two Route objects of held_state: lengths(label, seed)
row("route_query", [("D", {"w": ROUTE_WEIGHTS[n % 2], "src": hub("D", 10 * n), "dst": hub("D", 400 + 37 * n)}) for n in range(8)],
    None, _route_model, _query_fake,
    lambda inp, a, want, got: rt.check(inp.begin, inp.idx, lengths(inp.label, a["w"]), a["src"], a["dst"], want, got, a), table=EXTRA)

# scc, wcc: the checkers make the call themselves
row("scc", [("D", {}), ("B", {})], lambda g, inp, a: g.scc(),
    lambda inp, a: tsc.expect(Replay(inp)),
    lambda inp, a, w: (w[1].copy(), w[0], stats(vertices_reached=int(np.bincount(w[1]).max()))),
    lambda inp, a, want, got: tsc.check(Replay(inp, scc=lambda: got)))
row("wcc", [("D", {}), ("B", {})], lambda g, inp, a: g.wcc(),
    lambda inp, a: scipy_wcc(inp.V, inp.stored[0], inp.stored[1]),
    lambda inp, a, w: (w[1].copy(), w[0], stats(vertices_reached=int(np.bincount(w[1]).max()))),
    lambda inp, a, want, got: twc.check(Replay(inp, wcc=lambda: got), want))

# kcore
KCORE_LINE = last_line(tkc.LOG, tkc.LOG_FIELDS)
row("kcore", [("S", {"mode": "in"}), ("S", {"mode": "both"})],
    lambda g, inp, a: g.kcore(a["mode"], layers=True),
    lambda inp, a: kcore_model(inp.V, inp.begin, inp.idx, a["mode"]),
    lambda inp, a, w: (w["core"].copy(), w["layer"].copy(), w["max_core"], stats(vertices_reached=w["top"], iterations=w["rounds"], edges_examined=w["slots"]),
                       {k: w[k] for k in ("levels", "rounds", "scanned")}),
    lambda inp, a, want, got: tkc.agrees(got, want, inp.E, a["mode"]), log=("GMX_KCORE_LOG", KCORE_LINE))


# msf: the checker calls with and without the component array
def _msf_model(inp, a):
    src = np.repeat(np.arange(inp.V), np.diff(inp.begin))
    return msf_model(inp.V, src, inp.idx.astype(np.int64), lengths(inp.label, a["w"]), np.arange(inp.E))


def _msf_fake(inp, a, m):
    st = dict(iterations=m["rounds"], edges_examined=m["slots"])
    full = (m["in_forest"].copy(), m["count"], m["total"], m["comp"].copy(), inp.V - m["count"], stats(vertices_reached=int(np.bincount(m["comp"]).max()), **st))
    return full, (full[0].copy(), m["count"], m["total"], stats(**st))


row("msf", [("S", {"w": 23}), ("S", {"w": 24})],
    lambda g, inp, a: (g.msf(lengths(inp.label, a["w"]), components=True), g.msf(lengths(inp.label, a["w"]))),
    _msf_model, _msf_fake,
    lambda inp, a, want, got: tms.check(Replay(inp, msf=lambda w, components=False: got[0] if components else got[1]), lengths(inp.label, a["w"]), want))


# coloring
def _prio(inp, a):
    return None if a["prio"] is None else vertex_ints(inp.label, a["prio"], 0, 50)


def _color_fake(inp, a, w):
    block = w["L"] >= tco.BLOCK_MIN
    wave = ~block & (w["L"] >= tco.WAVE_MIN)
    f = {"env": {}, "group": int((~block & ~wave).sum()), "wave": int(wave.sum()), "block": int(block.sum()), "passes": w["passes"](tco.WINDOW)}
    return w["color"].copy(), w["depth"].copy(), w["num_colors"], stats(vertices_reached=w["class0"], iterations=w["rounds"], edges_examined=6 * inp.E), f


def _color_line(err):
    f = last_line(tco.LOG, tco.LOG_FIELDS)(err)
    f["env"] = {}
    return f


row("coloring", [("S", {"prio": None}), ("S", {"prio": 25})],
    lambda g, inp, a: g.coloring(_prio(inp, a), depth=True),
    lambda inp, a: greedy_model(inp.V, inp.begin, inp.idx, _prio(inp, a)), _color_fake,
    lambda inp, a, want, got: tco.agrees(got, want, inp.E), log=("GMX_COLOR_LOG", _color_line))


# closeness over a list of pivots
def _close_check(inp, a, want, got):
    assert len(got) == 5
    tcl.same(got[:4], want)


row("closeness", [("D", {"mode": "out", "src": 26, "n": 70}), ("D", {"mode": "both", "src": 27, "n": 130})],
    lambda g, inp, a: g.closeness(a["mode"], pivots(inp.label, a["src"], a["n"])),
    lambda inp, a: closeness_model(inp.V, inp.begin, inp.idx, a["mode"], pivots(inp.label, a["src"], a["n"])),
    lambda inp, a, w: tuple(x.copy() for x in w) + (stats(),), _close_check)

# communities
row("communities", [("S", {"max_rounds": 1000}), ("S", {"max_rounds": 1})],
    lambda g, inp, a: g.communities(a["max_rounds"]),
    lambda inp, a: tcm.ref_of("handle_sequences/" + inp.label, inp.begin, inp.idx, a["max_rounds"]),
    lambda inp, a, w: (w[0].copy(), w[1], w[2], stats(iterations=w[1])),
    lambda inp, a, want, got: tcm.check(Replay(inp, communities=lambda max_rounds: got), "handle_sequences/" + inp.label, inp.begin, inp.idx, a["max_rounds"]))


# potential_friends (all vertices through the file's check, a range against the same restatement) and the sizing call
def _pf_model(inp, a):
    if a["lo"] is None:
        return tpf.pf_ref_of("handle_sequences/" + inp.label, inp.begin, inp.idx)
    return _frozen(*potential_friends_ref(inp.begin, inp.idx, a["lo"], a["hi"]))


def _pf_fake(inp, a, w):
    L, _ = tpf.two_hop_lengths(inp.begin, inp.idx)
    return w[0].copy(), w[1].copy(), stats(edges_examined=int(L.sum()), vertices_reached=int(np.count_nonzero(np.diff(w[0]))), iterations=1)


def _pf_check(inp, a, want, got):
    if a["lo"] is None:
        tpf.check(Replay(inp, potential_friends=lambda: got), "handle_sequences/" + inp.label, inp.begin, inp.idx)
        return
    pb, pi, st = got
    assert pb.dtype == np.int64 and pi.dtype == np.int32
    assert np.array_equal(pb, want[0]) and np.array_equal(pi, want[1])
    assert st["vertices_reached"] == int(np.count_nonzero(np.diff(want[0])))


def _pfc_check(inp, a, want, got):
    assert got.dtype == np.int64 and np.array_equal(got, np.diff(want[0]))


row("potential_friends", [("D", {"lo": None, "hi": None}), ("D", {"lo": 1000, "hi": 3001})],
    lambda g, inp, a: g.potential_friends() if a["lo"] is None else g.potential_friends(a["lo"], a["hi"]), _pf_model, _pf_fake, _pf_check)
row("potential_friend_counts", [("D", {"lo": 0, "hi": 2000}), ("D", {"lo": 2000, "hi": 4096})],
    lambda g, inp, a: g.potential_friend_counts(a["lo"], a["hi"]), _pf_model, lambda inp, a, w: np.diff(w[0]), _pfc_check)


# avg_teen_cnt, conduct: the integers exactly, the float32 bit for bit
def _teen_check(inp, a, want, got):
    avg, cnt, _ = got
    assert np.array_equal(cnt, want[1]) and np.float32(avg).tobytes() == np.float32(want[0]).tobytes()


row("avg_teen_cnt", [("D", {"age": 28, "K": 5}), ("D", {"age": 29, "K": 30})],
    lambda g, inp, a: g.avg_teen_cnt(vertex_ints(inp.label, a["age"], 0, 40), a["K"]),
    lambda inp, a: po.avg_teen_cnt(inp.og, vertex_ints(inp.label, a["age"], 0, 40), a["K"]),
    lambda inp, a, w: (w[0], w[1].copy(), stats()), _teen_check)


def _conduct_check(inp, a, want, got):
    assert np.float32(got[0]).tobytes() == np.float32(want).tobytes()


row("conduct", [("D", {"member": 30, "num": 1}), ("D", {"member": 31, "num": 3})],
    lambda g, inp, a: g.conduct(vertex_ints(inp.label, a["member"], 0, 4), a["num"]),
    lambda inp, a: po.conduct(inp.og, vertex_ints(inp.label, a["member"], 0, 4), a["num"]),
    lambda inp, a, w: (w, stats()), _conduct_check)


# the counting entries and the iterator they share their graph state with
def _cn_check(inp, a, want, got):
    assert got.dtype == want.dtype and np.array_equal(got, want)


def _cn_pair(label, n):
    """The n-th pair of two large rows that have common neighbours."""
    order = by_out_degree(label)
    return {"s": int(order[2 * n]), "d": int(order[2 * n + 1])}


row("common_nbrs", [("D", _cn_pair("D", 0)), ("D", _cn_pair("D", 3)), ("S", _cn_pair("S", 1)), ("S", _cn_pair("S", 4))],
    lambda g, inp, a: g.common_nbrs(a["s"], a["d"]),
    lambda inp, a: po.common_nbrs(inp.og, a["s"], a["d"]), lambda inp, a, w: w.copy(), _cn_check)


def _pairs(inp, a):
    rng = np.random.default_rng(a["pairs"])
    return by_out_degree(inp.label)[rng.integers(0, 600, (2, a["n"]))].astype(np.int32)


def _cnc_model(inp, a):
    s, d = _pairs(inp, a)
    return np.array([len(po.common_nbrs(inp.og, int(x), int(y))) for x, y in zip(s, d)], np.int64)


row("common_nbr_counts", [("D", {"pairs": 32, "n": 300}), ("D", {"pairs": 33, "n": 301}), ("S", {"pairs": 34, "n": 200})],
    lambda g, inp, a: g.common_nbr_counts(*_pairs(inp, a)), _cnc_model, lambda inp, a, w: w.copy(), _cn_check)


def _count_check(inp, a, want, got):
    assert got[0] == want


row("triangle_counting_cn", [("D", {}), ("S", {})], lambda g, inp, a: g.triangle_counting_cn(),
    lambda inp, a: po.triangle_counting_cn(inp.og), lambda inp, a, w: (w, stats()), _count_check)


def _parts_call(entry):
    def call(g, inp, a):
        if a["nparts"] == 1:
            return getattr(g, entry)()
        got = [getattr(g, entry)(p, a["nparts"]) for p in range(a["nparts"])]
        return sum(t for t, _ in got), got[-1][1]
    return call


# (the parts of a count have no model of their own: their sum is the count, as the entries' own tests state it)
row("triangle_counting", [("S", {"nparts": 1}), ("D", {"nparts": 1}), ("S", {"nparts": 3}), ("D", {"nparts": 2})],
    _parts_call("triangle_counting"), lambda inp, a: po.triangle_counting(inp.og), lambda inp, a, w: (w, stats()), _count_check)


def _aa_check(inp, a, want, got):
    aa, st = got
    taa.compare(aa, want[0], want[1], inp.label)
    assert st["edges_examined"] == int(want[1].sum()) and st["iterations"] == 1 and st["kernel_ms"] > 0


def _aa_call(g, inp, a):
    aa = g.adamic_adar()
    return aa, g.last_stats


row("adamic_adar", [("D", {}), ("S", {})], _aa_call,
    lambda inp, a: _frozen(*aa_vectorised(inp.begin, inp.idx)),
    lambda inp, a, w: (w[0].copy(), stats(edges_examined=int(w[1].sum()), iterations=1)), _aa_check)


# v_cover, random_bipartite_matching
def _vc_model(inp, a):
    want = v_cover_ref(inp.begin, inp.idx)
    return want[0], _frozen(want[1])[0]


row("v_cover", [("D", {}), ("B", {})], lambda g, inp, a: g.v_cover(), _vc_model,
    lambda inp, a, w: (w[1].copy(), w[0], stats(vertices_reached=w[0], edges_reached=int(w[1].sum())), {}),
    lambda inp, a, want, got: tvc.check(want, got[0], got[1], got[2]), log=("GMX_VC_LOG", last_line(tvc.LINE, tvc.FIELDS, keep=("plan", "build_ms", "grid_ms", "tail_ms", "finish_ms"))))
row("random_bipartite_matching", [("B", {"left": 2}), ("B", {"left": 4})],
    lambda g, inp, a: g.random_bipartite_matching(lefts(inp.label, a["left"])),
    lambda inp, a: rbm_model(inp.begin, inp.idx, lefts(inp.label, a["left"])),
    lambda inp, a, w: (w[1].copy(), w[0], stats(vertices_reached=w[0], iterations=w[2], edges_reached=w[3])),
    lambda inp, a, want, got: rbm.check(want, *got))


# the sampling programs: the one-thread loops, as bytes
def _walk_check(inp, a, want, got):
    tsa.same(got, want)
    st = got[5]
    assert (st["iterations"], st["vertices_reached"], st["edges_examined"]) == (want[3], want[2], want[3] * a["tokens"])


row("random_walk_sampling", [("D", {"p_size": 0.3, "p_jump": 0.15, "tokens": 64, "x": sc.X0}), ("D", {"p_size": 0.2, "p_jump": 0.3, "tokens": 3000, "x": sc.X0 + 5})],
    lambda g, inp, a: g.random_walk_sampling(a["p_size"], a["p_jump"], a["tokens"], a["x"]),
    lambda inp, a: sc.walk_loop(inp.begin, inp.idx, a["p_size"], a["p_jump"], a["tokens"], INT_MAX, a["x"]),
    lambda inp, a, w: (w[0].copy(), w[1].copy(), w[2], w[3], w[4], stats(iterations=w[3], vertices_reached=w[2], edges_examined=w[3] * a["tokens"])),
    _walk_check)


def _node_check(inp, a, want, got):
    sel, cnt, x, st = got
    assert sel.dtype == np.uint8 and sel.tobytes() == want[0].tobytes() and (cnt, x) == want[1:] and st["vertices_reached"] == cnt


row("node_sampling", [("D", {"by_degree": 0, "N": 7, "x": sc.X0}), ("D", {"by_degree": 1, "N": 1000, "x": sc.X0 + 9})],
    lambda g, inp, a: g.node_sampling(a["by_degree"], a["N"], a["x"]),
    lambda inp, a: sc.node_loop(inp.begin, a["by_degree"], a["N"], a["x"]),
    lambda inp, a, w: (w[0].copy(), w[1], w[2], stats(vertices_reached=w[1], iterations=1)), _node_check)


# the plan triangle_counting_directed, clustering and ktruss share; each with its own order knob
def _tcd_check(inp, a, want, got):
    assert got[0] == want
    ttd.check_stats(got[1])


def _tcd_line(err):
    """The last line's fields; built = 1 when any of the step's calls (one per part) built the plan."""
    f = last_line(ttd.LINE, ttd.FIELDS, keep=("order", "build_ms"))(err)
    f["built"] = max(int(line[ttd.FIELDS.index("built")]) for line in ttd.LINE.findall(err))
    return f


row("triangle_counting_directed", [("D", {"nparts": 1}), ("S", {"nparts": 1}), ("D", {"nparts": 3}), ("D", {"nparts": 1, "_env": {"GMX_TCD_NO_ORDER": "1"}})],
    _parts_call("triangle_counting_directed"), lambda inp, a: tcd_ref(inp.begin, inp.idx),
    lambda inp, a, w: (w, stats(iterations=1), {}), _tcd_check, log=("GMX_TCD_LOG", _tcd_line))


def _lcc_fake(inp, a, w):
    f = {"up": w["up"], "order": "degree", "staged": w.get("items", 0), "memory": 0, "alone": w.get("slots", 0), "list": 0, "tail": 0, "hub": 0, "empty": 0}
    return w["tri"].copy(), w["deg"].copy(), w["lcc"].copy(), w["triangles"], w["wedges"], stats(iterations=1, vertices_reached=int((w["tri"] > 0).sum())), f


# (D read as an undirected simple graph is S: the argument set that differs runs on B, which has no triangle)
row("clustering", [("S", {}), ("B", {}), ("D", {}), ("D", {"_env": {"GMX_LCC_NO_ORDER": "1"}})], lambda g, inp, a: g.clustering(),
    lambda inp, a: clustering_model(inp.V, inp.begin, inp.idx), _lcc_fake,
    lambda inp, a, want, got: tlc.agrees(got, want), log=("GMX_LCC_LOG", named_line(tlc.LOG, keep=("order", "w"))))


def _kt_fake(inp, a, w):
    f = {k: w[k] for k in ("triangles", "levels", "rounds", "slots", "top", "scanned")}
    return w["truss"].copy(), w["support"].copy(), w["max_truss"], w["num_edges"], stats(iterations=w["rounds"], edges_examined=w["slots"], vertices_reached=w["top"]), f


row("ktruss", [("S", {}), ("D", {}), ("D", {"_env": {"GMX_KTRUSS_NO_ORDER": "1"}})], lambda g, inp, a: g.ktruss(),
    lambda inp, a: ktruss_model(inp.V, inp.begin, inp.idx), _kt_fake,
    lambda inp, a, want, got: tkt.agrees(got, want), log=("GMX_KTRUSS_LOG", named_line(tkt.LOG, keep=("order", "support"))))


# biconnected: the oracle's arrays and counts, the schedule model's forest
def _bicc_model(inp, a):
    return hopcroft_tarjan(inp.V, inp.begin, inp.idx), forest_model(inp.V, inp.begin, inp.idx)


def _bicc_result(raw, f):
    bridge, artic, block, tecc, nblocks, nbridges, nartic, ntecc, st = raw
    assert bridge.dtype == bool and artic.dtype == bool and block.dtype == np.int32 and tecc.dtype == np.int32
    return {"bridge": bridge.astype(np.uint8), "artic": artic.astype(np.uint8), "block": block, "tecc": tecc, "num_blocks": nblocks,
            "num_bridges": nbridges, "num_artic": nartic, "num_tecc": ntecc, "stats": st, "log": f}


def _bicc_fake(inp, a, w):
    want, model = w
    out = {k: want[k].copy() for k in tbi.ARRAYS}
    out.update({k: want[k] for k in ("num_blocks", "num_bridges", "num_artic", "num_tecc")})
    out.update(stats=stats(), log={k: model[k] for k in ("levels", "roots", "tree", "walks")})
    return out


row("biconnected", [("S", {}), ("D", {})], lambda g, inp, a: g.biconnected(), _bicc_model, _bicc_fake,
    lambda inp, a, want, got: tbi.agrees(got, want[0], want[1]), log=("GMX_BICC_LOG", named_line(tbi.LOG)))


def with_log(entry, raw, err):
    """What a logged row's checker is given: the entry's result and the fields of the line it printed (err: its stderr)."""
    f = ROWS[entry].log[1](err)
    return _bicc_result(raw, f) if entry == "biconnected" else tuple(raw) + (f,)


# ---------------------------------------------------------------- the state objects of held_state
def _bfs_state_check(inp, a, want, got):
    if a["op"] == "download":
        _dist_check(inp, a, want, got)
    else:
        assert got is None


row("bfs_state", [("D", {"op": "download", "root": hub("D", 2)}), ("D", {"op": "download", "root": hub("D", 60)}),
                  ("D", {"op": "start", "root": hub("D", 2)}), ("D", {"op": "step"})],
    None, lambda inp, a: po.bfs_queue(inp.og, a["root"]) if a["op"] == "download" else None,
    lambda inp, a, w: None if w is None else (w.copy(), stats()), _bfs_state_check, table=EXTRA)

PR_STATE_ELEM = 8


def _pr_state_check(inp, a, want, got):
    if a["op"] == "download":
        assert rel_err(got, want) < PR_RTOL_F64, rel_err(got, want)   # test_gpu_parity's bar for the stepping API
    else:
        assert got is None


row("pr_state", [("D", {"op": "download", "steps": 3}), ("D", {"op": "download", "steps": 6}), ("D", {"op": "reset"}), ("D", {"op": "step"})],
    None, lambda inp, a: _frozen(po.pagerank(inp.og, 1e-300, 0.85, a["steps"])[0])[0] if a["op"] == "download" else None,
    lambda inp, a, w: None if w is None else w.copy(), _pr_state_check, table=EXTRA)


# ---------------------------------------------------------------- refusals by argument checks (GMX_ERR_ARG, before any work)
# key -> (the entry, the call that must be refused, a word of its message); each is one its entry's own tests expect
def _bad_len(g, inp):
    bad = lengths(inp.label, 13).copy()
    bad[inp.E // 2] = -1
    return g.sssp_path(bad, hub("D"))


def _bad_cost(value):
    def call(g, inp):
        bad = costs(inp.label, 15).copy()
        bad[inp.E // 3] = value
        return g.sssp_path_f64(bad, hub("D"), -1)
    return call


REFUSALS = collections.OrderedDict([
    ("sssp_path:negative_len", ("sssp_path", _bad_len, "len")),
    ("sssp_path_f64:negative_cost", ("sssp_path_f64", _bad_cost(-0.5), "cost")),
    ("sssp_path_f64:nan_cost", ("sssp_path_f64", _bad_cost(float("nan")), "cost")),
    ("sssp_path_f64:end_out_of_range", ("sssp_path_f64", lambda g, inp: g.sssp_path_f64(costs(inp.label, 15), hub("D"), inp.V), "end")),
    ("triangle_counting:part", ("triangle_counting", lambda g, inp: g.triangle_counting(3, 3), "part")),
    ("triangle_counting_directed:part", ("triangle_counting_directed", lambda g, inp: g.triangle_counting_directed(2, 2), "part")),
    ("bc_batch:width", ("bc_batch", lambda g, inp: g.bc_batch(pivots(inp.label, 3, 20), True, 3), "width")),
])


def refusal_message(key):
    """What gmx.GmxError says for the refused call (the fake device's answer)."""
    return "gmx status %d: %s" % (GMX_ERR_ARG, REFUSALS[key][2])


def check_refusal(key, message):
    assert isinstance(message, str) and message.startswith("gmx status %d:" % GMX_ERR_ARG) and REFUSALS[key][2] in message, message


# ---------------------------------------------------------------- steps, references, the runner
def table(entry):
    return ROWS[entry] if entry in ROWS else EXTRA[entry]


def args_of(step):
    label, a = table(step.entry).args[step.k]
    inp = input_of(step.handle)
    assert inp.label == label or (inp.label, label) == ("R", "D"), step
    return inp, a


_WANT = {}


def want_of(entry, k, label):
    """The CPU model's result for an argument set on an input: computed once, shared, left unchanged."""
    r = table(entry)
    a = {x: v for x, v in r.args[k][1].items() if x != "_env"}   # (a knob changes how a result is computed, not the result)
    key = (entry, label, repr(sorted(a.items())))
    if key not in _WANT:
        _WANT[key] = r.model(inputs()[label], a)
    return _WANT[key]


def check_step(step, result):
    """The reference is the CPU model for the step's arguments, never a result from the device."""
    if isinstance(step.k, str):
        return check_refusal(step.k, result)
    inp, a = args_of(step)
    table(step.entry).check(inp, a, want_of(step.entry, step.k, inp.label), result)


def fake_call(step):
    """A device that is always right: the model's own result in the form the entry returns it."""
    if isinstance(step.k, str):
        return refusal_message(step.k)
    inp, a = args_of(step)
    return table(step.entry).fake(inp, a, want_of(step.entry, step.k, inp.label))


def describe(step):
    return "%s[%s]@%s" % step


class SequenceFailure(AssertionError):
    def __init__(self, index, step, before, cause):
        self.index, self.step, self.before, self.cause = index, step, list(before), cause
        AssertionError.__init__(self, "step %d %s failed: %r\n  after %s" % (index, describe(step), cause, [describe(s) for s in before] or "nothing"))


def run(sequence, call, check):
    """call(step), then check(step, result), for every step in order; the first failure names its step and the steps before it."""
    done = []
    for n, step in enumerate(sequence):
        try:
            check(step, call(step))
        except Exception as e:   # whatever a checker or a call raises: the step failed
            raise SequenceFailure(n, step, done, e) from e
        done.append(step)
    return len(done)


# ---------------------------------------------------------------- the named sequences (plain data)
def first_on(entry, label, nth=0):
    """The nth argument set of an entry that runs on the input (the last one there when it has fewer)."""
    ks = [k for k, (lab, a) in enumerate(table(entry).args) if lab == label and set(a.get("_env", {})) <= {"GMX_SSSP_PATH_SCHEDULE"}]
    return ks[min(nth, len(ks) - 1)] if ks else None


def home(entry, k):
    return table(entry).args[k][0]


def pass_over(names, k):
    return [Step(e, k, home(e, k)) for e in names]


def forward():
    return pass_over(list(ROWS), 0)


def reverse():
    return pass_over(list(ROWS)[::-1], 1)


def shuffled():
    order = [list(ROWS)[i] for i in np.random.default_rng(2012).permutation(len(ROWS))]
    return pass_over(order, 0) + pass_over(order, 1)


# the groups of entries that share state on a handle (csrc/gmx_internal.h, struct gmx_graph), and the input each runs on
GROUPS = collections.OrderedDict([
    ("traversal", ("D", ("hop_dist", "bfs_levels", "bc", "bc_batch", "bc_all", "scc", "closeness"))),
    ("counting", ("S", ("triangle_counting", "triangle_counting_cn", "common_nbrs", "adamic_adar"))),
    ("tcd_plan", ("D", ("triangle_counting_directed", "clustering", "ktruss"))),
    ("pagerank", ("D", tuple("pagerank/%d" % k for k in range(len(PR_ARGS))))),
])
NO_ORDER = {"triangle_counting_directed": "GMX_TCD_NO_ORDER", "clustering": "GMX_LCC_NO_ORDER", "ktruss": "GMX_KTRUSS_NO_ORDER"}


def _knobbed(entry):
    return next(k for k, (_, a) in enumerate(ROWS[entry].args) if NO_ORDER[entry] in a.get("_env", {}))


def family(group, a, b):
    """a, b, a on a fresh handle with differing arguments; the plan's trio as a, b, a and b under their own order knobs, a:
    built, reused, rebuilt for the other order, reused, rebuilt."""
    label, members = GROUPS[group]
    assert a in members and b in members and a != b
    h = "%s#%s" % (label, group)
    if group == "pagerank":
        ka, kb = int(a.split("/")[1]), int(b.split("/")[1])
        return [Step("pagerank", ka, h), Step("pagerank", kb, h), Step("pagerank", ka, h)]
    if group == "tcd_plan":
        return [Step(a, first_on(a, label), h), Step(b, first_on(b, label), h), Step(a, _knobbed(a), h), Step(b, _knobbed(b), h), Step(a, first_on(a, label, 1), h)]
    return [Step(a, first_on(a, label), h), Step(b, first_on(b, label), h), Step(a, first_on(a, label, 1), h)]


def families(group, first=None):
    """Every ordered pair of the group (or those that begin with `first`), each on a handle of its own."""
    members = GROUPS[group][1]
    return [family(group, a, b) for a, b in itertools.permutations(members, 2) if first in (None, a)]


def plan_builds(steps):
    """built (1 / 0) the log line of every step of a tcd_plan family must report: a handle's plan is built at the first
    call and again whenever the calling entry's own knob asks for the other order."""
    order, out = None, []
    for s in steps:
        wanted = "identity" if NO_ORDER[s.entry] in ROWS[s.entry].args[s.k][1].get("_env", {}) else "degree"
        out.append(int(order != wanted))
        order = wanted
    return out


R_ENTRIES = ("hop_dist", "sssp", "sssp_path", "sssp_path_f64", "bidir_dijkstra", "scc", "pagerank")
DS_ENTRIES = ("triangle_counting", "triangle_counting_cn", "common_nbrs", "common_nbr_counts", "adamic_adar", "triangle_counting_directed",
              "clustering", "ktruss", "biconnected")


def two_handles():
    """(D and its second upload R with e_idx2idx, D and S): the steps alternate between the two handles."""
    dr = [Step(e, first_on(e, "D", n), h) for n in (0, 1) for e in R_ENTRIES for h in ("D", "R")]
    ds = [Step(e, first_on(e, h, n), h) for n in (0, 1) for e in DS_ENTRIES for h in ("D", "S")]
    return dr, ds


def held_state():
    """(routes, bfs, pagerank): two Route objects with different weights whose queries interleave with the other weighted
    searches; a BfsState stepped level by level and a PageRankState stepped with other traversals / pagerank() between."""
    q = [Step("route_query", n, "D") for n in range(len(EXTRA["route_query"].args))]
    between = [Step("bidir_dijkstra", 0, "D"), Step("sssp", 0, "D"), Step("sssp_path", 0, "D"), Step("sssp_path", 1, "D"), Step("sssp_path_f64", 0, "D"),
               Step("bidir_dijkstra", 1, "D"), Step("sssp_path_f64", 1, "D"), Step("sssp", 1, "D")]
    routes = [s for pair in zip(q, between) for s in pair]
    visitors = itertools.cycle([Step("hop_dist", 0, "D"), Step("bc", 0, "D"), Step("scc", 0, "D"), Step("hop_dist", 1, "D"), Step("bc", 1, "D")])
    bfs = [Step("bfs_state", 2, "D")]
    for _ in range(BFS_STATE_STEPS):
        bfs += [Step("bfs_state", 3, "D"), next(visitors)]
    bfs.append(Step("bfs_state", 0, "D"))
    pr = [Step("pr_state", 2, "D")]
    for n in range(6):
        pr += [Step("pr_state", 3, "D"), Step("pagerank", n % 4, "D")]
        if n == 2:
            pr.append(Step("pr_state", 0, "D"))
    pr.append(Step("pr_state", 1, "D"))
    return routes, bfs, pr


BFS_STATE_STEPS = 12   # more levels than any traversal of D has: a step past the last level finds nothing


def refused():
    """After every refused call the same entry's next good call, then one other entry, on the same handle."""
    other = {"sssp_path": "sssp", "sssp_path_f64": "sssp_path", "triangle_counting": "triangle_counting_cn",
             "triangle_counting_directed": "clustering", "bc_batch": "hop_dist"}
    out = []
    for n, (key, (entry, _, _)) in enumerate(REFUSALS.items()):
        label = "S" if entry == "triangle_counting" else "D"
        out += [Step(entry, key, label), Step(entry, first_on(entry, label, n % 2), label), Step(other[entry], first_on(other[entry], label), label)]
    return out


def all_sequences():
    """name -> steps, for the checks that need every sequence at once."""
    out = collections.OrderedDict([("forward", forward()), ("reverse", reverse()), ("shuffled", shuffled()), ("refused", refused())])
    for group in GROUPS:
        for n, steps in enumerate(families(group)):
            out["families/%s/%d" % (group, n)] = steps
    for name, seqs in (("two_handles", two_handles()), ("held_state", held_state())):
        for n, steps in enumerate(seqs):
            out["%s/%d" % (name, n)] = steps
    return out
