"""Designed graphs for the binned PageRank sweep (csrc/gmx_pr_cold.hip), and a host model of the plan it builds for them.

Options RELABEL | HOT_LDS | SLICED | COLD_PB, one rank.  The relabelling sorts by descending out-degree and, with four
slices, deals the j-th hottest vertex to position (j % 4) * 2048 + j // 4 for j < 8192: when exactly 8192 vertices have
out-edges they occupy positions 0 .. 8191, which is tile 0 for all four tile sizes (classed 32767 / 19447 sources for
fp32 / fp64, generic 31727 / 15351).  With one tile a (tile, row) pair is a row and its length the row's in-degree, so the
in-degree histogram decides how long every class stream is, i.e. how many whole super-steps (1024 groups = 32768 entries)
the phase-1 prefetch loop runs for every form.

  A    V = 300 000, 8192 sources drawn per edge with weights uniform(1, 3); rows = a random subset of all vertices
       (sources included, so their ranks move) with the in-degree histogram HIST_A.  Class streams E1 / E2 / E4 / E8 / H:
       5 / 4 / 3 / 2 / 1 whole super-steps plus a leftover of several blocks.  Class H pads every pair to whole lanes
       (9 edges take 16 entries), so the nine-edge rows alone weigh 16 entries each: 1400 of them, with the other H rows,
       give 46 400 entries (1400 * 16 + 100 * 56 + 20 * 200 + 4 * 1544 + 2 * 4112).  The H lengths sit on both sides of
       the lane multiple (8), the wave (64) and the plan-time cut at 512-entry blocks.  The generic pair form of the same
       graph is one stream of 16 super-steps: items of 5, 5, 5 and 1 at GMX_PR_COLD_CHUNK1 = 5120.
  B    V = 2^19, 8192 sources of out-degree 8 .. 18, uniformly random destinations: almost every (tile, row) pair is a
       single edge, so the tile is stored SINGLES (every edge an item of class E1: 3 super-steps plus a leftover), or in the
       edge form with GMX_PR_COLD_CLASS_DENSITY = 0.
  A'   A plus 8192 hotter sources (out-degree above every original one, destinations among A's rows).  With
       GMX_PR_COLD = 8192 the hot half stays with the pull sweep, the original sources are the cold ones and still one
       tile, and the finish is the unfused one.
  Am / Am'   A and A' with 8378 fewer rows of one in-edge, so that 300 active rows are left over for the last bin of
       either element type (262 444 = 16 * 16384 + 300 = 32 * 8192 + 300), and with the in-degrees dealt to the rows in
       descending order of vertex id instead of at random.  Stored SINGLES (GMX_PR_COLD_PAIR_X100 = 400) a bin then holds
       as many items as its rows have in-edges: bins of three kinds of size in one plan (see FINISH).

plan_model() restates, in numpy, the arithmetic of pr_cold_create for a plan of one tile: which tile mode, how long every
stream is, which segments the phase-1 items are cut into, how many items every bin holds and how phases 2-3 finish it.
The tests without a device assert the design against the model; the tests with one assert the model against
gmx_pr_cold_shape, so a graph that stopped exercising a path fails on either side."""
import functools

import numpy as np

NSRC = 8192
V_A, V_B = 300_000, 1 << 19
HIST_A = {1: 166840, 2: 66536, 3: 12538, 4: 12538, 5: 2123, 6: 2123, 7: 2123, 8: 4223, 9: 1400, 15: 100, 16: 100, 17: 100,
          63: 20, 64: 20, 65: 20, 511: 4, 512: 4, 513: 4, 1023: 2, 1025: 2, 2049: 2}
HIST_AM = dict(HIST_A)
HIST_AM[1] -= 8378
ITERS, DAMP = 4, 0.85
MIN_TERM = 1e-4                  # a row's smallest term / the row's sum: 100 x the fp32 bar

G, BLK_GROUPS, SUPER_GROUPS, FEW_SLOTS = 32, 16, 1024, 8
FORMS = ("edge", "pair", "E1", "E2", "E4", "E8", "H")
TILE_SRC = {(4, True): 32767, (8, True): 19447, (4, False): 31727, (8, False): 15351}   # (elem, every tile classed)
BINROWS = {4: 16384, 8: 8192}

# phase-2 / phase-3 settings per element type: GMX_PR_COLD_CHUNK (groups per chunk; a bin is split when it holds more
# than CHUNK * GMX_PR_COLD_SPLIT_X100 / 100 groups, 300 by default).  On A / A' a full bin holds binrows / 32 groups
# plus a few of padding (one item per row): 512+ / 256+.
#   sole    defaults (chunk 2048): no bin is split
#   few     a fifth of a full bin, rounded down to 8: six chunks
#   many    8 groups: 30 chunks and more
#   mixed   on Am / Am' stored SINGLES: a quarter of what a full bin of one-edge rows holds -- those bins 4 chunks, the
#           bins of two-edge rows 8, the bins of the longer rows more, the 300 rows of the last bin less than the threshold
FINISH = {"sole": {4: None, 8: None}, "few": {4: 96, 8: 48}, "many": {4: 8, 8: 8}, "mixed": {4: 128, 8: 64}}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rows_with_histogram(rng, V, hist, sorted_desc):
    """(row ids, in-degree of each): sum(hist.values()) distinct vertices; the in-degrees at random, or descending with the id."""
    n = sum(hist.values())
    rows = np.sort(rng.choice(V, n, replace=False))
    deg = np.repeat(np.array(list(hist.keys())), np.array(list(hist.values())))
    deg = np.sort(deg)[::-1].copy() if sorted_desc else rng.permutation(deg)
    return rows, deg


def _graph_a(hist, sorted_desc, seed):
    rng = np.random.default_rng(seed)
    srcs = np.sort(rng.choice(V_A, NSRC, replace=False))
    w = rng.uniform(1.0, 3.0, NSRC)
    rows, deg = _rows_with_histogram(rng, V_A, hist, sorted_desc)
    dst = np.repeat(rows, deg)
    src = srcs[rng.choice(NSRC, len(dst), p=w / w.sum())]
    return srcs, rows, src.astype(np.int64), dst.astype(np.int64)


def _add_hot(srcs, rows, src, dst, seed):
    """8192 more sources, each with one out-edge more than the busiest original source, destinations among `rows`."""
    rng = np.random.default_rng(seed)
    others = np.setdiff1d(np.arange(V_A), srcs)
    hot = np.sort(rng.choice(others, NSRC, replace=False))
    d = int(np.bincount(src, minlength=V_A).max()) + 1
    hsrc = np.repeat(hot, d)
    hdst = rows[rng.integers(0, len(rows), len(hsrc))]
    return np.concatenate([src, hsrc]), np.concatenate([dst, hdst])


@functools.lru_cache(maxsize=None)
def edges(name):
    """(V, src, dst) of a designed graph, int64, read-only."""
    if name in ("A", "A'"):
        srcs, rows, src, dst = _graph_a(HIST_A, False, 20240)
        if name == "A'":
            src, dst = _add_hot(srcs, rows, src, dst, 20241)
        return (V_A,) + _freeze(src, dst)
    if name in ("Am", "Am'"):
        srcs, rows, src, dst = _graph_a(HIST_AM, True, 20242)
        if name == "Am'":
            src, dst = _add_hot(srcs, rows, src, dst, 20243)
        return (V_A,) + _freeze(src, dst)
    assert name == "B"
    rng = np.random.default_rng(20244)
    srcs = np.sort(rng.choice(V_B, NSRC, replace=False))
    src = np.repeat(srcs, rng.integers(8, 19, NSRC))
    dst = rng.integers(0, V_B, len(src))
    return (V_B,) + _freeze(src.astype(np.int64), dst.astype(np.int64))


def hot_ids(name):
    """GMX_PR_COLD for the graph: the primed graphs leave their hotter half to the pull sweep."""
    return NSRC if name.endswith("'") else 0


@functools.lru_cache(maxsize=None)
def csr(name):
    """(V, begin, node_idx) with the rows ascending and every row's targets ascending."""
    V, src, dst = edges(name)
    order = np.lexsort((dst, src))
    begin = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int32)
    return (V,) + _freeze(begin, dst[order].astype(np.int32))


@functools.lru_cache(maxsize=None)
def row_term_ratio(name):
    """Over ITERS iterations in float64: the smallest (term / row sum) of any row, the fewest distinct contributions the
    sources hold at the start of an iteration after the first (a term that lands in the wrong row is then a different
    number from the one it displaces), and the final ranks."""
    V, src, dst = edges(name)
    order = np.argsort(dst, kind="stable")
    s, d = src[order], dst[order]
    first = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    rows = d[first]
    outdeg = np.bincount(src, minlength=V).astype(np.float64)
    rank = np.full(V, 1.0 / V)
    worst, distinct = np.inf, V
    for it in range(ITERS):
        contrib = np.divide(rank, outdeg, out=np.zeros(V), where=outdeg > 0)
        if it > 0:
            distinct = min(distinct, len(np.unique(contrib[outdeg > 0])))
        term = contrib[s]
        sums, mins = np.add.reduceat(term, first), np.minimum.reduceat(term, first)
        worst = min(worst, float((mins / sums).min()))
        rank = np.full(V, (1.0 - DAMP) / V)
        rank[rows] += DAMP * sums
    return worst, distinct, rank


def relabel(outdeg, ns=4, run=2048):
    """perm[v] = internal id of vertex v: descending out-degree (ties by id), dealt to `ns` slices in runs of `run` ids."""
    order = np.argsort(-outdeg.astype(np.int64), kind="stable")
    j = np.arange(len(outdeg), dtype=np.int64)
    sl, q = j % ns, j // ns
    perm = np.empty(len(outdeg), np.int64)
    perm[order] = ((q // run) * ns + sl) * run + q % run
    return perm


def _class_of_len(n):
    return np.select([n <= 1, n == 2, n <= 4, n <= 8], [1, 2, 3, 4], 5)


def _padded_len(cls, n):
    return np.where(cls == 5, (n + 7) // 8 * 8, 1 << (np.maximum(cls, 1) - 1))


def _ceil(a, b):
    return (a + b - 1) // b


@functools.lru_cache(maxsize=None)
def plan_model(name, elem, density=1, pair_x100=125, chunk1=None, chunk2=None, split_x100=300):
    """What pr_cold_create builds for the graph (one rank, every cold source in tile 0), as the dictionary
    PageRankState.cold_shape() returns, plus "bin_groups": the bin-major groups of every bin."""
    V, src, dst = edges(name)
    T = hot_ids(name)
    perm = relabel(np.bincount(src, minlength=V))
    psrc, pdst = perm[src], perm[dst]
    assert T % 8192 == 0 and psrc.max() < T + NSRC <= T + TILE_SRC[(elem, density == 1)]   # one tile holds every cold source
    active = np.unique(pdst)                                    # rows with in-edges, by internal id
    binrows = BINROWS[elem]
    nbins = _ceil(len(active), binrows)
    cold = psrc >= T
    a = np.searchsorted(active, pdst[cold])                     # active-row index of every binned edge
    prow, plen = np.unique(a, return_counts=True)               # the (tile, row) pairs: one tile, so one per row
    pbin = prow // binrows
    ne, npt, ncells = int(cold.sum()), len(prow), len(np.unique(pbin))
    mode = "pair" if ne * 100 >= pair_x100 * npt else "edge"
    if mode == "pair" and density > 0 and ne >= density * ncells:
        mode = "classed"
    elif mode == "edge" and density == 1:
        mode = "singles"
    if mode == "singles" or mode == "edge":                     # every edge an item
        prow, plen = np.sort(a), np.ones(len(a), np.int64)
        pbin = prow // binrows
    cls = _class_of_len(plen) if mode == "classed" else np.full(len(plen), 1 if mode == "singles" else 0)
    padded = _padded_len(cls, plen) if mode in ("classed", "singles") else plen
    # tile-major: cells (class, bin) in key order, each padded to whole groups; a stream to whole blocks / super-steps
    order = np.lexsort((prow, pbin, cls))
    cls, pbin, plen, padded = cls[order], pbin[order], plen[order], padded[order]
    cell = cls * nbins + pbin
    cfirst = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
    centries = np.add.reduceat(padded, cfirst)
    cgroups = _ceil(centries, G)
    ccls = cls[cfirst]
    stream_raw = np.bincount(ccls, weights=cgroups, minlength=6).astype(np.int64)
    unit = np.where(np.arange(6) == 0, SUPER_GROUPS if mode == "pair" else BLK_GROUPS, BLK_GROUPS)
    stream = _ceil(stream_raw, unit) * unit
    vstart = np.concatenate([[0], np.cumsum(stream)])
    # where every pair starts in its stream (entries), for the cuts at the ends of the 512-entry blocks
    cstart = np.concatenate([[0], np.cumsum(cgroups)])[:-1] * G                 # raw: cells follow each other ...
    cstart += (vstart[ccls] - np.concatenate([[0], np.cumsum(stream_raw)])[ccls]) * G   # ... streams start on their boundaries
    within = np.cumsum(padded) - padded
    within -= np.repeat(within[cfirst], np.diff(np.concatenate([cfirst, [len(padded)]])))
    pstart = np.repeat(cstart, np.diff(np.concatenate([cfirst, [len(padded)]]))) + within
    cut = (mode == "pair") | (cls == 5)
    items = 1 + np.where(cut, (pstart + plen - 1) // 512 - pstart // 512, 0)
    # phase-1 work items and the segments the kernel cuts them into
    ch1 = min(262144, max(SUPER_GROUPS, SUPER_GROUPS if chunk1 is None else chunk1)) // SUPER_GROUPS * SUPER_GROUPS
    groups = dict.fromkeys(FORMS, 0)
    steps = {f: set() for f in FORMS}

    def seen(form, n, nsuper):
        groups[form] += int(n)
        steps[form].add(min(int(nsuper), 31))

    if mode in ("classed", "singles"):
        g0, g1 = int(vstart[1]), int(vstart[6])
        for g in range(g0, g1, ch1):
            for c in range(1, 6):
                lo, hi = max(g, int(vstart[c])), min(g + ch1, g1, int(vstart[c + 1]))
                if lo < hi:
                    seen(FORMS[c + 1], hi - lo, (hi - lo) // BLK_GROUPS // 64)
    elif mode == "pair":
        for g in range(0, int(vstart[1]), ch1):
            n = min(ch1, int(vstart[1]) - g)
            seen("pair", n, n // SUPER_GROUPS)
    else:
        for g in range(0, int(stream_raw[0]), ch1):
            seen("edge", min(ch1, int(stream_raw[0]) - g), 0)
    # bin-major: a cell's items padded to whole groups, a bin's cells behind each other
    citems = np.add.reduceat(items, cfirst)
    bin_groups = np.bincount(pbin[cfirst], weights=_ceil(citems, G), minlength=nbins).astype(np.int64)
    ch2 = min(32768, max(8, 2048 if chunk2 is None else chunk2)) // 8 * 8
    thr2 = ch2 * split_x100 // 100
    live = bin_groups[bin_groups > 0]
    nslots = _ceil(live[live > thr2], ch2)
    return {"groups": groups, "supersteps": steps, "items2_sole": int((live <= thr2).sum()), "items2_chunk": int(nslots.sum()),
            "bins_few": int((nslots <= FEW_SLOTS).sum()), "bins_many": int((nslots > FEW_SLOTS).sum()),
            "tiles_by_mode": {m: int(m == mode) for m in ("edge", "pair", "classed", "singles")},
            "fused": T == 0 and bool((bin_groups > 0).all()), "bin_groups": bin_groups, "nactive": len(active)}
