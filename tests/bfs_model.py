"""hop_dist's level schedule (csrc/gmx_bfs.hip: gmx_bfs_start / gmx_bfs_step_begin / gmx_bfs_step_end) restated in numpy: no
device, no oracle library.  Given the CSRs as the device stores them it predicts, level by level, which form
gmx_bfs_step_begin takes, how many entries the level's kernel inspects and what it finds -- all of it integer-exact, because
the direction decisions depend on counts only and every counter is a sum over sets that do not depend on the order in which
the device's appends fill a queue.

    run(begin, node_idx, r_begin, r_node_idx, rows_sorted, root, rank, nranks, plain, hub_min_v) -> Result
      .dist     hop levels, INT_MAX = unreached
      .stats    iterations, vertices_reached, edges_reached, edges_examined (this rank's, as gmx_bfs_download reports it)
      .levels   one Level(level, direction, form, frontier, frontier_edges, inspected, next_frontier, encoding) per level
      .detail   per level, what the boundary facts of test_bfs_model_host.py are derived from

`form` is one of FORMS; a bottom-up form is followed by where its frontier bitmap came from (ORIGINS), a top-down form
by ` from-bitmap` when its queue was rebuilt from the bitmap a bottom-up level found.  `encoding` is how the bottom-up hints
are coded (None: vertex ids with the only-flag and no hub list, what graphs under BFS_HUB_MIN_V vertices get);
`frontier_edges` is None in a bottom-up level, which never counts them."""
import collections

import numpy as np

INT_MAX = 2**31 - 1
# the constants of the schedule, named as in csrc/gmx_bfs.hip / csrc/gmx_frontier.h
BFS_ITEMS = 2048            # merge-path items per workgroup (also the slots per workgroup of the level out of the root)
BFS_SMALL_SCAN = 16384      # queues up to here: offsets by the single-workgroup scan
BFS_SPARSE_OWN = 16         # out-edges a lane of the sparse kernel walks before the wave takes the rest of a row
BFS_HINT_SCAN = 32          # in-row entries the hint is chosen from
BFS_BU_OWN = 32             # in-row entries a vertex walks alone before its wave helps
BFS_HUBS = 131072
BFS_HUB_MIN_V = 1 << 25
TOPDOWN_TO_BOTTOMUP_V = 20  # bottom-up when the queue holds more than V / 20 vertices ...
TOPDOWN_TO_BOTTOMUP_E = 14  # ... or more than (E - explored) / 14 out-edges
BOTTOMUP_STAYS_V = 24       # a bitmap frontier stays bottom-up while it holds more than V / 24 vertices
SPARSE_MAX_N = 1 << 20      # sparse: n <= 2^20 && m_f <= 2 n + 1024


def sparse_rule(n, m_f):
    return n <= SPARSE_MAX_N and m_f <= 2 * n + 1024


def with_bm_rule(has_reverse, bm_clean, m_f, V):
    return has_reverse and bm_clean and m_f >= 64 and m_f >= V // 1024


FORMS = ["first", "first+bitmap", "sparse", "tiles/small-scan", "tiles/scan", "bottom-up/dist", "bottom-up/cand"]
ORIGINS = ["prewritten", "from-queue", "kept"]
ENCODINGS = [None, "plain", "hubs-mem", "hubs-lds"]

Level = collections.namedtuple("Level", "level direction form frontier frontier_edges inspected next_frontier encoding")
Result = collections.namedtuple("Result", "dist stats levels detail")


def build_csr(V, src, dst):
    """(begin, node_idx, r_begin, r_node_idx) of an edge list, every row ascending: the sort every upload form applies."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    o = np.lexsort((dst, src))
    begin = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int32)
    r = np.lexsort((src, dst))
    r_begin = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=V))]).astype(np.int32)
    return begin, dst[o].astype(np.int32), r_begin, src[r].astype(np.int32)


def gather_rows(begin, idx, q):
    """the entries of the rows q[], concatenated"""
    b, d = begin[q].astype(np.int64), (begin[q + 1] - begin[q]).astype(np.int64)
    n = int(d.sum())
    if n == 0:
        return np.empty(0, idx.dtype)
    start = np.repeat(b - np.concatenate([[0], np.cumsum(d)[:-1]]), d)
    return idx[start + np.arange(n)]


def hints(begin, r_begin, r_node_idx):
    """bfs_hint_kernel: of the first BFS_HINT_SCAN entries of the in-row the FIRST with the largest out-degree; -1: no in-edges"""
    V = len(begin) - 1
    deg, indeg = np.diff(begin).astype(np.int64), np.diff(r_begin).astype(np.int64)
    best, best_deg = np.full(V, -1, np.int64), np.full(V, -1, np.int64)
    for k in range(BFS_HINT_SCAN):
        ok = indeg > k
        if not ok.any():
            break
        w = r_node_idx[np.where(ok, r_begin[:-1].astype(np.int64) + k, 0)] if len(r_node_idx) else np.zeros(V, np.int64)
        upd = ok & (deg[w] > best_deg)
        best[upd], best_deg[upd] = w[upd], deg[w][upd]
    return best


def rows_ascending(begin, idx):
    """gmx_graph::rows_sorted as the upload's validation finds it: no row holds an entry smaller than the one before"""
    if len(idx) < 2:
        return True
    down = np.flatnonzero(idx[1:] < idx[:-1]) + 1          # slots smaller than the slot before
    return bool(np.isin(down, begin).all())                # ... all of them first slots of a row


def hub_threshold(begin):
    """out-degree of the BFS_HUBS-th vertex of the hub list's sort: a vertex strictly above it is a hub slot, one strictly
    below it is not; at the threshold itself the sort decides"""
    deg = np.sort(np.diff(begin))[::-1]
    return int(deg[BFS_HUBS - 1]) if len(deg) >= BFS_HUBS else -1


def bottomup_counts(r_begin, r_node_idx, hint, frontier, looking, only_flag):
    """One bottom-up level over the vertices looking[] (unvisited).  Returns per vertex of looking[] (found, inspected, detail
    columns): one hint probe per vertex with in-edges; where it misses and the vertex is not only-flagged, the entries walked
    up to and including the first hit among the first BFS_BU_OWN, then the wave part in steps of 64 entries, every entry of
    every step walked counted, up to and including the step with the first hit."""
    b = r_begin[looking].astype(np.int64)
    indeg = r_begin[looking + 1].astype(np.int64) - b
    has_in = indeg > 0
    h = hint[looking]
    hint_hit = has_in & frontier[np.where(has_in, h, 0)]
    only = has_in & (indeg == 1) & only_flag
    walks = has_in & ~hint_hit & ~only
    # the first in-row position whose vertex is in the frontier
    hits = np.flatnonzero(frontier[r_node_idx]) if len(r_node_idx) else np.empty(0, np.int64)
    if len(hits):
        at = np.searchsorted(hits, b)
        nxt = np.where(at < len(hits), hits[np.minimum(at, len(hits) - 1)], -1)
    else:
        nxt = np.full(len(b), -1, np.int64)
    pos = np.where((nxt >= 0) & (nxt < b + indeg), nxt - b, -1)   # -1: no parent in the row
    own = np.minimum(indeg, BFS_BU_OWN)
    own_hit = walks & (pos >= 0) & (pos < own)
    own_cnt = np.where(own_hit, pos + 1, own)
    wave = walks & ~own_hit & (indeg > BFS_BU_OWN)
    rest = indeg - BFS_BU_OWN
    wave_hit = wave & (pos >= 0)
    wave_cnt = np.where(wave_hit, np.minimum(rest, ((pos - BFS_BU_OWN) // 64 + 1) * 64), rest)
    inspected = has_in.astype(np.int64) + np.where(walks, own_cnt, 0) + np.where(wave, wave_cnt, 0)
    found = hint_hit | own_hit | wave_hit
    cols = dict(v=looking, indeg=indeg, hint=h, hint_hit=hint_hit, only=only, walks=walks, pos=pos, own_hit=own_hit, wave=wave,
                wave_hit=wave_hit, found=found, inspected=inspected)
    return found, inspected, cols


def run(begin, node_idx, r_begin=None, r_node_idx=None, rows_sorted=True, root=0, rank=0, nranks=1, plain=False,
        hub_min_v=BFS_HUB_MIN_V):
    begin, node_idx = np.asarray(begin), np.asarray(node_idx)
    V, E = len(begin) - 1, len(node_idx)
    has_reverse = r_begin is not None
    assert nranks == 1 or has_reverse
    deg = np.diff(begin).astype(np.int64)
    dist = np.full(V, INT_MAX, np.int32)
    levels, detail = [], []
    root_ok = 0 <= root < V
    if has_reverse:   # bfs_build_hints
        hint = hints(begin, r_begin, r_node_idx)
        hint_plain = plain or V > 0x3FFFFFFF
        hubs = (not hint_plain) and V >= hub_min_v and V > BFS_HUBS
    words = (V + 63) // 64
    slice_words = max((words + nranks - 1) // nranks, 1)
    v_lo = rank * slice_words * 64
    v_hi = v_lo + slice_words * 64
    # gmx_bfs_start
    level, reached, explored, edges = 0, (1 if root_ok else 0), 0, 0
    queue = np.array([root], np.int64) if root_ok else np.empty(0, np.int64)
    if root_ok:
        dist[root] = 0
    cur_edges = int(deg[root]) if root_ok else -1
    frontier_is_bitmap = frontier_bm_valid = cand_valid = False
    fr, bm_clean, first_bm_level = 0, [True, True], -1
    bm = [np.zeros(V, bool), np.zeros(V, bool)]   # the two bitmaps WITH whatever earlier levels left in them
    while len(queue) > 0:
        n = len(queue)
        # ---- gmx_bfs_step_begin
        m_f = None
        if frontier_is_bitmap:
            bottom_up = n > V // BOTTOMUP_STAYS_V
        else:
            m_f = cur_edges
            bottom_up = has_reverse and (n > V // TOPDOWN_TO_BOTTOMUP_V or m_f > (E - explored) // TOPDOWN_TO_BOTTOMUP_E)
            explored += m_f
        info = {}
        if bottom_up:
            form = "bottom-up/cand" if cand_valid else "bottom-up/dist"
            if frontier_bm_valid:
                origin = "kept"
            elif first_bm_level == level:
                origin = "prewritten"
            else:
                origin = "from-queue"
                if not bm_clean[fr]:
                    bm[fr][:] = False
                bm[fr][queue] = True
            bm_clean = [False, False]
            use_lds = hubs and not cand_valid and v_hi - v_lo >= hub_min_v
            encoding = "plain" if hint_plain else "hubs-lds" if use_lds else "hubs-mem" if hubs else None
            looking = np.flatnonzero(dist == INT_MAX)   # (from dist[] or from cand: the same set where a vertex has in-edges)
            found, insp, cols = bottomup_counts(r_begin, r_node_idx, hint, bm[fr], looking, not hint_plain)
            mine = (looking >= v_lo) & (looking < v_hi)
            inspected = int(insp[mine].sum())
            nxt = looking[found]
            dist[nxt] = level + 1
            bm[1 - fr][:] = False
            bm[1 - fr][nxt] = True
            fr = 1 - fr
            info = dict(cols, frontier=bm[1 - fr].copy(), mine=mine, v_lo=v_lo, v_hi=min(v_hi, words * 64), nw_last=slice_words % 4, cand=cand_valid)
            cand_valid = frontier_is_bitmap = frontier_bm_valid = True
            cur_edges = -1
            form = form + " " + origin
            direction = "bottom-up"
        else:
            direction, encoding, suffix = "top-down", None, ""
            cand_valid = False
            if frontier_is_bitmap:
                suffix = " from-bitmap"
                m_f = int(deg[queue].sum())   # bfs_bitmap_queue_kernel counts them
                frontier_is_bitmap = False
                explored += m_f
            frontier_bm_valid = False
            inspected = m_f
            if level == 0 and n == 1 and rows_sorted:
                row = node_idx[begin[root]:begin[root + 1]].astype(np.int64)
                won = (row != root) & (row != np.concatenate([[-1], row])[:len(row)])   # a repeat sits next to its copy
                nxt = row[won]
                assert len(np.unique(nxt)) == len(nxt)
                with_bm = with_bm_rule(has_reverse, bm_clean[fr], m_f, V) and m_f > 0
                if with_bm:
                    bm[fr][nxt] = True
                    bm_clean[fr] = False
                    first_bm_level = 1
                form = "first+bitmap" if with_bm else "first"
                info = dict(slots=m_f, self_loop=bool((row == root).any()), repeats=int((row[1:] == row[:-1]).sum()))
            else:
                nbr = gather_rows(begin, node_idx, queue).astype(np.int64)
                nxt = np.unique(nbr[dist[nbr] == INT_MAX])
                if sparse_rule(n, m_f):
                    form = "sparse"
                    info = dict(queue=queue, row_len=deg[queue], nbr=nbr)
                else:
                    form = "tiles/small-scan" if n <= BFS_SMALL_SCAN else "tiles/scan"
            form += suffix
            dist[nxt] = level + 1
            cur_edges = int(deg[nxt].sum())   # next_edges, summed from the winners' degrees
        # ---- gmx_bfs_step_end
        edges += inspected
        levels.append(Level(level, direction, form, n, None if bottom_up else m_f, inspected, len(nxt), encoding))
        detail.append(info)
        queue = nxt
        reached += len(nxt)
        level += 1
    stats = dict(iterations=level, vertices_reached=reached, edges_examined=edges,
                 edges_reached=int(deg[dist != INT_MAX].sum()))
    return Result(dist, stats, levels, detail)


def parse_debug(err):
    """The GMX_BFS_DEBUG lines of a captured stderr as Level records, in the order printed."""
    import re
    pat = re.compile(r"gmx bfs: level (\d+) (top-down|bottom-up): frontier (\d+) -> inspected (\d+), next frontier (\d+), "
                     r"form (\S+)((?: (?:prewritten|from-queue|kept|from-bitmap))?)((?: (?:plain|hubs-mem|hubs-lds))?)"
                     r"(?:, frontier edges (\d+))?$")
    out = []
    for line in err.splitlines():
        if not line.startswith("gmx bfs: level"):
            continue
        m = pat.match(line)
        assert m, line
        out.append(Level(int(m.group(1)), m.group(2), m.group(6) + m.group(7), int(m.group(3)),
                         int(m.group(9)) if m.group(9) is not None else None, int(m.group(4)), int(m.group(5)),
                         m.group(8).strip() or None))
    return out
