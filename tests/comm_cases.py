"""gmx_communities' paths (csrc/gmx_comm.hip) without a device: the kernels' constants read from the source, the host loop
restated with its work list (work_model: which rows every round evaluates, in which regime, and what it changes), order-free
bounds on when a label table fills, and the graphs that reach the loops no other test reaches.  test_comm_cases_host.py proves
from these which path every case takes; test_gpu_comm_paths.py runs them.

Nothing here simulates an insertion order: the device has none.  What is order-free about an open-addressing table with linear
probing is (1) more distinct labels than slots cannot fit, (2) more than COMM_PROBES labels on ONE start slot cannot fit (the
last of them to claim a slot has passed the others), (3) the SET of slots that end up occupied is the same under every order
(and under concurrent compare-and-swap claims, which are some order), and an insert only ever steps over slots of its own
final cluster of occupied slots: where every cluster is at most COMM_PROBES long, no insert runs out of probes."""
import collections
import functools
import os
import re

import numpy as np

from conftest import ROOT
from test_communities_host import csr, fmix32, half_of

SRC = os.path.join(ROOT, "green-marl_amd", "csrc", "gmx_comm.hip")
HUGE = 1 << 30


def _constants():
    text = open(SRC).read()
    names = ["COMM_THREADS", "COMM_COMPACT_THREADS", "COMM_CHUNK", "COMM_PROBES", "COMM_STAGE", "COMM_WAVE_MIN", "COMM_BLOCK_MIN",
             "COMM_LDS_SLOTS", "COMM_LDS_SLOTS_MIN", "COMM_REV_BLOCK", "COMM_WAVE_SHARE"]
    k = {}
    for n in names:
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % n, text, re.M)
        assert len(m) == 1, n
        k[n] = int(m[0])
    grids = dict(re.findall(r"const int (\w+)_grid = comm_grid\([^;]*,\s*(\d+)\);", text))
    assert sorted(grids) == ["block", "compact", "list", "row", "wave", "word"], grids
    k["GRID"] = {n: int(v) for n, v in grids.items()}
    return k


K = _constants()
COMM_THREADS, COMM_PROBES, COMM_STAGE = K["COMM_THREADS"], K["COMM_PROBES"], K["COMM_STAGE"]
COMM_WAVE_MIN, COMM_BLOCK_MIN, COMM_LDS_SLOTS = K["COMM_WAVE_MIN"], K["COMM_BLOCK_MIN"], K["COMM_LDS_SLOTS"]
COMM_LDS_SLOTS_MIN, COMM_REV_BLOCK, COMM_WAVE_SHARE = K["COMM_LDS_SLOTS_MIN"], K["COMM_REV_BLOCK"], K["COMM_WAVE_SHARE"]
GRID = K["GRID"]
WAVES = COMM_THREADS // 64
SHORT_ROWS_PER_PASS = GRID["row"] * WAVES * 4          # comm_short_kernel: four rows per wave and trip
WAVE_ROWS_PER_PASS = GRID["wave"] * WAVES              # comm_wave_kernel: a row per wave and trip
# comm_stage_push flushes inside the loop once a wave has staged more than COMM_STAGE - 64 entries
STAGE_FLUSH_AT = COMM_STAGE - 64


def block_grid(V):
    return max(1, min(V, GRID["block"]))


def table_for(length, cap):
    """comm_table_for"""
    while cap > 64 and cap // 8 >= length:
        cap >>= 1
    return cap


def lp0_of(length, cap):
    """comm_overflow_kernel's first class level of a row"""
    lp0 = 0
    while lp0 < 31 and (length >> lp0) > cap // 2:
        lp0 += 1
    return lp0


# ---------------------------------------------------------------------------------------------------- table bounds

def clusters(starts, cap):
    """Lengths of the maximal runs of occupied slots (cyclic) after the labels with these start slots are in a table of cap
    slots with linear probing -- the same under every insertion order.  len(starts) <= cap."""
    cnt = np.bincount(np.asarray(starts, np.int64), minlength=cap).astype(np.int64)
    total = int(cnt.sum())
    assert total <= cap
    if total == cap:
        return [cap]
    # slot s is occupied iff labels start on it or are carried into it; one of them stays.  Some slot stays empty and carries
    # nothing on, so the first lap (which starts with nothing carried into slot 0) ends with what really wraps around.
    occ = np.zeros(cap, bool)
    carry = 0
    for lap in range(2):
        for s, n in enumerate(cnt.tolist()):
            have = n + carry
            occ[s] = have > 0
            carry = max(0, have - 1)
    assert int(occ.sum()) == total
    first = int(np.flatnonzero(~occ)[0])
    o = np.roll(occ, -first)                # starts with an empty slot
    edges = np.flatnonzero(np.diff(np.concatenate([[0], o.astype(np.int8), [0]])))
    return (edges[1::2] - edges[::2]).tolist()


def table_fate(labels, lp, cap):
    """'fills', 'fits' or 'open' for one count pass of DISTINCT labels (all of one class at level lp) into cap slots"""
    labels = np.unique(np.asarray(labels, np.int64))
    if len(labels) == 0:
        return "fits"
    if len(labels) > cap:
        return "fills"
    starts = ((fmix32(labels) >> np.uint64(lp)) & np.uint64(cap - 1)).astype(np.int64)
    limit = min(cap, COMM_PROBES)
    if np.bincount(starts).max() > limit:
        return "fills"
    return "fits" if max(clusters(starts, cap)) <= limit else "open"


def class_levels(labels, lp0, c0, cap):
    """Class c0 of an overflowed row at comm_overflow_kernel's levels lp0, lp0 + 1, ...: per level the list of (part, number of
    distinct labels, fate) up to and including the first part that fills -- the kernel stops a level there -- and the walk ends
    with the first level no part of which fills.  An 'open' part makes the walk undecidable: asserted away by the host test."""
    labels = np.unique(np.asarray(labels, np.int64))
    h = fmix32(labels).astype(np.int64)
    out = []
    for lp in range(lp0, 32):
        parts, full = [], False
        for c in range(c0, 1 << lp, 1 << lp0):
            mine = labels[(h & ((1 << lp) - 1)) == c]
            fate = table_fate(mine, lp, cap)
            parts.append((c, len(mine), fate))
            if fate != "fits":
                full = fate == "fills"
                break
        out.append((lp, parts))
        if not full:
            break
    return out


# ---------------------------------------------------------------------------------------------------- the host loop

Round = collections.namedtuple("Round", "short wave block slots changes ovf_lo ovf_hi")
Work = collections.namedtuple("Work", "rounds_log comm rounds converged changed_indeg evals slots half_rows")


def work_model(begin, node_idx, wave_min=COMM_WAVE_MIN, block_min=COMM_BLOCK_MIN, worklist=True, max_rounds=1000,
               lds_slots=COMM_LDS_SLOTS):
    """gmx_communities' host loop.  dirty starts as "has out-edges"; round r, half h evaluates S = dirty & half_of(v, r) == h,
    clears S from dirty, commits the changed vertices and -- with the work list -- marks the sources of every slot that points
    at one; without it dirty is "has out-edges" again at the start of every later round.  Per round: rows evaluated as short /
    wave / block by length (comm_compact_kernel's order: block_min first), slots, changes, and the two-sided bound on the rows
    whose table fills (more distinct labels than its table / more than COMM_PROBES).  evals / slots: the sums the library
    reports as vertices_reached / edges_examined.  When max_rounds cuts the run, converged comes from one pass over all dirty
    vertices that is neither counted nor committed.  changed_indeg: the in-degrees of the vertices that changed, per commit.
    half_rows: rows selected per half-round."""
    begin = np.asarray(begin, np.int64)
    node_idx = np.asarray(node_idx, np.int64)
    V = len(begin) - 1
    deg = np.diff(begin)
    src = np.repeat(np.arange(V, dtype=np.int64), deg)
    indeg = np.bincount(node_idx, minlength=V)
    has = deg > 0
    cap = COMM_LDS_SLOTS_MIN
    while cap * 2 <= lds_slots:
        cap *= 2
    # the table of a row by its length: none for short rows
    regime = np.where(deg >= block_min, 2, np.where(deg >= wave_min, 1, 0))
    tab = np.zeros(V, np.int64)
    for length in np.unique(deg[has & (regime > 0)]):
        m = has & (deg == length)
        tab[m & (regime == 1)] = table_for(int(length), cap // COMM_WAVE_SHARE)
        tab[m & (regime == 2)] = table_for(int(length), cap)
    comm = np.arange(V, dtype=np.int64)

    def evaluate(S):
        """(vertices that move, their labels, distinct labels per row of S as a V-array)"""
        keep = S[src]
        key, cnt = np.unique(src[keep] * V + comm[node_idx[keep]], return_counts=True)
        distinct = np.zeros(V, np.int64)
        if len(key) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), distinct
        ks, kl = key // V, key % V
        first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
        vs = ks[first]
        n = np.diff(np.concatenate([first, [len(key)]]))
        distinct[vs] = n
        mx = np.maximum.reduceat(cnt, first)
        top = cnt == np.repeat(mx, n)
        at = np.minimum.reduceat(np.where(top, np.arange(len(key)), len(key)), first)   # keys ascend: the smallest label at the top
        best = kl[at]
        me = vs * V + comm[vs]
        p = np.minimum(np.searchsorted(key, me), len(key) - 1)
        own = np.where(key[p] == me, cnt[p], 0)
        move = own != mx
        return vs[move], best[move], distinct

    dirty = has.copy()
    log, changed_indeg, half_rows = [], [], []
    rounds, fix = 0, False
    evals = slots = 0
    for r in range(max_rounds):
        if fix:
            break
        if not worklist and r > 0:
            dirty = has.copy()
        h = half_of(V, r)
        rec = np.zeros(7, np.int64)
        for half in (0, 1):
            S = dirty & (h == half) & has
            dirty &= ~S
            half_rows.append(int(S.sum()))
            mv, ml, distinct = evaluate(S)
            rec[:3] += np.bincount(regime[S], minlength=3)
            rec[3] += int(deg[S].sum())
            rec[4] += len(mv)
            table_rows = S & (regime > 0)
            rec[5] += int((table_rows & (distinct > tab)).sum())
            rec[6] += int((table_rows & (distinct > COMM_PROBES)).sum())
            comm[mv] = ml
            changed_indeg.append(indeg[mv])
            if worklist and len(mv):
                moved = np.zeros(V, bool)
                moved[mv] = True
                dirty[src[moved[node_idx]]] = True
        log.append(Round(*(int(x) for x in rec)))
        evals += int(rec[:3].sum())
        slots += int(rec[3])
        if rec[4] == 0:
            fix = True
        else:
            rounds += 1
    if not fix:
        if not worklist and max_rounds > 0:
            dirty = has.copy()
        mv, _, _ = evaluate(dirty & has)
        fix = len(mv) == 0
    comm = comm.astype(np.int32)
    comm.setflags(write=False)
    return Work(log, comm, rounds, int(fix), changed_indeg, evals, slots, half_rows)


# ---------------------------------------------------------------------------------------------------- graphs

def class_ids(V, bits, value, n):
    """the first n vertex ids in 1 .. V-1 with fmix32(id) & (2^bits - 1) == value"""
    ids = np.arange(1, V, dtype=np.int64)
    ids = ids[(fmix32(ids).astype(np.int64) & ((1 << bits) - 1)) == value]
    assert len(ids) >= n, (V, bits, value, len(ids))
    return ids[:n]


def one_row(V, row):
    """vertex 0 with this row; nobody else has out-edges"""
    return csr(V, np.zeros(len(row), np.int64), row)


SPLIT_CLASS = 5   # the label class (mod 8) all neighbours of the split rows fall into


def split_row_labels(cap):
    """The row of the split_count cases: 4 * cap distinct neighbours, all with fmix32(id) & 7 == SPLIT_CLASS, in
    V = 128 * cap vertices (cap 512: 2048 of the 8087 such ids below 65 536)."""
    return 128 * cap, class_ids(128 * cap, 3, SPLIT_CLASS, 4 * cap)


def deepest_parts(cap):
    """(deepest level, its parts in the order comm_overflow_kernel counts them) of the split_count row's class"""
    V, ids = split_row_labels(cap)
    lv = class_levels(ids, lp0_of(len(ids), cap), SPLIT_CLASS, cap)
    lp, parts = lv[-1]
    return lp, [c for c, _, _ in parts]


def _split_count(cap, variant):
    """Re-splitting a label class by COUNT.  A row of 4 * cap distinct labels fills the hub table (cap slots); lp0 is the
    first level with len >> lp0 <= cap / 2, i.e. 3, so there are 8 classes and ALL labels are in class 5: it holds 4 * cap
    labels at level 3, and by pigeonhole one of its 2 parts at level 4 more than cap and one of its 4 parts at level 5 at least
    cap (cap 512: 1057 + 991, then 524, 518, 533, 473; the kernel stops a level at the first part that fills).  Level 6's eight
    parts hold about cap / 2 each.  With fewer than 4 * cap labels lp0 would be 2 or level 5 could fit: this is the smallest
    row whose class must fill three times.  V = 128 * cap is what holds 4 * cap ids of one class mod 8 with room to spare.
    variant "distinct": every label once, the winner is the smallest.  "last": one neighbour of the part counted LAST at the
    deepest level is repeated, "middle": one of a part in the middle -- the winner is then not the smallest label; a merge that
    keeps only the first part's result misses both, one that keeps only the last part's misses the middle one."""
    V, ids = split_row_labels(cap)
    row = ids.copy()
    if variant != "distinct":
        lp, parts = deepest_parts(cap)
        part = parts[-1] if variant == "last" else parts[len(parts) // 2]
        mine = ids[(fmix32(ids).astype(np.int64) & ((1 << lp) - 1)) == part]
        w = int(mine[-1])
        row = np.insert(ids, len(ids) // 3, w)        # (the repeat apart from its first occurrence)
    return one_row(V, row)


PROBE_LABELS = 70


def probe_residue():
    """the first residue r whose first PROBE_LABELS ids with fmix32(id) & 511 == r fit at level 1 by the order-free condition"""
    cap = COMM_LDS_SLOTS_MIN
    for r in range(cap):
        ids = class_ids(65536, 9, r, PROBE_LABELS)
        lv = class_levels(ids, 0, 0, cap)
        if len(lv) == 2 and lv[0][1][-1][2] == "fills" and all(f == "fits" for _, _, f in lv[1][1]):
            return r, ids
    raise AssertionError("no residue fits")


def _split_probe():
    """Re-splitting by the PROBE LIMIT.  70 labels whose fmix32 agree in their low 9 bits start on one slot of a 512-slot table
    at level 0: more than COMM_PROBES = 64 on one start slot cannot fit, in comm_block_kernel and again in the overflow kernel's
    first pass (lp0 = 0: the row has COMM_BLOCK_MIN = 256 slots, not more than cap / 2).  At level 1 the start slot is bits 1..9:
    two slots 256 apart, clusters of about 35.  65 labels are the least that must fill; 70 leave either level-1 cluster room
    below 64.  The row is padded to COMM_BLOCK_MIN slots (the smallest hub row) with repeats, most of the largest labels, so
    that the winner is not the smallest."""
    r, ids = probe_residue()
    extra = COMM_BLOCK_MIN - PROBE_LABELS
    assert extra > 0
    row = np.concatenate([ids, ids[::-1][np.arange(extra) % PROBE_LABELS]])
    rng = np.random.default_rng(11)
    return one_row(65536, rng.permutation(row))


MANY_V, MANY_SLOTS = 600, 1 << 18


def many_classes_winner():
    """the smallest label of 1 .. 599 whose class at level 10 is one the first trip of a grid of 600 does not reach"""
    ids = np.arange(1, MANY_V, dtype=np.int64)
    lp0 = lp0_of(MANY_SLOTS, COMM_LDS_SLOTS_MIN)
    late = ids[(fmix32(ids).astype(np.int64) & ((1 << lp0) - 1)) >= block_grid(MANY_V)]
    return int(late[0])


def _many_classes():
    """More classes than workgroups.  The grid of the overflow kernel is min(V, 1024) workgroups and a row has 2^lp0 classes,
    lp0 the first level with len >> lp0 <= cap / 2 = 256: more classes than workgroups needs len > 256 * V -- with V = 600
    (599 possible labels, more than the 512 slots that must be exceeded for the row to overflow at all) a row of 2^18 slots,
    lp0 = 10, 1024 classes over 600 workgroups.  Every label 1 .. 599 occurs 437 times and the winner 381 times more; the
    winner's class is >= 600, reached only by `c0 += gridDim.x`."""
    w = many_classes_winner()
    per = MANY_SLOTS // (MANY_V - 1)
    row = np.concatenate([np.repeat(np.arange(1, MANY_V), per), np.full(MANY_SLOTS - per * (MANY_V - 1), w)])
    rng = np.random.default_rng(12)
    return one_row(MANY_V, rng.permutation(row))


MANY_OVF_V, MANY_OVF_DEG = 16384, 100


def _many_overflows():
    """More than COMM_THREADS overflowed rows in a half-round, and more rows than one pass of comm_wave_kernel.  Every vertex
    has 100 distinct out-neighbours: with every row in the wave kernel and the smallest tables (512 / 8 = 64 slots per wave)
    every row of round 0 holds 100 > 64 distinct labels and must overflow, about V / 2 per half-round.  V = 16 384 is the
    first power of two with V / 2 > 5120 rows per pass (1280 workgroups of four waves) -- which also makes 32 batches of 256
    overflowed rows, the rows from 1024 on dealt to workgroup i mod 1024."""
    V, d = MANY_OVF_V, MANY_OVF_DEG
    rng = np.random.default_rng(13)
    nb = rng.integers(0, V, (V, d))
    while True:
        nb.sort(axis=1)
        dup = np.zeros(nb.shape, bool)
        dup[:, 1:] = nb[:, 1:] == nb[:, :-1]
        if not dup.any():
            break
        nb[dup] = rng.integers(0, V, int(dup.sum()))
    nb = rng.permuted(nb, axis=1)
    return np.arange(0, V * d + 1, d, dtype=np.int32), np.ascontiguousarray(nb.reshape(-1), np.int32)


def pairs(V):
    """Edges 2k -> 2k+1 only.  Every even vertex changes in round 0 and nothing points at a vertex that changes."""
    begin = ((np.arange(V + 1, dtype=np.int64) + 1) // 2).astype(np.int32)
    return begin, np.arange(1, V, 2, dtype=np.int32)


def pairs_closed_form(V):
    """(comm, rounds, converged): comm[2k] = comm[2k+1] = 2k+1 after one round"""
    return (np.arange(V, dtype=np.int32) | 1), 1, 1


PAIRS_V = 1 << 23


def pairs_half_rows(V):
    """rows selected in the two half-rounds of round 0"""
    h = half_of(V, 0)[0::2]
    return int((h == 0).sum()), int((h == 1).sum())


COMMIT_INDEG = [16, 17, COMM_REV_BLOCK, COMM_REV_BLOCK + 1, 5000]
COMMIT_CENTRES = 8


def _commit_regimes():
    """The commit's reverse-row regimes at their boundaries: in-rows of 16 (a lane each), 17 and COMM_REV_BLOCK = 2048 (the
    wave), 2049 and 5000 (comm_commit_big_kernel: two strides of 4 * 256 slots and one more, then four and a tail).  Eight
    centres per in-degree, each with that many leaves pointing at it and one out-edge to a sink of its own, numbered by a fixed
    permutation that puts the centres 16 ids apart into the first 1024, the regimes alternating, leaves between them: their
    rows are neighbours in the row list and their changes reach the pending list together.  Every centre takes its
    sink's label in round 0; its leaves are then dirty whichever half they are in, and end with that label."""
    src, dst, nxt = [], [], 0
    for d in COMMIT_INDEG:
        for _ in range(COMMIT_CENTRES):
            centre, sink = nxt, nxt + 1
            leaves = nxt + 2 + np.arange(d)
            nxt += 2 + d
            src += [[centre], leaves]
            dst += [[sink], np.full(d, centre)]
    V = nxt
    # the centres (the vertices with an out-edge to a vertex without in-edges from leaves: every 2 + d-th id above) at ids
    # 5, 21, 37, ... in the order 16, 17, 2048, ... repeating; everybody else shuffled over the other ids
    centres = np.concatenate([[0], np.cumsum(np.repeat(np.array(COMMIT_INDEG) + 2, COMMIT_CENTRES))[:-1]])
    centres = centres.reshape(len(COMMIT_INDEG), COMMIT_CENTRES).T.reshape(-1)
    at = 5 + 16 * np.arange(len(centres))
    assert at[-1] < 1024
    perm = np.empty(V, np.int64)
    perm[centres] = at
    rest = np.setdiff1d(np.arange(V), centres)
    perm[rest] = np.random.default_rng(14).permutation(np.setdiff1d(np.arange(V), at))
    return csr(V, perm[np.concatenate(src).astype(np.int64)], perm[np.concatenate(dst).astype(np.int64)])


BUILDERS = {
    "split_count_512": lambda: _split_count(512, "distinct"),
    "split_count_512_last": lambda: _split_count(512, "last"),
    "split_count_512_middle": lambda: _split_count(512, "middle"),
    "split_count_4096": lambda: _split_count(4096, "last"),
    "split_probe": _split_probe,
    "many_classes": _many_classes,
    "many_overflows": _many_overflows,
    "commit_regimes": _commit_regimes,
    "pairs23": lambda: pairs(PAIRS_V),
}
CASES = list(BUILDERS)
MODEL_CASES = [c for c in CASES if c != "pairs23"]   # pairs23: its closed form

SMALL = {"GMX_COMM_LDS_SLOTS": str(COMM_LDS_SLOTS_MIN)}
ALL_WAVE = {"GMX_COMM_WAVE_MIN": "1", "GMX_COMM_BLOCK_MIN": str(HUGE)}
ALL_BLOCK = {"GMX_COMM_BLOCK_MIN": "1"}
# case -> the knob sets it runs under
RUNS = {
    "split_count_512": [SMALL],
    "split_count_512_last": [SMALL],
    "split_count_512_middle": [SMALL],
    "split_count_4096": [{}],
    "split_probe": [SMALL],
    "many_classes": [SMALL],
    "many_overflows": [dict(ALL_WAVE, **SMALL), {}],
    "commit_regimes": [{}],
    "pairs23": [{}, ALL_WAVE, ALL_BLOCK],
}
SPLIT_COUNT_CASES = [c for c in CASES if c.startswith("split_count")]
CUT_CASES = ["split_count_512_last", "many_classes", "many_overflows"]
UPLOAD_CASES = ["commit_regimes", "split_count_512_last"]


def knob_id(env):
    return ",".join("%s=%s" % (k[len("GMX_COMM_"):].lower(), "huge" if v == str(HUGE) else v) for k, v in sorted(env.items())) or "default"


@functools.lru_cache(maxsize=None)
def case(name):
    b, i = BUILDERS[name]()
    b, i = np.ascontiguousarray(b, np.int32), np.ascontiguousarray(i, np.int32)
    b.setflags(write=False)
    i.setflags(write=False)
    return b, i


_MODELS = {}


def model_of(name, begin, node_idx, env=None, worklist=True, max_rounds=1000):
    """work_model under a knob set, computed once per (graph name, knobs, work list, bound)"""
    env = env or {}
    key = (name, tuple(sorted(env.items())), worklist, max_rounds)
    if key not in _MODELS:
        _MODELS[key] = work_model(begin, node_idx, int(env.get("GMX_COMM_WAVE_MIN", COMM_WAVE_MIN)),
                                  int(env.get("GMX_COMM_BLOCK_MIN", COMM_BLOCK_MIN)), worklist, max_rounds,
                                  int(env.get("GMX_COMM_LDS_SLOTS", COMM_LDS_SLOTS)))
    return _MODELS[key]


def model(name, env=None, worklist=True, max_rounds=1000):
    return model_of(name, *case(name), env=env, worklist=worklist, max_rounds=max_rounds)
