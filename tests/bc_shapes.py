"""Designed graphs for comp_BC's per-seed visits (csrc/gmx_bfs.hip: bfs_visit_kernel / bfs_visit_big_kernel) and the
batched sweeps that promise its bytes, a census of the kernel forms a graph's rows take, and two models of comp_BC
written from include/gmx.h (the comment on gmx_bc_batch), not from the oracle's C.

Every Sum of comp_BC is a float32 chain in row-slot order.  On RMAT graphs up to scale 18 every path count stays an
integer below 2^24, so every partial sum of the forward visit is exact and any order gives the same bits.  The layered
graphs here multiply the path count by a layer's fan-in at every level: a few thousand vertices reach 10^12 and more,
and the forward sums round differently in another order.

  layered(widths, p, back, seed, dup)
      a root (widths[0] == 1) and layer k of widths[k] vertices; an edge from a vertex of layer k to one of layer k + 1 with
      probability p (1 from a layer of one vertex), every vertex with at least one in-edge; a share `dup` of these edges
      repeated; `back` edges from a vertex to one in the same or a shallower layer (self-loops among them) -- they change
      no level from the root and are the slots that do not pass, in both visits; vertices the root does not reach with
      edges into the layers (reverse slots whose source has no level) and among themselves; probes; the ids permuted, and
      every row in a random slot order, so slot order is neither id order nor layer order.  Uploaded verbatim.
  probes
      extra vertices of a deep layer whose reverse row (forward visit) or forward row (reverse visit) is laid out slot by
      slot: a prescribed length on either side of BFS_VISIT_SMALL, 64 and one step of 64 * BFS_BIG_CHUNKS slots, and
      prescribed passing slots (exactly 1 / BFS_DENSE_PASS / BFS_DENSE_PASS + 1 / 64 of a chunk, an empty chunk between
      two others, the last slot of a partial chunk -- the one the lanes past the row's end are clamped to -- and a row
      whose only passing slot lies in its second step).  They follow the constants parsed from gmx_bfs.hip.

census(og, seed) counts, for both visits of one seed, the rows and 64-slot chunks in every such class."""
import functools
import os
import re

import numpy as np

import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_HIP = os.path.join(ROOT, "green-marl_amd", "csrc", "gmx_bfs.hip")
INT_MAX = 2147483647
NOLEVEL = -9                      # the models' level of a vertex the seed does not reach (never one off a real level)
U32 = 2.0 ** -24                  # unit roundoff of float32
U64 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """(BFS_VISIT_SMALL, BFS_DENSE_PASS, BFS_BIG_CHUNKS) as gmx_bfs.hip defines them."""
    text = open(BFS_HIP).read()
    out = []
    for name in ("BFS_VISIT_SMALL", "BFS_DENSE_PASS", "BFS_BIG_CHUNKS"):
        m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, text, re.M)
        assert m, "%s is not defined in %s" % (name, BFS_HIP)
        out.append(int(m.group(1)))
    return tuple(out)


def census_classes():
    S, D, C = kernel_constants()
    step = 64 * C
    lens = [S - 1, S, S + 1, 63, 64, 65, step - 1, step, step + 1]
    return (["len%d" % n for n in lens] + ["three_steps"] + ["chunk_pass%d" % n for n in (1, D, D + 1, 64)] +
            ["empty_chunk_between", "partial_last_passes", "partial_last_fails", "passes_only_past_step1", "level_two_wave_rows"])


# ---- the generator

def probe_patterns(rng):
    """Rows as bool arrays, True = the slot passes; every one has a passing slot."""
    S, D, C = kernel_constants()
    step = 64 * C
    assert 2 < S < 63 and 1 < D < 62 and C >= 3

    def row(n, chunks=None, on=(), off=(), fill=0.3):
        """n slots; chunks: {chunk: passing lanes of it}, the other chunks at random with density `fill`"""
        p = rng.random(n) < fill
        for c, k in (chunks or {}).items():
            lo, hi = 64 * c, min(64 * c + 64, n)
            p[lo:hi] = False
            p[lo + rng.choice(hi - lo, k, replace=False)] = True
        p[list(on)] = True
        p[list(off)] = False
        assert p.any()
        return p

    only_late = np.zeros(step + 1, bool)
    only_late[step] = True                                   # the one passing slot is the one the second step's idle lanes clamp to
    long_row = row(2 * step + 70, {c: 0 for c in range(C)}, on=[2 * step + 69], fill=0.05)
    long_row[step:step + 5 * 64] = np.concatenate([row(64, {0: 1}), row(64, {0: D}), row(64, {0: D + 1}), np.ones(64, bool), np.zeros(64, bool)])
    return [row(S - 1, on=[0]), row(S, on=[S - 1]), row(S + 1, on=[S]),
            row(63, on=[0], off=[62]), np.ones(64, bool), row(65, {0: D}, on=[64]),
            row(step - 1, {0: D + 1, 1: 0, 2: D}, on=[step - 2], fill=0.1),
            row(step, {0: 64, 1: 0, 2: 1}, on=[step - 1], fill=0.2),
            only_late, row(step + 1, on=[step], fill=0.4), row(step + 1, off=[step], on=[1], fill=0.02),
            long_row]


class Shape:
    """og: the oracle's graph (both CSRs, as uploaded); layer[v]: v's layer = its level from `root`, -2 where the root does
    not reach; probes: {"fw": ids, "rv": ids}; first_of[branch, layer]: the smallest id of that layer; extra: the vertices
    the root does not reach."""

    def __init__(self, og, layer, root, probes, first_of, extra):
        self.og, self.layer, self.root, self.probes, self.first_of, self.extra = og, layer, root, probes, first_of, extra
        self.V = og.N


def _csr(V, row, col, key):
    order = np.lexsort((key, row))
    begin = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=V))]).astype(np.int32)
    return begin, np.ascontiguousarray(col[order], np.int32)


def assemble(branches, back, seed, dup, unreached=300, probes=True):
    """branches: [(widths, p)], each hanging under the one root (vertex 0 before the ids are permuted)."""
    rng = np.random.default_rng(seed)
    layer, branch = [0], [-1]
    src, dst = [], []
    nv = 1
    for b, (widths, p) in enumerate(branches):
        prev = np.zeros(1, np.int64)                         # the root
        for k, w in enumerate(widths, start=1):
            cur = nv + np.arange(w)
            nv += w
            layer += [k] * w
            branch += [b] * w
            m = rng.random((len(prev), w)) < (1.0 if len(prev) == 1 else p)
            lone = np.flatnonzero(~m.any(axis=0))
            m[rng.integers(0, len(prev), len(lone)), lone] = True
            i, j = np.nonzero(m)
            src.append(prev[i])
            dst.append(cur[j])
            prev = cur
    src, dst = np.concatenate(src), np.concatenate(dst)
    again = rng.choice(len(src), int(dup * len(src)), replace=False)
    src, dst = np.concatenate([src, src[again]]), np.concatenate([dst, dst[again]])
    layer, branch = np.array(layer), np.array(branch)
    nord = nv                                                # the ordinary vertices: random edges end only at these
    by_layer = np.argsort(layer, kind="stable")
    upto = np.cumsum(np.bincount(layer))                     # upto[k]: vertices of layer <= k
    bs = rng.integers(0, nord, back)
    bd = by_layer[(rng.random(back) * upto[layer[bs]]).astype(np.int64)]
    assert (layer[bd] <= layer[bs]).all()
    src, dst = np.concatenate([src, bs]), np.concatenate([dst, bd])
    extra = nv + np.arange(unreached)
    nv += unreached
    layer = np.concatenate([layer, np.full(unreached, -2)])
    if unreached:
        es = np.repeat(extra, 24)
        ed = rng.integers(0, nord, len(es))
        ed[::8] = extra[rng.integers(0, unreached, len(ed[::8]))]   # an eighth of them among themselves
        src, dst = np.concatenate([src, es]), np.concatenate([dst, ed])
    fkey, rkey = rng.random(len(src)), rng.random(len(src))
    made = {"fw": [], "rv": []}
    if probes:
        assert len(branches) == 1 and unreached
        k = max(2, len(branches[0][0]) - 2)                 # a layer deep enough that the terms of its rows are inexact
        of_layer = lambda lo, hi: np.flatnonzero((layer[:nord] >= lo) & (layer[:nord] <= hi))
        for direction in ("fw", "rv"):
            for pat in probe_patterns(rng):
                q, n = nv, len(pat)
                nv += 1
                layer = np.append(layer, k)
                if direction == "fw":                        # q's reverse row: sources one layer up pass, deeper or unreached ones do not
                    deeper, src_deeper, src_nolevel = rng.random(n) < 0.8, rng.choice(of_layer(k, 99), n), rng.choice(extra, n)
                    ends = np.where(pat, rng.choice(of_layer(k - 1, k - 1), n), np.where(deeper, src_deeper, src_nolevel))
                    s, d, fk, rk = ends, np.full(n, q), rng.random(n), np.arange(n, dtype=np.float64)
                else:                                        # q's forward row: targets one layer down pass, same or shallower ones do not
                    ends = np.where(pat, rng.choice(of_layer(k + 1, k + 1), n), rng.choice(of_layer(0, k), n))
                    s, d, fk, rk = np.full(n, q), ends, np.arange(n, dtype=np.float64), rng.random(n)
                    s, d = np.append(s, rng.choice(of_layer(k - 1, k - 1))), np.append(d, q)   # and one edge that reaches q
                    fk, rk = np.append(fk, rng.random()), np.append(rk, rng.random())
                src, dst, fkey, rkey = np.concatenate([src, s]), np.concatenate([dst, d]), np.concatenate([fkey, fk]), np.concatenate([rkey, rk])
                made[direction].append(q)
    perm = rng.permutation(nv)
    src, dst = perm[src], perm[dst]
    begin, idx = _csr(nv, src, dst, fkey)
    r_begin, r_idx = _csr(nv, dst, src, rkey)
    lay = np.empty(nv, np.int64)
    lay[perm] = layer
    for a in (begin, idx, r_begin, r_idx, lay):
        a.setflags(write=False)
    og = po.Graph(nv, begin, idx, r_begin, r_idx)
    first_of = {(int(b), int(k)): int(perm[np.flatnonzero((branch == b) & (layer[:nord] == k))].min()) for b, k in set(zip(branch[1:].tolist(), layer[1:nord].tolist()))}
    return Shape(og, lay, int(perm[0]), {d: perm[np.array(v, np.int64)] for d, v in made.items()}, first_of, np.sort(perm[extra]))


def layered(widths, p, back, seed, dup, unreached=300, probes=True):
    assert widths[0] == 1
    return assemble([(list(widths[1:]), p)], back, seed, dup, unreached, probes)


FAMILIES = ("inexact", "sparse", "overflow", "small")


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "inexact":    # path counts beyond 10^12; lane rows (the 500-wide layer), one-step wave rows and rows past 512 slots (fan-in 1600 * p)
        return layered([1, 40, 700, 700, 1600, 700, 40, 500, 200], 0.35, 200_000, 2024, 0.1)
    if name == "sparse":     # few passing slots among many: chunks with at most BFS_DENSE_PASS passing lanes
        return layered([1, 64, 1200, 1200, 1200, 64], 0.02, 1_500_000, 2025, 0.1)
    if name == "overflow":   # 48^k paths: inf from level 24 on, NaN above it; the second branch stays finite
        return assemble([([48] * 30, 1.0), ([1, 40, 300, 300, 40], 0.3)], 20_000, 2026, 0.0, unreached=100, probes=False)
    assert name == "small"   # `inexact` at a size where every vertex can be a source
    return layered([1, 20, 150, 150, 300, 150, 20, 100, 50], 0.35, 20_000, 2027, 0.1, unreached=60)


@functools.lru_cache(maxsize=None)
def seeds(name):
    """The root, vertices of the first, a middle and a deep layer, the root again (duplicate seeds are independent), one the
    root does not reach, a probe of either kind where the family has them."""
    sh = family(name)
    mid, extra = sh.first_of, sh.extra
    depth = max(k for b, k in mid if b == 0)
    s = [sh.root, mid[0, 1], mid[0, depth // 2], sh.root, int(extra[0]), mid[0, depth - 1]]
    if name == "overflow":
        s.append(mid[1, 2])
    else:
        s += [int(sh.probes["rv"][-1]), int(sh.probes["fw"][0])]
    out = np.array(s, np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def seeds70(name):
    """seeds(name) and random vertices up to 70: widths 16 / 32 / 64 all end on a partial batch."""
    sh = family(name)
    out = np.concatenate([seeds(name), np.random.default_rng(70).integers(0, sh.V, 70 - len(seeds(name)))]).astype(np.int32)
    out.setflags(write=False)
    return out


# ---- the census

def _census_visit(begin, idx, dist, seed, d):
    S, D, C = kernel_constants()
    step = 64 * C
    N = len(begin) - 1
    begin = begin.astype(np.int64)
    deg = np.diff(begin)
    reached = dist != INT_MAX
    row_of = np.repeat(np.arange(N), deg)
    passing = reached[row_of] & (dist[idx] == dist[row_of] + d)
    visited = reached.copy()
    visited[seed] = False                                    # with skip_root the seed's row is not walked: not counted
    L = deg[visited]
    out = dict.fromkeys(census_classes(), 0)
    for n in (S - 1, S, S + 1, 63, 64, 65, step - 1, step, step + 1):
        out["len%d" % n] = int((L == n).sum())
    out["three_steps"] = int((L > 2 * step).sum())
    wave = np.flatnonzero(visited & (deg >= S))
    out["level_two_wave_rows"] = int((np.bincount(dist[wave]) >= 2).sum()) if len(wave) else 0
    for v in wave:
        p = passing[begin[v]:begin[v + 1]]
        n = len(p)
        cnt = np.concatenate([p, np.zeros(-n % 64, bool)]).reshape(-1, 64).sum(axis=1)
        for k in (1, D, D + 1, 64):
            out["chunk_pass%d" % k] += int((cnt == k).sum())
        nz = np.flatnonzero(cnt)
        out["empty_chunk_between"] += int(len(nz) > 0 and nz[-1] - nz[0] + 1 > len(nz))
        if n % 64:
            out["partial_last_passes" if p[-1] else "partial_last_fails"] += 1
        out["passes_only_past_step1"] += int(n > step and p.any() and not p[:step].any())
    return out


def census(og, seed):
    """{"fw": {class: count}, "rv": {class: count}} for the two visits of comp_BC from `seed`: fw walks the reverse rows (slot
    w passes when level[w] == level[v] - 1), rv the forward rows (level[w] == level[v] + 1).  len*: rows of that length;
    three_steps: rows of more than two steps of 64 * BFS_BIG_CHUNKS slots; chunk_pass*: 64-slot chunks of wave rows (length
    >= BFS_VISIT_SMALL) with that many passing lanes; the rest as named, counted in wave rows / levels."""
    dist = po.bfs_queue(og, int(seed)).astype(np.int64)
    return {"fw": _census_visit(og.r_begin, og.r_node_idx, dist, int(seed), -1),
            "rv": _census_visit(og.begin, og.node_idx, dist, int(seed), +1)}


# ---- the models

def levels(og, s):
    """level[v] from s over the forward rows, NOLEVEL where s does not reach; the number of levels."""
    begin = og.begin.astype(np.int64)
    level = np.full(og.N, NOLEVEL, np.int64)
    level[s] = 0
    front, l = np.array([s], np.int64), 0
    while len(front):
        cnt = begin[front + 1] - begin[front]
        slots = np.repeat(begin[front] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
        nbr = og.node_idx[slots]
        front = np.unique(nbr[level[nbr] == NOLEVEL]).astype(np.int64)
        l += 1
        level[front] = l
    return level, l


def ordered_row_sums(nrows, row, term, reverse=False):
    """float32[nrows]: for every row the chain S = +0.0f; S = S + term, over its terms as they stand in `term` (with
    `reverse`: last term first).  row[i]: the row of term[i], non-decreasing.  The rows are laid side by side, padded with
    +0.0f behind their last term (x + (+0.0f) is x for every x a chain of non-negative terms can hold), and every row is
    accumulated left to right in float32: np.cumsum is the sequential loop, not a pairwise reduction."""
    out = np.zeros(nrows, np.float32)
    if len(row) == 0:
        return out
    cnt = np.bincount(row, minlength=nrows)
    rank = np.arange(len(row)) - (np.cumsum(cnt) - cnt)[row]
    if reverse:
        rank = cnt[row] - 1 - rank
    m = np.zeros((nrows, int(cnt.max())), np.float32)
    m[row, rank] = term
    return np.cumsum(m, axis=1, dtype=np.float32)[:, -1]


def _slot_rows(begin):
    return np.repeat(np.arange(len(begin) - 1), np.diff(begin))


def seed_pass_f32(og, s, skip_root, reverse_slots=False):
    """(level, sigma, delta) of one seed as gmx.h states them: sigma[v] the float32 sum over v's reverse-row slots whose
    source is one level up, in slot order from +0.0f (the seed starts at 1 and, unless skipped, is overwritten by its own
    empty sum); delta[v] the float32 sum over v's forward-row slots whose target is one level down of
    sigma[v] / sigma[w] * (1 + delta[w]); deepest level first."""
    level, nlev = levels(og, s)
    reached = level != NOLEVEL
    sigma, delta = np.zeros(og.N, np.float32), np.zeros(og.N, np.float32)
    sigma[s] = 1
    with np.errstate(all="ignore"):
        for begin, idx, d, order in ((og.r_begin, og.r_node_idx, -1, range(nlev)), (og.begin, og.node_idx, +1, range(nlev - 1, -1, -1))):
            row = _slot_rows(begin)
            keep = reached[row] & (level[idx] == level[row] + d)
            if skip_root:
                keep &= row != s
            row, nbr = row[keep], idx[keep]
            for l in order:
                vs = np.flatnonzero(level == l)
                if skip_root:
                    vs = vs[vs != s]
                sel = level[row] == l
                v, w = row[sel], nbr[sel]
                if d < 0:
                    sigma[vs] = ordered_row_sums(len(vs), np.searchsorted(vs, v), sigma[w], reverse_slots)
                else:
                    term = sigma[v] / sigma[w] * (np.float32(1) + delta[w])
                    assert term.dtype == np.float32
                    delta[vs] = ordered_row_sums(len(vs), np.searchsorted(vs, v), term, reverse_slots)
    return level, sigma, delta


def bc_model_f32(og, seeds, skip_root, reverse_slots=False):
    """comp_BC as gmx.h states it: BC[v] = BC[v] + delta_s[v] once per seed, in seed order, for the seeds that reach v and,
    with skip_root, not for v == s.  reverse_slots: every sum in descending slot order -- the mutant the inputs must tell apart."""
    bc = np.zeros(og.N, np.float32)
    for s in seeds:
        level, _, delta = seed_pass_f32(og, int(s), skip_root, reverse_slots)
        upd = level != NOLEVEL
        if skip_root:
            upd[s] = False
        with np.errstate(all="ignore"):
            bc[upd] = bc[upd] + delta[upd]
    return bc


def brandes_f64(og, seeds):
    """Brandes' accumulation in float64 over the edge list, an edge repeated counting as often: (BC without the seeds' own
    terms, the largest path count met)."""
    src, dst = _slot_rows(og.begin), og.node_idx
    bc, top = np.zeros(og.N), 0.0
    for s in seeds:
        level, nlev = levels(og, int(s))
        tree = (level[src] != NOLEVEL) & (level[dst] == level[src] + 1)
        ts, td, tl = src[tree], dst[tree], level[src[tree]]
        sigma, delta = np.zeros(og.N), np.zeros(og.N)
        sigma[s] = 1.0
        for l in range(nlev):
            m = tl == l
            sigma += np.bincount(td[m], weights=sigma[ts[m]], minlength=og.N)
        for l in range(nlev - 1, -1, -1):
            m = tl == l
            delta += np.bincount(ts[m], weights=sigma[ts[m]] / sigma[td[m]] * (1.0 + delta[td[m]]), minlength=og.N)
        delta[s] = 0.0
        bc += delta
        top = max(top, float(sigma.max()))
    return bc, top


def f32_error_bound(og, seeds):
    """A bound on |BC_f32 - BC| / BC for comp_BC with skip_root over `seeds`, from the graph alone.

    Every term is non-negative, so nothing cancels and every rounding is a factor (1 + e), |e| <= u = 2^-24, on the exact
    value; k such factors, in numerator or denominator, are 1 + t with |t| <= gamma_k = k u / (1 - k u) (Higham, Accuracy
    and Stability of Numerical Algorithms, Lemma 3.1).  Count the factors, with R / F the longest reverse / forward row and
    L the deepest level of any seed:
      sigma at level l: a chain of at most R terms is R - 1 adds on top of the terms' own factors: s_l = l (R - 1);
      a term of delta at level l: sigma[v] / sigma[w] carries s_l + s_(l+1), 1 + delta[w] at most delta[w]'s factors d_(l+1)
        (1 is exact and both are non-negative), and the division, the add and the multiply one each: 3;
      delta at level l: d_l = s_l + s_(l+1) + d_(l+1) + 3 + (F - 1), d_L = 0 (an empty sum);
      so d_0 = sum over l < L of ((2 l + 1)(R - 1) + F + 2) = L^2 (R - 1) + L (F + 2), and no level has more;
      BC: one add per seed.
    The float64 reference has the same count with u = 2^-53."""
    R, F = int(np.diff(og.r_begin).max()), int(np.diff(og.begin).max())
    L = max(levels(og, int(s))[1] for s in seeds) - 1
    k = L * L * (R - 1) + L * (F + 2) + len(seeds)
    assert k * U32 < 0.5
    return k * U32 / (1 - k * U32) + k * U64 / (1 - k * U64), k
