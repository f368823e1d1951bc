"""gmx_louvain's definition (include/gmx.h) in plain Python: the one-thread run of the schedule that the device must equal
byte for byte.  Every sum and product that decides something is a Python int; numpy only builds the merged adjacency of a
level and adds up intra, in int64 sums that the definition bounds below 2^63 (m2 < 2^63).

louvain_model(V, begin, idx, weight, max_levels, max_rounds) -> dict with comm (int32, numbered by ascending smallest
member), num_comms, num_levels, intra, qnum, m2, modularity and the counters of the GMX_LOUVAIN_LOG line and the stats:
levels, rounds (run), rollbacks, cuts, moves, iterations (rounds that kept a move), edges_examined, sizes [(n, nnz) of every
level run], trace [Qnum after every kept half-round, the first entry the singletons'].

float_scores=True is NOT the definition: the same schedule with every score formed in float64, for the search of an input on
which that differs (tests/test_gpu_louvain.py)."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def half_of(i, r):
    return fmix32(i ^ ((r * 0x9E3779B9) & M32)) & 1


def _merge(rows, cols, w):
    """The entries (rows, cols, w) merged by (row, col), ascending: rows, cols, w as int64 arrays."""
    key = (rows.astype(np.int64) << 32) | cols.astype(np.int64)
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    first = np.ones(len(key), bool)
    first[1:] = key[1:] != key[:-1]
    at = np.flatnonzero(first)
    return key[at] >> 32, key[at] & M32, np.add.reduceat(w, at) if len(at) else w[:0]


def level0(V, begin, idx, weight):
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    E = int(begin[V]) if V else 0
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(begin[:V + 1]))
    x = np.ones(E, np.int64) if weight is None else np.asarray(weight).astype(np.int64)
    return _merge(np.concatenate([src, idx[:E]]), np.concatenate([idx[:E], src]), np.concatenate([x, x]))


def qnum_of(rows, cols, w, comm, m2):
    """(Qnum, intra) of a labelling of a level, from scratch."""
    c = np.asarray(comm, np.int64)
    intra = int(w[c[rows] == c[cols]].sum()) if len(w) else 0
    k = np.zeros(len(c), np.int64)
    np.add.at(k, rows, w)
    tot = {}
    for lab, kv in zip(c.tolist(), k.tolist()):
        tot[lab] = tot.get(lab, 0) + kv
    return m2 * intra - sum(t * t for t in tot.values()), intra


def modularity_of(qnum, m2):
    return float(qnum) / (float(m2) * float(m2)) if m2 else 0.0


def canonical(labels):
    """Labels renumbered by ascending smallest member, as wcc() numbers components."""
    new, out = {}, []
    for lab in labels:
        if lab not in new:
            new[lab] = len(new)
        out.append(new[lab])
    return np.asarray(out, np.int32), len(new)


def louvain_model(V, begin, idx, weight=None, max_levels=32, max_rounds=64, float_scores=False):
    assert max_levels >= 0 and max_rounds >= 1
    if weight is not None:
        assert len(weight) == 0 or int(np.min(weight)) >= 1
    rows, cols, w = level0(V, begin, idx, weight)
    m2 = int(w.sum()) if len(w) else 0
    of = list(range(V))   # the level vertex of every original vertex
    n = V
    out = dict(levels=0, rounds=0, rollbacks=0, cuts=0, moves=0, iterations=0, edges_examined=0, sizes=[], m2=m2)
    q, intra = qnum_of(rows, cols, w, range(n), m2)
    trace = [q]
    if m2 == 0:
        max_levels = 0
    for _ in range(max_levels):
        nnz = len(w)
        out["sizes"].append((n, nnz))
        beg = np.searchsorted(rows, np.arange(n + 1)).tolist()
        cl, wl = cols.tolist(), w.tolist()
        adj = [(cl[beg[i]:beg[i + 1]], wl[beg[i]:beg[i + 1]]) for i in range(n)]
        k = [sum(a[1]) for a in adj]
        comm, tot = list(range(n)), list(k)
        level_moves, ended = 0, False
        for r in range(max_rounds):
            kept = 0
            for half in (0, 1):
                pending = []
                for i in range(n):
                    nb, ws = adj[i]
                    if not nb or half_of(i, r) != half:
                        continue
                    c, ki = comm[i], k[i]
                    e = {c: 0}
                    for u, x in zip(nb, ws):
                        if u != i:
                            d = comm[u]
                            e[d] = e.get(d, 0) + x
                    if float_scores:
                        best, best_s = c, float(m2) * float(e[c]) - float(ki) * float(tot[c] - ki)
                    else:
                        best, best_s = c, m2 * e[c] - ki * (tot[c] - ki)
                    for d, ed in e.items():
                        if d == c:
                            continue
                        s = float(m2) * float(ed) - float(ki) * float(tot[d]) if float_scores else m2 * ed - ki * tot[d]
                        if s > best_s or (s == best_s and best != c and d < best):
                            best, best_s = d, s
                    if best != c:
                        pending.append((i, c, best))
                if not pending:
                    continue
                for i, c, d in pending:
                    comm[i] = d
                    tot[c] -= k[i]
                    tot[d] += k[i]
                ca = np.asarray(comm, np.int64)
                new_intra = int(w[ca[rows] == ca[cols]].sum())
                new_q = m2 * new_intra - sum(t * t for t in tot)
                if new_q > q:
                    q, intra = new_q, new_intra
                    kept += len(pending)
                    trace.append(q)
                else:
                    out["rollbacks"] += 1
                    for i, c, d in pending:
                        comm[i] = c
                        tot[c] += k[i]
                        tot[d] -= k[i]
            out["rounds"] += 1
            out["edges_examined"] += nnz
            if kept == 0:
                ended = True
                break
            out["iterations"] += 1
            level_moves += kept
        if not ended:
            out["cuts"] += 1
        if level_moves == 0:
            break
        out["moves"] += level_moves
        out["levels"] += 1
        labels = sorted(set(comm))
        newid = {lab: j for j, lab in enumerate(labels)}
        lmap = np.asarray([newid[c] for c in comm], np.int64)
        of = [int(lmap[x]) for x in of]
        rows, cols, w = _merge(lmap[rows], lmap[cols], w)
        n = len(labels)
    comm_out, nc = canonical(of)
    out.update(comm=comm_out, num_comms=nc, num_levels=out["levels"], intra=intra, qnum=q, modularity=modularity_of(q, m2), trace=trace)
    return out


def csr_of(V, edges):
    """begin, idx (int32) of a list of (u, w) slots, in the order given within each row."""
    rows = [[] for _ in range(V)]
    for u, x in edges:
        rows[u].append(x)
    begin = np.zeros(V + 1, np.int32)
    begin[1:] = np.cumsum([len(r) for r in rows])
    return begin, np.asarray([x for r in rows for x in r], np.int32)
