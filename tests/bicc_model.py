"""Host models for gmx_biconnected (no GPU).  The stored slots are read as an undirected simple graph: slot u -> w with
u != w is the edge {u, w}, repeats and the other orientation are the same edge, self loops are ignored.

  definition_oracle   from the definitions alone (remove a vertex or an edge, count components with scipy): V <= 64
  hopcroft_tarjan     the linear lowpoint algorithm, for larger inputs
  forest_model        the schedule: the smallest vertex of every component as root, BFS levels, the smallest vertex of the
                      previous level as parent, and the cursor moves of the walks without jumps (GMX_BICC_SKIP=0)

Both oracles return the arrays as gmx_biconnected numbers them (`canonical`): bridge and block by slot of the CSR given,
block ids increasing with each block's smallest slot, tecc numbered by smallest vertex."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


def csr_from_edges(V, src, dst):
    """Forward CSR of an edge list with every row in the order given (stable)."""
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    order = np.argsort(src, kind="stable")
    begin = np.zeros(V + 1, np.int64)
    np.add.at(begin, src + 1, 1)
    return np.cumsum(begin).astype(np.int32), dst[order].astype(np.int32)


def slot_ends(V, begin, idx):
    begin, idx = np.asarray(begin, np.int64), np.asarray(idx, np.int64)
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(begin)), idx


def simple_edges(V, begin, idx):
    """The distinct undirected edges as (a < b) pairs, sorted."""
    u, w = slot_ends(V, begin, idx)
    keep = u != w
    a, b = np.minimum(u[keep], w[keep]), np.maximum(u[keep], w[keep])
    key = np.unique(a * V + b)
    return key // max(V, 1), key % max(V, 1)


def _components(V, a, b):
    """(count, label by vertex) with the labels dense in order of each component's smallest vertex."""
    if V == 0:
        return 0, np.zeros(0, np.int32)
    m = sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(V, V)).tocsr()
    n, lab = connected_components(m, directed=False)
    _, first = np.unique(lab, return_index=True)
    rank = np.empty(n, np.int64)
    rank[np.argsort(first)] = np.arange(n)
    return int(n), rank[lab].astype(np.int32)


def canonical(V, begin, idx, bridge_edges, artic, label_of_slot):
    """The result arrays from: the set of bridges as (a < b) pairs, the articulation points, and any labelling of the
    non-loop slots by block (label_of_slot[s], ignored at self-loop slots)."""
    u, w = slot_ends(V, begin, idx)
    E = len(u)
    loop = u == w
    bkey = set(int(a) * V + int(b) for a, b in bridge_edges)
    key = np.minimum(u, w) * V + np.maximum(u, w)
    bridge = np.zeros(E, np.uint8)
    if bkey:
        bridge[~loop & np.isin(key, np.fromiter(bkey, np.int64, len(bkey)))] = 1
    block = np.full(E, -1, np.int32)
    s = np.flatnonzero(~loop)
    if len(s):
        _, first, inv = np.unique(np.asarray(label_of_slot)[s], return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))
        block[s] = rank[inv.reshape(-1)]
    art = np.zeros(V, np.uint8)
    art[list(artic)] = 1
    a, b = simple_edges(V, begin, idx)
    keep = ~np.isin(a * V + b, np.fromiter(bkey, np.int64, len(bkey))) if bkey else np.ones(len(a), bool)
    ntecc, tecc = _components(V, a[keep], b[keep])
    ncomp, _ = _components(V, a, b)
    nblocks = int(block.max()) + 1 if len(s) else 0
    edges_per_block = np.zeros(nblocks, np.int64)
    if len(s):
        _, one = np.unique(key[s], return_index=True)   # one slot per undirected edge
        np.add.at(edges_per_block, block[s][one], 1)
    return {"bridge": bridge, "artic": art, "block": block, "tecc": tecc, "num_blocks": nblocks, "num_bridges": len(bkey),
            "num_artic": int(art.sum()), "num_tecc": ntecc, "num_comps": ncomp,
            "largest_block_edges": int(edges_per_block.max()) if nblocks else 0}


def definition_oracle(V, begin, idx):
    """Bridges: edges whose removal raises the number of components.  Articulation points: vertices whose removal does.
    Blocks: two edges are in one block when no single vertex separates them -- for every vertex x, what is left of both
    lies in one component of G - x (Menger, on the edges' midpoints)."""
    assert V <= 64
    a, b = simple_edges(V, begin, idx)
    n0, _ = _components(V, a, b)
    bridges = []
    for i in range(len(a)):
        keep = np.arange(len(a)) != i
        if _components(V, a[keep], b[keep])[0] > n0:
            bridges.append((int(a[i]), int(b[i])))
    artic = []
    sig = np.zeros((len(a), V), np.int64)   # per edge and removed vertex: the component of what is left of the edge
    for x in range(V):
        keep = (a != x) & (b != x)
        n, lab = _components(V, a[keep], b[keep])
        if n - 1 > n0:   # (x itself is left behind as a component of its own)
            artic.append(x)
        sig[:, x] = np.where(a != x, lab[a], lab[b])
    u, w = slot_ends(V, begin, idx)
    label = np.zeros(len(u), np.int64)
    if len(a):
        _, edge_label = np.unique(sig, axis=0, return_inverse=True)
        pos = np.searchsorted(a * V + b, np.minimum(u, w) * V + np.maximum(u, w))
        pos = np.minimum(pos, len(a) - 1)
        label = edge_label.reshape(-1)[pos]
    return canonical(V, begin, idx, bridges, artic, label)


def _sym_csr(V, begin, idx):
    a, b = simple_edges(V, begin, idx)
    s, d = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((d, s))
    nb = np.zeros(V + 1, np.int64)
    np.add.at(nb, s + 1, 1)
    return np.cumsum(nb), d[order]


def hopcroft_tarjan(V, begin, idx):
    """disc / low by an iterative DFS (roots in id order, neighbours ascending).  The tree edge into c opens a block when
    low[c] >= disc[parent]; a back edge belongs to the block of its descendant end's tree edge."""
    nb, nd = _sym_csr(V, begin, idx)
    nbl, ndl = nb.tolist(), nd.tolist()
    disc, low, parent, label = [-1] * V, [0] * V, [-1] * V, [-1] * V
    children_of_root = [0] * V
    bridges, artic = [], set()
    t = 0
    for r in range(V):
        if disc[r] >= 0:
            continue
        disc[r] = low[r] = t
        t += 1
        stack, ptr = [r], {r: nbl[r]}
        while stack:
            v = stack[-1]
            i = ptr[v]
            if i < nbl[v + 1]:
                ptr[v] = i + 1
                w = ndl[i]
                if disc[w] < 0:
                    parent[w] = v
                    disc[w] = low[w] = t
                    t += 1
                    stack.append(w)
                    ptr[w] = nbl[w]
                elif w != parent[v] and disc[w] < low[v]:
                    low[v] = disc[w]
            else:
                stack.pop()
                p = parent[v]
                if p >= 0:
                    if low[v] < low[p]:
                        low[p] = low[v]
                    if low[v] > disc[p]:
                        bridges.append((min(p, v), max(p, v)))
                    if p == r:
                        children_of_root[r] += 1
                    elif low[v] >= disc[p]:
                        artic.add(p)
        if children_of_root[r] > 1:
            artic.add(r)
    disc_a, low_a, par_a = np.array(disc, np.int64), np.array(low, np.int64), np.array(parent, np.int64)
    # label[c] in discovery order: c itself where the edge into c opens a block, else its parent's label
    lab = np.arange(V, dtype=np.int64)
    for c in np.argsort(disc_a).tolist():
        p = parent[c]
        if p >= 0 and parent[p] >= 0 and low[c] < disc[p]:
            lab[c] = lab[p]
    u, w = slot_ends(V, begin, idx)
    deeper = np.where(disc_a[u] > disc_a[w], u, w) if len(u) else u
    child = np.where(par_a[w] == u, w, np.where(par_a[u] == w, u, deeper)) if len(u) else u
    return canonical(V, begin, idx, bridges, artic, lab[child] if len(u) else [])


def forest_model(V, begin, idx):
    """The forest gmx_biconnected builds and the work of its walks without jumps: {"level", "par", "levels", "roots", "tree",
    "walks", "steps"} -- steps: over every slot u -> w that is no self loop and no tree slot, the two path lengths from u and
    from w to their lowest common ancestor."""
    nb, nd = _sym_csr(V, begin, idx)
    a, b = simple_edges(V, begin, idx)
    ncomp, comp = _components(V, a, b)
    level = np.full(V, -1, np.int64)
    par = np.arange(V, dtype=np.int64)
    if V:
        _, roots = np.unique(comp, return_index=True)
        level[roots] = 0
        front, L = roots, 0
        while len(front):
            deg = nb[front + 1] - nb[front]
            src = np.repeat(front, deg)
            pos = np.repeat(nb[front] - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(int(deg.sum()))
            dst = nd[pos]
            new = level[dst] < 0
            level[dst[new]] = L + 1
            hit = level[dst] == L + 1
            par[dst[hit]] = V
            np.minimum.at(par, dst[hit], src[hit])
            front, L = np.unique(dst[new]), L + 1
    u, w = slot_ends(V, begin, idx)
    walk = (u != w) & (par[u] != w) & (par[w] != u) if len(u) else np.zeros(0, bool)
    x, y = u[walk].copy(), w[walk].copy()
    steps = 0
    while True:
        live = x != y
        if not live.any():
            break
        x, y = x[live], y[live]
        steps += len(x)
        dx = level[x] >= level[y]
        x, y = np.where(dx, par[x], x), np.where(dx, y, par[y])
    return {"level": level, "par": par, "levels": int(level.max()) + 1 if V else 0, "roots": ncomp, "tree": V - ncomp,
            "walks": int(walk.sum()), "steps": int(steps)}
