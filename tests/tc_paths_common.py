"""Inputs that send tc_oriented_kernel (green-marl_amd/csrc/gmx_tc.hip) down every one of its code paths, and a numpy
restatement of the kernel's path SELECTION that says how many slots of an input take each path under a set of knobs.

The census decides whether an input is fit for purpose; it never supplies an expected value.  Expected triangle counts
come from the oracle (pyoracle.triangle_counting_merge, pyoracle.triangle_counting) and from closed forms.

Every builder returns (begin, node_idx) of a symmetric simple CSR with sorted rows: the reverse CSR is the same arrays."""
import numpy as np

import pyoracle as po

# The kernel's defaults -- gmx_tc.hip: TCO_ALONE, TCO_RATIO, TCO_HUB_TAIL, TCO_CAP, the 64-slot work items of
# tc_groups_kernel, and the hub count chosen in tc_counting_graph (TCO_HUB_MAX, half of it up to 2^24 vertices).  If the
# kernel is retuned and a census assertion of test_tc_paths_host.py fails, re-point the inputs: that is the signal.
ALONE = 4
RATIO = 4
HUB_TAIL = 4
CAP = 1024
GROUP = 64
HUB_MAX = 131072

BRANCHES = ("A-hubtail", "A-walkUpU", "A-tailSearch", "W-hub", "W-streamUpU", "W-streamTail")
# (branch, where the group's list is): W-streamUpU searches the staged list, so it has no in-memory form
PAIRS = tuple((b, w) for b in BRANCHES for w in ("lds", "mem") if (b, w) != ("W-streamUpU", "mem"))


# ---------------------------------------------------------------- graphs
def csr_from_pairs(V, a, b):
    """Symmetric simple CSR of the undirected pairs {a[k], b[k]}: self-pairs dropped, both directions, de-duplicated."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    key = np.unique(np.concatenate([a * V + b, b * V + a]))
    src, dst = key // V, key % V
    begin = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=begin[1:])
    return begin.astype(np.int32), dst.astype(np.int32)


def clique(n):
    iu, ju = np.triu_indices(n, 1)
    return csr_from_pairs(n, iu, ju)


def clique_triangles(n):
    return n * (n - 1) * (n - 2) // 6


def crown(a):
    """Complete bipartite X = [0, a), Y = [a, 2a) plus y_j ~ y_j+1, y_j+2, y_j+3: every x has all of Y above it (more than
    the staged capacity for a > 1024) and every y at most three upper neighbours of its own."""
    x, y = np.meshgrid(np.arange(a), np.arange(a, 2 * a), indexing="ij")
    s, d = [x.ravel()], [y.ravel()]
    for k in (1, 2, 3):
        s.append(np.arange(a, 2 * a - k))
        d.append(np.arange(a + k, 2 * a))
    return csr_from_pairs(2 * a, np.concatenate(s), np.concatenate(d))


def crown_triangles(a):
    """An x with each of the 3a - 6 edges inside Y, plus the triples of Y within a window of four: {j, j+1, j+2},
    {j, j+1, j+3}, {j, j+2, j+3}."""
    assert a >= 4
    return a * (3 * a - 6) + (3 * a - 8)


def pendants(n=1400, att=1030, P=8, Q=16):
    """K_n plus P vertices adjacent to the clique members [0, att) and Q vertices adjacent to the members [att, n).  In
    degree order the P vertices have att > 1024 upper neighbours u, each with |Up(u)| = tail + (n - att): against a
    non-hub the tail is the strictly shorter side."""
    iu, ju = np.triu_indices(n, 1)
    s, d = [iu], [ju]
    for k in range(P):
        s.append(np.full(att, n + k))
        d.append(np.arange(att))
    for k in range(Q):
        s.append(np.full(n - att, n + P + k))
        d.append(np.arange(att, n))
    return csr_from_pairs(n + P + Q, np.concatenate(s), np.concatenate(d))


def pendants_triangles(n=1400, att=1030, P=8, Q=16):
    return clique_triangles(n) + P * (att * (att - 1) // 2) + Q * ((n - att) * (n - att - 1) // 2)


def sparse17():
    """2^17 vertices: 6 V random pairs and 200 000 random pairs inside 1500 core vertices.  More vertices than the default
    65536 hubs, so the non-hubs are a real population (hub_base = 65536)."""
    V = 1 << 17
    rng = np.random.default_rng(20240617)
    a, b = rng.integers(0, V, 6 * V), rng.integers(0, V, 6 * V)
    core = rng.choice(V, 1500, replace=False)
    ca, cb = core[rng.integers(0, 1500, 200000)], core[rng.integers(0, 1500, 200000)]
    return csr_from_pairs(V, np.concatenate([a, ca]), np.concatenate([b, cb]))


def sym_rmat(scale):
    g = po.symmetrize(po.rmat_graph(scale, permute=True))
    return g.begin, g.node_idx


def oracle_graph(begin, node_idx):
    """The host graph the oracle counts on (symmetric: the in-rows are the out-rows)."""
    return po.Graph(len(begin) - 1, begin, node_idx, np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(node_idx, np.int32))


# name -> (builder, closed form or None)
GRAPHS = {
    "clique1100": (lambda: clique(1100), lambda: clique_triangles(1100)),
    "crown1100": (lambda: crown(1100), lambda: crown_triangles(1100)),
    "pendants": (pendants, pendants_triangles),
    "sparse17": (sparse17, None),
    "sym_rmat12": (lambda: sym_rmat(12), None),
}
TINY = {
    "clique40": (lambda: clique(40), lambda: clique_triangles(40)),      # H = 0: no hub matrix
    "clique65": (lambda: clique(65), lambda: clique_triangles(65)),      # H = 64, hub_base = 1
    "clique100": (lambda: clique(100), lambda: clique_triangles(100)),   # H = 64, hub_base = 36
}

# ---------------------------------------------------------------- knobs
# GMX_TC_HUBS is read when the oriented copy is built (a fresh upload per value), the other three on every call.  The
# kernel multiplies GMX_TC_RATIO and GMX_TC_HUB_TAIL by list lengths in int32: with lists under 2^15 entries these values
# stay far below 2^31; do not pass larger ones.
KNOBS = {
    "default": {},
    "hubs0": {"GMX_TC_HUBS": "0"},
    "hubs64": {"GMX_TC_HUBS": "64"},
    "alone0": {"GMX_TC_ALONE": "0"},
    "aloneBig": {"GMX_TC_ALONE": "1000000"},
    "hubs0+alone0": {"GMX_TC_HUBS": "0", "GMX_TC_ALONE": "0"},
    "hubs0+aloneBig": {"GMX_TC_HUBS": "0", "GMX_TC_ALONE": "1000000"},
    "hubs0+ratio0": {"GMX_TC_HUBS": "0", "GMX_TC_RATIO": "0"},
    "hubs0+ratioBig": {"GMX_TC_HUBS": "0", "GMX_TC_RATIO": "65536"},
    "hubtail0": {"GMX_TC_HUB_TAIL": "0"},
    "hubtailBig": {"GMX_TC_HUB_TAIL": "1024"},
    "hubs64+alone0": {"GMX_TC_HUBS": "64", "GMX_TC_ALONE": "0"},
}
KNOB_VARS = ("GMX_TC_HUBS", "GMX_TC_ALONE", "GMX_TC_RATIO", "GMX_TC_HUB_TAIL")


def census_args(knobs):
    """The census arguments of a knob set."""
    env = KNOBS[knobs]
    return dict(hubs=int(env["GMX_TC_HUBS"]) if "GMX_TC_HUBS" in env else None, alone=int(env.get("GMX_TC_ALONE", ALONE)),
                ratio=int(env.get("GMX_TC_RATIO", RATIO)), hub_tail=int(env.get("GMX_TC_HUB_TAIL", HUB_TAIL)))


# ---------------------------------------------------------------- the kernel's path selection, restated
def hub_count(V, hubs=None):
    H = hubs if hubs is not None else (HUB_MAX // 2 if V <= (1 << 24) else HUB_MAX)
    return min(H, V) & ~63


_SLOTS = {}


def oriented_slots(begin, node_idx):
    """Per slot s of Up(v) with s + 1 < |Up(v)|, on the copy relabelled by ascending degree: u, |Up(u)|, the length of the
    tail above s, and the length of the list from the slot's 64-slot group on.  Cached per pair of arrays."""
    key = (id(begin), id(node_idx))
    if key in _SLOTS:
        return _SLOTS[key][2]
    V = len(begin) - 1
    deg = np.diff(begin)
    order = np.argsort(deg, kind="stable")          # as the device's stable radix sort by degree
    perm = np.empty(V, np.int64)
    perm[order] = np.arange(V)
    ns = perm[np.repeat(np.arange(V), deg)]
    nd = perm[node_idx]
    up = nd > ns
    k = np.sort(ns[up] * V + nd[up])                # Up(v), sorted, row after row
    v, u = k // V, k % V
    nup = np.bincount(v, minlength=V)
    ub = np.concatenate([[0], np.cumsum(nup)])
    s = np.arange(len(k)) - ub[v]
    dv = nup[v]
    m = s + 1 < dv
    s, dv, u = s[m], dv[m], u[m]
    out = {"V": V, "u": u, "db": nup[u], "ta": dv - (s + 1), "da": dv - GROUP * (s // GROUP)}
    _SLOTS[key] = (begin, node_idx, out)           # (the arrays are kept alive: their ids stay theirs)
    return out


def census(begin, node_idx, hubs=None, alone=ALONE, ratio=RATIO, hub_tail=HUB_TAIL):
    """{(branch, "lds" | "mem"): slots} for every pair of PAIRS, plus "hub_base" and "idle" (slots with an empty side)."""
    S = oriented_slots(begin, node_idx)
    V, u, db, ta, da = S["V"], S["u"], S["db"], S["ta"], S["da"]
    hub_base = V - hub_count(V, hubs)
    in_lds = da <= CAP
    hubu = u >= hub_base
    hub_side = hubu & (ta <= hub_tail * db)
    tail_side = np.where(hubu, hub_side, ta < db)
    shorter = np.where((db == 0) | (ta == 0), 0, np.where(tail_side, ta, db))
    lone = (shorter > 0) & (shorter <= alone)
    wave = shorter > alone
    stream_up = wave & ~hub_side & in_lds & (db <= ratio * ta)
    branch = {
        "A-hubtail": lone & tail_side & hubu,
        "A-walkUpU": lone & ~tail_side,
        "A-tailSearch": lone & tail_side & ~hubu,
        "W-hub": wave & hub_side,
        "W-streamUpU": stream_up,
        "W-streamTail": wave & ~hub_side & ~stream_up,
    }
    out = {"hub_base": int(hub_base), "idle": int((shorter == 0).sum())}
    for name, m in branch.items():
        out[(name, "lds")] = int((m & in_lds).sum())
        out[(name, "mem")] = int((m & ~in_lds).sum())
    assert out[("W-streamUpU", "mem")] == 0
    del out[("W-streamUpU", "mem")]
    assert out["idle"] + sum(out[p] for p in PAIRS) == len(u)
    return out
