"""What the sampling tests share: the 48-bit stream, the literal one-thread loops of the sampling programs (the arbiter),
a numpy model of the parallel scheme the device follows, and the small graphs with their pinned results."""
import numpy as np

A, C48, MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1
X0 = 0x0AA849495101          # {0x330E, 1, 0} after the shim's warm-up draw


class Stream:
    """x = (A x + C) mod 2^48; a draw yields x / 2^48, which is what erand48 returns."""

    def __init__(self, x):
        self.x = x & MASK

    def uniform(self):
        self.x = (A * self.x + C48) & MASK
        return self.x / 281474976710656.0

    def pick(self, V):
        return int(self.uniform() * float(V))


def jump_map(n):
    """(a, c) of n single steps"""
    ra, rc, pa, pc = 1, 0, A, C48
    while n:
        if n & 1:
            ra, rc = (pa * ra) & MASK, (pa * rc + pc) & MASK
        pa, pc = (pa * pa) & MASK, (pa * pc + pc) & MASK
        n >>= 1
    return ra, rc


def jump(x, n):
    a, c = jump_map(n)
    return (a * x + c) & MASK


def walk_n(V, p_size):
    return int(np.float32(V) * np.float32(p_size))


def walk_loop(begin, node_idx, p_size, p_jump, num_tokens, max_rounds, x):
    """parallel_random_walk_jump_sampling as one thread runs it -> (selected u8[V], token i32[V], count, rounds, state)"""
    V = len(begin) - 1
    begin = [int(b) for b in begin]
    node_idx = [int(t) for t in node_idx]
    s = Stream(x)
    pj = float(np.float32(p_jump))
    token = [0] * V
    selected = np.zeros(V, np.uint8)
    S = set()
    while True:
        S.add(s.pick(V))
        if len(S) >= num_tokens:
            break
    for n in S:
        token[n] = 1
    N = walk_n(V, p_size)
    count = rounds = 0
    while count < N and rounds < max_rounds:
        nxt = [0] * V
        for n in range(V):
            if token[n] > 0:
                if not selected[n]:
                    selected[n] = 1
                    count += 1
                deg = begin[n + 1] - begin[n]
                for _ in range(token[n]):
                    if deg == 0 or s.uniform() < pj:
                        m = s.pick(V)
                    else:
                        m = node_idx[begin[n] + int(s.uniform() * float(deg))]
                    nxt[m] += 1
        token = nxt
        rounds += 1
    return selected, np.array(token, np.int32), count, rounds, s.x


def node_loop(begin, by_degree, N, x):
    """random_node_sampling / random_degree_node_sampling -> (selected u8[V], count, state)"""
    V = len(begin) - 1
    s = Stream(x)
    sel = np.zeros(V, np.uint8)
    deg_sum = np.float64(int(begin[V]) - int(begin[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        for v in range(V):
            dice = np.float64(s.uniform())
            if by_degree:
                prob = (np.float64(int(begin[v + 1]) - int(begin[v])) / deg_sum) * np.float64(N)
            else:
                prob = np.float64(1.0) / np.float64(N)
            sel[v] = 1 if dice < prob else 0
    return sel, int(sel.sum()), s.x


def single_walk_loop(begin, node_idx, N, c, x):
    """random_walk_sampling_with_random_jump: one walker, N steps -> (members sorted, state)"""
    V = len(begin) - 1
    s = Stream(x)
    n = s.pick(V)
    S = set()
    count = 0
    while count < N:
        S.add(n)
        count += 1
        deg = int(begin[n + 1]) - int(begin[n])
        if deg == 0 or s.uniform() < c:
            n = s.pick(V)
        else:
            n = int(node_idx[int(begin[n]) + int(s.uniform() * float(deg))])
    return sorted(S), s.x


# ---- the parallel scheme, vectorised: what the device does, stated with numpy
def _states(x, offs):
    """the state after offs[i] draws from x (offs >= 0), by the 2^k table"""
    offs = np.asarray(offs, np.int64)
    out = [x] * len(offs)
    tab = [jump_map(1 << k) for k in range(48)]
    for i, o in enumerate(offs):
        y, k, o = x, 0, int(o)
        while o:
            if o & 1:
                y = (tab[k][0] * y + tab[k][1]) & MASK
            o >>= 1
            k += 1
        out[i] = y
    return out


def walk_model(begin, node_idx, p_size, p_jump, num_tokens, max_rounds, x, batch=64):
    V = len(begin) - 1
    begin = np.asarray(begin, np.int64)
    deg = begin[1:] - begin[:-1]
    pj = float(np.float32(p_jump))
    token = np.zeros(V, np.int64)
    have = 0
    while have < num_tokens:                   # the initial set in batches
        st = _states(x, np.arange(1, batch + 1))
        p = np.array([int((y / 281474976710656.0) * float(V)) for y in st])
        first = np.full(V, batch, np.int64)
        np.minimum.at(first, p, np.arange(batch))
        new = (token[p] == 0) & (first[p] == np.arange(batch))
        incl = np.cumsum(new)
        need = num_tokens - have
        cut = batch
        hit = np.nonzero(new & (incl == need))[0]
        if len(hit):
            cut = int(hit[0]) + 1
        token[p[:cut][new[:cut]]] = 1
        have += int(new[:cut].sum())
        x = st[cut - 1]
    N = walk_n(V, p_size)
    selected = np.zeros(V, np.uint8)
    count = rounds = 0
    while count < N and rounds < max_rounds:
        live = np.nonzero(token)[0]
        count += int((selected[live] == 0).sum())
        selected[live] = 1
        dpt = np.where(deg[live] == 0, 1, 2)
        draws = token[live] * dpt
        base = np.concatenate(([0], np.cumsum(draws)))
        nxt = np.zeros(V, np.int64)
        for i, n in enumerate(live):
            offs = base[i] + np.arange(token[n]) * dpt[i]
            for y in _states(x, offs):
                s = Stream(y)
                if deg[n] == 0 or s.uniform() < pj:
                    m = s.pick(V)
                else:
                    m = int(node_idx[begin[n] + int(s.uniform() * float(deg[n]))])
                nxt[m] += 1
        x = jump(x, int(base[-1]))
        token = nxt
        rounds += 1
    return selected, token.astype(np.int32), count, rounds, x


# ---- graphs
def csr(V, edges):
    """rows in the order given (no sorting): the CSR a test uploads"""
    rows = [[] for _ in range(V)]
    for s, t in edges:
        rows[s].append(t)
    begin = np.zeros(V + 1, np.int32)
    begin[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([t for r in rows for t in r], np.int32)
    return begin, idx


def ring64():
    return csr(64, [(v, (v + 1) % 64) for v in range(64)])


def star64():
    return csr(64, [(0, t) for t in range(1, 48)] + [(v, 0) for v in range(1, 48)])


# graph, p_size, p_jump, tokens -> count, rounds, selsum, tokw, state after (all from X0)
WALK_TABLE = [
    ("ring64", 0.5, 0.15, 4, 33, 9, 1035, 78, 0x32016502343D),
    ("ring64", 0.5, 0.0, 4, 33, 9, 1293, 175, 0x32016502343D),
    ("ring64", 1.0, 1.0, 64, 64, 1, 2016, 2086, 0xBBFF476612F5),
    ("ring64", 0.25, 0.15, 1, 16, 16, 409, 41, 0x0315F52A9E98),
    ("star64", 0.75, 0.15, 8, 48, 22, 1357, 92, 0x03B1D38E4E6E),
    ("star64", 1.0, 0.5, 32, 64, 11, 2016, 557, 0xB721867720A8),
]
GRAPHS = {"ring64": ring64, "star64": star64}
# graph, by_degree, N -> selected, id sum; the state after is NODE_STATE for both
NODE_TABLE = [("ring64", 0, 4, 15, 364), ("star64", 1, 16, 10, 180)]
NODE_STATE = 0x340B5E010841


def summarize(selected, token):
    ids = np.arange(len(selected), dtype=np.int64)
    return int(ids[selected != 0].sum()), int((ids * token.astype(np.int64)).sum())
