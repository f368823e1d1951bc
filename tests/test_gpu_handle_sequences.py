"""The sequences of handle_sequences.py on the device: many entries interleaved on one graph handle, each result against the
CPU model of its own arguments (the entry's own checker, as strict as in its own test file).  What a handle keeps between
calls -- the traversal object, the oriented copy, the shared tcd plan, the PageRank plans, v_cover's plan, sssp_path_f64's
scratch -- and the process-wide workspace underneath are what is under test: a stale plan, a scratch word carried over or a
pointer into rewound workspace memory shows as a wrong answer in a later step, and run() names that step.

The log lines the entries already print show that the cached path ran (built 1 at a plan's first call, built 0 afterwards,
built 1 right after an order-knob flip; v_cover's plan built, then reused)."""
import contextlib
import os

import numpy as np
import pytest

import handle_sequences as hs

pytestmark = pytest.mark.gpu
LOGS = ("GMX_TCD_LOG", "GMX_LCC_LOG", "GMX_KTRUSS_LOG", "GMX_VC_LOG", "GMX_KCORE_LOG", "GMX_COLOR_LOG", "GMX_BICC_LOG")
KNOBS = LOGS + tuple(hs.NO_ORDER.values()) + ("GMX_PR_RANKS", "GMX_SSSP_PATH_SCHEDULE", "GMX_TC_HUBS")


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@contextlib.contextmanager
def knobs(**kw):
    """The library reads its knobs from the environment at every call."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Device:
    """The handles of one test by label (uploaded at first use), the Route and state objects held on them, and call(step)."""

    def __init__(self, gmx, capfd):
        self.gmx, self.capfd = gmx, capfd
        self.handles, self.routes, self.held = {}, {}, []
        self.bfs = self.pr = self.pr_alone = None
        self.bfs_done = True
        self.results = []   # (step, result) of every call

    def handle(self, label):
        if label not in self.handles:
            self.handles[label] = hs.upload(self.gmx, hs.input_of(label))
        return self.handles[label]

    def route(self, label, seed):
        if (label, seed) not in self.routes:
            self.routes[label, seed] = self.handle(label).route(hs.lengths(hs.input_of(label).label, seed))
        return self.routes[label, seed]

    def state(self, step, inp, a):
        gmx, g = self.gmx, self.handle(step.handle)
        if step.entry == "route_query":
            return self.route(step.handle, a["w"]).query(a["src"], a["dst"])
        if step.entry == "bfs_state":
            if a["op"] == "start":
                self.bfs = self.bfs or gmx.BfsState(g, 0, 1)
                self.bfs.start(a["root"])
                self.bfs_done = False
            elif a["op"] == "step":
                if not self.bfs_done:   # (a traversal that has found nothing new is over)
                    assert not self.bfs.step_begin()   # one rank: nothing to exchange
                    self.bfs_done = self.bfs.step_end() == 0
            else:
                assert self.bfs_done
                return self.bfs.download()
            return None
        # pr_state: the same steps on a handle of its own alongside; the downloads must be the same bytes
        if a["op"] == "reset":
            options = gmx.GMX_PR_RELABEL | gmx.GMX_PR_HOT_LDS | gmx.GMX_PR_SLICED
            self.pr = gmx.PageRankState(g, hs.PR_STATE_ELEM, 0, 1, options)
            self.pr_alone = gmx.PageRankState(self.handle(step.handle + "#alone"), hs.PR_STATE_ELEM, 0, 1, options)
            for st in (self.pr, self.pr_alone):
                st.reset(0.85)
        elif a["op"] == "step":
            self.pr.step()
            self.pr_alone.step()
        else:
            got, alone = self.pr.download(), self.pr_alone.download()
            assert got.tobytes() == alone.tobytes()
            return got
        return None

    def call(self, step):
        if isinstance(step.k, str):   # a call its entry's own tests expect to be refused
            try:
                hs.REFUSALS[step.k][1](self.handle(step.handle), hs.input_of(step.handle))
            except self.gmx.GmxError as e:
                result = str(e)
            else:
                result = "not refused"
            self.results.append((step, result))
            return result
        inp, a = hs.args_of(step)
        env = dict(a.get("_env", {}))
        a = {k: v for k, v in a.items() if k != "_env"}
        r = hs.table(step.entry)
        if r.log:
            env[r.log[0]] = "1"
        self.capfd.readouterr()
        with knobs(**env):
            raw = self.state(step, inp, a) if step.entry in hs.EXTRA else r.call(self.handle(step.handle), inp, a)
        err = self.capfd.readouterr().err
        result = hs.with_log(step.entry, raw, err) if r.log else raw
        self.results.append((step, result))
        return result

    def run(self, steps):
        return hs.run(steps, self.call, hs.check_step)

    def free(self):
        for st in (self.bfs, self.pr, self.pr_alone):
            if st is not None:
                st.free()
        for r in self.routes.values():
            r.free()
        for g in self.handles.values():
            g.free()
        self.handles, self.routes = {}, {}


@pytest.fixture
def dev(gmx, capfd):
    d = Device(gmx, capfd)
    yield d
    d.free()


def payload(x):
    """The bytes of a result: its arrays and numbers, without the statistics and the log fields (times differ)."""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, dict):
        return b"" if "kernel_ms" in x or "V" in x or x == {} else b"".join(payload(x[k]) for k in sorted(x) if k not in ("stats", "log"))
    if isinstance(x, (tuple, list)):
        return b"|".join(payload(y) for y in x)
    return repr(x).encode()


def test_forward(dev, gmx, capfd):
    """Every row in table order on the shared handles, and each result the bytes of the same call on a handle of its own
    (bidir_dijkstra aside: which shortest route it returns is not specified)."""
    steps = hs.forward()
    assert dev.run(steps) == len(steps)
    shared = list(dev.results)
    for step, result in shared:
        if step.entry == "bidir_dijkstra":
            continue
        alone = Device(gmx, capfd)
        try:
            assert payload(alone.call(step)) == payload(result), hs.describe(step)
        finally:
            alone.free()


def test_reverse(dev):
    steps = hs.reverse()
    assert dev.run(steps) == len(steps)


def test_shuffled(dev):
    """A fixed permutation of all rows, twice: the second pass, with the other argument sets, meets what the first left."""
    steps = hs.shuffled()
    assert dev.run(steps) == len(steps)


def family_ids():
    return ["%s-%s" % (group, m.replace("/", "")) for group, (_, members) in hs.GROUPS.items() for m in members]


@pytest.mark.parametrize("case", family_ids())
def test_families(gmx, capfd, case):
    """Every ordered pair (a, b) of a group of entries that share state, a given: a, b, a on a fresh handle."""
    group, first = case.split("-")
    first = first.replace("pagerank", "pagerank/")
    for steps in hs.families(group, first):
        d = Device(gmx, capfd)
        try:
            assert d.run(steps) == len(steps)
            if group == "tcd_plan":   # the cached plan really was used, and rebuilt when the calling entry's knob changed the order
                built = [result[-1]["built"] for _, result in d.results]
                orders = [result[-1]["order"] for _, result in d.results]
                assert built == hs.plan_builds(steps) == [1, 0, 1, 0, 1], (case, built)
                assert orders == ["degree", "degree", "identity", "identity", "degree"], (case, orders)
        finally:
            d.free()


def test_two_handles_an_upload_and_its_sorted_twin(dev):
    dr, _ = hs.two_handles()
    assert dev.handle("R").edge_order() is not None and dev.handle("D").edge_order() is None
    assert dev.run(dr) == len(dr)


def test_two_handles_directed_and_symmetric(dev):
    _, ds = hs.two_handles()
    assert dev.run(ds) == len(ds)


def test_held_routes(dev):
    """Two Route objects with different weights, both open from the start; their queries interleave with the other weighted
    searches of the same handle."""
    routes, _, _ = hs.held_state()
    for seed in hs.ROUTE_WEIGHTS:
        dev.route("D", seed)
    assert dev.run(routes) == len(routes)


def test_held_bfs_state(dev):
    _, bfs, _ = hs.held_state()
    assert dev.run(bfs) == len(bfs)
    assert dev.bfs_done


def test_held_pagerank_state(dev):
    _, _, pr = hs.held_state()
    assert dev.run(pr) == len(pr)


def test_refused(dev):
    steps = hs.refused()
    assert dev.run(steps) == len(steps)
    assert [r for s, r in dev.results if isinstance(s.k, str) and "status -1" not in r] == []


def test_workspace(dev, gmx):
    """The arena rewinds and does not grow on a repeat; after it has been given back, the handles' cached plans and the open
    Route still answer right, and the arena is taken again."""
    L = gmx.lib()
    fwd, rev = hs.forward(), hs.reverse()
    q = [hs.Step("route_query", n, "D") for n in range(4)]
    assert dev.run(fwd + q[:1]) == len(fwd) + 1
    used = L.gmx_workspace_bytes()
    assert used > 0
    assert dev.run(fwd + q[1:2]) == len(fwd) + 1
    assert L.gmx_workspace_bytes() == used
    plans = [r[3]["plan"] for s, r in dev.results if s.entry == "v_cover"]
    assert plans == ["built", "reused"]
    builds = {e: [r[-1]["built"] for s, r in dev.results if s.entry == e] for e in ("clustering", "ktruss")}
    assert builds == {"clustering": [1, 0], "ktruss": [0, 0]}, builds   # (ktruss comes after clustering on S: it finds the plan)
    assert L.gmx_workspace_release() == 0
    assert L.gmx_workspace_bytes() == 0
    assert dev.run(q[2:3] + rev + q[3:]) == len(rev) + 2
    assert L.gmx_workspace_bytes() > 0


@pytest.mark.parametrize("first", ["0", None, "1000000"])
def test_triangle_counting_hub_knob_after_the_first_call(gmx, first):
    """GMX_TC_HUBS is read when the oriented copy is built, at the first call on a symmetric graph: whatever it says then and
    on later calls, the count is the oracle's."""
    inp = hs.inputs()["S"]
    want = hs.want_of("triangle_counting", 0, "S")
    g = hs.upload(gmx, inp)
    try:
        for hubs in (first, "64", None, "0", "1000000", first):
            with knobs(**({} if hubs is None else {"GMX_TC_HUBS": hubs})):
                assert g.triangle_counting()[0] == want, (first, hubs)
                assert sum(g.triangle_counting(p, 3)[0] for p in range(3)) == want, (first, hubs)
                assert g.triangle_counting_cn()[0] == hs.want_of("triangle_counting_cn", 1, "S"), (first, hubs)
    finally:
        g.free()
