"""graphlets' row in the table of interleaved entries (handle_sequences.ROWS): its argument sets, its CPU model, the fake
device's answer and the check, in the form of the rows defined in handle_sequences.py itself.

The row is added when this module is imported, and both graphlets test files import it, exactly as squares_sequences.py does
for squares: in a run that collects tests/ the table's forward, reverse and shuffled passes, its workspace test and its
one-at-a-time host checks then include graphlets like every other entry, and `test_every_entry_of_the_graph_class_is_a_row`
finds Graph.graphlets in the table.  The row belongs in handle_sequences.py, next to squares', where the next change that may
edit that file should move it (and add graphlets to GROUPS["tcd_plan"], NO_ORDER and DS_ENTRIES there).

The identity-order argument set runs on D only: test_gpu_handle_sequences.py::test_workspace counts the plan builds of S."""
import re

import handle_sequences as hs
from graphlets_model import graphlets_formulas

LOG = re.compile(r"gmx graphlets: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) adj_built (?P<adj_built>\d) "
                 r"groups_built (?P<groups_built>\d) squares_built (?P<squares_built>\d) kclique_built (?P<kclique_built>\d); cap (?P<cap>\d+) long (?P<long>\d+) "
                 r"counts (?P<counts>\w+) induced (?P<induced>\d); items (?P<staged>\d+) staged \+ (?P<memory>\d+) memory; long_rows (?P<long_rows>\d+); "
                 r"triangles (?P<triangles>\d+); totals (?P<totals>\d+(?: \d+){8})\n")
ARGS = [("S", {"per_vertex": True, "induced": True}), ("B", {"per_vertex": True, "induced": False}), ("D", {"per_vertex": False, "induced": True}),
        ("D", {"per_vertex": True, "induced": True, "_env": {"GMX_GRAPHLETS_NO_ORDER": "1"}})]


def log_fields(err):
    m = LOG.search(err)
    assert m, err
    f = {k: (v if k in ("order", "counts", "totals") else int(v)) for k, v in m.groupdict().items()}
    f["totals"] = [int(x) for x in f["totals"].split()]
    return f


def _model(inp, a):
    w = graphlets_formulas(inp.V, inp.begin, inp.idx, a["induced"])
    w["gdv"].setflags(write=False)
    w["totals"].setflags(write=False)
    return w


def _walked(a, w):
    return w["triangles"] if a["per_vertex"] else 0


def _nonzero(a, w):
    return w["nonzero"] if a["per_vertex"] else 0


def _check(inp, a, want, got):
    gdv, totals, st, f = got
    assert (gdv is None) == (not a["per_vertex"]) and (gdv is None or (gdv.shape == want["gdv"].shape and gdv.tobytes() == want["gdv"].tobytes()))
    assert totals.tobytes() == want["totals"].tobytes() and f["totals"] == want["totals"].tolist() and f["triangles"] == _walked(a, want)
    assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == (1, _walked(a, want), _nonzero(a, want))


def _fake(inp, a, want):
    return (want["gdv"].copy() if a["per_vertex"] else None, want["totals"].copy(),
            hs.stats(iterations=1, edges_examined=_walked(a, want), vertices_reached=_nonzero(a, want)), {"totals": want["totals"].tolist(), "triangles": _walked(a, want)})


if "graphlets" not in hs.ROWS:
    hs.row("graphlets", ARGS, lambda g, inp, a: g.graphlets(per_vertex=a["per_vertex"], induced=a["induced"]), _model, _fake, _check,
           log=("GMX_GRAPHLETS_LOG", log_fields))
