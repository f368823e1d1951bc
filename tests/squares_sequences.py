"""squares' row in the table of interleaved entries (handle_sequences.ROWS): its argument sets, its CPU model, the fake
device's answer and the check, in the form of the rows defined in handle_sequences.py itself.

The row is added when this module is imported, and both squares test files import it, exactly as kclique_sequences.py does
for kclique: in a run that collects tests/ the table's forward, reverse and shuffled passes, its workspace test and its
one-at-a-time host checks then include squares like every other entry, and `test_every_entry_of_the_graph_class_is_a_row`
finds Graph.squares in the table.  The row belongs in handle_sequences.py, next to kclique's, where the next change that may
edit that file should move it (and add squares to GROUPS["tcd_plan"], NO_ORDER and DS_ENTRIES there).

The identity-order argument set runs on D only: test_gpu_handle_sequences.py::test_workspace counts the plan builds of S."""
import re

import handle_sequences as hs
from squares_model import squares_schedule

LOG = re.compile(r"gmx squares: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) adj_built (?P<adj_built>\d) "
                 r"classes_built (?P<classes_built>\d); wave_max (?P<wave_max>\d+) lds_slots (?P<lds_slots>\d+) split (?P<split>\d+) batch_bytes (?P<batch_bytes>\d+) "
                 r"counts (?P<counts>\w+); items (?P<wave>\d+) wave \+ (?P<block>\d+) block \+ (?P<glob>\d+) global \((?P<nsplit>\d+) split\) \+ "
                 r"(?P<skipped>\d+) skipped; wedges (?P<wedges>\d+) batches (?P<batches>\d+) squares (?P<squares>\d+)\n")
ARGS = [("S", {"per_vertex": True}), ("B", {"per_vertex": True}), ("D", {"per_vertex": False}), ("D", {"per_vertex": True, "_env": {"GMX_SQUARES_NO_ORDER": "1"}})]


def _model(inp, a):
    # (per_vertex only says what is asked of the device; the order changes D, W and wedges but no result)
    return {True: squares_schedule(inp.V, inp.begin, inp.idx, True), False: squares_schedule(inp.V, inp.begin, inp.idx, False)}


def _want(a, want):
    return want["GMX_SQUARES_NO_ORDER" not in a.get("_env", {})]


def _nonzero(a, w):
    return int((w["count"] > 0).sum()) if a["per_vertex"] else 0


def _check(inp, a, want, got):
    cnt, n, st, f = got
    w = _want(a, want)
    assert (cnt is None) == (not a["per_vertex"]) and (cnt is None or cnt.tobytes() == w["count"].tobytes())
    assert n == w["squares"] == f["squares"] and f.get("wedges", w["wedges"]) == w["wedges"]
    assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == (1, w["wedges"], _nonzero(a, w))


def _fake(inp, a, want):
    w = _want(a, want)
    return (w["count"].copy() if a["per_vertex"] else None, w["squares"], hs.stats(iterations=1, edges_examined=w["wedges"], vertices_reached=_nonzero(a, w)),
            {"squares": w["squares"], "wedges": w["wedges"]})


if "squares" not in hs.ROWS:
    hs.row("squares", ARGS, lambda g, inp, a: g.squares(per_vertex=a["per_vertex"]), _model, _fake, _check,
           log=("GMX_SQUARES_LOG", hs.named_line(LOG, keep=("order", "counts"))))
