"""kclique's row in the table of interleaved entries (handle_sequences.ROWS): its argument sets, its CPU model, the fake
device's answer and the check, in the form of the rows defined in handle_sequences.py itself.

The row is added when this module is imported, and both kclique test files import it: in a run that collects tests/ the
table's forward, reverse and shuffled passes, its workspace test and its one-at-a-time host checks then include kclique
like every other entry, and `test_every_entry_of_the_graph_class_is_a_row` finds Graph.kclique in the table.  A run that
collects tests/test_handle_sequences_host.py WITHOUT either kclique file does not import this module and that test then
reports Graph.kclique as an entry without a row: the row belongs in handle_sequences.py, next to ktruss's, where the next
change that may edit that file should move it (and add kclique to GROUPS["tcd_plan"], NO_ORDER and DS_ENTRIES there)."""
import re

import handle_sequences as hs
from kclique_model import kclique_model

LOG = re.compile(r"gmx kclique: plan V (?P<V>\d+) E (?P<E>\d+) up (?P<up>\d+) order (?P<order>\w+) built (?P<built>\d) classes_built (?P<classes_built>\d); "
                 r"k (?P<k>\d) cap (?P<cap>\d+) counts (?P<counts>\w+); items (?P<wave>\d+) wave \+ (?P<small>\d+) small \+ (?P<large>\d+) large \+ "
                 r"(?P<glob>\d+) global \+ (?P<skipped>\d+) skipped; batches (?P<batches>\d+) cliques (?P<cliques>\d+)\n")
ARGS = [("S", {"k": 4}), ("D", {"k": 3}), ("D", {"k": 4, "_env": {"GMX_KCLIQUE_NO_ORDER": "1"}})]


def _nonzero(w):
    return int((w["count"] > 0).sum())


def _check(inp, a, want, got):
    cnt, n, st, f = got
    assert cnt.tobytes() == want["count"].tobytes() and n == want["cliques"] == f["cliques"]
    assert (st["iterations"], st["edges_examined"], st["vertices_reached"]) == (1, want["up"], _nonzero(want))


def _fake(inp, a, w):
    return w["count"].copy(), w["cliques"], hs.stats(iterations=1, edges_examined=w["up"], vertices_reached=_nonzero(w)), {"cliques": w["cliques"]}


if "kclique" not in hs.ROWS:
    hs.row("kclique", ARGS, lambda g, inp, a: g.kclique(a["k"]), lambda inp, a: kclique_model(inp.V, inp.begin, inp.idx, a["k"]), _fake, _check,
           log=("GMX_KCLIQUE_LOG", hs.named_line(LOG, keep=("order", "counts"))))
