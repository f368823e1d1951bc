"""louvain's row in the table of interleaved entries (handle_sequences.ROWS): its argument sets, its CPU model, the fake
device's answer and the check, in the form of the rows defined in handle_sequences.py itself.

The row is added when this module is imported, and both louvain test files import it, exactly as kclique_sequences.py does
for kclique: in a run that collects tests/ the table's forward, reverse and shuffled passes, its workspace test and its
one-at-a-time host checks then include louvain like every other entry, and `test_every_entry_of_the_graph_class_is_a_row`
finds Graph.louvain in the table.  The row belongs in handle_sequences.py, next to kclique's, where the next change that may
edit that file should move it."""
import re
import struct

import handle_sequences as hs
from louvain_model import louvain_model

LOG = re.compile(r"gmx louvain: V (?P<V>\d+) E (?P<E>\d+) weighted (?P<weighted>[01]) levels (?P<levels>\d+) rounds (?P<rounds>\d+) rollbacks (?P<rollbacks>\d+) "
                 r"cuts (?P<cuts>\d+) moves (?P<moves>\d+) sizes (?P<sizes>[-\d/,]+) comms (?P<comms>\d+) intra (?P<intra>\d+) overflowed (?P<overflowed>\d+)\n")
COUNTERS = ("levels", "rounds", "rollbacks", "cuts", "moves")
# unweighted on S; weighted on D (and on R, where the same weights sit on other slots: another graph); one level on D
ARGS = [("S", {"w": None}), ("D", {"w": 31}), ("D", {"w": 32, "max_levels": 1, "max_rounds": 3})]


def sizes_text(sizes):
    return ",".join("%d/%d" % s for s in sizes) if sizes else "-"


def weights(inp, a):
    return None if a["w"] is None else hs.lengths(inp.label, a["w"])


def same(want, got, fields=None):
    """got = Graph.louvain()'s tuple (with the log line's fields behind it, or fields given) against the model's dict: the
    partition, the counts and the 8 bytes of the modularity, the three stats and the log's counters."""
    comm, nc, nl, q, intra, st = got[:6]
    f = got[6] if fields is None and len(got) > 6 else fields
    assert comm.dtype == want["comm"].dtype and comm.tobytes() == want["comm"].tobytes()
    assert (nc, nl, intra) == (want["num_comms"], want["num_levels"], want["intra"])
    assert struct.pack("<d", q) == struct.pack("<d", want["modularity"]), (q, want["modularity"])
    assert (st["iterations"], st["vertices_reached"], st["edges_examined"]) == (want["iterations"], want["num_comms"], want["edges_examined"])
    if f is not None:
        assert {k: f[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, (f, {k: want[k] for k in COUNTERS})
        assert f["sizes"] == sizes_text(want["sizes"]) and (f["comms"], f["intra"]) == (want["num_comms"], want["intra"])


def _model(inp, a):
    return louvain_model(inp.V, inp.begin, inp.idx, weights(inp, a), a.get("max_levels", 32), a.get("max_rounds", 64))


def _fake(inp, a, w):
    f = {k: w[k] for k in COUNTERS}
    f.update(V=inp.V, E=inp.E, weighted=int(a["w"] is not None), sizes=sizes_text(w["sizes"]), comms=w["num_comms"], intra=w["intra"], overflowed=0)
    return (w["comm"].copy(), w["num_comms"], w["num_levels"], w["modularity"], w["intra"],
            hs.stats(iterations=w["iterations"], vertices_reached=w["num_comms"], edges_examined=w["edges_examined"]), f)


if "louvain" not in hs.ROWS:
    hs.row("louvain", ARGS, lambda g, inp, a: g.louvain(weights(inp, a), a.get("max_levels", 32), a.get("max_rounds", 64)), _model, _fake,
           lambda inp, a, want, got: same(want, got), log=("GMX_LOUVAIN_LOG", hs.named_line(LOG, keep=("sizes",))))
