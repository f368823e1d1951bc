"""CPU: the designed graphs of bc_shapes.py are what test_gpu_bc_shapes.py takes them for, and the oracle's comp_BC on them
is what include/gmx.h promises.

The oracle against the float32 model written from gmx.h, bit for bit; the oracle against Brandes' accumulation in float64
within a bound derived from the graph; and the conditions that make the inputs worth their time on the device: every
form boundary of the per-seed visit kernels is hit in both visits, the forward sums round differently when added in the
opposite slot order in every kind of row, and path counts overflow into NaN next to finite values.

The inputs the suite had before do not tell summation orders apart in the forward visit.  Largest path count, measured
with brandes_f64 (2^24 = 1.68e7 is where a float32 sum of integers can first round):
    test_bc_vs_oracle_larger (the hub + 4 seeds)   RMAT-12 1.7e3, RMAT-14 permuted 1.9e3, RMAT-16 5.3e3, RMAT-18 permuted 1.2e4
    test_bc_random_host.GRAPHS (70 seeds each)     rmat10 1.2e3, rmat12p 2.3e3, rmat14 5.4e3
(a statement about those inputs as they are, not a test: better inputs there are welcome)."""
import numpy as np
import pytest

import bc_shapes as S
import pyoracle as po
from test_bc_random_host import same_f32

WITH_F64 = ("inexact", "sparse", "small")


def bits_differ(a, b):
    return a.view(np.uint32) != b.view(np.uint32)


def test_constants_are_parsed():
    small, dense, chunks = S.kernel_constants()
    assert 2 < small < 63 and 1 < dense < 62 and chunks >= 3     # what probe_patterns() lays its rows out for
    assert len(set(S.census_classes())) == 19


def test_ordered_row_sums_is_the_sequential_chain():
    """The models' sum against the loop it stands for, on terms where the order changes the bits."""
    rng = np.random.default_rng(1)
    cnt = np.array([0, 1, 700, 33, 0, 64, 2])
    row = np.repeat(np.arange(len(cnt)), cnt)
    term = (rng.random(len(row)) * 10.0 ** rng.integers(0, 12, len(row))).astype(np.float32)
    want_fw, want_bw = np.zeros(len(cnt), np.float32), np.zeros(len(cnt), np.float32)
    for r in range(len(cnt)):
        for t in term[row == r]:
            want_fw[r] = want_fw[r] + t
        for t in term[row == r][::-1]:
            want_bw[r] = want_bw[r] + t
    assert same_f32(S.ordered_row_sums(len(cnt), row, term), want_fw)
    assert same_f32(S.ordered_row_sums(len(cnt), row, term, reverse=True), want_bw)
    assert bits_differ(want_fw, want_bw).any()
    nan_inf = np.array([np.inf, 1, np.nan, 2, np.inf], np.float32)   # the padding leaves inf and NaN as they are
    got = S.ordered_row_sums(3, np.array([0, 0, 1, 1, 2]), nan_inf)
    assert np.isinf(got[0]) and np.isnan(got[1]) and np.isinf(got[2])


@pytest.mark.parametrize("name", S.FAMILIES)
def test_construction(name):
    """The layers are the levels from the root; back edges, repeated edges, self-loops and slots from vertices without a
    level are all there; rows are not in id order."""
    sh = S.family(name)
    og = sh.og
    dist = po.bfs_queue(og, sh.root)
    assert np.array_equal(np.where(dist == S.INT_MAX, -2, dist), sh.layer)
    assert (sh.layer[sh.extra] == -2).all() and int((sh.layer == -2).sum()) == len(sh.extra) >= 60
    src = np.repeat(np.arange(og.N), np.diff(og.begin))
    dst = og.node_idx
    r_dst = np.repeat(np.arange(og.N), np.diff(og.r_begin))
    assert np.array_equal(np.sort(src * og.N + dst), np.sort(og.r_node_idx.astype(np.int64) * og.N + r_dst))   # the reverse CSR mirrors the forward one
    ls, ld = sh.layer[src], sh.layer[dst]
    assert ((ls == -2) | (ld <= ls + 1)).all()                                   # no edge skips a layer
    assert int(((ls >= 0) & (ld <= ls)).sum()) >= 10_000 and int((src == dst).sum()) >= 1
    assert set(ld[ls == -2].tolist()) >= set(range(1, int(sh.layer.max()) + 1))   # unreached sources in every layer's reverse rows
    if name != "overflow":
        assert len(np.unique(src * og.N + dst)) < len(src) - 1000                   # repeated edges
    for begin, idx in ((og.begin, og.node_idx), (og.r_begin, og.r_node_idx)):
        same_row = np.diff(np.repeat(np.arange(og.N), np.diff(begin))) == 0
        assert int(((np.diff(idx) < 0) & same_row).sum()) >= og.M // 4
    assert og.M <= 1_700_000 and og.N <= 5000


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", S.FAMILIES)
def test_oracle_is_the_f32_model(name, skip):
    """po.bc == bc_model_f32 bit for bit; the model with every sum in descending slot order is a different function on
    the families with inexact path counts."""
    sh = S.family(name)
    seeds = S.seeds(name)
    assert seeds[0] == seeds[3] == sh.root and sh.layer[seeds[4]] == -2 and 0 < sh.layer[seeds[2]] < sh.layer.max()
    want = po.bc(sh.og, seeds, skip)
    assert same_f32(S.bc_model_f32(sh.og, seeds, skip), want)
    if skip and name in ("inexact", "small"):
        mutant = S.bc_model_f32(sh.og, seeds, skip, reverse_slots=True)
        assert int(bits_differ(mutant, want).sum()) >= sh.V // 2
    if not skip:     # the literal form: every sigma 0, NaN wherever a reached vertex has a BFS child
        assert not (np.isfinite(want) & (want != 0)).any() and np.isnan(want).sum() >= sh.V // 2


@pytest.mark.parametrize("name", WITH_F64)
def test_oracle_against_float64(name):
    """|po.bc - brandes_f64| / brandes_f64 <= f32_error_bound() (its docstring is the derivation: gamma_k for k = L^2 (R - 1) +
    L (F + 2) + seeds rounding factors, R / F the longest reverse / forward row, L the deepest level), and exact zeros
    where Brandes has zero.  Bound and largest error observed, 8 seeds:
        inexact   k = 78728  bound 4.7e-3   observed 9.3e-7
        sparse    k = 99016  bound 5.9e-3   observed 7.7e-7
        small     k = 78728  bound 4.7e-3   observed 4.2e-7
    The bound is a worst case over rows of up to 1100 slots; the errors observed are those of sums that mostly round
    both ways."""
    sh = S.family(name)
    seeds = S.seeds(name)
    ref, top = S.brandes_f64(sh.og, seeds)
    got = po.bc(sh.og, seeds, True)
    bound, k = S.f32_error_bound(sh.og, seeds)
    nz = ref > 0
    err = float((np.abs(got[nz].astype(np.float64) - ref[nz]) / ref[nz]).max())
    print(name, "k", k, "bound %.3g" % bound, "largest error %.3g" % err, "largest path count %.3g" % top)
    assert np.isfinite(got).all() and top < 1e30                 # no overflow here: the bound's model holds
    assert int(nz.sum()) >= sh.V // 2 and not got[~nz].any()
    assert err <= bound < 0.01


@pytest.fixture(scope="module")
def censuses():
    return {(name, int(s)): S.census(S.family(name).og, int(s)) for name in S.FAMILIES for s in set(S.seeds(name)[:3].tolist())}


def test_every_form_boundary_is_hit_in_both_visits(censuses):
    """Rows one short of, at and one past BFS_VISIT_SMALL, 64 and a step; a row of three steps; chunks with 1, BFS_DENSE_PASS,
    BFS_DENSE_PASS + 1 and 64 passing lanes; and the rest of census_classes(), over the families and their first seeds --
    and in `inexact` from its root alone, where the path counts are inexact."""
    for visit in ("fw", "rv"):
        total = {c: sum(v[visit][c] for v in censuses.values()) for c in S.census_classes()}
        print(visit, total)
        assert all(n >= 1 for n in total.values()), (visit, total)
        sh = S.family("inexact")
        alone = censuses["inexact", sh.root][visit]
        assert all(n >= 1 for n in alone.values()), (visit, alone)
    small, dense, chunks = S.kernel_constants()
    sparse = censuses["sparse", S.family("sparse").root]
    for visit in ("fw", "rv"):      # many chunks on the side of BFS_DENSE_PASS where the set bits are walked
        assert sparse[visit]["chunk_pass1"] >= 1000 and sparse[visit]["empty_chunk_between"] >= 100


def test_census_per_family(censuses):
    """The census from each family's root, printed for the record (pytest -s)."""
    for name in S.FAMILIES:
        c = censuses[name, S.family(name).root]
        for visit in ("fw", "rv"):
            print(name, visit, c[visit])
        assert c["fw"]["level_two_wave_rows"] >= 2 and c["rv"]["level_two_wave_rows"] >= 2


def test_summation_order_shows_in_every_kind_of_row():
    """Forward-visit sigma from the root of `inexact`, slot order against descending slot order: at least 50 vertices differ
    among the lane rows, among the wave rows of one step and among the rows of several steps."""
    sh = S.family("inexact")
    small, dense, chunks = S.kernel_constants()
    _, a, _ = S.seed_pass_f32(sh.og, sh.root, True)
    _, b, _ = S.seed_pass_f32(sh.og, sh.root, True, reverse_slots=True)
    differ = bits_differ(a, b)
    n = np.diff(sh.og.r_begin)
    kinds = {"lane": n < small, "one step": (n >= small) & (n <= 64 * chunks), "several steps": n > 64 * chunks}
    count = {k: int((differ & m).sum()) for k, m in kinds.items()}
    print(count, "largest sigma %.3g" % float(a.max()))
    assert all(c >= 50 for c in count.values()), count
    probes = sh.probes["fw"]            # the laid-out rows too: their terms are inexact path counts
    print("probe rows that differ", int(differ[probes].sum()), "of", len(probes))
    assert int(differ[probes].sum()) >= len(probes) // 2
    assert float(a.max()) > 2.0 ** 36 and np.isfinite(a).all()


def test_overflow_has_nan_next_to_finite_values():
    sh = S.family("overflow")
    _, sigma, _ = S.seed_pass_f32(sh.og, sh.root, True)
    assert np.isinf(sigma).sum() >= 48 * 5 and int(sh.layer.max()) == 30 < 254     # the batched paths keep levels as bytes
    bc = po.bc(sh.og, S.seeds("overflow"), True)
    assert int(np.isnan(bc).sum()) >= 1000 and int((np.isfinite(bc) & (bc != 0)).sum()) >= 300


def test_small_is_cheap_for_every_source():
    """gmx_bc_all's input: inexact path counts from its root, small enough that the oracle sweeps every source."""
    sh = S.family("small")
    assert sh.V <= 1100
    _, a, _ = S.seed_pass_f32(sh.og, sh.root, True)
    _, b, _ = S.seed_pass_f32(sh.og, sh.root, True, reverse_slots=True)
    assert int(bits_differ(a, b).sum()) >= 100
