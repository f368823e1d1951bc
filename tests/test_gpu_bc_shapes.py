"""comp_BC on the device on the designed graphs of bc_shapes.py: path counts far beyond 2^24, so the forward visit's sums
round differently in any other slot order; path counts that overflow, so NaN terms go through the ordered adds; and rows
on both sides of every form boundary of the per-seed visit kernels (test_bc_shapes_host.py asserts all of that on the
CPU).  gmx_bc against the oracle's bits; gmx_bc_batch and gmx_bc_all against the oracle's bits and gmx_bc's bytes for
every width, both row-length regimes forced, and both ways of getting a batch's levels."""
import contextlib
import functools
import os

import numpy as np
import pytest

import bc_shapes as S
import pyoracle as po
from test_bc_random_host import same_f32
from test_gpu_bc_all import traced as traced_all
from test_gpu_bc_batch import HUGE, bytes_equal, traced

pytestmark = pytest.mark.gpu
WIDTHS = (16, 32, 64, 0)


@pytest.fixture(scope="module")
def gmx():
    import gmx as m
    m.require_device()
    return m


@pytest.fixture(scope="module")
def dev(gmx):
    """family -> its graph on the device, both CSRs uploaded verbatim, once."""
    cache = {}

    def get(name):
        if name not in cache:
            og = S.family(name).og
            g = gmx.Graph.upload(og.begin, og.node_idx, og.r_begin, og.r_node_idx)
            for held, sent in zip(g.download(), (og.begin, og.node_idx, og.r_begin, og.r_node_idx)):
                assert np.array_equal(held, sent)               # the slot order under test is the one the oracle walks
            cache[name] = g
        return cache[name]
    yield get
    for g in cache.values():
        g.free()


@functools.lru_cache(maxsize=None)
def oracle(name, which, skip):
    sh = S.family(name)
    seeds = {"few": S.seeds, "70": S.seeds70, "all": lambda _: np.arange(sh.V, dtype=np.int32)}[which](name)
    out = po.bc(sh.og, seeds, skip)
    out.setflags(write=False)
    return out


@contextlib.contextmanager
def msbfs(value):
    """GMX_BCB_MSBFS for the calls inside (read at every call); restored afterwards."""
    old = os.environ.get("GMX_BCB_MSBFS")
    os.environ["GMX_BCB_MSBFS"] = value
    try:
        yield
    finally:
        os.environ.pop("GMX_BCB_MSBFS", None)
        if old is not None:
            os.environ["GMX_BCB_MSBFS"] = old


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", S.FAMILIES)
def test_bc_per_seed(dev, name, skip):
    """gmx_bc: the oracle's bits for the seeds of the host test, all of them and one at a time; the reached count; the
    levels from the root are the layers."""
    sh, g, seeds = S.family(name), dev(name), S.seeds(name)
    got, st = g.bc(seeds, skip)
    assert same_f32(got, oracle(name, "few", skip))
    reached = [int((po.bfs_queue(sh.og, int(s)) != S.INT_MAX).sum()) for s in seeds]
    assert st["vertices_reached"] == sum(reached) and st["iterations"] == len(seeds)
    for s in seeds[[0, 2, 4]]:           # a seed alone: nothing a later seed adds can cover a wrong sum
        one = np.array([s], np.int32)
        assert same_f32(g.bc(one, skip)[0], po.bc(sh.og, one, skip)), int(s)
    lv, n = g.bfs_levels(sh.root)
    assert np.array_equal(lv, sh.layer.astype(np.int16)) and n == int(sh.layer.max()) + 1
    if skip and name == "overflow":
        assert np.isnan(got).sum() >= 1000 and int((np.isfinite(got) & (got != 0)).sum()) >= 300


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", ["inexact", "sparse", "overflow"])
def test_bc_batch(dev, capfd, name, skip):
    """gmx_bc_batch, 70 seeds (a partial last batch at every width): the oracle's bits and gmx_bc's bytes and reached count
    for widths 16 / 32 / 64 / 0, the default row regimes, every row by a workgroup and every row by a lane group, the
    levels from one traversal per seed and from the multi-source traversal; the batched path ran every time."""
    g, seeds = dev(name), S.seeds70(name)
    want = oracle(name, "70", skip)
    ref, ref_st = g.bc(seeds, skip)
    assert same_f32(ref, want)
    for ms in ("0", "1"):
        for kw in ({}, {"GMX_BCB_LONG_MIN": "1"}, {"GMX_BCB_LONG_MIN": HUGE}):
            for width in WIDTHS:
                with msbfs(ms):
                    got, st, tr = traced(capfd, g, seeds, skip, width, **kw)
                where = (ms, kw, width)
                assert bytes_equal(got, ref) and same_f32(got, want), where
                assert st["vertices_reached"] == ref_st["vertices_reached"] and st["iterations"] == len(seeds), where
                assert tr and all(t["path"] == "batched" for t in tr) and sum(t["seeds"] for t in tr) == len(seeds), (where, tr)
                if width:
                    assert [t["seeds"] for t in tr] == [width] * (len(seeds) // width) + [len(seeds) % width], (where, tr)
                if kw:
                    forced = "long" if kw["GMX_BCB_LONG_MIN"] == "1" else "short"
                    idle = "short" if forced == "long" else "long"
                    assert all(t[forced] > 0 and t[idle] == 0 for t in tr), (where, tr)
                elif name != "overflow":     # (no row of `overflow` reaches the default GMX_BCB_LONG_MIN)
                    assert all(t["short"] > 0 and t["long"] > 0 for t in tr), (where, tr)


@pytest.mark.parametrize("skip", [False, True])
def test_bc_all(dev, capfd, skip):
    """gmx_bc_all on `small`, every vertex a source: the oracle's bits and the bytes of gmx_bc over arange(V)."""
    sh, g = S.family("small"), dev("small")
    want = oracle("small", "all", skip)
    ref, ref_st = g.bc(np.arange(sh.V, dtype=np.int32), skip)
    assert same_f32(ref, want)
    for ms in ("0", "1"):
        for width in (16, 64, 0):
            got, st, tr = traced_all(capfd, lambda: g.bc_all(skip, width), GMX_BCB_MSBFS=ms)
            assert bytes_equal(got, ref) and same_f32(got, want), (ms, width)
            assert st["vertices_reached"] == ref_st["vertices_reached"] and st["iterations"] == sh.V
            assert tr and all(t["path"] == "batched" and (t["ms_batch"] is not None) == (ms == "1") for t in tr), (ms, width, tr[:2])
