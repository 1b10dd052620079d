"""The import chain on the device at the counts and table ends the small worlds of tests/test_gpu_resolve.py and
tests/test_gpu_polygons.py do not reach (osmt_resolve_refs: csrc/osmt_resolve.hip; osmt_assemble_multipolygons:
csrc/osmt_polygons.hip).

  * probes that cross the end of a table: the vertex table of k_mpa_vertices / k_mpa_canon, and the LDS pair table of
    k_res_short, also where the table fills the launch's LDS (slots == slots_cap: the last key slot adjoins tpos);
  * 65 535, 65 536 and 65 537 ways or relations: k_res_short, k_mpa_walk and k_mpa_emit go from a 1-D grid to a 2-D one, the
    emit one relation earlier than the walk; a node id table of 257 sort blocks, and the long sort's own buffers past 256;
  * relations but no segment.

Every array and count is held byte for byte against the host twins (tests/_resolve.py: twin, tests/_polygons.py: twin), on the
poisoned allocator tests/conftest.py switches on.  The worlds come from tests/_probe_slots.py; that they cross, and how many
owners they have, is counted on the CPU with the kernels' own slot arithmetic (csrc/osmt_probe_slots.h) and asserted in
tests/test_probe_slots_cpu.py — the guards are repeated here where they are cheap, so a world that stopped crossing fails
beside the comparison it was built for."""
import time

import numpy as np
import pytest

from osm_renderer_amd import lib
from tests import _polygons as mp
from tests import _probe_slots as ps
from tests import _resolve as rs

pytestmark = pytest.mark.gpu

W = rs.SHORT_WAY_MAX
COUNTS = [ps.OWNERS - 1, ps.OWNERS, ps.OWNERS + 1]


def _timed(what, call):
    t = time.perf_counter()
    got = call()
    print(f"{what}: device call {time.perf_counter() - t:.3f} s")
    return got


def _resolve_under(ctx, bound, world):
    if bound == W:
        return ctx.resolve_refs(world.r)
    ctx.debug_resolve_short_way_max(bound)
    try:
        return ctx.resolve_refs(world.r)
    finally:
        ctx.debug_resolve_short_way_max(W)


def test_these_tests_run_on_poisoned_memory():
    assert lib.load().osmt_debug_poison_enabled() == 1


# ---- wrapping probes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.RING_WORLDS))
def test_vertex_probes_that_cross_the_tables_end(gpu_ctx, name):
    build, slots, rings = ps.RING_WORLDS[name]
    w = build()
    crossings, _, got_slots, _ = ps.crossings_vertices(w.r)
    assert got_slots == slots and crossings >= ps.RING_MIN_CROSSINGS
    want = mp.twin(w)
    got = _timed(f"{name} ({crossings} crossing steps in {slots} slots)", lambda: gpu_ctx.assemble_multipolygons(w.r))
    mp.same(got, want)
    assert got["status"].tolist() == [(1, rings, 0)] * len(w.relations)
    assert [len(p) for p in mp.polygons_of(got)] == [rings] * len(w.relations)


@pytest.mark.parametrize("bound", [W, ps.PATH_BOUND, 0])
def test_pair_probes_that_cross_the_tables_end(gpu_ctx, bound):
    """at the default bound the ways of 8 .. 256 references dedup in LDS, the way of 256 in a table of slots_cap slots, and
    the way of 1024 goes through the sort; at 1024 all five are in LDS and the longest fills it; at 0 the sort does them all"""
    w, want, _ = ps.made("path")
    n, per_way = ps.crossings_pairs(w.resolved_off, w.resolved_refs, short_max=ps.PATH_BOUND)
    assert n == len(ps.PATH_LENGTHS) and (per_way[:, 1] >= ps.PATH_MIN_CHAIN).all()
    got = _timed(f"paths under bound {bound}", lambda: _resolve_under(gpu_ctx, bound, w))
    rs.same(got, want)
    assert np.diff(got["way_node_off"]).tolist() == w.kept


# ---- many owners -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ways", COUNTS)
def test_many_ways(gpu_ctx, n_ways):
    w, want, seconds = ps.made("ways", n_ways)
    assert len(w.r.way_ids) == n_ways and -(-len(w.r.node_ids) // rs.SORT_BLOCK) == 257
    got = _timed(f"{n_ways} ways (twin {seconds:.2f} s)", lambda: gpu_ctx.resolve_refs(w.r))
    rs.same(got, want)
    assert got["counts"][1] == w.members


def test_many_ways_through_the_sort(gpu_ctx):
    """bound 0: every pair of the 65 537 ways goes through the long sort, whose own buffers then hold more than 256 sort blocks"""
    w, want, seconds = ps.made("ways", ps.OWNERS + 1)
    pairs = int(np.maximum(np.diff(w.resolved_off.astype(np.int64)) - 1, 0).sum())
    assert pairs > 256 * rs.SORT_BLOCK
    got = _timed(f"{ps.OWNERS + 1} ways under bound 0, {pairs} pairs (twin {seconds:.2f} s)", lambda: _resolve_under(gpu_ctx, 0, w))
    rs.same(got, want)


@pytest.mark.parametrize("n_rels", COUNTS)
def test_many_relations(gpu_ctx, n_rels):
    """at 65 536 the walk's grid is still 1-D and the emit's, one block longer, is 2-D"""
    w, want, seconds = ps.made("relations", n_rels)
    st = want["status"]
    assert len(st) == n_rels and (st["accepted"] == 1).sum() >= 2000 and (st["accepted"] == 0).sum() >= 2000
    assert st[-1]["accepted"] == 1 and st[-1]["rings_built"] >= 1
    got = _timed(f"{n_rels} relations (twin {seconds:.2f} s)", lambda: gpu_ctx.assemble_multipolygons(w.r))
    mp.same(got, want)
    assert got["multipolygon_relation"][-1] == n_rels - 1


# ---- no segments -------------------------------------------------------------------------------------------------------------
def test_relations_without_a_segment_then_an_ordinary_world(gpu_ctx):
    w = ps.no_segments_world()
    got = gpu_ctx.assemble_multipolygons(w.r)
    mp.same(got, mp.twin(w))
    assert got["status"].tolist() == [(1, 0, 0)] * 3 and got["multipolygon_relation"].tolist() == [0, 1, 2]
    assert len(got["multipolygon_ids"]) == 3 and len(got["polygon_node_off"]) == 1 and len(got["polygon_nodes"]) == 0
    assert not got["multipolygon_polygon_off"].any()
    after = mp.random_world(12, 60)
    mp.same(gpu_ctx.assemble_multipolygons(after.r), mp.twin(after))
