"""OSM ids resolved on the device (osmt_resolve_refs, osm_renderer_amd/csrc/osmt_resolve.hip): way and relation references
to local indices, the ways' references deduped.

Every array of every resolution — way_node_off, way_nodes, relation_way_off, relation_ways, relation_way_inner — and the five
counts are held byte for byte against the host twin osmt::resolve_refs_host (host/osmt_resolve.hpp through
tests/resolve_shim.cpp), which tests/test_resolve_cpu.py holds against the Python model of the importer's steps.  The worlds sit
at the sizes where a kernel takes another path: way lengths around a wave and around the bound W between the dedup's two
paths, each all-distinct and as a walk there and back; the same worlds again with the bound at 0 and at 2, so both paths see
every shape; reference totals and element counts at the edges of the scan (256) and of the sort (OSMT_PYR_SORT_BLOCK); runs of
one global id across sort blocks; ids that differ only in the key bytes the sort did not reach before."""
import ctypes as C
import threading

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _polygons as mp
from tests import _resolve as rs
from tests import _tileindexbuild as tib

pytestmark = pytest.mark.gpu

W, SORT_BLOCK = rs.SHORT_WAY_MAX, rs.SORT_BLOCK
LENGTHS = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1]

WORLDS = {f"row: {r[0]}": (lambda r=r: rs.table_world(r)) for r in rs.TABLE}
WORLDS["all rows"] = rs.table_world_all
for n in LENGTHS:  # one way of the length alone, and all of them in one world below
    WORLDS[f"way of {n} distinct"] = lambda n=n: rs.way_length_world([n], False)
    WORLDS[f"way of {n} there and back"] = lambda n=n: rs.way_length_world([n], True)
WORLDS["all lengths distinct"] = lambda: rs.way_length_world(LENGTHS, False)
WORLDS["all lengths there and back"] = lambda: rs.way_length_world(LENGTHS, True)
WORLDS["all lengths there and back, with misses"] = lambda: rs.way_length_world(LENGTHS, True, miss_every=3)
for k, n in enumerate((255, 256, 257, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1)):
    WORLDS[f"{n} node references"] = lambda k=k, n=n: rs.counted_world(10 + k, 90, 23, n, 3, 10)
    WORLDS[f"{n} way references"] = lambda k=k, n=n: rs.counted_world(20 + k, 30, 70, 100, 19, n, with_seen=True)
    WORLDS[f"{n} nodes"] = lambda k=k, n=n: rs.counted_world(30 + k, n, 11, 300, 2, 6, with_seen=k % 2 == 1)
    WORLDS[f"{n} ways"] = lambda k=k, n=n: rs.counted_world(40 + k, 50, n, 2 * n + 3, 7, 300)
    WORLDS[f"{n} relations"] = lambda k=k, n=n: rs.counted_world(50 + k, 20, 40, 60, n, n + 5, with_seen=k % 2 == 0)
for n in (1, 64, 65, SORT_BLOCK + 1):  # a run crosses sort blocks and the bisection's end
    WORLDS[f"run of {n}"] = lambda n=n: rs.run_world(n, False)
    WORLDS[f"run of {n} with seen"] = lambda n=n: rs.run_world(n, True)
WORLDS["ids that differ in key bytes 5..7"] = lambda: rs.key_byte_world([40, 48, 56])
WORLDS["ids that differ in key byte 7"] = lambda: rs.key_byte_world([56])
WORLDS["ids that differ in key byte 0"] = lambda: rs.key_byte_world([0])
WORLDS["nothing"] = lambda: rs.World([], [], [])
WORLDS["nodes only"] = lambda: rs.World([5, 6, 5], [], [])
WORLDS["every reference unresolved"] = lambda: rs.World([5, 6], [(1, [7, 8, 7]), (2, []), (3, [9])], [[(4, 0), (5, 1)], [], [(6, 0)]])
WORLDS["every reference unseen"] = lambda: rs.World([5, 6], [(1, [5, 6, 5]), (2, [6])], [[(1, 0), (2, 1)]], [0, 0], [0])
WORLDS["random 7"] = lambda: rs.counted_world(7, 300, 120, 2000, 40, 300, with_seen=True)
WORLDS["random 8"] = lambda: rs.counted_world(8, 40, 30, 3000, 10, 50)  # few nodes, long ways: pairs repeat

_twins = {}


def _world(name):
    """the world and its twin's arrays, made once"""
    if name not in _twins:
        w = WORLDS[name]()
        _twins[name] = (w, rs.twin(w))
    return _twins[name]


def _checks(name, got):
    if name.startswith("row: "):  # and the issue's table itself
        rs.same(got, rs.table_arrays(next(r for r in rs.TABLE if r[0] == name[5:])))
    if name.startswith("way of "):
        n = int(name.split()[2])
        kept = n if "distinct" in name else min(n, n // 2 + 1)
        assert got["counts"] == (kept, 1, 0, n - kept, 0)
    if name in ("nothing", "nodes only", "every reference unresolved", "every reference unseen"):
        assert got["counts"][:2] == (0, 0) and not got["way_node_off"].any() and not got["relation_way_off"].any()
        assert len(got["way_nodes"]) == len(got["relation_ways"]) == len(got["relation_way_inner"]) == 0
    if name == "random 7":  # every kind of outcome, in numbers
        c = got["counts"]
        assert c[0] > 100 and c[1] > 5 and c[2] > 100 and c[4] > 5, c
    if name == "random 8":
        assert got["counts"][3] > 100, got["counts"]


@pytest.mark.parametrize("name", list(WORLDS))
def test_resolution_equals_the_twin(gpu_ctx, name):
    w, want = _world(name)
    got = gpu_ctx.resolve_refs(w.r)
    rs.same(got, want)
    _checks(name, got)


@pytest.mark.parametrize("bound", [0, 2])
@pytest.mark.parametrize("name", list(WORLDS))
def test_the_short_way_bound_does_not_change_the_result(gpu_ctx, name, bound):
    w, want = _world(name)
    gpu_ctx.debug_resolve_short_way_max(bound)
    try:
        rs.same(gpu_ctx.resolve_refs(w.r), want)
    finally:
        gpu_ctx.debug_resolve_short_way_max(W)


def test_the_bound_at_its_cap_and_past_it(gpu_ctx):
    """every way of "all lengths" and one of 1024 and 1025 references in LDS at the cap; a bound above the cap is refused"""
    w = rs.way_length_world(LENGTHS + [1023, 1024, 1025], True, miss_every=7)
    want = rs.twin(w)
    gpu_ctx.debug_resolve_short_way_max(1024)
    try:
        rs.same(gpu_ctx.resolve_refs(w.r), want)
    finally:
        gpu_ctx.debug_resolve_short_way_max(W)
    rs.same(gpu_ctx.resolve_refs(w.r), want)
    with pytest.raises(OsmtError, match="short way bound 1025"):
        gpu_ctx.debug_resolve_short_way_max(1025)


def test_the_suite_runs_on_poisoned_memory(gpu_ctx):
    """tests/conftest.py sets OSMT_POISON_ALLOC=1 before the library loads: every buffer a resolution takes is filled with a
    pattern first, so a word read before it is written shows in the arrays.  Twice, so the second call takes the first one's
    buffers back from the cache."""
    assert lib.load().osmt_debug_poison_enabled() == 1
    w, want = _world("random 7")
    rs.same(gpu_ctx.resolve_refs(w.r), want)
    rs.same(gpu_ctx.resolve_refs(w.r), want)
    small, want_small = _world("all rows")
    rs.same(gpu_ctx.resolve_refs(small.r), want_small)


def test_two_resolutions_from_two_threads(gpu_ctx):
    worlds = [_world("random 7"), _world("random 8")]
    out, errs = [None, None], []

    def run(i):
        try:
            out[i] = [gpu_ctx.resolve_refs(worlds[i][0].r) for _ in range(3)]
        except Exception as e:  # noqa: BLE001 — reported below
            errs.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(2):
        for got in out[i]:
            rs.same(got, worlds[i][1])


def test_a_refused_call_then_a_good_one(gpu_ctx):
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]], [3, 4], [2])
    L, d, h = lib.load(), w.r.as_desc(), C.c_void_p()
    rc = L.osmt_resolve_refs(gpu_ctx._h, C.byref(d), C.byref(h))  # the C entry itself, without the binding's validate call
    assert rc == abi.INVALID_ARG and not h.value and "way_nodes_seen[1] = 4" in L.osmt_last_error().decode()
    with pytest.raises(OsmtError, match=r"way_nodes_seen\[1\] = 4") as e:
        gpu_ctx.resolve_refs(w.r)
    assert e.value.code == abi.INVALID_ARG
    good, want = _world("all rows")
    rs.same(gpu_ctx.resolve_refs(good.r), want)


# ---- the chain: raw elements -> resolved -> multipolygons -> geodata -> tile index -------------------------------------------
def _chain_world():
    """about 300 elements around (48.1, 11.5): rings cut into ways whose node references repeat and miss, relations that name
    ways by id (one id twice in the file, one id that is no way), nodes under duplicate ids"""
    rng = np.random.default_rng(5)
    pos, node_ids, ways, rels = [], [], [], []
    for r in range(16):
        members = []
        for k, role in enumerate((0, 1)):
            n = 5 + r % 4 + k
            c = np.array([48.1 + 0.002 * (r % 4), 11.5 + 0.003 * (r // 4)])
            ang = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
            first = len(node_ids)
            pos += (c + (0.0015 - 0.0007 * k) * np.stack([np.sin(ang), np.cos(ang)], axis=1) + rng.random((n, 2)) * 1e-5).tolist()
            node_ids += [100000 + 10 * (first + i) for i in range(n)]
            ring = node_ids[first:] + [node_ids[first]]
            cut = n // 2
            a, b = ring[: cut + 1], ring[cut:][::-1]
            if r % 3 == 0:
                a = a[:2] + [a[0], a[1]] + a[2:]  # a step back and again forth: the dedup takes both out
            if r % 4 == 1:
                b = b[:1] + [99] + b[1:]  # no node
            members += [(3000 + len(ways), role), (3001 + len(ways), role)]
            ways += [(3000 + len(ways), a), (3001 + len(ways), b)]
        if r == 2:
            members = members[:-1]  # an open inner ring: rejected
        if r == 5:
            members.insert(1, (2999, 0))  # no way
        rels.append(members)
    pos.append(pos[0]), node_ids.append(node_ids[3])  # a later node under an id in use: it wins, at another position
    return np.array(pos), rs.World(node_ids, ways, rels)


def _chain(ctx, pos, w, resolved):
    relations = styled.Relations.from_resolved(pos, w.r.relation_ids, resolved)
    polygons = ctx.assemble_multipolygons(relations)
    g = styled.Geodata.from_arrays(pos, w.r.way_ids, resolved["way_node_off"], resolved["way_nodes"], polygons)
    d = g.as_desc()
    assert lib.load().osmt_validate_geodata(C.byref(d)) == abi.OK, lib.load().osmt_last_error().decode()
    gid = ctx.register_geodata(g)
    ctx.register_node_mercator(gid, tib.mercator_factors(pos))
    ctx.build_tile_index(gid)
    ix = ctx.read_tile_index(gid)
    return polygons, tuple(ix[k].tobytes() for k in sorted(ix))


def test_the_chain_from_raw_elements_to_the_tile_index(gpu_ctx):
    from osm_renderer_amd.renderer import Context

    pos, w = _chain_world()
    assert 280 <= len(w.node_ids) + len(w.ways) + len(w.relations) <= 320
    got, want = gpu_ctx.resolve_refs(w.r), rs.model(w)
    rs.same(got, want)
    assert got["counts"][2] > 0 and got["counts"][3] > 0 and got["counts"][4] == 1
    sides = []
    for resolved in (got, want):
        ctx = Context(0)
        try:
            sides.append(_chain(ctx, pos, w, resolved))
        finally:
            ctx.close()
    (mine_p, mine_ix), (theirs_p, theirs_ix) = sides
    mp.same(mine_p, theirs_p)
    acc = mine_p["status"]["accepted"]
    assert acc.sum() >= 8 and (acc == 0).sum() >= 1 and len(mine_p["polygon_nodes"]) > 50
    assert mine_ix == theirs_ix and sum(len(b) for b in mine_ix) > 100
