"""Multipolygon rings assembled on the device (osmt_assemble_multipolygons, osm_renderer_amd/csrc/osmt_polygons.hip) from
relations' member ways.

Every array of every assembly — the five arrays osmt_geodata_desc takes, every relation's status with the two figures of the
importer's message, and the relation of every multipolygon — is held byte for byte against the host twin
osmt::assemble_multipolygons_host (host/osmt_polygons.hpp through tests/polygons_shim.cpp), which tests/test_polygons_cpu.py
holds against the Python restatement of find_polygons.rs.  The worlds sit at the sizes where the kernels take another path: a
vertex list as long as a wave and longer, rings of 120 and 960 segments and one more or less (the two LDS budgets of the walk
as it was first built; the walk that stayed reads device memory at every size), relation counts and segment totals at the edges
of the owner bisection, the scan and the sort."""
import ctypes as C
import threading

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _polygons as mp
from tests import _tileindexbuild as tib

pytestmark = pytest.mark.gpu

LDS, SMALL, SORT_BLOCK = 960, 120, 1024  # the LDS budgets the walk was measured with; OSMT_PYR_SORT_BLOCK (csrc/osmt_internal.h)


def _empties():
    """relations without way references, ways of 0 and 1 nodes, between two triangles"""
    t = mp.table_world(mp.TABLE[0])
    ways = t.ways + [[], [1], [2]]
    return mp.World(t.nodes, ways, [[], [(0, 0), (3, 0), (1, 0), (4, 1), (2, 0)], [], [(3, 0), (4, 0)], [(5, 1)], [(0, 1), (1, 1), (2, 1)], []])


WORLDS = {f"row: {r[0]}": (lambda r=r: mp.table_world(r)) for r in mp.TABLE}
WORLDS["all rows"] = lambda: mp.concat([mp.table_world(r) for r in mp.TABLE])
# a vertex list of 1, 63, 64, 65 and 130 entries: the ballot scan within a wave's width, at it and past it
WORLDS["star 1"] = lambda: mp.star_world(0, dangling=True)
WORLDS["star 63"] = lambda: mp.star_world(31, dangling=True)
WORLDS["star 64"] = lambda: mp.star_world(32)
WORLDS["star 65"] = lambda: mp.star_world(32, dangling=True)
WORLDS["star 130"] = lambda: mp.star_world(65)
WORLDS["star 130 shared by two relations"] = lambda: mp.star_world(65, relations=2)
WORLDS["star 65 shared by three relations"] = lambda: mp.star_world(32, relations=3, dangling=True)
for budget in (SMALL, LDS):  # one ring of exactly a budget, one segment below and above it
    for n in (budget - 1, budget, budget + 1):
        WORLDS[f"ring {n}"] = lambda n=n: mp.ring_world([n])
WORLDS["two rings in the large budget"] = lambda: mp.ring_world([LDS // 2, LDS // 2], roles=[0, 1])
WORLDS["two rings in the small budget"] = lambda: mp.ring_world([SMALL // 2, SMALL // 2])
WORLDS["two rings of the large budget each"] = lambda: mp.ring_world([LDS, LDS], way_len=7)
for n in (255, 256, 257, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1):  # relation counts; 3 n segments
    WORLDS[f"{n} relations"] = lambda n=n: mp.counted_world(n, 3 * n)
for s in (255, 256, 257, SORT_BLOCK // 2 - 1, SORT_BLOCK // 2, SORT_BLOCK // 2 + 1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1):  # 2 s pairs are sorted
    WORLDS[f"{s} segments"] = lambda s=s: mp.counted_world(s // 5, s)
WORLDS["empty relations and short ways"] = _empties
WORLDS["nothing"] = lambda: mp.World(np.zeros((0, 2)), [], [])
WORLDS["no relations"] = lambda: mp.World([(1.0, 2.0), (2.0, 3.0)], [[0, 1]], [])
WORLDS["random 11"] = lambda: mp.random_world(11, 300)
WORLDS["random 12"] = lambda: mp.random_world(12, 300)

_twins = {}


def _world(name):
    """the world and its twin's arrays, made once"""
    if name not in _twins:
        w = WORLDS[name]()
        _twins[name] = (w, mp.twin(w))
    return _twins[name]


@pytest.mark.parametrize("name", list(WORLDS))
def test_assembly_equals_the_twin(gpu_ctx, name):
    w, want = _world(name)
    got = gpu_ctx.assemble_multipolygons(w.r)
    mp.same(got, want)
    if name.startswith("row: "):  # and the issue's table itself
        mp.same(got, mp.table_arrays(next(r for r in mp.TABLE if r[0] == name[5:])))
    if name == "all rows":  # an accepted relation after a rejected one
        acc = got["status"]["accepted"].tolist()
        assert any(a == 0 and b == 1 for a, b in zip(acc, acc[1:]))
    if name.startswith("star") and "shared" not in name:
        n = int(name.split()[1])
        assert got["status"].tolist() == [(1 - n % 2, n // 2, n % 2)]
    if name.startswith("ring "):
        assert got["status"].tolist() == [(1, 1, 0)] and len(got["polygon_nodes"]) == int(name.split()[1]) + 1
    if name == "two rings of the large budget each":
        assert got["status"].tolist() == [(1, 2, 0)]
    if name == "empty relations and short ways":
        assert got["status"]["accepted"].tolist() == [1, 1, 1, 1, 1, 1, 1] and got["status"]["rings_built"].tolist() == [0, 1, 0, 0, 0, 1, 0]
    if name.startswith("random"):
        acc = got["status"]["accepted"]
        assert acc.sum() >= 150 and (acc == 0).sum() >= 30


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("name", list(WORLDS))
def test_the_vertex_hash_does_not_change_the_result(gpu_ctx, name, bits):
    w, want = _world(name)
    gpu_ctx.debug_vertex_hash_bits(bits)
    try:
        mp.same(gpu_ctx.assemble_multipolygons(w.r), want)
    finally:
        gpu_ctx.debug_vertex_hash_bits(32)


def test_hash_bits_above_32_are_refused(gpu_ctx):
    with pytest.raises(OsmtError, match="hash bits 33"):
        gpu_ctx.debug_vertex_hash_bits(33)


def test_positions_by_bits_on_the_device(gpu_ctx):
    nan_a = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    nan_b = np.array([0x7FF8000000000002], dtype=np.uint64).view(np.float64)[0]
    tri = lambda last: mp.World([(nan_a, 5.0), (1.0, 0.0), (2.0, 0.0), last], [[0, 1], [1, 2], [2, 3]], [[(0, 0), (1, 0), (2, 0)]])
    w = mp.concat([tri((nan_a, 5.0)), tri((nan_b, 5.0)), mp.World([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (-0.0, 0.0)], [[0, 1], [1, 2], [2, 3]], [[(0, 0), (1, 0), (2, 0)]])])
    got = gpu_ctx.assemble_multipolygons(w.r)
    mp.same(got, mp.twin(w))
    assert got["status"]["accepted"].tolist() == [1, 0, 0]


def test_two_assemblies_are_equal_also_from_two_threads(gpu_ctx):
    w, want = _world("random 11")
    a, b = gpu_ctx.assemble_multipolygons(w.r), gpu_ctx.assemble_multipolygons(w.r)
    mp.same(a, b)
    out, errs = [None, None], []

    def run(i):
        try:
            out[i] = gpu_ctx.assemble_multipolygons(w.r)
        except Exception as e:  # noqa: BLE001 — reported below
            errs.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    mp.same(out[0], want)
    mp.same(out[1], want)


def test_a_total_past_2_31_is_refused_with_the_figure(gpu_ctx):
    """a way of 2^16 + 1 nodes named 2^15 times: 2^31 segments, 400 KB to upload.  Refused before any pair buffer exists; the
    context then assembles as before"""
    n, refs = 2**16 + 1, 2**15
    r = styled.Relations(np.zeros((1, 2)), [], [])
    r.way_node_off, r.way_nodes = np.array([0, n], np.uint32), np.zeros(n, np.uint32)
    r.relation_ids, r.relation_way_off = np.array([1], np.uint64), np.array([0, refs], np.uint32)
    r.relation_ways, r.relation_way_inner = np.zeros(refs, np.uint32), np.zeros(refs, np.uint8)
    L, d, h = lib.load(), r.as_desc(), C.c_void_p()
    rc = L.osmt_assemble_multipolygons(gpu_ctx._h, C.byref(d), C.byref(h))  # the C entry itself, without the binding's validate call
    assert rc == abi.UNSUPPORTED and not h.value and str(2**31) in L.osmt_last_error().decode()
    with pytest.raises(OsmtError, match=str(2**31)) as e:
        gpu_ctx.assemble_multipolygons(r)
    assert e.value.code == abi.UNSUPPORTED
    w, want = _world("all rows")
    mp.same(gpu_ctx.assemble_multipolygons(w.r), want)


def test_invalid_relations_are_refused_by_the_call(gpu_ctx):
    w = mp.table_world(mp.TABLE[0])
    w.r.relation_way_inner[1] = 3
    with pytest.raises(OsmtError, match=r"relation_way_inner\[1\] = 3") as e:
        gpu_ctx.assemble_multipolygons(w.r)
    assert e.value.code == abi.INVALID_ARG


# ---- the chain: relations -> geodata -> factors -> tile index -> tiles ---------------------------------------------------------
def _chain_world():
    """rings of a few z18 tiles around (48.1, 11.5): two relations with an outer and an inner ring, one rejected, one plain way"""
    rng = np.random.default_rng(3)
    nodes, ways, rels = [], [], []
    for r in range(4):
        members = []
        for k, role in enumerate((0, 1)):
            n = 5 + r + k
            c = np.array([48.1 + 0.002 * r, 11.5 + 0.003 * r])
            ang = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
            ring = [len(nodes) + i for i in range(n)]
            nodes += (c + (0.0015 - 0.0007 * k) * np.stack([np.sin(ang), np.cos(ang)], axis=1) + rng.random((n, 2)) * 1e-5).tolist()
            ring.append(ring[0])
            cut = n // 2
            members += [(len(ways), role), (len(ways) + 1, role)]
            ways += [ring[: cut + 1], ring[cut:][::-1]]
        if r == 2:
            members = members[:-1]  # an open inner ring: rejected
        rels.append(members)
    return mp.World(nodes, ways, rels)


def _chain(ctx, w, polygons):
    """the rest of the chain over `polygons`; returns what a tile batch builds"""
    L = lib.load()
    g = styled.Geodata.from_arrays(w.nodes, 5000 + np.arange(len(w.ways)), w.r.way_node_off, w.r.way_nodes, polygons)
    d = g.as_desc()
    assert L.osmt_validate_geodata(C.byref(d)) == abi.OK, L.osmt_last_error().decode()
    gid = ctx.register_geodata(g)
    f = tib.mercator_factors(w.nodes)
    ctx.register_node_mercator(gid, f)
    ctx.build_tile_index(gid)
    st = np.zeros(2, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"] = 1, [(200, 30, 40), (20, 130, 240)]
    st["has_color"], st["color"], st["has_width"], st["width"] = 1, (1, 2, 3), 1, [1.5, 2.5]
    first = ctx.register_styles(st)
    n_mps = len(g.multipolygon_ids)
    bid = ctx.register_style_bindings(styled.StyleBindings(gid, 12, 18, [[first + 1]] * len(w.ways), [[first]] * n_mps))
    t18 = (f[0] * (1 << 18)).astype(np.int64)
    tiles = [(18, int(t18[0]), int(t18[1])), (16, int(t18[0]) >> 2, int(t18[1]) >> 2), (14, int(t18[0]) >> 4, int(t18[1]) >> 4)]
    scene = ctx.build_tiles(styled.TileBatch(gid, tiles, {z: bid for z in range(12, 19)}))
    try:
        t, a = scene.read_styled_areas()
        dl = scene.read_display_list()
        return t.tobytes(), a.tobytes(), dl.jobs.tobytes(), dl.ops.tobytes(), dl.rings.tobytes(), np.asarray(dl.coords).tobytes(), len(a)
    finally:
        scene.free()


def test_the_chain_from_relations_to_tiles(gpu_ctx):
    from osm_renderer_amd.renderer import Context

    w = _chain_world()
    got = gpu_ctx.assemble_multipolygons(w.r)
    want = mp.twin(w)
    mp.same(got, want)
    assert got["status"]["accepted"].tolist() == [1, 1, 0, 1] and got["multipolygon_relation"].tolist() == [0, 1, 3]
    # each side in a context of its own: the style ids a registration returns depend on what the context holds already
    sides = []
    for polygons in (got, want):
        ctx = Context(0)
        try:
            sides.append(_chain(ctx, w, polygons))
        finally:
            ctx.close()
    mine, theirs = sides
    assert mine[-1] > 3  # multipolygons and ways are drawn
    assert mine == theirs
