"""The z18 tile index built on the device (osmt_build_tile_index, osm_renderer_amd/csrc/osmt_tileindex.hip) from the registered
Mercator factors and the topology of a geodata file.

Every index is read back (osmt_read_tile_index) and held, array for array and byte for byte, against the host twin
osmt::tile_index_of (host/osmt_tilequery.hpp through tests/tile_index_build_shim.cpp), which tests/test_tile_index_build_cpu.py
holds against the Python restatement of saver.rs.  The worlds place their nodes by factors stated exactly: the factors are an
input of the build.  Scenes, labels and files over a built index are held against the same build over the same index registered
from the twin's arrays in a context of its own: where the index comes from changes nothing that comes out."""
import ctypes as C
import threading

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _idfilter as idf
from tests import _tileindexbuild as tib
from tests.test_gpu_area_labels import CANVAS, TEXTS
from tests.test_gpu_tile_pyramid import ALL, MIXED, Side, _town

pytestmark = pytest.mark.gpu

B, HI, WORLD = tib.B, tib.HI, tib.WORLD


def _build(ctx, w, node_ids=True):
    gid = ctx.register_geodata(w.g)
    ctx.register_node_mercator(gid, w.factors)
    ctx.build_tile_index(gid, w.node_gids if node_ids else None)
    return gid


def _check(ctx, w, node_ids=True):
    """builds the world's index, holds it against the twin; returns (geodata id, the index read back)"""
    gid = _build(ctx, w, node_ids)
    got = ctx.read_tile_index(gid)
    tib.same(got, tib.twin(w))
    return gid, got


def _tile(got, x, y):
    i = got["tile_xy"].tolist().index([x, y])
    return tuple(got[p][got[o][i] : got[o][i + 1]].tolist() for o, p in (("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes")))


# ---- shapes of entities, rectangles, tile edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tib.EDGE_WORLDS))
def test_edge_worlds_equal_the_twin(gpu_ctx, name):
    w = tib.EDGE_WORLDS[name]()
    gid, got = _check(gpu_ctx, w)
    if name == "nothing":  # an empty index, then an empty tile batch builds
        assert all(len(got[k]) == 0 for k in ("tile_xy", "ways", "mps", "nodes")) and got["way_off"].tolist() == [0]
        scene = gpu_ctx.build_tiles(styled.TileBatch(gid, [], {}))
        t, a = scene.read_styled_areas()
        assert len(t) == len(a) == 0
        scene.free()
    if name == "one node":
        assert got["tile_xy"].tolist() == [[HI, 0]] and got["nodes"].tolist() == [0]
    if name == "rectangles":
        X, Y = 5000, 7000
        assert _tile(got, X + 101, Y + 102) == ([4, 5], [0], [])  # inside the diagonal's rectangle: it exists, holds no node
        assert _tile(got, X + 200, Y) == ([], [], [6])  # a node and nothing else
        assert int((got["ways"] == 3).sum()) == 1600
    if name == "shapes":
        assert set(got["ways"].tolist()) == {2, 3, 6, 7} and set(got["mps"].tolist()) == {3, 4, 5, 6}
    if name == "edges":
        k = 77777
        assert _tile(got, k - 1, k)[2] == [1] and _tile(got, k, k - 1)[2] == [2] and _tile(got, HI, HI)[2] == [4] and _tile(got, 0, 0)[2] == [3]
        assert _tile(got, 0, HI)[2] == [5] and _tile(got, HI, 0)[2] == [6]


@pytest.mark.parametrize("seed", [11, 12])
def test_random_worlds_equal_the_twin(gpu_ctx, seed):
    w = tib.random_world(seed, n_nodes=3000, n_ways=900, n_polys=300, n_mps=150)
    _, got = _check(gpu_ctx, w, node_ids=bool(seed % 2))
    assert len(got["tile_xy"]) > 300 and len(got["ways"]) > 3000 and len(got["mps"]) > 300


@pytest.mark.parametrize("bad, node, axis", [((1.0, 0.5), 1, "x"), ((0.5, 1.0), 1, "y"), ((1.0, 1.0), 1, "x")])
def test_a_factor_of_one_is_refused_and_names_the_lowest_node(gpu_ctx, bad, node, axis):
    L = lib.load()
    f = np.array([(0.25, 0.25), bad, (1.0, 0.1), (0.3, 1.0)] + [(0.5, 0.5)] * 300)  # two more offenders behind the first
    w = tib.World(f, [[0, 1], [2, 3]])
    gid = gpu_ctx.register_geodata(w.g)
    gpu_ctx.register_node_mercator(gid, w.factors)
    with pytest.raises(OsmtError, match=f"node {node}: {axis} factor is exactly 1.0") as e:
        gpu_ctx.build_tile_index(gid, w.node_gids)
    assert e.value.code == abi.UNSUPPORTED
    # nothing is registered: no index to read, and the id may still be built for
    with pytest.raises(OsmtError, match="has no tile index"):
        gpu_ctx.read_tile_index(gid)
    assert L.osmt_validate_tile_index_build(gid, None, 0, gpu_ctx._h) == abi.OK
    # the same context builds the corrected file
    f[1], f[2], f[3] = (0.25 + 3.0 / WORLD, 0.25 + 2.0 / WORLD), (np.nextafter(1.0, 0.0), 0.1), (0.3, np.nextafter(1.0, 0.0))
    _check(gpu_ctx, tib.World(f, [[0, 1]]))


# ---- wave and workgroup edges of the per-reference kernels -------------------------------------------------------------------
def _block_world(rng, n_nodes, ways, polys=(), mps=(), side=6, at=(40000, 90000)):
    t = np.array(at) + rng.integers(0, side, (n_nodes, 2))
    return tib.World((t + rng.random((n_nodes, 2))) / WORLD, ways, polys, mps)


def test_entities_at_wave_edges(gpu_ctx):
    """entities of 63, 64, 65, 129 and 1025 references in a row: the second run starts at lane 63 of the first wave, the third at
    lane 63 of the second, the last crosses workgroups; once as ways, once as the polygons of multipolygons with empty
    entities in between"""
    rng = np.random.default_rng(5)
    sizes = (63, 64, 65, 129, 1025)
    lists = [rng.integers(0, 500, n).tolist() for n in sizes]
    polys = [lists[0], [], lists[1], lists[2], [], [], lists[3], lists[4]]
    w = _block_world(rng, 500, lists, polys, [[0, 1], [2], [], [3, 4, 5], [7, 6]])
    gid, got = _check(gpu_ctx, w)
    assert set(got["ways"].tolist()) == set(range(5)) and set(got["mps"].tolist()) == {0, 1, 3, 4}
    # every entity alone in the first lanes of a grid too
    for n in sizes:
        one = rng.integers(0, 500, n).tolist()
        _check(gpu_ctx, _block_world(rng, 500, [one], [one], [[0]]), node_ids=False)


def test_one_run_covers_whole_waves(gpu_ctx):
    """5000 references of one entity, all but two in one tile: the segmented reduction where a run fills 78 waves"""
    X, Y = 123456, 654 + 1000
    w = tib.World.at_tiles([(X, Y), (X + 2, Y + 1), (X - 1, Y + 3)], [[0] * 2499 + [1] + [0] * 2499 + [2], [0]], [[0] * 3000 + [2] + [0] * 1998 + [1], []], [[1, 0]])
    _, got = _check(gpu_ctx, w)
    assert int((got["ways"] == 0).sum()) == 4 * 4 and int((got["mps"] == 0).sum()) == 16 and int((got["ways"] == 1).sum()) == 1


def _rects(total, corner):
    """rectangles of `total` tiles in all: 512 x q and 1 x r, as node tiles [(a, b)] per rectangle"""
    q, r = divmod(total, 512)
    x, y = corner
    out = []
    if q:
        out.append([(x, y), (x + 511, y + q - 1)])
    if r:
        out.append([(x + 600, y), (x + 600, y + r - 1)])
    return out


@pytest.mark.parametrize("n_nodes, way_total, mp_total", [(B - 1, 1, B), (B, B + 1, B - 1), (B + 1, B - 1, 1), (256 * B + 1, B, B + 1), (8, 256 * B + 1, 256 * B + 1)])
def test_reference_totals_at_the_edges_of_a_workgroup_and_of_the_scan(gpu_ctx, n_nodes, way_total, mp_total):
    """node, way and multipolygon reference totals of 1, B - 1, B, B + 1 and 256 B + 1 (0: the worlds above): the scan over
    (digit, workgroup) counts then has 256 * 257 words, more than the 256 blocks one pass of the block-total scan takes"""
    rng = np.random.default_rng(n_nodes + way_total)
    tiles, ways, polys = [], [], []
    for total, into, corner in ((way_total, ways, (10000, 20000)), (mp_total, polys, (30000, 20000))):
        for rect in _rects(total, corner):
            into.append(list(range(len(tiles), len(tiles) + len(rect))))
            tiles += rect
    assert len(tiles) <= n_nodes
    fill = n_nodes - len(tiles)
    tiles += (np.array((50000, 50000)) + rng.integers(0, 30, (fill, 2))).tolist()
    w = tib.World.at_tiles(tiles, ways, polys, [[p] for p in range(len(polys))])
    _, got = _check(gpu_ctx, w)
    assert (len(got["nodes"]), len(got["ways"]), len(got["mps"])) == (n_nodes, way_total, mp_total)


# ---- limits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["way", "multipolygon"])
def test_a_rectangle_over_the_whole_world_is_refused_with_the_figure(gpu_ctx, kind):
    """a two-node entity from corner to corner of the world lists 2^36 tiles: refused from the 64-bit total, before any pair has
    a buffer — a pair buffer of 2^36 pairs would be 1.4 TB — and the context builds on"""
    corners = [(0, 0), (HI, HI), (5, 5)]
    w = tib.World.at_tiles(corners, [[0, 1]] if kind == "way" else [[2]], [[0], [1]], [] if kind == "way" else [[0, 1]])
    gid = gpu_ctx.register_geodata(w.g)
    gpu_ctx.register_node_mercator(gid, w.factors)
    with pytest.raises(OsmtError, match=f"{1 << 36} {kind} references") as e:
        gpu_ctx.build_tile_index(gid)
    assert e.value.code == abi.UNSUPPORTED
    with pytest.raises(OsmtError, match="has no tile index"):
        gpu_ctx.read_tile_index(gid)
    _check(gpu_ctx, tib.World.at_tiles(corners, [[0, 2]], [[2]], [[0]]))


# ---- registration ------------------------------------------------------------------------------------------------------------
def _index_of(arrays):
    n = len(arrays["tile_xy"])
    cut = lambda o, p, i: arrays[p][arrays[o][i] : arrays[o][i + 1]].tolist()
    tiles = [(tuple(arrays["tile_xy"][i].tolist()), cut("way_off", "ways", i), cut("mp_off", "mps", i)) for i in range(n)]
    return styled.TileIndex(tiles), [cut("node_off", "nodes", i) for i in range(n)]


def _register_twin(ctx, w, twin, nodes=True):
    gid = ctx.register_geodata(w.g)
    index, node_lists = _index_of(twin)
    ctx.register_tile_index(gid, index)
    if nodes:
        ctx.register_node_index(gid, styled.NodeIndex(w.node_gids, node_lists))
    return gid


def test_a_build_with_node_ids_leaves_what_the_two_registrations_leave(gpu_ctx):
    from osm_renderer_amd.renderer import Context

    w = tib.random_world(21)
    twin = tib.twin(w)
    built = _build(gpu_ctx, w)
    other = Context(0)
    try:
        reg = _register_twin(other, w, twin)
        tib.same(gpu_ctx.read_tile_index(built), other.read_tile_index(reg))
        # an osm_ids filter: the node plane comes from the global ids the build registered
        ids = np.concatenate([w.node_gids[::3], w.g.way_ids[::2], w.g.multipolygon_ids[1::2], np.array([7], np.uint64)])
        a, b = gpu_ctx.read_id_filter(gpu_ctx.register_id_filter(built, ids)), other.read_id_filter(other.register_id_filter(reg, ids))
        for pa, pb in zip(a, b):
            assert pa.tobytes() == pb.tobytes()
        assert len(a[2]) > 0 and a[2].any()
        # a registered index is read back in its registered order: lists as handed over, repeats and all
        loose = other.register_geodata(w.g)
        tiles = [((5, 9), [3, 1, 3], [2, 0]), ((5, 10), [], []), ((70, 1), [0], [1, 1])]
        other.register_tile_index(loose, styled.TileIndex(tiles))
        got = other.read_tile_index(loose)
        assert got["tile_xy"].tolist() == [[5, 9], [5, 10], [70, 1]] and got["ways"].tolist() == [3, 1, 3, 0] and got["mps"].tolist() == [2, 0, 1, 1]
        assert got["way_off"].tolist() == [0, 3, 3, 4] and len(got["nodes"]) == 0 and not got["node_off"].any()
    finally:
        other.close()


def test_without_node_ids_no_node_index_is_registered(gpu_ctx):
    w = tib.random_world(22)
    gid, got = _check(gpu_ctx, w, node_ids=False)
    assert len(got["nodes"]) == len(w.factors)  # the lists are built all the same
    flt = gpu_ctx.register_id_filter(gid, w.node_gids)
    assert len(gpu_ctx.read_id_filter(flt)[2]) == 0  # no node plane: no node index
    _, node_lists = _index_of(got)
    gpu_ctx.register_node_index(gid, styled.NodeIndex(w.node_gids, node_lists))  # from the lists read back
    tib.same(gpu_ctx.read_tile_index(gid), got)
    assert gpu_ctx.read_id_filter(gpu_ctx.register_id_filter(gid, w.node_gids[:40]))[2].any()
    with pytest.raises(OsmtError, match="node index already"):
        gpu_ctx.register_node_index(gid, styled.NodeIndex(w.node_gids, node_lists))


def test_refusals_of_the_validator_and_one_index_per_file(gpu_ctx):
    L, ctx = lib.load(), gpu_ctx
    w = tib.shapes_world()
    twin = tib.twin(w)
    ids = w.node_gids.ctypes.data_as(C.POINTER(C.c_uint64))

    def refused(gid, node_ids, n, *words):
        rc = L.osmt_validate_tile_index_build(gid, node_ids, n, ctx._h)
        msg = L.osmt_last_error().decode()
        assert rc == abi.INVALID_ARG and all(x in msg for x in words), (rc, msg)
        assert L.osmt_build_tile_index(ctx._h, gid, node_ids, n) == abi.INVALID_ARG

    refused(10**6, None, 0, "geodata id 1000000", "is not registered")
    bare = ctx.register_geodata(w.g)
    refused(bare, None, 0, f"geodata id {bare}", "no Mercator factors")
    ctx.register_node_mercator(bare, w.factors)
    refused(bare, ids, len(w.factors) - 1, f"n_nodes = {len(w.factors) - 1}", f"has {len(w.factors)} nodes")
    # built, then registered or built again
    ctx.build_tile_index(bare, w.node_gids)
    refused(bare, None, 0, "tile index already")
    with pytest.raises(OsmtError, match="tile index already"):
        ctx.register_tile_index(bare, _index_of(twin)[0])
    with pytest.raises(OsmtError, match="node index already"):
        ctx.register_node_index(bare, styled.NodeIndex(w.node_gids, _index_of(twin)[1]))
    tib.same(ctx.read_tile_index(bare), twin)
    # registered, then built
    reg = _register_twin(ctx, w, twin, nodes=False)
    ctx.register_node_mercator(reg, w.factors)
    refused(reg, None, 0, "tile index already")
    with pytest.raises(OsmtError, match="is not registered"):
        ctx.read_tile_index(10**6)
    # a capacity that is too small
    counts, caps = (C.c_size_t * 4)(), (C.c_size_t * 4)(0, 0, 0, 0)
    buf = np.zeros(4096, np.uint32)
    assert L.osmt_read_tile_index(ctx._h, bare, None, None, None, None, None, None, buf.ctypes.data, caps, counts) == abi.INVALID_ARG
    assert "caps[3]" in L.osmt_last_error().decode() and counts[3] == len(w.factors)


def test_two_threads_build_one_id(gpu_ctx):
    L = lib.load()
    w = tib.random_world(23, n_nodes=20000, n_ways=4000, n_polys=500, n_mps=200)
    gid = gpu_ctx.register_geodata(w.g)
    gpu_ctx.register_node_mercator(gid, w.factors)
    ids = w.node_gids.ctypes.data_as(C.POINTER(C.c_uint64))
    gate, rcs = threading.Barrier(2), [None, None]

    def run(k):
        gate.wait()
        rcs[k] = L.osmt_build_tile_index(gpu_ctx._h, gid, ids, len(w.node_gids))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert sorted(rcs) == sorted([abi.OK, abi.INVALID_ARG]), rcs
    tib.same(gpu_ctx.read_tile_index(gid), tib.twin(w))


def test_pyramid_levels_over_a_built_index_equal_those_over_the_registered_one(gpu_ctx):
    w = tib.random_world(24, n_nodes=2000, n_ways=600, n_polys=100, n_mps=60)
    built, reg = _build(gpu_ctx, w), _register_twin(gpu_ctx, w, tib.twin(w))
    mask = (1 << 18) | (1 << 12)
    for gid in (built, reg):
        gpu_ctx.register_tile_pyramid(gid, mask)
        assert gpu_ctx.tile_pyramid_levels(gid) == (mask, mask)
    for level in (18, 12):
        a, b = gpu_ctx.read_tile_pyramid(built, level), gpu_ctx.read_tile_pyramid(reg, level)
        tib.same(a, b)
        assert len(a["nodes"]) == len(w.factors) and len(a["ways"]) > 0
    assert len(gpu_ctx.read_tile_pyramid(built, 12)["tile_xy"]) < len(gpu_ctx.read_tile_pyramid(built, 18)["tile_xy"])


# ---- end to end --------------------------------------------------------------------------------------------------------------
NODE_GID0 = 7000  # the town's nodes have the global ids 7000 + index


def _hook(ctx, how, seen):
    """The town registers the index its file states, which is not the index of its geometry.  While the town is made, the
    context's registrations are answered with the index DERIVED from the factors the town registers: registered from the
    twin's arrays (how == 'registered'), or built on the device as soon as the factors are there (how == 'built')."""
    real = {n: getattr(ctx, n) for n in ("register_geodata", "register_tile_index", "register_node_mercator", "register_node_index")}

    def register_geodata(g):
        # everything the other three answers need, from the geodata alone: no answer depends on the order of the calls behind it
        seen["g"] = g
        seen["f"] = an.mercator_factors(g.nodes)  # what the town registers below: the equality is one of construction
        seen["twin"] = tib.twin_of(g, seen["f"])
        seen["gids"] = np.arange(len(seen["f"]), dtype=np.uint64) + np.uint64(NODE_GID0)
        return real["register_geodata"](g)

    def register_tile_index(gid, index):
        if how == "registered":
            real["register_tile_index"](gid, _index_of(seen["twin"])[0])

    def register_node_mercator(gid, f):
        assert np.ascontiguousarray(f).tobytes() == seen["f"].tobytes()
        real["register_node_mercator"](gid, f)
        if how == "built":
            ctx.build_tile_index(gid, seen["gids"])

    def register_node_index(gid, index):
        assert index.node_ids.tobytes() == seen["gids"].tobytes()
        if how == "registered":
            real["register_node_index"](gid, styled.NodeIndex(seen["gids"], _index_of(seen["twin"])[1]))

    for f in (register_geodata, register_tile_index, register_node_mercator, register_node_index):
        setattr(ctx, f.__name__, f)
    return lambda: [delattr(ctx, n) for n in real]


class DerivedSide(Side):
    """a Side of tests/test_gpu_tile_pyramid.py whose tile index and node index are those of the town's geometry"""

    def __init__(self, path, how, mask):
        from osm_renderer_amd.renderer import Context

        self.ctx, self.seen = Context(0), {}
        unhook = _hook(self.ctx, how, self.seen)
        self.W = _town(self.ctx, path / "town.bin")
        self.feed = idf.Feed(self.ctx, self.W, path / "town_nodes.bin", TEXTS, CANVAS)
        unhook()
        if mask is not None:
            self.ctx.register_tile_pyramid(self.W.gid, mask)
        self.flt = self.ctx.register_id_filter(self.W.gid, idf.half_of_the_ids(self.feed, seed=13))
        self.binds = ({z: self.W.all[0] for z in range(19)}, {z: self.feed.node_bind for z in range(19)})
        kw = dict(area_label_bindings=self.binds[0], node_label_bindings=self.binds[1], canvas=CANVAS)
        self.server = self.ctx.tile_server(self.W.gid, {z: self.feed.draw for z in range(19)}, **kw)
        self.filtered = self.ctx.tile_server(self.W.gid, {z: self.feed.draw for z in range(19)}, id_filter=self.flt, **kw)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    made = {}
    for name, how, mask in (("registered", "registered", None), ("built", "built", None), ("built + pyramid", "built", ALL)):
        made[name] = DerivedSide(tmp_path_factory.mktemp("tix_" + name.replace(" + ", "_")), how, mask)
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("filtered", [False, True])
def test_a_mixed_zoom_batch_is_the_same_bytes(sides, filtered):
    """display list, styled areas, node and area label batches, declined anchors, the scene's PNG files and the tile server's:
    the same bytes over the registered index, the built one, and the built one with all pyramid levels"""
    want, area0, node0, sizes = sides["registered"].everything(MIXED, filtered)
    assert sizes[0] > 20 and sizes[1] > 20 and sizes[2] > 20 and len(want["files"]) == len(MIXED)
    for name in ("built", "built + pyramid"):
        got, area1, node1, _ = sides[name].everything(MIXED, filtered)
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key] == want[key], (name, key)
        if name == "built":
            assert (area1, node1) == (area0, node0)  # the same index: the same candidates gathered
        else:
            assert area1[1] < area0[1] and area1[0] < area0[0] and node1[0] < node0[0] and node1[3] <= node0[3]  # the levels were read
    s = sides["built + pyramid"]
    assert s.ctx.tile_pyramid_levels(s.W.gid) == (ALL, ALL)  # node lists: the build registered the node index
    tib.same(sides["built"].ctx.read_tile_index(sides["built"].W.gid), sides["registered"].ctx.read_tile_index(sides["registered"].W.gid))


@pytest.mark.parametrize("filtered", [False, True])
def test_one_request_through_the_worker(sides, filtered):
    """osmt_worker_render_tile_png's files, through the plain server and through the one with the osm_ids filter"""
    files = {}
    for name, s in sides.items():
        wk = s.ctx.worker()
        files[name] = [wk.render_tile_png(s.filtered if filtered else s.server, t) for t in (MIXED[0], MIXED[2])]
        wk.close()
    assert files["built"] == files["registered"] == files["built + pyramid"] and len(set(files["registered"])) == 2
    if filtered:  # not vacuous: the filter changes the files
        wk = sides["registered"].ctx.worker()
        assert [wk.render_tile_png(sides["registered"].server, t) for t in (MIXED[0], MIXED[2])] != files["registered"]
        wk.close()
