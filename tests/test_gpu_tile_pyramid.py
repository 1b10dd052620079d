"""The tile index pyramid (osmt_register_tile_pyramid, osm_renderer_amd/csrc/osmt_tilepyramid.hip): coarser levels of a
registered z18 tile index, built on the device, and the tile query reading the smallest registered level >= a tile's zoom.

The levels are held, array for array and byte for byte, against the host twin osmt::tile_pyramid_level
(host/osmt_tilequery.hpp, through tests/tile_pyramid_shim.cpp), which tests/test_tile_pyramid_cpu.py holds against the
definition.  Scenes, labels and files built with a pyramid are held against the same build without one in a second context
over the same file: the pyramid changes what is gathered, never what comes out.  Two builds that the z18 index refuses for
their candidate count are held against the mirror of the tile query."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _arealabels as al
from tests import _idfilter as idf
from tests import _tilelabels as tl
from tests import _tilepyramid as tp
from tests import _tilequery as tq
from tests._styled_feed import fill_only_styles, geodata_of, recs_of
from tests.test_gpu_area_labels import CANVAS, ICONS, NS, TEXTS, TX, TY, World, Z
from tests.test_tile_pyramid_cpu import HI, INDICES, corner_tiles, sparse_tiles

pytestmark = pytest.mark.gpu

ALL = abi.PYRAMID_ALL_LEVELS
B = 1024  # pairs one workgroup of the sort takes (OSMT_PYR_SORT_BLOCK)
CX, CY = tq.center_z18()
N_WAYS, MP_POLYGONS = 70000, (1, 1, 1, 1, 1, 3)


def _mask(levels):
    return sum(1 << lv for lv in levels)


@pytest.fixture(scope="module")
def base(gpu_ctx, tmp_path_factory):
    """one file of 70 000 ways, 6 multipolygons and 34 nodes: registered once per index below (the index is not the file's)"""
    r, _ = tq.make_world(str(tmp_path_factory.mktemp("pyr") / "base.bin"), N_WAYS, MP_POLYGONS, tile_refs={(CX, CY): ([], [0], [0])}, shared_nodes=True)
    g = geodata_of(r)
    gids = np.array([r.global_id(0, i) for i in range(r.n_nodes)], dtype=np.uint64)
    yield gpu_ctx, g, gids, r
    r.close()


def _register(base, tiles, nodes="before"):
    """a new geodata id with `tiles` ([((x, y), ways, mps, nodes)]) as its index; the node index before the pyramid, after it or never.
    Returns (gid, index, node lists, register-the-node-index-now)"""
    ctx, g, gids, _ = base
    index, node_lists = tp.index_of(tiles)
    gid = ctx.register_geodata(g)
    ctx.register_tile_index(gid, index)
    late = lambda: ctx.register_node_index(gid, styled.NodeIndex(gids, node_lists))
    if nodes == "before":
        late()
    return gid, index, node_lists, late


def _check_levels(base, tiles, levels, nodes="before"):
    ctx = base[0]
    gid, index, node_lists, _ = _register(base, tiles, nodes)
    assert ctx.tile_pyramid_levels(gid) == (0, 0)
    ctx.register_tile_pyramid(gid, _mask(levels))
    assert ctx.tile_pyramid_levels(gid) == (_mask(levels), _mask(levels) if nodes == "before" else 0)
    for lv in levels:
        tp.same_level(ctx.read_tile_pyramid(gid, lv), tp.twin_level(index, lv, node_lists if nodes == "before" else None))
    return gid


# ---- levels read back -------------------------------------------------------------------------------------------------
def _random_tiles(rng, n=200):
    """about 200 tiles in a few clusters, lists in any order with repeats, some empty"""
    tiles = {}
    while len(tiles) < n:
        cx, cy = [(CX, CY), (CX + 300, CY - 40), (1000, 200000), (HI - 30, HI - 30)][int(rng.integers(0, 4))]
        x, y = min(HI, cx + int(rng.integers(-12, 13))), min(HI, cy + int(rng.integers(-12, 13)))
        w = rng.integers(0, N_WAYS, int(rng.integers(0, 9))).tolist()
        tiles[(x, y)] = (w + w[:2], rng.integers(0, 6, int(rng.integers(0, 3))).tolist(), rng.integers(0, 34, int(rng.integers(0, 4))).tolist())
    return [(k, *tiles[k]) for k in sorted(tiles)]


def test_every_level_equals_the_twin(base):
    tiles = _random_tiles(np.random.default_rng(201))
    gid = _check_levels(base, tiles, range(19))
    ctx = base[0]
    top = ctx.read_tile_pyramid(gid, 0)
    assert top["tile_xy"].tolist() == [[0, 0]] and len(top["ways"]) == len({w for _, ws, _, _ in tiles for w in ws}) and len(top["nodes"]) > 20
    assert len(ctx.read_tile_pyramid(gid, 18)["tile_xy"]) == len(tiles)
    # a level that was not registered, a capacity that is too small
    other = _check_levels(base, [t for t in tiles if t[1]][:5], (3,))  # five tiles of the first cluster: one tile at level 3, with ways
    with pytest.raises(OsmtError, match="no level 4"):
        ctx.read_tile_pyramid(other, 4)
    L, counts, caps = lib.load(), (C.c_size_t * 4)(), (C.c_size_t * 4)(0, 0, 0, 0)
    buf = np.zeros(64, np.uint32)
    assert L.osmt_read_tile_pyramid(ctx._h, other, 3, None, None, buf.ctypes.data, None, None, None, None, caps, counts) == abi.INVALID_ARG
    assert "caps[1]" in L.osmt_last_error().decode() and counts[0] == 1


def test_a_sparse_mask_builds_each_level_from_the_one_above(base):
    _check_levels(base, _random_tiles(np.random.default_rng(202)), (18, 12, 8))  # 12 from 18, 8 from 12
    _check_levels(base, sparse_tiles(np.random.default_rng(203)), (17, 9, 1, 0))  # 17 from the registered index


@pytest.mark.parametrize("name", ["corners", "no tile", "one tile", "one empty tile"])
def test_corner_and_tiny_indices(base, name):
    tiles = INDICES[name](np.random.default_rng(len(name)))
    gid = _check_levels(base, tiles, range(19))
    n = [len(base[0].read_tile_pyramid(gid, lv)["tile_xy"]) for lv in range(19)]
    if name == "no tile":
        assert n == [0] * 19
    elif name.startswith("one"):
        assert n == [1] * 19
    else:
        assert n[0] == 1 and n[1] == 4 and n[18] == len(tiles)


def test_node_lists_exist_iff_the_node_index_came_first(base):
    ctx = base[0]
    tiles = corner_tiles(np.random.default_rng(5))
    before = _check_levels(base, tiles, (18, 10), nodes="before")
    assert len(ctx.read_tile_pyramid(before, 10)["nodes"]) > 0
    gid, index, node_lists, late = _register(base, tiles, nodes="after")
    ctx.register_tile_pyramid(gid, _mask((18, 10)))
    late()
    assert ctx.tile_pyramid_levels(gid) == (_mask((18, 10)), 0)
    got = ctx.read_tile_pyramid(gid, 10)
    tp.same_level(got, tp.twin_level(index, 10, None))
    assert len(got["nodes"]) == 0 and not got["node_off"].any()


# ---- the sort at its edges ----------------------------------------------------------------------------------------------
def _spread(rng, total, n_ids, per_tile=37, x0=CX - 2000):
    """`total` references over tiles of at most per_tile, ids below n_ids with repeats: [lists]"""
    out, left = [], total
    while left:
        k = min(left, int(rng.integers(1, per_tile + 1)))
        out.append(rng.integers(0, n_ids, k).tolist())
        left -= k
    return out


@pytest.mark.parametrize("totals", [(0, 1, B - 1), (B, B + 1, 2 * B + 1), (256 * B + 1, 0, 3)], ids=lambda t: "-".join(map(str, t)))
def test_reference_totals_at_the_edges_of_a_workgroup_and_of_the_scan(base, totals):
    """way, multipolygon and node totals of 0, 1, B - 1, B, B + 1, 2 B + 1, and 256 B + 1: the scan over (digit, workgroup) counts
    then has 256 * 257 words, more than the 256 blocks one pass of the block-total scan takes"""
    rng = np.random.default_rng(sum(totals))
    lists = [_spread(rng, totals[0], N_WAYS), _spread(rng, totals[1], 6), _spread(rng, totals[2], 34)]
    n = max(len(v) for v in lists) + 3
    coords = sorted({(CX - 3000 + int(rng.integers(0, 700)), CY + int(rng.integers(0, 700))) for _ in range(2 * n)})[:n]
    assert len(coords) == n
    order = [rng.permutation(n) for _ in lists]
    tiles = [[k, [], [], []] for k in coords]
    for kind, (v, o) in enumerate(zip(lists, order)):
        for j, ids in enumerate(v):
            tiles[int(o[j])][1 + kind] = ids
    tiles = [tuple(t) for t in tiles]
    assert tuple(sum(len(t[1 + k]) for t in tiles) for k in range(3)) == totals
    _check_levels(base, tiles, (18, 14, 0))


def test_ids_and_keys_at_the_edges_of_their_digits(base):
    n = N_WAYS
    edge_ids = [0, 255, 256, 65535, 65536, n - 1]
    descending = list(range(3000, -1, -1))  # all pairs distinct, handed over in descending order
    tiles = [((0, 5), edge_ids[::-1] + edge_ids, [5, 0, 5], [33, 0]),
             ((1 << 17, 5), [n - 1, 0, 65536], [0], [1]),  # its key differs from (0, 5)'s in the key's highest used bit only
             ((HI, HI), descending, [], []),
             ((CX, CY), [256] * 3000, [3] * (B + 1), [7] * 5)]  # all pairs equal
    gid = _check_levels(base, tiles, (18, 17, 1, 0))
    l18 = base[0].read_tile_pyramid(gid, 18)
    assert l18["ways"][: l18["way_off"][1]].tolist() == edge_ids and l18["tile_xy"].tolist() == [[0, 5], [1 << 17, 5], [CX, CY], [HI, HI]]
    assert l18["ways"][l18["way_off"][2] : l18["way_off"][3]].tolist() == [256]
    # one tile, one distinct pair: no digit differs, no pass runs
    _check_levels(base, [((CX, CY), [9] * (2 * B + 1), [], [])], (18, 0))
    _check_levels(base, [((HI, HI), descending, [], [])], (18, 9))


# ---- what the feature is for ----------------------------------------------------------------------------------------------
class Draw:
    """fill styles and a bindings table for a geodata id of `base`, and the mirror over a file that lists `file_refs`"""

    def __init__(self, base, path, file_refs, n_ways=700):
        ctx = base[0]
        rng = np.random.default_rng(7)
        st, pool = fill_only_styles(rng, 8)
        self.first = ctx.register_styles(recs_of(st), pool)
        self.ws = [[self.first + int(rng.integers(0, 8))] if i < n_ways else [] for i in range(N_WAYS)]
        self.ms = [[self.first + 3] for _ in MP_POLYGONS]
        self.r, _ = tq.make_world(str(path), N_WAYS, MP_POLYGONS, tile_refs=file_refs, shared_nodes=True)
        self.mir = tq.Mirror(self.r, self.ws, self.ms)

    def bind(self, ctx, gid):
        return ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, self.ws, self.ms))

    def close(self):
        self.mir.close(), self.r.close()


def _refused(ctx, tb):
    L, b, h = lib.load(), tb.as_batch(), C.c_void_p(1)
    rc = L.osmt_scene_build_tiles(ctx._h, C.byref(b), C.byref(h))
    msg = L.osmt_last_error().decode()
    assert rc == abi.UNSUPPORTED and not h.value, (rc, msg)
    return msg


def _areas_equal_the_mirror(ctx, gid, bid, draw, tiles):
    scene = ctx.build_tiles(styled.TileBatch(gid, tiles, {z: bid for z in range(19)}, canvas=CANVAS))
    got_tiles, got = scene.read_styled_areas()
    want = [draw.mir.areas(z, x, y) for z, x, y in tiles]
    assert [int(t["n_areas"]) for t in got_tiles] == [len(a) for a in want]
    assert got.tobytes() == (np.concatenate(want) if want else got).tobytes()
    scene.free()
    return want


def test_case_a_one_tile_over_the_limit_builds_from_level_18(base, tmp_path):
    """2^20 + 1 references to 16 ways in one z18 tile: refused from the z18 index, 16 candidates from level 18"""
    ctx = base[0]
    LIM = abi.QUERY_MAX_TILE_CANDIDATES
    ids = np.random.default_rng(108).integers(0, 16, LIM + 1).tolist()
    tiles = [((CX, CY), ids, [], []), ((CX + 40, CY), [63, 63], [0], [])]
    draw = Draw(base, tmp_path / "a.bin", {(CX, CY): ([], list(range(16)), []), (CX + 40, CY): ([], [63], [0])})
    plain, _, _, _ = _register(base, tiles)
    b0 = draw.bind(ctx, plain)
    ask = [(18, CX + 40, CY), (18, CX - 1, CY)]
    msg = _refused(ctx, styled.TileBatch(plain, ask, {18: b0}))
    assert "tile 1" in msg and str(LIM + 1) in msg and "way" in msg
    _areas_equal_the_mirror(ctx, plain, b0, draw, ask[:1])  # the context builds on
    gid, _, _, _ = _register(base, tiles)
    b1 = draw.bind(ctx, gid)
    ctx.register_tile_pyramid(gid, 1 << 18)
    want = _areas_equal_the_mirror(ctx, gid, b1, draw, ask)
    assert len({int(e) for e in want[1]["entity"]}) == 16
    assert ctx.tile_query_stats() == (2, 16 + 1, 1, 0)
    draw.close()


def test_case_b_a_street_grid_at_zoom_13_builds_from_level_13(base, tmp_path):
    """700 ways, each listed in every tile of a 40 x 40 block of z18 tiles: 1 120 000 references, refused at zoom 13 from the z18
    index; level 13 names each way once per level tile the block touches"""
    ctx = base[0]
    bx, by = (CX >> 5 << 5) + 4, (CY >> 5 << 5) + 4  # inside one zoom-13 tile... the block spans two of them per axis
    ways = list(range(700))
    tiles = [((bx + i, by + j), ways, [], []) for i in range(40) for j in range(40)]
    assert sum(len(t[1]) for t in tiles) == 1_120_000 > abi.QUERY_MAX_TILE_CANDIDATES
    draw = Draw(base, tmp_path / "b.bin", {(bx, by): ([], ways, [])})
    ask = [(13, bx >> 5, by >> 5)]
    plain, _, _, _ = _register(base, tiles, nodes="never")
    b0 = draw.bind(ctx, plain)
    msg = _refused(ctx, styled.TileBatch(plain, ask, {13: b0}))
    assert "tile 0" in msg and "1120000" in msg and "way" in msg
    _areas_equal_the_mirror(ctx, plain, b0, draw, [(18, bx, by)])  # the context builds on
    gid, _, _, _ = _register(base, tiles, nodes="never")
    b1 = draw.bind(ctx, gid)
    ctx.register_tile_pyramid(gid, 1 << 13)
    want = _areas_equal_the_mirror(ctx, gid, b1, draw, ask)
    assert len(want[0]) == 700
    items, n_way, n_mp, n_node = ctx.tile_query_stats()
    assert 700 <= n_way <= 9 * 700 and n_mp == 0 and n_node == 0 and items <= 3
    draw.close()


def test_a_level_below_the_zoom_is_not_read(base, tmp_path):
    """with level 12 alone a zoom-18 batch gathers what it gathers without a pyramid; zooms 12 and 10 gather less"""
    ctx = base[0]
    rng = np.random.default_rng(31)
    tiles = [t for t in _random_tiles(rng, 150) if abs(t[0][0] - CX) < 400]
    tiles = [(k, [w % 700 for w in ws] * 2, ms, ns) for k, ws, ms, ns in tiles]
    draw = Draw(base, tmp_path / "c.bin", {k: (ns, ws, ms) for k, ws, ms, ns in tiles})
    plain, _, _, _ = _register(base, tiles)
    gid, _, _, _ = _register(base, tiles)
    ctx.register_tile_pyramid(gid, 1 << 12)
    b0, b1 = draw.bind(ctx, plain), draw.bind(ctx, gid)
    z18 = [(18, *t[0]) for t in tiles[:40]]
    low = [(12, CX >> 6, CY >> 6), (10, CX >> 8, CY >> 8), (12, (CX + 300) >> 6, (CY - 40) >> 6)]
    stats = {}
    for name, g, b in (("plain", plain, b0), ("level 12", gid, b1)):
        for ask in (z18, low):
            want = _areas_equal_the_mirror(ctx, g, b, draw, ask)
            assert sum(len(a) for a in want) > 0
            stats[(name, len(ask))] = ctx.tile_query_stats()
    assert stats[("plain", 40)] == stats[("level 12", 40)] and stats[("plain", 40)][1] > 0
    assert stats[("level 12", 3)][1] < stats[("plain", 3)][1] and stats[("level 12", 3)][0] < stats[("plain", 3)][0]
    draw.close()


# ---- scenes are the same bytes ------------------------------------------------------------------------------------------
def _tables(ctx):
    """the glyphs, the font and the icons of tests/test_gpu_area_labels.py::tables, in a context of this file's"""
    syn = labels.synth_glyph_table()
    ctx.register_glyphs(syn)
    shapes = [NS - 1] + [(g - 1) % (NS - 1) for g in range(1, 13)] + [NS - 1]
    cmap = [(0x20, 13)] + [(0x41 + i, 1 + i) for i in range(12)]
    font = labels.FontTable(cmap, [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]], [syn.first_id + s for s in shapes], [(1, 2, 17), (3, 5, -45)])
    ctx.register_font(font)
    rng = np.random.default_rng(23)
    imgs, ids = [], []
    for h, w in ICONS:
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img[: h // 2, :, 3] = 255
        imgs.append(img)
        ids.append(ctx.register_image(img))
    return syn, font, imgs, ids


def _town(ctx, path):
    """the town of tests/test_gpu_area_labels.py on 6 x 4 tiles of zoom 16, every entity listed in four z18 tiles of its z16 tile:
    a neighbourhood names it many times, a level once per level tile"""
    rng = np.random.default_rng(41)
    w = al.World((0, 0))
    way_rows, mp_rows, draw = [], [], []

    def shape(i, j, pts):
        ids = []
        for fx, fy in pts:
            lat, lon = tl.latlon_of(Z, TX + i + fx, TY + j + fy)
            w.nodes.append((7000 + len(w.nodes), lat, lon, {}))
            ids.append(len(w.nodes) - 1)
        return ids

    box = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    for j in range(4):
        for i in range(6):
            k18 = [((TX + i) * 4 + a, (TY + j) * 4 + b) for a in (1, 2) for b in (0, 1)]
            gid = lambda: int(rng.integers(1, 1 << 60))
            w.way(shape(i, j, [(0.08, 0.2), (0.4, 0.16), (0.9, 0.21)]), gid(), k18)
            way_rows.append([(0, 2 if i % 4 else 3)])
            draw.append([0])
            w.way(shape(i, j, box(0.2, 0.4, 0.25, 0.2)), gid(), k18)
            way_rows.append([(2, 0), (4, 4)])
            draw.append([0])
            w.mp([w.polygon(shape(i, j, box(0.55, 0.55, 0.1, 0.1))), w.polygon(shape(i, j, box(0.6, 0.5, 0.3, 0.4)))], gid(), k18[:3])
            mp_rows.append([(0, 2), (1, None)])
    W = World(ctx, _tables(ctx), path, w, draw)
    W.all = W.bind(way_rows, mp_rows)
    return W


class Side:
    """a context of its own with the town, its node index, bindings and a tile server; `mask`: the pyramid, None: none"""

    def __init__(self, path, mask):
        from osm_renderer_amd.renderer import Context

        self.ctx = Context(0)
        self.W = _town(self.ctx, path / "town.bin")
        self.feed = idf.Feed(self.ctx, self.W, path / "town_nodes.bin", TEXTS, CANVAS)
        if mask is not None:
            self.ctx.register_tile_pyramid(self.W.gid, mask)
        self.flt = self.ctx.register_id_filter(self.W.gid, idf.half_of_the_ids(self.feed, seed=13))
        self.binds = ({z: self.W.all[0] for z in range(19)}, {z: self.feed.node_bind for z in range(19)})
        kw = dict(area_label_bindings=self.binds[0], node_label_bindings=self.binds[1], canvas=CANVAS)
        self.server = self.ctx.tile_server(self.W.gid, {z: self.feed.draw for z in range(19)}, **kw)
        self.filtered = self.ctx.tile_server(self.W.gid, {z: self.feed.draw for z in range(19)}, id_filter=self.flt, **kw)

    def everything(self, tiles, filtered):
        """every byte a request can be asked for, and the query's counts"""
        sc = self.feed.scene(tiles, 1, flt=self.flt if filtered else None)
        area_stats = self.ctx.tile_query_stats()
        area, node = sc.build_tile_labels_all(*self.binds)
        node_stats = self.ctx.tile_query_stats()
        dl, (st_tiles, st_areas) = sc.read_display_list(), sc.read_styled_areas()
        out = {"files": self.ctx.render_scene_png(sc), "server": (self.filtered if filtered else self.server).render_png(tiles, 1),
               "declined": sc.read_declined_anchors().tobytes(), "styled tiles": st_tiles.tobytes(), "styled areas": st_areas.tobytes()}
        for name in ("jobs", "ops", "rings", "coords", "dashes"):
            out["list " + name] = getattr(dl, name).tobytes()
        for kind, batch in (("area", area), ("node", node)):
            for name in ("labels", "job_label_off", "runs", "chars", "way_pts", "way_sincos"):
                out[f"{kind} {name}"] = np.ascontiguousarray(getattr(batch, name)).tobytes()
        sc.free()
        return out, area_stats, node_stats, (len(st_areas), len(area.labels), len(node.labels))

    def close(self):
        self.server.close(), self.filtered.close(), self.feed.close(), self.W.close(), self.ctx.close()


MIXED = [(15, (TX + 2) >> 1, (TY + 1) >> 1), (18, (TX + 1) * 4 + 1, (TY + 1) * 4 + 1), (12, TX >> 4, TY >> 4), (17, (TX + 3) * 2, (TY + 2) * 2),
         (18, (TX + 4) * 4 + 2, (TY + 2) * 4), (17, (TX + 1) * 2 + 1, TY * 2), (15, (TX + 4) >> 1, (TY + 3) >> 1), (12, (TX >> 4) + 1, TY >> 4)]


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    made = {}
    for name, mask in (("plain", None), ("all", ALL), ("sparse", _mask((18, 16, 13)))):  # sparse: 17 reads 18, 15 reads 16, 12 reads 13
        d = tmp_path_factory.mktemp("side_" + name)
        made[name] = Side(d, mask)
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("name", ["all", "sparse"])
def test_a_mixed_zoom_batch_is_the_same_bytes(sides, name, filtered):
    want, area0, node0, sizes = sides["plain"].everything(MIXED, filtered)
    got, area1, node1, _ = sides[name].everything(MIXED, filtered)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    assert sizes[0] > 20 and sizes[1] > 20 and sizes[2] > 20 and len(want["files"]) == len(MIXED)
    assert sides[name].ctx.tile_pyramid_levels(sides[name].W.gid)[1] != 0  # node lists: the node index came first
    # not vacuous: the levels were read — fewer candidates gathered, of areas and of nodes
    assert area1[1] < area0[1] and area1[2] < area0[2] and area1[0] < area0[0], (area0, area1)
    assert node1[3] < node0[3] and node0[1] == node1[1] == 0, (node0, node1)


def test_one_request_through_the_worker(sides):
    files = {}
    for name, s in sides.items():
        wk = s.ctx.worker()
        files[name] = [wk.render_tile_png(s.server, t) for t in (MIXED[0], MIXED[2])]
        wk.close()
    assert files["all"] == files["plain"] == files["sparse"] and len(set(files["plain"])) == 2


# ---- refusals that need a context ---------------------------------------------------------------------------------------
def test_refusals_and_later_registrations(base, tmp_path):
    ctx, g, _, _ = base
    L = lib.load()
    tiles = _random_tiles(np.random.default_rng(77), 60)
    tiles = [(k, [w % 700 for w in ws], ms, ns) for k, ws, ms, ns in tiles]
    draw = Draw(base, tmp_path / "r.bin", {k: (ns, ws, ms) for k, ws, ms, ns in tiles})
    gid, _, _, _ = _register(base, tiles)
    bid = draw.bind(ctx, gid)
    ctx.register_tile_pyramid(gid, _mask((18, 15, 11)))
    with pytest.raises(OsmtError, match="tile pyramid already") as e:
        ctx.register_tile_pyramid(gid, 1 << 3)  # a second registration, also of other levels
    assert e.value.code == abi.INVALID_ARG and ctx.tile_pyramid_levels(gid)[0] == _mask((18, 15, 11))
    no_index = ctx.register_geodata(g)
    assert L.osmt_validate_tile_pyramid(no_index, ALL, ctx._h) == abi.INVALID_ARG and "no tile index" in L.osmt_last_error().decode()
    with pytest.raises(OsmtError, match=f"geodata id {no_index} has no tile index"):
        ctx.register_tile_pyramid(no_index)
    with pytest.raises(OsmtError, match="is not registered"):
        ctx.register_tile_pyramid(10**6)
    with pytest.raises(OsmtError, match="mask 0"):
        ctx.register_tile_pyramid(gid, 0)
    assert ctx.tile_pyramid_levels(no_index) == (0, 0)
    # a scene built from the pyramid, then another file with its own index and pyramid: the scene is not disturbed
    ask = [(15, CX >> 3, CY >> 3), (12, CX >> 6, CY >> 6), (18, *tiles[0][0])]
    scene = ctx.build_tiles(styled.TileBatch(gid, ask, {z: bid for z in range(19)}, canvas=CANVAS))
    before, px = scene.read_styled_areas()[1].tobytes(), ctx.render(scene).cpu().numpy()
    assert len(before) > 0
    _check_levels(base, corner_tiles(np.random.default_rng(3)), (18, 2))
    assert scene.read_styled_areas()[1].tobytes() == before and np.array_equal(ctx.render(scene).cpu().numpy(), px)
    scene.free()
    _areas_equal_the_mirror(ctx, gid, bid, draw, ask)
    draw.close()
