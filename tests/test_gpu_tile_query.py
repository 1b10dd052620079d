"""Scenes built from tile coordinates (osmt_scene_build_tiles, osm_renderer_amd/csrc/osmt_tilequery.hip): a registered tile
index + registered style bindings + 16 bytes per tile in, an ordinary OSMT_COORD_NODE_REF scene out.

Every case checks two things against code that is not under test.  The styled batch the device derived
(osmt_scene_read_styled_areas) must equal, tile by tile and element by element, what the host mirror
osmt::styled_areas_of_tile (host/osmt_tilequery.hpp, through tests/tilequery_shim.cpp) makes over GeodataReader's own column
walk; and the display list must equal, byte for byte, the one osmt_scene_build_styled builds from the mirror's batch.  The
worlds are written with tests/_geodata.write_geodata, whose tile_refs argument places index tiles and id lists freely."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _tilequery as tq
from tests._styled_feed import fill_only_styles, geodata_of, recs_of
from tests.test_styled_builder import _random_styles

pytestmark = pytest.mark.gpu

CANVAS = (241, 238, 232)
CX, CY = tq.center_z18()
CASES = ("rectangle", "edges", "tiny indices", "dedup", "candidate counts", "item counts", "many tiles", "area limit", "candidate limit", "snapshots",
         "pixels")
_STATS = {}  # case -> (requested tiles, tiles with a non-empty area list), from the mirror's output


def _record(case, want):
    n, k = _STATS.get(case, (0, 0))
    _STATS[case] = (n + len(want), k + sum(len(a) > 0 for a in want))


class World:
    """a geodata file with its topology, styles and tile index registered"""

    def __init__(self, gpu_ctx, path, n_ways, mp_polygons, refs, st, pool, shared_nodes=True, shuffle=None, index=True):
        self.ctx = gpu_ctx
        self.r, self.refs = tq.make_world(str(path), n_ways, mp_polygons, tile_refs=refs, shared_nodes=shared_nodes)
        self.n_polys = list(mp_polygons)
        self.gid = gpu_ctx.register_geodata(geodata_of(self.r))
        self.first = gpu_ctx.register_styles(recs_of(st), pool)
        self.n_styles = len(st)
        if index:
            gpu_ctx.register_tile_index(self.gid, tq.index_of(self.refs, shuffle))
        self.mirrors = []

    def bind(self, ws, ms, zoom_lo=0, zoom_hi=18, first=None):
        """registers a bindings table (style ids relative to this world's first style); returns (bindings id, mirror)"""
        first = self.first if first is None else first
        ws, ms = [[s + first for s in v] for v in ws], [[s + first for s in v] for v in ms]
        bid = self.ctx.register_style_bindings(styled.StyleBindings(self.gid, zoom_lo, zoom_hi, ws, ms))
        mir = tq.Mirror(self.r, ws, ms, self.gid, zoom_lo, zoom_hi)
        mir.ws, mir.ms = ws, ms
        self.mirrors.append(mir)
        return bid, mir

    def close(self):
        for m in self.mirrors:
            m.close()
        self.r.close()


def _falling(rng, n, n_styles, counts=(0, 1, 3)):
    """per entity 0, 1 or 3 style ids, falling: binding order is not id order"""
    return [sorted(rng.choice(n_styles, counts[i % len(counts)], replace=False).tolist(), reverse=True) for i in range(n)]


def _mirror_batch(gid, tiles, want, scale, use_caps):
    sb = styled.StyledBatch(gid, [(z, x, y, [], []) for z, x, y in tiles], scale=scale, use_caps_for_dashes=use_caps, canvas=CANVAS)
    off = 0
    for t, a in zip(sb.tiles, want):
        t["area_off"], t["n_areas"] = off, len(a)
        off += len(a)
    sb.areas = np.concatenate(want) if want else np.zeros(0, styled.STYLED_AREA_DTYPE)
    return sb


def _assert_same_list(got, want):
    for name in ("jobs", "ops", "rings", "coords", "dashes"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


def _check(w, tiles, bind_of_zoom, case, scale=1, use_caps=True, keep=False):
    """builds `tiles` on the device, compares the derived batch with the mirror's and the display list with the one
    osmt_scene_build_styled makes of the mirror's batch; returns (mirror's areas per tile, scene, twin scene) — the scenes freed
    unless `keep`"""
    tb = styled.TileBatch(w.gid, tiles, {z: b for z, (b, _) in bind_of_zoom.items()}, scale=scale, use_caps_for_dashes=use_caps, canvas=CANVAS)
    w.ctx.validate_tiles(tb)
    scene = w.ctx.build_tiles(tb)
    got_tiles, got_areas = scene.read_styled_areas()
    want = [bind_of_zoom[z][1].areas(z, x, y) for z, x, y in tiles]
    _record(case, want)
    assert len(got_tiles) == len(tiles) and len(got_areas) == sum(len(a) for a in want)
    off = 0
    for i, ((z, x, y), a) in enumerate(zip(tiles, want)):
        t = got_tiles[i]
        assert (int(t["zoom"]), int(t["x"]), int(t["y"]), int(t["has_canvas"]), tuple(t["canvas_rgb"])) == (z, x, y, 1, CANVAS), i
        assert (int(t["area_off"]), int(t["n_areas"])) == (off, len(a)), (i, z, x, y)
        assert got_areas[off : off + len(a)].tobytes() == a.tobytes(), (i, z, x, y)
        off += len(a)
    twin = w.ctx.build_styled(_mirror_batch(w.gid, tiles, want, scale, use_caps))
    _assert_same_list(scene.read_display_list(), twin.read_display_list())
    assert scene.max_tile_ops() == twin.max_tile_ops()
    if keep:
        return want, scene, twin
    scene.free()
    twin.free()
    return want, None, None


def _dedup_seen(w, mir, tiles):
    """tiles whose neighbourhood names an entity more than once"""
    n = 0
    for z, x, y in tiles:
        _, raw, distinct = tq.restate(w.refs, w.n_polys, mir.ws, mir.ms, z, x, y)
        n += raw > distinct
    return n


def _refused(ctx, tb, code=abi.UNSUPPORTED):
    L, b, h = lib.load(), tb.as_batch(), C.c_void_p(1)
    rc = L.osmt_scene_build_tiles(ctx._h, C.byref(b), C.byref(h))
    msg = L.osmt_last_error().decode()
    assert rc == code and not h.value, (rc, msg)
    return msg


# ---- rectangle ------------------------------------------------------------------------------------------------------
def _holes_refs(rng, n_ways, n_mps):
    """around the zoom-15 tile of (CX, CY): columns that are absent, columns whose tiles all lie below or above the y range, and
    the last tile of the index inside the range"""
    X, Y = CX // 8, CY // 8
    x0, y0, y1 = (X - 1) * 8, (Y - 1) * 8, (Y + 2) * 8 - 1
    refs = {}

    def put(x, y):
        w = rng.integers(0, n_ways, int(rng.integers(1, 6))).tolist()
        refs[(x, y)] = ([], w + w[:1], rng.integers(0, n_mps, int(rng.integers(0, 3))).tolist())

    for c in (0, 1, 3, 4, 8, 9, 15, 16, 22):
        for dy in (0, 5, 7, 8, 16, 23):
            put(x0 + c, y0 + dy)
    for c in (2, 10):  # only below the range
        put(x0 + c, y0 - 3), put(x0 + c, y0 - 1)
    for c in (5, 11):  # only above
        put(x0 + c, y1 + 1), put(x0 + c, y1 + 9)
    for c in (6, 17):  # on both sides, none inside
        put(x0 + c, y0 - 1), put(x0 + c, y1 + 1)
    put(x0 + 7, y0 - 1), put(x0 + 7, y0), put(x0 + 7, y1), put(x0 + 7, y1 + 1)  # the range's own rim
    put(x0 - 1, y0 + 3), put(x0 - 40, y0 + 3)  # left of the rectangle
    put(x0 + 23, y0 + 10)  # the last tile of the index: the walk ends inside the range
    return refs, (X, Y)


def test_rectangle_holes_and_mixed_zooms(tmp_path, gpu_ctx):
    rng = np.random.default_rng(101)
    st, pool = fill_only_styles(rng, 40)
    refs, (X, Y) = _holes_refs(rng, 60, 4)
    w = World(gpu_ctx, tmp_path / "a.bin", 60, (1, 0, 3, 2), refs, st, pool)
    assert max(w.refs) == ((X - 1) * 8 + 23, (Y - 1) * 8 + 10)
    lo = w.bind(_falling(rng, 60, 40), _falling(rng, 4, 40, (1, 3, 1, 3)), 0, 15)
    hi = w.bind(_falling(rng, 60, 40, (3, 1, 1)), _falling(rng, 4, 40, (3, 3, 1, 1)), 16, 18)
    assert lo[0] != hi[0]
    bz = {z: lo for z in range(16)}
    bz.update({z: hi for z in (16, 17, 18)})
    x0, y0 = (X - 1) * 8, (Y - 1) * 8
    tiles = [(15, X, Y), (15, X + 10, Y),  # the neighbourhood with the holes; an empty neighbourhood
             (0, 0, 0), (15, X, Y),  # the whole index; the same tile again
             (18, x0 + 8, y0 + 6), (18, x0 + 1, y0 + 1), (18, x0 + 23, y0 + 10), (18, x0 + 6, y0),  # 3 x 3 z18 tiles
             (17, (x0 + 8) // 2, (y0 + 6) // 2), (17, (x0 + 22) // 2, (y0 + 8) // 2), (16, (x0 + 4) // 4, (y0 + 8) // 4),
             (15, X, Y), (15, X - 1, Y), (15, X + 1, Y + 1), (15, X, Y - 2), (14, X // 2, Y // 2), (10, X >> 5, Y >> 5)]
    want, _, _ = _check(w, tiles, bz, "rectangle")
    assert len(want[1]) == 0 and len(want[2]) >= len(want[0]) > 0
    assert want[0].tobytes() == want[3].tobytes() == want[11].tobytes()
    assert _dedup_seen(w, lo[1], [t for t in tiles if t[0] <= 15]) >= 5
    # the same at scale 2 without caps for dashes: the derived batch does not depend on either
    _check(w, tiles[:6], bz, "rectangle", scale=2, use_caps=False)
    w.close()


def test_world_edges_and_corners(tmp_path, gpu_ctx):
    rng = np.random.default_rng(102)
    st, pool = fill_only_styles(rng, 20)
    hi = tq.WORLD - 1
    refs = {}
    for x, y in [(0, 0), (1, 1), (7, 7), (8, 8), (15, 15), (16, 0), (0, 16), (15, 16), (hi, hi), (hi - 15, hi - 15), (hi - 16, hi), (hi, hi - 16), (0, hi),
                 (15, hi - 15), (16, hi - 3), (hi, 0), (hi - 15, 15), (hi - 16, 3), (0, 800), (15, 807), (16, 800), (3, 784), (3, 783), (800, 0), (807, 15),
                 (800, 16), (hi, 800), (hi - 16, 800), (800, hi), (800, hi - 16)]:
        w_ = rng.integers(0, 30, int(rng.integers(1, 5))).tolist()
        refs[(x, y)] = ([], w_ + w_[:1], rng.integers(0, 3, 2).tolist())
    w = World(gpu_ctx, tmp_path / "e.bin", 30, (1, 3, 0), refs, st, pool)
    b = w.bind(_falling(rng, 30, 20, (1, 3, 1)), _falling(rng, 3, 20, (1, 3, 1)))
    n = 1 << 15
    tiles = [(15, 0, 0), (15, n - 1, 0), (15, 0, n - 1), (15, n - 1, n - 1), (15, 0, 100), (15, 100, 0), (15, n - 1, 100), (15, 100, n - 1),
             (15, 1, 1), (15, n - 2, n - 2), (18, 0, 0), (18, hi, hi), (18, 0, hi), (18, hi, 0), (17, 0, 0), (17, (1 << 17) - 1, (1 << 17) - 1), (0, 0, 0),
             (1, 0, 0), (1, 1, 1), (1, 0, 1), (1, 1, 0)]
    want, _, _ = _check(w, tiles, {z: b for z in (0, 1, 15, 17, 18)}, "edges")
    assert all(len(a) > 0 for a in want)
    assert _dedup_seen(w, b[1], tiles) >= 10
    w.close()


def test_indices_of_no_tile_and_of_one(tmp_path, gpu_ctx):
    rng = np.random.default_rng(103)
    st, pool = fill_only_styles(rng, 8)
    none = World(gpu_ctx, tmp_path / "n.bin", 5, (1,), {}, st, pool)
    b0 = none.bind(_falling(rng, 5, 8, (1, 3)), [[2]])
    want, _, _ = _check(none, [(15, CX // 8, CY // 8), (0, 0, 0), (18, 0, 0)], {z: b0 for z in (0, 15, 18)}, "tiny indices")
    assert all(len(a) == 0 for a in want)
    none.close()
    one = World(gpu_ctx, tmp_path / "o.bin", 5, (1,), {(CX, CY): ([], [4, 0, 4, 2], [0, 0])}, st, pool)
    b1 = one.bind(_falling(rng, 5, 8, (1, 3)), [[2]])
    tiles = [(18, CX, CY), (18, CX + 1, CY - 1), (18, CX + 2, CY), (15, CX // 8, CY // 8), (0, 0, 0), (18, CX - 1, CY + 1), (17, CX // 2, CY // 2), (18, CX, CY + 1),
             (18, CX, CY - 1), (18, CX + 1, CY + 1), (18, CX - 1, CY - 1), (16, CX // 4, CY // 4)]
    want, _, _ = _check(one, tiles, {z: b1 for z in (0, 15, 16, 17, 18)}, "tiny indices")
    assert len(want[2]) == 0 and all(len(a) > 0 for i, a in enumerate(want) if i != 2)
    assert _dedup_seen(one, b1[1], tiles) == len(tiles) - 1
    # a batch of no tiles builds an empty scene
    tb = styled.TileBatch(one.gid, [], {})
    scene = gpu_ctx.build_tiles(tb)
    t, a = scene.read_styled_areas()
    dl = scene.read_display_list()
    assert len(t) == len(a) == len(dl.jobs) == len(dl.ops) == 0
    scene.free()
    one.close()


# ---- dedup and order ------------------------------------------------------------------------------------------------
def test_dedup_order_and_nothing_bound(tmp_path, gpu_ctx):
    rng = np.random.default_rng(104)
    n_ways, polys = 50, (0, 1, 3, 1)
    st, pool = fill_only_styles(rng, 30)
    X, Y = CX // 8, CY // 8
    refs = {}
    for x in range((X - 1) * 8, (X + 2) * 8):
        for y in range((Y - 1) * 8, (Y + 2) * 8):  # way 7 in all 576 z18 tiles of the neighbourhood
            refs[(x, y)] = ([], [7], [])
    for k in range(40):
        x, y = (X - 1) * 8 + int(rng.integers(0, 24)), (Y - 1) * 8 + int(rng.integers(0, 24))
        refs[(x, y)] = ([], [7, 0, n_ways - 1, 7] + rng.integers(0, n_ways, 4).tolist(), rng.integers(0, 4, 3).tolist() + [0, 2])
    w = World(gpu_ctx, tmp_path / "d.bin", n_ways, polys, refs, st, pool, shuffle=rng)  # the lists handed over in random order
    assert len(w.refs) == 576
    ws = _falling(rng, n_ways, 30)
    ws[7], ws[0], ws[n_ways - 1] = [29, 12, 3], [5], [28, 27, 1]
    ms = [[9, 4], [8], [20, 10, 0], []]  # multipolygon 0 has no polygon: dropped whatever is bound to it; 3 has nothing bound
    b = w.bind(ws, ms)
    tiles = [(15, X, Y), (16, (CX // 4), (CY // 4)), (15, X + 1, Y), (15, X, Y - 1)]
    want, _, _ = _check(w, tiles, {15: b, 16: b}, "dedup")
    got = tq.pairs(want[0])
    f = w.first
    assert got[0] == (0, 5 + f) and [p for p in got if p[0] == 7] == [(7, 29 + f), (7, 12 + f), (7, 3 + f)]
    assert [p for p in got if p[0] == n_ways - 1] == [(n_ways - 1, 28 + f), (n_ways - 1, 27 + f), (n_ways - 1, 1 + f)]
    mp = abi.STYLED_MULTIPOLYGON
    assert [p for p in got if p[0] & mp] == [(1 | mp, 8 + f), (2 | mp, 20 + f), (2 | mp, 10 + f), (2 | mp, f)]
    assert [p[0] for p in got if not p[0] & mp] == sorted(p[0] for p in got if not p[0] & mp)
    assert any(not ws[i] for i in range(n_ways)) and _dedup_seen(w, b[1], tiles) == len(tiles)
    # a table in which nothing is bound: every tile is empty, the jobs are still written, the render shows the canvas
    nb = w.bind([[] for _ in range(n_ways)], [[] for _ in polys])
    want, scene, twin = _check(w, tiles[:3], {15: nb, 16: nb}, "nothing bound", keep=True)
    assert all(len(a) == 0 for a in want)
    dl = scene.read_display_list()
    assert len(dl.jobs) == 3 and len(dl.ops) == 0 and [int(z) for z in dl.jobs["zoom"]] == [15, 16, 15]
    px = gpu_ctx.render(scene).cpu().numpy()
    scene.check()
    assert (px == np.array(CANVAS + (255,), np.uint8)).all()
    scene.free()
    twin.free()
    w.close()


# ---- sizes where a scan, a bisection or the sort can go wrong ---------------------------------------------------------
def test_candidate_and_item_counts(tmp_path, gpu_ctx):
    rng = np.random.default_rng(105)
    n_ways, polys = 300, (1, 2)
    st, pool = fill_only_styles(rng, 16)
    LDS = abi.QUERY_LDS_CANDIDATES
    counts = [0, 1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 20000]
    refs = {}
    for k, n in enumerate(counts):  # one lone z18 tile per count, ten tiles apart
        if n == 20000:
            ids = rng.choice([3, 299, 0, 17, 150], n).tolist()  # the device tier with 5 distinct ids
        else:
            ids = rng.integers(0, n_ways, n).tolist()
        if n:
            refs[(CX + 10 * k, CY)] = ([], ids, [1, 0, 1][: k % 4])
    # (tile, column) items: zoom-13 tiles (96 columns) over 0, 1, 64 and 65 columns that exist, far from the tiles above
    X13, Y13 = CX // 32 + 50, CY // 32 + 200
    regions = [(X13 + 10 * j, m) for j, m in enumerate((0, 1, 64, 65))]
    for X, m in regions:
        for c in rng.choice(96, m, replace=False).tolist():
            x = (X - 1) * 32 + c
            refs[(x, (Y13 - 1) * 32 + int(rng.integers(0, 96)))] = ([], [c % n_ways, (7 * c) % n_ways], [c % 2])
            if c % 3 == 0:
                refs[(x, (Y13 - 1) * 32 - 1 - c)] = ([], [1], [])  # a tile of the column outside the y range
    w = World(gpu_ctx, tmp_path / "c.bin", n_ways, polys, refs, st, pool)
    b = w.bind(_falling(rng, n_ways, 16, (1, 3, 1)), [[4], [2, 1]])
    tiles = [(18, CX + 10 * k, CY) for k in range(len(counts))]
    want, _, _ = _check(w, tiles, {18: b}, "candidate counts")
    assert [len(a) > 0 for a in want] == [n > 0 for n in counts]
    assert len({e for e, _ in tq.pairs(want[-1]) if not e & abi.STYLED_MULTIPOLYGON}) == 5
    assert _dedup_seen(w, b[1], tiles) >= 6
    tiles = [(13, X, Y13) for X, _ in regions]
    want, _, _ = _check(w, tiles, {13: b}, "item counts")
    assert [len(a) > 0 for a in want] == [False, True, True, True]
    assert _dedup_seen(w, b[1], tiles) >= 2
    w.close()


def test_more_tiles_than_one_block_in_any_order(tmp_path, gpu_ctx):
    rng = np.random.default_rng(106)
    n_ways, polys = 200, (1, 3, 1)
    st, pool = fill_only_styles(rng, 16)
    x0, y0, nx, ny = CX - 20, CY - 5000, 40, 28
    refs = {}
    for x in range(x0, x0 + nx):
        for y in range(y0, y0 + ny):
            if rng.random() < 0.9:
                refs[(x, y)] = ([], [(3 * x + y) % n_ways, (x + 5 * y) % n_ways, int(rng.integers(0, n_ways))], [int(rng.integers(0, 3))] if (x + y) % 4 == 0 else [])
    w = World(gpu_ctx, tmp_path / "m.bin", n_ways, polys, refs, st, pool)
    b = w.bind(_falling(rng, n_ways, 16, (1, 1, 3)), [[1], [6, 5, 0], [2]])
    tiles = [(18, x, y) for x in range(x0, x0 + nx) for y in range(y0, y0 + ny)][:1100]
    assert len(tiles) == 1100
    perm = rng.permutation(len(tiles))
    shuffled = [tiles[i] for i in perm]
    want, _, _ = _check(w, shuffled, {18: b}, "many tiles")
    assert sum(len(a) > 0 for a in want) == len(tiles)
    assert _dedup_seen(w, b[1], shuffled[:50]) >= 25
    w.close()


# ---- limits ---------------------------------------------------------------------------------------------------------
def test_the_area_limit_of_a_tile(tmp_path, gpu_ctx):
    rng = np.random.default_rng(107)
    n_ways = 2048
    st, pool = fill_only_styles(rng, 40)
    w = World(gpu_ctx, tmp_path / "l.bin", n_ways, (), {(CX, CY): ([], list(range(n_ways)) + [5, 5], [])}, st, pool)
    per = abi.STYLED_MAX_TILE_AREAS // n_ways
    assert per * n_ways == abi.STYLED_MAX_TILE_AREAS and per < 40
    ws = [list(range(per - 1, -1, -1)) for _ in range(n_ways)]
    full = w.bind(ws, [])
    ws2 = [list(v) for v in ws]
    ws2[1000].append(39)
    over = w.bind(ws2, [])
    tiles = [(18, CX + 1, CY), (18, CX + 5, CY), (18, CX, CY)]
    want, _, _ = _check(w, tiles, {18: full}, "area limit")
    assert [len(a) for a in want] == [abi.STYLED_MAX_TILE_AREAS, 0, abi.STYLED_MAX_TILE_AREAS]
    msg = _refused(gpu_ctx, styled.TileBatch(w.gid, tiles[1:], {18: over[0]}))
    assert "tile 1" in msg and str(abi.STYLED_MAX_TILE_AREAS + 1) in msg
    _check(w, tiles[:1], {18: full}, "area limit")  # the context builds on
    w.close()


def test_the_candidate_limit_of_a_tile_and_of_a_batch(tmp_path, gpu_ctx):
    rng = np.random.default_rng(108)
    LIM = abi.QUERY_MAX_TILE_CANDIDATES
    n_ways = 64
    st, pool = fill_only_styles(rng, 8)
    ids = rng.integers(0, 16, LIM).tolist()  # 2^20 references to 16 ways
    w = World(gpu_ctx, tmp_path / "q.bin", n_ways, (1,), {(CX, CY): ([], ids, []), (CX + 40, CY): ([], [63, 63], [0])}, st, pool)
    b = w.bind(_falling(rng, n_ways, 8, (1, 3)), [[3]])
    tiles = [(18, CX, CY), (18, CX + 40, CY), (18, CX + 1, CY + 1)]
    want, _, _ = _check(w, tiles, {18: b}, "candidate limit")
    assert len({e for e, _ in tq.pairs(want[0])}) == 16 and len(want[1]) > 0
    # one reference more: a second registration of the same file, its index one id longer
    gid2 = gpu_ctx.register_geodata(geodata_of(w.r))
    gpu_ctx.register_tile_index(gid2, styled.TileIndex({(CX, CY): (ids + [3], []), (CX + 40, CY): ([63, 63], [0])}))
    b2 = gpu_ctx.register_style_bindings(styled.StyleBindings(gid2, 0, 18, b[1].ws, b[1].ms))
    msg = _refused(gpu_ctx, styled.TileBatch(gid2, [(18, CX + 40, CY), (18, CX - 1, CY)], {18: b2}))
    assert "tile 1" in msg and str(LIM + 1) in msg and "way" in msg
    scene = gpu_ctx.build_tiles(styled.TileBatch(gid2, [(18, CX + 40, CY)], {18: b2}))
    assert scene.read_styled_areas()[1].tobytes() == want[1].tobytes()
    scene.free()
    # 4097 copies of the 2^20-reference tile: 2^32 + 2^20 candidates, refused from the counts alone
    msg = _refused(gpu_ctx, styled.TileBatch(w.gid, [(18, CX, CY)] * 4097, {18: b[0]}))
    assert 4097 * LIM == 2**32 + 2**20 and str(4097 * LIM) in msg
    _check(w, tiles[1:], {18: b}, "candidate limit")
    w.close()


# ---- snapshots and the refusals that need a context -------------------------------------------------------------------
def test_snapshots_later_registrations_and_refusals(tmp_path, gpu_ctx):
    rng = np.random.default_rng(109)
    st, pool = _random_styles(rng, 12)
    w = World(gpu_ctx, tmp_path / "p.bin", 40, (1, 3), None, st, pool, shared_nodes=False)
    ws, ms = _falling(rng, 40, 12, (1, 3, 1)), [[3], [7, 2]]
    b = w.bind(ws, ms)
    X, Y = CX // 8, CY // 8
    tiles = [(15, X, Y), (15, X + 1, Y), (16, CX // 4, CY // 4)]
    want, scene, twin = _check(w, tiles, {15: b, 16: b}, "snapshots", keep=True)
    assert _dedup_seen(w, b[1], tiles) >= 1
    before = gpu_ctx.render(scene).cpu().numpy()
    assert len(np.unique(before.reshape(-1, 4), axis=0)) > 20
    dl_before = scene.read_display_list()
    # later: more styles (a new style table on the device), bindings over them, another file with its own index
    st2, pool2 = _random_styles(rng, 6)
    first2 = gpu_ctx.register_styles(recs_of(st2), pool2)
    b2 = w.bind(_falling(rng, 40, 6, (3, 1, 1)), [[5, 0], [1]], first=first2)
    other = World(gpu_ctx, tmp_path / "p2.bin", 10, (1,), {(CX, CY): ([], [1, 2], [0])}, st2, pool2)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), before)
    _assert_same_list(scene.read_display_list(), dl_before)
    assert scene.read_styled_areas()[1].tobytes() == np.concatenate(want).tobytes()
    want2, _, _ = _check(w, tiles, {15: b2, 16: b2}, "snapshots")
    assert _dedup_seen(w, b2[1], tiles) >= 1
    assert np.concatenate(want2).tobytes() != np.concatenate(want).tobytes()
    _check(w, tiles, {15: b, 16: b2}, "snapshots")
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), before)
    scene.free()
    # a scene from another source has no derived batch
    n = C.c_size_t()
    assert lib.load().osmt_scene_read_styled_areas(gpu_ctx._h, twin._h, None, None, 0, C.byref(n)) == abi.INVALID_ARG
    twin.free()
    # one index per geodata id
    with pytest.raises(OsmtError, match="tile index already"):
        gpu_ctx.register_tile_index(w.gid, tq.index_of(w.refs))
    with pytest.raises(OsmtError, match="geodata id"):
        gpu_ctx.register_tile_index(10**6, tq.index_of(w.refs))
    with pytest.raises(OsmtError, match=r"ways\[0\]"):
        gpu_ctx.register_tile_index(gpu_ctx.register_geodata(geodata_of(other.r)), styled.TileIndex({(1, 1): ([10], [])}))

    # bindings: every rule that compares with the context's tables
    def bad_bindings(word, gid=w.gid, ws_=None, ms_=None):
        ws_ = [[w.first]] * 40 if ws_ is None else ws_
        ms_ = [[w.first]] * 2 if ms_ is None else ms_
        with pytest.raises(OsmtError, match=word) as e:
            gpu_ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, ws_, ms_))
        assert e.value.code == abi.INVALID_ARG

    gpu_ctx.register_style_bindings(styled.StyleBindings(w.gid, 0, 18, [[w.first]] * 40, [[w.first]] * 2))
    bad_bindings("geodata id", gid=10**6)
    bad_bindings(r"way_styles\[3\]", ws_=[[w.first]] * 3 + [[first2 + len(st2) + other.n_styles]] + [[w.first]] * 36)
    bad_bindings(r"multipolygon_styles\[1\]", ms_=[[w.first], [10**9]])
    sb = styled.StyleBindings(w.gid, 0, 18, [[w.first]] * 40, [[w.first]] * 2)
    sb.way_style_off[0] = 1
    d = sb.as_desc()
    L = lib.load()
    assert L.osmt_validate_style_bindings(C.byref(d), gpu_ctx._h) == abi.INVALID_ARG and "way_style_off[0]" in L.osmt_last_error().decode()
    sb.way_style_off[0], sb.way_style_off[5] = 0, 99
    assert L.osmt_validate_style_bindings(C.byref(d), gpu_ctx._h) == abi.INVALID_ARG and "way_style_off[6]" in L.osmt_last_error().decode()
    sb.way_style_off[5] = 5
    d.n_multipolygon_styles = 1  # the offsets end behind the pool
    assert L.osmt_validate_style_bindings(C.byref(d), gpu_ctx._h) == abi.INVALID_ARG and "multipolygon_style_off[2]" in L.osmt_last_error().decode()

    # tile batches
    def bad_batch(word, gid=w.gid, tl=tiles, bz=None, scale=1):
        tb = styled.TileBatch(gid, tl, {15: b[0], 16: b[0]} if bz is None else bz, scale=scale)
        bb = tb.as_batch()
        assert L.osmt_validate_tile_batch(C.byref(bb), gpu_ctx._h) == abi.INVALID_ARG and word in L.osmt_last_error().decode(), L.osmt_last_error()
        assert word in _refused(gpu_ctx, tb, abi.INVALID_ARG)

    no_index = gpu_ctx.register_geodata(geodata_of(other.r))
    low = w.bind([[0]] * 40, [[0]] * 2, 3, 15)
    bad_batch("geodata id", gid=10**6)
    bad_batch("no tile index", gid=no_index)
    bad_batch("zoom 16 has no bindings", bz={15: b[0]})
    bad_batch("is not registered", bz={15: b[0], 16: 10**6})
    bad_batch("belongs to geodata id", bz={15: b[0], 16: other.bind([[0]] * 10, [[0]])[0]})
    bad_batch("covers zooms 3..15", bz={15: low[0], 16: low[0]})
    bad_batch("zoom 19", tl=tiles + [(19, 0, 0)])
    bad_batch("outside", tl=tiles + [(15, 1 << 15, 0)])
    bad_batch("outside", tl=tiles + [(15, 0, 1 << 15)])
    bad_batch("scale", scale=abi.MAX_SCALE + 1)
    _check(w, tiles[:1], {15: low}, "snapshots")  # a zoom nobody asks for needs no bindings; the context builds on
    other.close()
    w.close()


# ---- pixels ---------------------------------------------------------------------------------------------------------
def test_pixels_and_points_of_a_big_and_a_small_batch(tmp_path, gpu_ctx):
    """The tiles are cut from a world of their own, not from the rectangle world: that one's ways share one pair of nodes (only
    their ids matter there) and would draw next to nothing.  Here every way is a square of its own and the index is what the
    file's writer derives from the geometry, so neighbouring tiles share ways as real data does."""
    rng = np.random.default_rng(110)
    st, pool = _random_styles(rng, 14)
    st[0]["has_fill_color"], st[1]["has_casing_color"], st[1]["has_casing_width"], st[1]["has_color"] = 1, 1, 1, 1
    pool = np.concatenate([pool, [5.0, 3.0]])
    st[2]["has_color"], st[2]["has_dashes"], st[2]["dashes_off"], st[2]["n_dashes"], st[2]["line_cap"] = 1, 1, len(pool) - 2, 2, abi.CAP_ROUND
    st[3]["has_color"], st[3]["line_cap"], st[3]["has_width"], st[3]["width"] = 1, abi.CAP_SQUARE, 1, 4.0
    w = World(gpu_ctx, tmp_path / "x.bin", 40, (1, 3), None, st, pool, shared_nodes=False)
    ws = _falling(rng, 40, 14, (1, 3, 1))
    for i in range(4):
        ws[i] = [i]
    b = w.bind(ws, [[0, 5], [1]])
    tiles = []
    for z, rx, ry in ((15, 1, 1), (16, 2, 2), (17, 3, 3)):
        f = 1 << (18 - z)
        tiles += [(z, CX // f + dx, CY // f + dy) for dx in range(-rx, rx + 1) for dy in range(-ry, ry + 1)]
    tiles = tiles[:70]
    assert len(tiles) == 70
    five = [tiles[4], tiles[0], tiles[20], tiles[4], tiles[40]]
    for batch, scale in ((tiles, 1), (five, 2), (five, 3), (five, 4)):
        want, scene, twin = _check(w, batch, {z: b for z in (15, 16, 17)}, "pixels", scale=scale, keep=True)
        px = gpu_ctx.render(scene).cpu().numpy()
        scene.check()
        assert np.array_equal(px, gpu_ctx.render(twin).cpu().numpy())
        assert len(np.unique(np.ascontiguousarray(px).view(np.uint32))) > 50  # distinct RGBA values
        pts = gpu_ctx.read_points(scene)
        assert len(pts) > 0 and np.array_equal(pts, gpu_ctx.read_points(twin))
        assert (scene.max_tile_ops() <= 128) == (twin.max_tile_ops() <= 128)
        assert _dedup_seen(w, b[1], batch[:5]) >= 3
        scene.free()
        twin.free()
    w.close()


# what each case asks for by construction: the share of its requested tiles that must have areas (rectangle: the empty
# neighbourhood, named in both batches; tiny indices: the index without tiles and one tile beside the lone index tile; item
# counts: the region without columns; area limit: one tile beside the full one; pixels: outer zoom-17 tiles beyond the geometry)
FLOORS = {"rectangle": 0.9, "edges": 1.0, "tiny indices": 0.7, "dedup": 1.0, "candidate counts": 0.9, "item counts": 0.75, "many tiles": 1.0,
          "area limit": 0.75, "candidate limit": 1.0, "snapshots": 1.0, "pixels": 0.6}
assert set(FLOORS) == set(CASES)


def test_the_cases_above_were_not_vacuous(tmp_path, gpu_ctx):
    """At least 90 % of the tiles requested in this file have areas, and every case keeps its own floor — from the mirror's
    output.  A case that has not run in this process (a selection by -k, --lf, a worker of its own) is run here first."""
    runs = {"rectangle": test_rectangle_holes_and_mixed_zooms, "edges": test_world_edges_and_corners, "tiny indices": test_indices_of_no_tile_and_of_one,
            "dedup": test_dedup_order_and_nothing_bound, "candidate counts": test_candidate_and_item_counts, "item counts": test_candidate_and_item_counts,
            "many tiles": test_more_tiles_than_one_block_in_any_order, "area limit": test_the_area_limit_of_a_tile,
            "candidate limit": test_the_candidate_limit_of_a_tile_and_of_a_batch, "snapshots": test_snapshots_later_registrations_and_refusals,
            "pixels": test_pixels_and_points_of_a_big_and_a_small_batch}
    for k, case in enumerate(CASES):
        if case not in _STATS:
            d = tmp_path / f"case{k}"
            d.mkdir()
            runs[case](d, gpu_ctx)
    for case in CASES:
        n, k = _STATS[case]
        assert n > 0 and k >= FLOORS[case] * n, (case, n, k)
    n, k = sum(v[0] for v in _STATS.values()), sum(v[1] for v in _STATS.values())
    assert n > 1000 and k >= 0.9 * n, (n, k, _STATS)
