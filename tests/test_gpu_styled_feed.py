"""Display lists built on the GPU (osmt_scene_build_styled, osm_renderer_amd/csrc/osmt_styled.hip): registered geodata +
registered styles + 8 bytes per styled area in, an ordinary OSMT_COORD_NODE_REF scene out.

Two things that are not under test serve as the yardstick: osmt::SceneBuilder (host/osmt_styled.hpp, through
tests/styled_shim.cpp and _build_cpp) — the built list must equal its batch array for array, byte for byte — and the Python
twin _twin_areas / _twin_ops of tests/test_styled_builder.py, written from styler.rs:163-203,246-272 and drawer.rs:60-219."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from osm_renderer_amd.display_list import DisplayList
from osm_renderer_amd.lib import OsmtError
from tests._styled_feed import LAT0, LON0, CachedReader, _center_tile, _file, _square, geodata_of, recs_of
from tests.test_styled_builder import (STYLE_DTYPE, _build_cpp, _icons, _lib, _ops_of, _random_styles, _scene, _styled, _twin_areas,
                                       _twin_ops)

pytestmark = pytest.mark.gpu


def _batch(gid, tiles, first, scale=1, use_caps=True):
    shift = lambda pairs: [(i, s + first) for i, s in pairs]
    return styled.StyledBatch(gid, [(z, x, y, shift(w), shift(m)) for z, x, y, w, m in tiles], scale=scale, use_caps_for_dashes=use_caps)


def _assert_same_list(got, want):
    for name in ("jobs", "ops", "rings", "coords", "dashes"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


def _validates(dl):
    L = lib.load()
    b = dl.as_batch()
    return L.osmt_validate_batch(C.byref(b)), L.osmt_last_error().decode()


def _build_both(gpu_ctx, r, gid, tiles, st, pool, first, scale=1, use_caps=True):
    """(scene built on the GPU, its list read back, the list osmt::SceneBuilder makes of the same input)"""
    want = _build_cpp(_lib(), r, tiles, st, pool, scale, use_caps)
    scene = gpu_ctx.build_styled(_batch(gid, tiles, first, scale, use_caps))
    return scene, scene.read_display_list(), want


@pytest.mark.parametrize("seed,n_ways,scale,use_caps,with_oracle", [(13, 80, 1, True, True), (14, 50, 2, False, False),
                                                                    (13, 80, 3, True, True), (14, 50, 4, False, False)])
def test_built_list_equals_the_scene_builders_bit_for_bit(tmp_path, gpu_ctx, oracle, seed, n_ways, scale, use_caps, with_oracle):
    r, rng = _scene(tmp_path, oracle, seed, n_ways=n_ways)
    st, pool = _random_styles(rng, 16 if with_oracle else 12, n_images=2)
    icons = _icons(rng)
    first_img = [gpu_ctx.register_image(im) for im in icons][0]
    st["fill_image"] += first_img
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    tiles = []
    for zoom, dx in ((15, 0), (15, 1), (16, 0), (14, 0))[: 4 if with_oracle else 2]:
        tx, ty = _center_tile(oracle, zoom, dx)
        _, way_ids, mp_ids = r.query(zoom, tx, ty, neighbours=True)
        tiles.append((zoom, tx, ty, _styled(rng, way_ids, len(st)), _styled(rng, mp_ids, len(st))))
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first, scale, use_caps)
    assert len(want.ops) > 100 and len(want.dashes) > 0 and (want.ops["kind"] == abi.OP_FILL_IMAGE).any()
    _assert_same_list(got, want)
    assert _validates(got)[0] == abi.OK
    again = gpu_ctx.build_styled(_batch(gid, tiles, first, scale, use_caps))
    _assert_same_list(again.read_display_list(), got)
    again.free()
    # same pixels as the host-built list through the host-buffer entry
    px = gpu_ctx.render(scene).cpu().numpy()
    scene.check()
    assert np.array_equal(px, gpu_ctx.render_batch_host(want))
    assert len(np.unique(np.ascontiguousarray(px).view(np.uint32))) > 100  # distinct RGBA values
    if with_oracle:
        dl_o = DisplayList(want.jobs, want.ops.copy(), want.rings, want.coords, want.dashes, abi.COORD_NODE_REF, scale, nodes=want.nodes)
        dl_o.ops["image_id"] -= first_img  # the oracle's icon list starts at 0
        assert np.array_equal(px, oracle.render_batch(dl_o, images=icons, threads=4))
    # the projected points of the built scene are those of the uploaded host-built list (both scenes rendered: a scene's
    # points are written by the projection stage of a render)
    twin = gpu_ctx.upload(want)
    assert np.array_equal(gpu_ctx.render(twin).cpu().numpy(), px)
    pts = gpu_ctx.read_points(scene)
    assert len(pts) == len(want.coords) and np.array_equal(pts, gpu_ctx.read_points(twin))
    twin.free()
    scene.free()
    r.close()


def test_order_one_rule_at_a_time(tmp_path, gpu_ctx, oracle):
    """compare_styled_entities and the merge of style_areas, each rule where nothing else decides, against the twin"""
    nodes = []

    def node(lat, lon):
        nodes.append((1000 + len(nodes), lat, lon, {}))
        return len(nodes) - 1

    HI = 1 << 32
    way_gids = [100, 101, 5, HI + 5, 2 * HI + 5, 777, 50, 3 * HI]
    ways = [(g, _square(node, k), {}) for k, g in enumerate(way_gids)]
    polygons = [_square(node, 8 + k) for k in range(3)]
    multis = [(777, [0], {}), (60, [1, 2], {})]  # relation 0 has the global id of way 5
    r = _file(tmp_path, oracle, nodes, ways, polygons, multis)
    st = np.zeros(12, STYLE_DTYPE)
    st["has_fill_color"], st["is_foreground_fill"], st["z_index"] = 1, 1, 3.0
    for k in range(len(st)):
        st[k]["fill_color"] = (10 * k, 255 - 10 * k, k)
    st[1]["z_index"], st[2]["z_index"] = 0.0, -0.0  # tie: falls through to the global id
    st[3]["z_index"], st[4]["z_index"], st[5]["z_index"] = -1e300, 1e300, -5.0
    st[6]["has_layer"], st[6]["layer"], st[6]["z_index"] = 1, np.iinfo(np.int64).min, 99.0
    st[7]["has_layer"], st[7]["layer"], st[7]["z_index"] = 1, np.iinfo(np.int64).max, -99.0
    st[8]["is_foreground_fill"], st[8]["z_index"] = 0, 50.0  # a background fill goes before every foreground one of its layer
    st[9]["has_layer"], st[9]["layer"], st[9]["z_index"] = 1, -1, 100.0
    st[10]["layer"] = 12345  # has_layer == 0: the key of style 0, another colour — input order decides between them
    # st[11]: the key of style 0 again
    pool = np.zeros(1)
    way_pairs = [(0, 0), (1, 0), (0, 4), (1, 3), (2, 5), (3, 7), (4, 6), (0, 8), (1, 9),  # layer > fill position > z-index > id
                 (1, 1), (0, 2), (0, 1), (1, 2),  # +0.0 against -0.0
                 (4, 0), (3, 0), (2, 0), (7, 0),  # ids that differ only above bit 32
                 (5, 0), (5, 11),  # way 5 and relation 0: same global id, equal styles
                 (6, 0), (6, 10), (6, 11), (6, 0), (6, 0)]  # equal keys on one entity keep input order; one pair three times
    mp_pairs = [(1, 0), (0, 11), (0, 0), (1, 8), (0, 7)]
    tx, ty = _center_tile(oracle)
    tiles = [(15, tx, ty, way_pairs, mp_pairs)]
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first)
    cr = CachedReader(r)
    twin = _twin_ops(cr, st, pool, _twin_areas(cr, st, way_pairs, mp_pairs, False), 1.0, True)
    assert _ops_of(got) == twin and len(twin) == len(way_pairs) + len(mp_pairs)
    _assert_same_list(got, want)
    # the relation goes first where it compares Equal to a way (styler.rs:186): relation 0 / style 0 sits right in front of
    # way 5 / style 0, and relation 0 / style 11 is in front of way 5 / style 11 too
    colours = [op[1] for op in _ops_of(got)]
    rings = [op[6] for op in _ops_of(got)]
    c0, way5, rel0 = tuple(st[0]["fill_color"]), [cr.way_nodes(5)], [cr.polygon_nodes(0)]
    i_rel = next(i for i, (c, rr) in enumerate(zip(colours, rings)) if c == c0 and rr == rel0)
    i_way = next(i for i, (c, rr) in enumerate(zip(colours, rings)) if c == c0 and rr == way5)
    assert i_rel < i_way
    # layer i64::MIN first, i64::MAX last
    assert colours[0] == tuple(st[6]["fill_color"]) and colours[-1] == tuple(st[7]["fill_color"])
    scene.free()
    r.close()


def _small_world(tmp_path, oracle):
    nodes = []

    def node(lat, lon):
        nodes.append((1000 + len(nodes), lat, lon, {}))
        return len(nodes) - 1

    ways = [(5000 + 3 * k, _square(node, k), {}) for k in range(6)]
    ways += [(6000 + k, _square(node, k + 1)[:3], {}) for k in range(4)]  # open ways of three nodes
    polygons = [_square(node, 2 + k, size=0.0008) for k in range(3)]
    multis = [(5003, [0, 1], {}), (9001, [2], {})]  # relation 0 shares the global id of way 1
    return _file(tmp_path, oracle, nodes, ways, polygons, multis)


def _cycled_tile(rng, zoom, tx, ty, n, n_ways, n_mps, n_styles):
    kinds = rng.random(n) < 0.8
    ways = [(int(rng.integers(0, n_ways)), int(rng.integers(0, n_styles))) for _ in range(int(kinds.sum()))]
    mps = [(int(rng.integers(0, n_mps)), int(rng.integers(0, n_styles))) for _ in range(n - len(ways))]
    return (zoom, tx, ty, ways, mps)


def test_sizes_where_a_sort_or_a_scan_can_go_wrong(tmp_path, gpu_ctx, oracle):
    """tiles without areas at the front, in the middle and at the end; one wave and one more; the LDS tier's limit and one
    more; the areas of a tile far apart in the caller's array"""
    r = _small_world(tmp_path, oracle)
    rng = np.random.default_rng(31)
    st, pool = _random_styles(rng, 8)
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    tx, ty = _center_tile(oracle)
    LDS = abi.STYLED_LDS_AREAS
    counts = [0, 1, 63, 0, 64, 65, LDS - 1, 0, 0, LDS, LDS + 1, 0]
    tiles = [_cycled_tile(rng, 15, tx + (k % 2), ty, n, 10, 2, len(st)) for k, n in enumerate(counts)]
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first)
    assert [int(n) for n in got.jobs["n_ops"]][0] == 0 and int(got.jobs["n_ops"][-1]) == 0 and int(got.jobs["n_ops"].max()) > LDS
    _assert_same_list(got, want)
    assert _validates(got)[0] == abi.OK
    scene.free()
    # the same tiles listed in another order than their areas lie in the array, with a gap nobody names
    sb = _batch(gid, tiles, first)
    sb.areas = np.concatenate([np.zeros(5, styled.STYLED_AREA_DTYPE), sb.areas])
    sb.areas[:5]["style"] = 0xFFFFFFFF  # never read
    sb.tiles["area_off"] += 5
    order = [5, 0, 10, 2, 1, 9, 3, 4, 11, 6, 7, 8]
    sb.tiles = sb.tiles[order].copy()
    scene = gpu_ctx.build_styled(sb)
    _assert_same_list(scene.read_display_list(), _build_cpp(_lib(), r, [tiles[k] for k in order], st, pool, 1, True))
    scene.free()
    # small enough to draw: empty tiles around drawn ones give the canvas, drawn ones the pixels of the host-built list
    few = [tiles[k] for k in (0, 1, 3, 4, 11)]
    scene, got, want = _build_both(gpu_ctx, r, gid, few, st, pool, first, scale=2)
    _assert_same_list(got, want)
    px = gpu_ctx.render(scene).cpu().numpy()
    scene.check()
    assert np.array_equal(px, gpu_ctx.render_batch_host(want))
    assert (px[0] == np.array([241, 238, 232, 255], np.uint8)).all() and (px[4] == px[0]).all() and not (px[3] == px[0]).all()
    scene.free()
    r.close()


def test_a_big_tile_of_ties_and_the_area_limit(tmp_path, gpu_ctx, oracle):
    """four times the LDS limit with three distinct keys: the device-memory tier orders by input position alone"""
    r = _small_world(tmp_path, oracle)
    rng = np.random.default_rng(37)
    st = np.zeros(2, STYLE_DTYPE)
    st["has_fill_color"], st["is_foreground_fill"], st["z_index"] = 1, 1, 1.0
    st["has_color"], st["has_width"], st["width"] = 1, 1, 1.5
    st[0]["fill_color"], st[1]["fill_color"], st[1]["z_index"] = (9, 9, 9), (200, 0, 0), 0.5
    st[1]["has_dashes"], st[1]["dashes_off"], st[1]["n_dashes"] = 1, 0, 2
    pool = np.array([3.0, 1.0, 0.0])
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    tx, ty = _center_tile(oracle)
    n = 4 * abi.STYLED_LDS_AREAS + 3
    keys = [(0, 0), (1, 0), (0, 1)]
    way_pairs = [keys[int(k)] for k in rng.integers(0, 3, n)]
    tiles = [(15, tx, ty, way_pairs[:70], []), (15, tx, ty, way_pairs, []), (15, tx + 1, ty, [(2, 1)], [(0, 0)])]
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first)
    _assert_same_list(got, want)
    cr = CachedReader(r)
    assert _ops_of(got, 1) == _twin_ops(cr, st, pool, _twin_areas(cr, st, way_pairs, [], False), 1.0, True)
    assert int(got.jobs["n_ops"][1]) == 2 * n
    scene.free()
    # one area more than a tile may have: refused, and no scene comes back
    sb = _batch(gid, [(15, tx, ty, [(0, 0)] * (abi.STYLED_MAX_TILE_AREAS + 1), [])], first)
    b, h = sb.as_batch(), C.c_void_p()
    rc = lib.load().osmt_scene_build_styled(gpu_ctx._h, C.byref(b), C.byref(h))
    assert rc == abi.UNSUPPORTED and not h.value and "65537" in lib.load().osmt_last_error().decode()
    r.close()


def test_emission_corners(tmp_path, gpu_ctx, oracle):
    nodes = []

    def node(lat, lon):
        nodes.append((1000 + len(nodes), lat, lon, {}))
        return len(nodes) - 1

    def zigzag(n, k):  # an open way of n nodes across the centre tile
        return [node(LAT0 - 0.003 + 0.00005 * i, LON0 - 0.004 + 0.0007 * k + (0.0004 if i % 2 else 0.0)) for i in range(n)]

    ways = [(7000, [], {}), (7001, [node(LAT0, LON0)], {}), (7002, zigzag(2, 0), {}), (7003, zigzag(65, 1), {}), (7004, zigzag(66, 2), {}),
            (7005, zigzag(130, 3), {}), (7006, _square(node, 6, size=0.001), {})]
    polygons = [_square(node, 2, size=0.0012), [node(LAT0, LON0)], _square(node, 4, size=0.0009), zigzag(70, 5) + [0]]
    polygons[3][-1] = polygons[3][0]  # a closed polygon of 71 nodes: a fill op with a block table
    multis = [(8000, [], {}), (8001, [0, 1, 2], {}), (8002, [1], {}), (8003, [3], {})]
    r = _file(tmp_path, oracle, nodes, ways, polygons, multis)
    st = np.zeros(7, STYLE_DTYPE)
    st["is_foreground_fill"], st["z_index"] = 1, 1.0
    pool = np.array([float(1 + (k % 5)) for k in range(16)] + [6.0, 2.0, 0.0])
    # 0: draws nothing (a casing colour without a width, a width without a colour)
    st[0]["has_casing_color"], st[0]["has_width"], st[0]["width"] = 1, 1, 3.0
    # 1: fill + casing + stroke: the way's refs appear three times
    st[1]["has_fill_color"], st[1]["fill_color"], st[1]["has_fill_opacity"], st[1]["fill_opacity"] = 1, (120, 200, 90), 1, 0.6
    st[1]["has_casing_color"], st[1]["casing_color"], st[1]["has_casing_width"], st[1]["casing_width"] = 1, (20, 20, 60), 1, 5.0
    st[1]["has_color"], st[1]["color"], st[1]["has_width"], st[1]["width"], st[1]["line_cap"] = 1, (250, 250, 0), 1, 2.0, abi.CAP_ROUND
    # 2: a stroke with 16 dashes and square caps
    st[2]["has_color"], st[2]["color"], st[2]["has_width"], st[2]["width"], st[2]["line_cap"] = 1, (200, 0, 0), 1, 3.0, abi.CAP_SQUARE
    st[2]["has_dashes"], st[2]["dashes_off"], st[2]["n_dashes"], st[2]["has_opacity"], st[2]["opacity"] = 1, 0, 16, 1, 0.8
    # 3: casing_dashes without dashes
    st[3]["has_casing_color"], st[3]["casing_color"], st[3]["has_casing_width"], st[3]["casing_width"] = 1, (0, 90, 200), 1, 4.0
    st[3]["has_casing_dashes"], st[3]["casing_dashes_off"], st[3]["n_casing_dashes"], st[3]["casing_line_cap"] = 1, 16, 2, abi.CAP_BUTT
    st[3]["has_color"], st[3]["color"] = 1, (255, 255, 255)  # width None: 1.0
    # 4: a plain fill; 5: a stroke without caps; 6: a background fill
    st[4]["has_fill_color"], st[4]["fill_color"] = 1, (90, 90, 200)
    st[5]["has_color"], st[5]["color"], st[5]["has_width"], st[5]["width"] = 1, (0, 0, 0), 1, 1.25
    st[6]["has_fill_color"], st[6]["fill_color"], st[6]["is_foreground_fill"] = 1, (230, 230, 200), 0
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    tx, ty = _center_tile(oracle)
    way_pairs = [(w, s) for w in range(len(ways)) for s in (0, 1, 2, 3, 5)]
    mp_pairs = [(m, s) for m in range(len(multis)) for s in (0, 4, 6, 1)]
    tiles = [(15, tx, ty, way_pairs, mp_pairs), (15, tx, ty, [(0, 2), (1, 3)], [(0, 4), (2, 4)])]  # the second: dashes, and no op at all
    for scale, use_caps in ((1, True), (2, False)):
        scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first, scale, use_caps)
        _assert_same_list(got, want)
        assert _validates(got)[0] == abi.OK
        cr = CachedReader(r)
        assert _ops_of(got, 0) == _twin_ops(cr, st, pool, _twin_areas(cr, st, way_pairs, mp_pairs, False), float(scale), use_caps)
        # the trap: a dashed stroke of a way without a usable ring leaves its dashes in the pool and emits no op
        assert int(got.jobs["n_ops"][1]) == 0 and int(got.jobs["n_pts"][1]) == 0
        used = sum(int(op["n_dashes"]) for op in got.ops)
        assert len(got.dashes) == used + 2 * (16 + 2) + (16 + 2) and len(got.dashes) > used
        assert sorted(set(int(x) for x in got.rings["n_pts"])) == [2, 5, 65, 66, 71, 130]
        px = gpu_ctx.render(scene).cpu().numpy()
        scene.check()
        assert np.array_equal(px, gpu_ctx.render_batch_host(want))
        assert len(np.unique(px[0].reshape(-1, 4), axis=0)) > 50 and (px[1] == np.array([241, 238, 232, 255], np.uint8)).all()
        scene.free()
    r.close()


def test_neighbours_labels_later_registrations_and_refusals(tmp_path, gpu_ctx, oracle):
    r, rng = _scene(tmp_path, oracle, 17, n_ways=40)
    st, pool = _random_styles(rng, 10)
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    tiles = []
    for dx in (0, 1):
        tx, ty = _center_tile(oracle, 15, dx)
        _, way_ids, mp_ids = r.query(15, tx, ty, neighbours=True)
        tiles.append((15, tx, ty, _styled(rng, way_ids, len(st)), _styled(rng, mp_ids, len(st))))
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first)
    _assert_same_list(got, want)
    before = gpu_ctx.render(scene).cpu().numpy()
    # the label pass of a built scene is the label pass of the uploaded twin scene
    ll = labels.make_labels(2, labels_per_tile=12, seed=4)
    twin = gpu_ctx.upload(want, ll)
    scene.set_labels(ll)
    a, b = gpu_ctx.render(scene).cpu().numpy(), gpu_ctx.render(twin).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, before)
    assert np.array_equal(scene.label_status(), twin.label_status()) and scene.label_status().any()
    scene.set_labels(None)
    twin.free()
    # later registrations — more styles (a new style table on the device), a second geodata file — do not disturb the scene
    st2, pool2 = _random_styles(rng, 5)
    first2 = gpu_ctx.register_styles(recs_of(st2), pool2)
    r2 = _small_world(tmp_path, oracle)
    gid2 = gpu_ctx.register_geodata(geodata_of(r2))
    assert first2 == first + len(st) and gid2 == gid + 1
    other = gpu_ctx.build_styled(_batch(gid2, [(15, tiles[0][1], tiles[0][2], [(0, 1), (7, 2)], [(1, 0)])], first2))
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), before)
    _assert_same_list(scene.read_display_list(), want)
    _assert_same_list(other.read_display_list(), _build_cpp(_lib(), r2, [(15, tiles[0][1], tiles[0][2], [(0, 1), (7, 2)], [(1, 0)])], st2, pool2, 1, True))
    other.free()
    scene.free()

    # every refusal of osmt_validate_styled_batch comes out of the build as well, and no scene with it
    def refused(edit, word, code=abi.INVALID_ARG, scale=1):
        sb = _batch(gid, tiles, first, scale=scale)
        edit(sb)
        L, b, h = lib.load(), sb.as_batch(), C.c_void_p(1)
        assert L.osmt_validate_styled_batch(C.byref(b), gpu_ctx._h) == code and word in L.osmt_last_error().decode()
        assert L.osmt_scene_build_styled(gpu_ctx._h, C.byref(b), C.byref(h)) == code and word in L.osmt_last_error().decode()
        assert not h.value
        with pytest.raises(OsmtError):
            gpu_ctx.build_styled(sb)

    refused(lambda sb: setattr(sb, "geodata_id", gid2 + 1), "geodata id")
    refused(lambda sb: sb.areas["entity"].__setitem__(3, r.n_ways), "way")
    refused(lambda sb: sb.areas["entity"].__setitem__(4, abi.STYLED_MULTIPOLYGON | r.n_multipolygons), "multipolygon")
    refused(lambda sb: sb.areas["style"].__setitem__(5, first2 + len(st2)), "style")
    refused(lambda sb: sb.tiles["zoom"].__setitem__(1, abi.MAX_ZOOM + 1), "zoom")
    refused(lambda sb: None, "scale", scale=abi.MAX_SCALE + 1)
    refused(lambda sb: sb.tiles["area_off"].__setitem__(1, 2), "overlap")
    refused(lambda sb: sb.tiles["n_areas"].__setitem__(1, len(sb.areas)), "out of bounds")
    # a style that would make an op osmt_validate_batch refuses is stopped at registration, with the context's icons known
    bad = recs_of(st[:1])
    bad["has_fill_image"], bad["fill_image"] = 1, 10**6
    with pytest.raises(OsmtError, match="fill_image"):
        gpu_ctx.register_styles(bad, pool)
    r.close()
    r2.close()
