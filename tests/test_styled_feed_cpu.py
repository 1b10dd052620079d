"""The host side of display lists built on the GPU (include/osmtile.h "display lists built on the GPU"): the helpers that fill
what a caller registers — osmt::style_rec_of (host/osmt_styled.hpp), osmt::GeodataDesc (host/osmt_geodata.hpp) — and the
three validations every registration / build runs first, none of which needs a device.  The build itself is checked on the
GPU in tests/test_gpu_styled_feed.py."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from tests._geodata import Reader, write_geodata
from tests import _styled_order_model as model
from tests._styled_feed import _center_tile, extreme_id_world, fill_only_styles, random_pairs, recs_of, shim
from tests.test_geodata_reader import _world
from tests.test_styled_builder import STYLE_DTYPE, _build_cpp, _lib, _random_styles


def _validate_styles(recs, pool, ctx=None):
    L = lib.load()
    recs = np.ascontiguousarray(recs, styled.STYLE_REC_DTYPE)
    pool = np.ascontiguousarray(pool, np.float64)
    rc = L.osmt_validate_styles(recs.ctypes.data_as(C.POINTER(abi.StyleRec)), len(recs), pool.ctypes.data_as(C.POINTER(C.c_double)), len(pool), ctx)
    return rc, L.osmt_last_error().decode()


def test_struct_layouts_match_the_header():
    s = shim().sf_sizeof
    assert s(0) == C.sizeof(abi.StyleRec) == styled.STYLE_REC_DTYPE.itemsize == 96
    assert s(1) == C.sizeof(abi.StyledArea) == styled.STYLED_AREA_DTYPE.itemsize == 8
    assert s(2) == C.sizeof(abi.StyledTile) == styled.STYLED_TILE_DTYPE.itemsize == 24
    assert s(3) == C.sizeof(abi.StyledBatch)
    assert s(4) == C.sizeof(abi.GeodataDesc)
    for k, name in ((10, "fill_image"), (11, "has_layer"), (12, "line_cap"), (13, "has_fill_image"), (14, "background_color")):
        assert s(k) == getattr(abi.StyleRec, name).offset == styled.STYLE_REC_DTYPE.fields[name][1], name
    assert s(20) == abi.StyledTile.area_off.offset == styled.STYLED_TILE_DTYPE.fields["area_off"][1]
    assert s(30) == abi.StyledBatch.geodata_id.offset
    assert s(40) == abi.GeodataDesc.multipolygon_polygons.offset
    for name in ("osmt_register_geodata", "osmt_register_styles", "osmt_scene_build_styled", "osmt_scene_read_display_list"):
        assert name in lib.EXPORTS and hasattr(lib.load(), name)


def test_style_rec_of_round_trip():
    """Style -> osmt_style_rec keeps every field the twin of test_styled_builder reads, on its random styles"""
    rng = np.random.default_rng(5)
    st, pool = _random_styles(rng, 60, n_images=3)
    out = np.zeros(len(st), styled.STYLE_REC_DTYPE)
    pool_out = np.zeros(len(pool) + 1, np.float64)
    n_pool = shim().sf_style_recs(st.ctypes.data, len(st), pool.ctypes.data, out.ctypes.data, pool_out.ctypes.data, len(pool_out))
    assert n_pool == len(pool) - 1  # (the test pool carries one spare entry at its end)
    seen = set()
    for a, b in zip(st, out):
        assert bool(a["has_layer"]) == bool(b["has_layer"]) and (not a["has_layer"] or a["layer"] == b["layer"])
        assert a["z_index"] == b["z_index"] and bool(a["is_foreground_fill"]) == bool(b["is_foreground_fill"])
        for key in ("color", "fill_color", "casing_color"):
            assert bool(a["has_" + key]) == bool(b["has_" + key])
            if a["has_" + key]:
                assert tuple(a[key]) == tuple(b[key])
        for key in ("opacity", "fill_opacity", "width", "casing_width"):
            assert bool(a["has_" + key]) == bool(b["has_" + key])
            if a["has_" + key]:
                assert a[key] == b[key]
        for key in ("dashes", "casing_dashes"):
            assert bool(a["has_" + key]) == bool(b["has_" + key])
            if a["has_" + key]:
                want = pool[a[key + "_off"] : a[key + "_off"] + a["n_" + key]]
                got = pool_out[b[key + "_off"] : b[key + "_off"] + b["n_" + key]]
                assert np.array_equal(want, got) and len(got) >= 1
                seen.add(key)
        assert a["line_cap"] == b["line_cap"] and a["casing_line_cap"] == b["casing_line_cap"]
        assert bool(a["has_fill_image"]) == bool(b["has_fill_image"]) and (not a["has_fill_image"] or a["fill_image"] == b["fill_image"])
        assert not b["has_background_color"] and b["_pad"] == 0
    assert seen == {"dashes", "casing_dashes"} and st["has_fill_image"].any() and st["has_layer"].any()
    # the field-by-field conversion the GPU tests use says the same, up to where the dash lists sit in the pool
    same = recs_of(st)
    for name in STYLE_DTYPE.names:
        if not name.endswith("_off"):
            assert np.array_equal(same[name], st[name]), name
    no_img = out.copy()
    no_img["has_fill_image"] = 0
    assert _validate_styles(no_img, pool_out[:n_pool])[0] == abi.OK


def test_geodata_desc_equals_the_reader(tmp_path, oracle):
    rng = np.random.default_rng(21)
    nodes, ways, polygons, multis = _world(oracle, rng, n_ways=40)
    p = str(tmp_path / "w.bin")
    write_geodata(p, nodes, ways, polygons, multis, max_zoom_tile=lambda a, b: oracle.coords_to_max_zoom_tile(a, b))
    r = Reader(p)
    S = shim()
    h = S.sf_desc_new(r.h)
    d = S.sf_desc_get(h).contents
    assert (d.n_nodes, d.n_ways, d.n_polygons, d.n_multipolygons) == (r.n_nodes, r.n_ways, r.n_polygons, r.n_multipolygons)
    arr = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].copy()
    assert np.array_equal(arr(d.nodes, 2 * d.n_nodes).reshape(-1, 2), r.node_table())
    woff, wn, wid = arr(d.way_node_off, d.n_ways + 1), arr(d.way_nodes, d.n_way_nodes), arr(d.way_ids, d.n_ways)
    poff, pn = arr(d.polygon_node_off, d.n_polygons + 1), arr(d.polygon_nodes, d.n_polygon_nodes)
    moff, mp, mid = arr(d.multipolygon_polygon_off, d.n_multipolygons + 1), arr(d.multipolygon_polygons, d.n_multipolygon_polygons), arr(d.multipolygon_ids, d.n_multipolygons)
    for i in range(r.n_ways):
        assert wid[i] == r.global_id(1, i) and wn[woff[i] : woff[i + 1]].tolist() == r.way_nodes(i)
    for i in range(r.n_polygons):
        assert pn[poff[i] : poff[i + 1]].tolist() == r.polygon_nodes(i)
    for i in range(r.n_multipolygons):
        assert mid[i] == r.global_id(2, i) and mp[moff[i] : moff[i + 1]].tolist() == r.multipolygon_polygons(i)
    assert r.multipolygon_polygons(r.n_multipolygons - 1) == []  # the relation without polygons is there, with an empty range
    L = lib.load()
    assert L.osmt_validate_geodata(S.sf_desc_get(h)) == abi.OK, L.osmt_last_error()
    S.sf_desc_free(h)
    r.close()


def _geo():
    nodes = [[55.75 + 0.001 * i, 37.61 + 0.001 * i] for i in range(6)]
    return styled.Geodata(nodes, ways=[(7, [0, 1, 2]), (8, [2, 3])], polygons=[[0, 1, 2, 0], [3, 4, 5, 3]], multipolygons=[(9, [0, 1])])


def _validate_geo(g):
    L = lib.load()
    d = g.as_desc()
    rc = L.osmt_validate_geodata(C.byref(d))
    return rc, L.osmt_last_error().decode()


def test_validate_geodata_refusals():
    assert _validate_geo(_geo())[0] == abi.OK
    cases = []

    def case(name, edit, word):
        g = _geo()
        edit(g)
        cases.append(name)
        rc, msg = _validate_geo(g)
        assert rc == abi.INVALID_ARG and word in msg, (name, rc, msg)

    case("first offset not 0", lambda g: g.way_node_off.__setitem__(0, 1), "way_node_off[0]")
    case("decreasing offsets", lambda g: g.polygon_node_off.__setitem__(1, 9), "polygon_node_off[2]")
    case("offsets that stop short", lambda g: g.multipolygon_polygon_off.__setitem__(1, 1), "multipolygon_polygon_off[1]")
    case("node index out of range", lambda g: g.way_nodes.__setitem__(4, 6), "way_nodes[4] = 6")
    case("polygon node out of range", lambda g: g.polygon_nodes.__setitem__(5, 77), "polygon_nodes[5] = 77")
    case("polygon index out of range", lambda g: g.multipolygon_polygons.__setitem__(1, 2), "multipolygon_polygons[1] = 2")
    case("node outside the Web-Mercator square", lambda g: g.nodes.__setitem__((3, 0), 89.0), "node 3")
    case("node not finite", lambda g: g.nodes.__setitem__((5, 1), np.nan), "node 5")
    assert len(cases) == 8


def _plain(n=1):
    st = np.zeros(n, styled.STYLE_REC_DTYPE)
    st["is_foreground_fill"], st["has_color"], st["has_width"], st["width"] = 1, 1, 1, 2.0
    return st


def test_validate_styles_refusals():
    pool = np.array([4.0, 2.0] + [1.0] * 17)
    assert _validate_styles(_plain(3), pool)[0] == abi.OK

    def refused(edit, code, word):
        st = _plain(3)
        edit(st[1])
        rc, msg = _validate_styles(st, pool)
        assert rc == code and "style 1" in msg and word in msg, (rc, msg)

    def set_(**kw):
        def f(s):
            for k, v in kw.items():
                s[k] = v
        return f

    refused(set_(z_index=np.nan), abi.INVALID_ARG, "z_index")
    refused(set_(has_opacity=1, opacity=-0.5), abi.INVALID_ARG, "opacity")
    refused(set_(has_fill_opacity=1, fill_opacity=2.0**53), abi.INVALID_ARG, "fill_opacity")
    refused(set_(has_opacity=1, opacity=np.nan), abi.INVALID_ARG, "opacity")
    refused(set_(width=np.inf), abi.INVALID_ARG, "width")
    refused(set_(has_casing_width=1, casing_width=1e308), abi.INVALID_ARG, "casing_width")  # finite, but not times OSMT_MAX_SCALE
    refused(set_(line_cap=4), abi.INVALID_ARG, "line_cap")
    refused(set_(casing_line_cap=9), abi.INVALID_ARG, "casing_line_cap")
    refused(set_(has_dashes=1, n_dashes=0), abi.INVALID_ARG, "empty dashes")
    refused(set_(has_casing_dashes=1, casing_dashes_off=2, n_casing_dashes=17), abi.UNSUPPORTED, "casing_dashes")
    refused(set_(has_dashes=1, dashes_off=18, n_dashes=2), abi.INVALID_ARG, "outside the pool")
    refused(set_(has_fill_image=1, fill_image=0), abi.INVALID_ARG, "fill_image 0 is not registered")  # no context: no icons
    # values behind a cleared has_* byte are not looked at
    st = _plain(2)
    st[1]["opacity"], st[1]["casing_width"], st[1]["n_dashes"], st[1]["fill_image"] = np.nan, np.inf, 99, 12345
    assert _validate_styles(st, pool)[0] == abi.OK


def test_a_garbage_layer_without_has_layer_is_accepted():
    st = _plain(2)
    st.view(np.uint8).reshape(2, -1)[1, :8] = 0xA5  # the bits of `layer`
    assert st[1]["has_layer"] == 0 and st[1]["layer"] != 0
    assert _validate_styles(st, np.zeros(1))[0] == abi.OK


def _validate_batch(sb, ctx=None):
    L = lib.load()
    b = sb.as_batch()
    rc = L.osmt_validate_styled_batch(C.byref(b), ctx)
    return rc, L.osmt_last_error().decode()


def test_validate_styled_batch_refusals_that_need_no_registration():
    """the batch's own shape is checked first; the ids are checked against the context's tables last (GPU tests)"""
    tiles = [(15, 1, 2, [(0, 0), (1, 0)], []), (15, 2, 2, [(0, 0)], [(0, 0)])]
    ok = styled.StyledBatch(0, tiles)
    rc, msg = _validate_batch(ok)
    assert rc == abi.INVALID_ARG and "geodata id 0 is not registered" in msg  # nothing else to object to
    for scale in (0, abi.MAX_SCALE + 1):
        rc, msg = _validate_batch(styled.StyledBatch(0, tiles, scale=scale))
        assert rc == abi.INVALID_ARG and "scale" in msg
    sb = styled.StyledBatch(0, tiles)
    sb.tiles["zoom"][1] = abi.MAX_ZOOM + 1
    rc, msg = _validate_batch(sb)
    assert rc == abi.INVALID_ARG and "tile 1" in msg and "zoom" in msg
    sb = styled.StyledBatch(0, tiles)
    sb.tiles["n_areas"][1] = 3
    rc, msg = _validate_batch(sb)
    assert rc == abi.INVALID_ARG and "tile 1" in msg and "out of bounds" in msg
    sb = styled.StyledBatch(0, tiles)
    sb.tiles["area_off"][1] = 1
    rc, msg = _validate_batch(sb)
    assert rc == abi.INVALID_ARG and "overlap" in msg
    sb = styled.StyledBatch(0, [(15, 1, 2, [(0, 0)] * (abi.STYLED_MAX_TILE_AREAS + 1), [])])
    rc, msg = _validate_batch(sb)
    assert rc == abi.UNSUPPORTED and "tile 0" in msg and "65537" in msg
    L = lib.load()
    assert L.osmt_validate_styled_batch(None, None) == abi.INVALID_ARG


@pytest.mark.parametrize("seed,n", [(41, abi.STYLED_MAX_TILE_AREAS), (42, 3001)])
def test_scene_builder_against_the_order_model(tmp_path, oracle, seed, n):
    """osmt::SceneBuilder, the yardstick of the GPU build, against a third statement of the order that shares no code with it
    (tests/_styled_order_model.py) — at the tile limit, where the Python twin is too slow to go, over global ids at both
    ends of 32, 63 and 64 bits, z-indices that include both zeros, 1e300 and the smallest denormal"""
    r = extreme_id_world(tmp_path, oracle)
    way_gids, mp_gids = model.gids(r)
    assert {0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 1} <= set(way_gids) and {2**63, 2**64 - 1} <= set(way_gids) & set(mp_gids)
    rng = np.random.default_rng(seed)
    st, pool = fill_only_styles(rng)
    assert len(st) == 200 and len({tuple(c) for c in st["fill_color"]}) == 200
    assert {0.0, 1.0, 2.5, -1.0, 1e300, 5e-324} <= set(st["z_index"].tolist()) and np.signbit(st["z_index"][st["z_index"] == 0.0]).any()
    n_w = int(0.8 * n)
    ways, mps = random_pairs(rng, n_w, r.n_ways, len(st)), random_pairs(rng, n - n_w, r.n_multipolygons, len(st))
    tx, ty = _center_tile(oracle)
    dl = _build_cpp(_lib(), r, [(15, tx, ty, ways, mps)], st, pool, 1, True)
    assert int(dl.jobs["n_ops"][0]) == n  # every entity has a ring, every style fills: one op per area
    want = model.expected_marks(ways, mps, st, way_gids, mp_gids, *model.first_nodes(r))
    assert np.array_equal(model.seen_marks(dl, 0), want)
    r.close()
