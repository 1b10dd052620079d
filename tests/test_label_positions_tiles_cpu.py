"""Label anchors from tile coordinates, the host half: the validators that need no context, osmt::mercator_factors and
osmt::label_rings_of (osm_renderer_amd/host) against Python restatements and against the oracle's projection, and the mirror
in a stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import math
import subprocess

import numpy as np

from osm_renderer_amd import abi, labels, lib, styled
from tests import _anchors as A

MP = abi.STYLED_MULTIPOLYGON


def _err():
    return lib.load().osmt_last_error().decode()


def test_exports_and_layouts():
    L = lib.load()
    for name in ("osmt_validate_node_mercator", "osmt_register_node_mercator", "osmt_validate_label_tile_batch", "osmt_label_positions_tiles",
                 "osmt_label_positions_tiles_begin", "osmt_label_tile_batch_expand"):
        assert name in lib.EXPORTS and hasattr(L, name)
    s = A.shim().an_sizeof
    assert s(0) == C.sizeof(abi.LabelTileRequest) == labels.LABEL_TILE_REQUEST_DTYPE.itemsize == 8
    assert s(1) == C.sizeof(abi.LabelTileBatch) == 40
    assert s(2) == C.sizeof(abi.QueryTile) == styled.QUERY_TILE_DTYPE.itemsize == 16


def test_validate_node_mercator_without_a_context():
    L = lib.load()
    dp = C.POINTER(C.c_double)
    assert L.osmt_validate_node_mercator(None, 3, 0, None) == abi.INVALID_ARG and "NULL" in _err()
    good = np.array([[0.0, 1.0], [0.5, 0.25], [1.0, 0.0]])
    # everything about the table itself passes; what is left is the geodata id, which a NULL context does not have
    assert L.osmt_validate_node_mercator(good.ctypes.data_as(dp), 3, 0, None) == abi.INVALID_ARG and "not registered" in _err()
    for bad, where in ((np.nan, "node 1: x"), (np.inf, "node 1: x"), (-np.inf, "node 1: x"), (-1e-300, "node 1: x"), (np.nextafter(1.0, 2.0), "node 1: x")):
        f = good.copy()
        f[1, 0] = bad
        assert L.osmt_validate_node_mercator(f.ctypes.data_as(dp), 3, 0, None) == abi.INVALID_ARG
        assert where in _err() and "[0, 1]" in _err(), _err()
    f = good.copy()
    f[2, 1] = 1.5
    assert L.osmt_validate_node_mercator(f.ctypes.data_as(dp), 3, 0, None) == abi.INVALID_ARG and "node 2: y" in _err()


def _batch(tiles, requests, scale=1, geodata_id=0):
    t = np.zeros(len(tiles), styled.QUERY_TILE_DTYPE)
    for rec, (zoom, x, y) in zip(t, tiles):
        rec["zoom"], rec["x"], rec["y"] = zoom, x, y
    r = np.array(requests, dtype=labels.LABEL_TILE_REQUEST_DTYPE).reshape(-1)
    b = abi.LabelTileBatch(requests=r.ctypes.data_as(C.POINTER(abi.LabelTileRequest)) if len(r) else None, n_requests=len(r),
                           tiles=t.ctypes.data_as(C.POINTER(abi.QueryTile)) if len(t) else None, n_tiles=len(t), geodata_id=geodata_id, scale=scale)
    return b, (t, r)


def test_validate_label_tile_batch_without_a_context():
    L = lib.load()
    v = L.osmt_validate_label_tile_batch
    assert v(None, None) == abi.INVALID_ARG
    b, _k = _batch([(15, 3, 4)], [(0, 0)])
    assert v(C.byref(b), None) == abi.INVALID_ARG and "not registered" in _err()  # all that a context-free check can pass
    b, _k = _batch([(15, 3, 4)], [(0, 0)])
    b.requests = None
    assert v(C.byref(b), None) == abi.INVALID_ARG and "NULL pool" in _err()
    b, _k = _batch([(15, 3, 4)], [(0, 0)])
    b.tiles = None
    assert v(C.byref(b), None) == abi.INVALID_ARG and "NULL pool" in _err()
    for scale in (0, 5, 0xFFFFFFFF):
        b, _k = _batch([(15, 3, 4)], [(0, 0)], scale=scale)
        assert v(C.byref(b), None) == abi.INVALID_ARG and "scale" in _err()
    for tile, what in (((19, 0, 0), "zoom"), ((18, 1 << 18, 0), "outside zoom"), ((18, 0, 1 << 18), "outside zoom"), ((0, 1, 0), "outside zoom"),
                       ((0, 0, 1), "outside zoom"), ((15, 0xFFFFFFFF, 0), "outside zoom")):
        b, _k = _batch([(15, 3, 4), tile], [(0, 0)])
        assert v(C.byref(b), None) == abi.INVALID_ARG and "tile 1" in _err() and what in _err(), (tile, _err())
    for t in (1, 2, 0xFFFFFFFF):
        b, _k = _batch([(15, 3, 4)], [(0, 0), (0, t)])
        assert v(C.byref(b), None) == abi.INVALID_ARG and "request 1" in _err() and "not a tile" in _err()
    # no tiles at all: any request's tile index is out of range
    b, _k = _batch([], [(0, 0)])
    assert v(C.byref(b), None) == abi.INVALID_ARG and "not a tile" in _err()


def test_mercator_factors_equal_the_python_restatement():
    rng = np.random.default_rng(5)
    ll = np.stack([rng.uniform(-85.05, 85.05, 4000), rng.uniform(-180.0, 180.0, 4000)], 1)
    ll[:6] = [[0.0, 0.0], [85.05, 180.0], [-85.05, -180.0], [0.0, 180.0], [-0.0, -0.0], [55.75, 37.61]]
    got = A.mercator_factors(ll)
    want = np.array([A.py_factors(la, lo) for la, lo in ll])
    assert np.array_equal(A.bits(got), A.bits(want))
    assert (got >= 0.0).all() and (got <= 1.0).all()  # the domain the registration admits
    assert got[3, 0] == 1.0 and got[2, 0] == 0.0


def _small_world():
    w = A.World()
    rng = np.random.default_rng(9)
    ways = [w.way(w.shape(rng.uniform(-300, 600, (n, 2)))) for n in (0, 1, 2, 7, 65)]
    p_empty, p_one = w.polygon([]), w.polygon(w.shape([[5.5, 6.5]]))
    p_a, p_b = w.polygon(w.shape(rng.uniform(0, 256, (5, 2)))), w.polygon(w.shape(rng.uniform(0, 256, (70, 2))))
    mps = [w.mp([p_a]), w.mp([p_empty, p_a]), w.mp([p_a, p_one, p_b]), w.mp([])]
    return w.geodata(), ways, mps


def _tiles_of_zooms():
    tx, ty = A.T18
    return [(0, 0, 0), (10, tx >> 8, ty >> 8), (15, tx >> 3, ty >> 3), (18, tx, ty), (18, 0, 0), (18, (1 << 18) - 1, (1 << 18) - 1)]


def test_label_rings_of_equals_the_python_restatement():
    g, ways, mps = _small_world()
    f = A.mercator_factors(g.nodes)
    for zoom, x, y in _tiles_of_zooms():
        for scale in (1, 2, 4):
            for e in ways + mps:
                ring_n, pts = A.label_rings(g, f, e, zoom, x, y, scale)
                nodes = A.entity_rings(g, e)
                assert ring_n.tolist() == [len(r) for r in nodes]  # ALL polygons, the empty and the one-node ones too
                flat = [n for r in nodes for n in r]
                want = np.array([A.py_project(A.py_factors(*g.nodes[n]), zoom, x, y, scale) for n in flat]).reshape(-1, 2)
                assert np.array_equal(A.bits(pts), A.bits(want)), (zoom, scale, e)
                assert np.array_equal(A.bits(pts), A.bits(A.np_project(f[flat], zoom, x, y, scale)))  # the yardstick of the GPU tests
                assert (np.abs(pts) <= 2.0 ** 28).all()
    assert A.label_rings(g, f, len(ways), 15, 1, 1, 1) is None and A.label_rings(g, f, len(mps) | MP, 15, 1, 1, 1) is None


def test_factor_projection_equals_the_whole_formula_in_every_bit():
    """what the feature rests on: splitting coords_to_xy behind the division by 2 PI changes no bit of nodes_to_points"""
    rng = np.random.default_rng(21)
    for zoom, x, y in _tiles_of_zooms():
        ll = np.stack([rng.uniform(-85.0, 85.0, 500), rng.uniform(-180.0, 180.0, 500)], 1)
        f = A.mercator_factors(ll)
        dim = float(256 * (1 << zoom))
        for scale in (1, 2, 4):
            got = A.np_project(f, zoom, x, y, scale)
            for (la, lo), p in zip(ll, got):
                lat_rad, lon_rad = la * (math.pi / 180.0), lo * (math.pi / 180.0)
                xx, yy = lon_rad + math.pi, math.pi - math.log(math.tan((math.pi / 4.0) + (lat_rad / 2.0)))
                wx = ((xx / (2.0 * math.pi)) * dim - float(x * 256)) * float(scale)
                wy = ((yy / (2.0 * math.pi)) * dim - float(y * 256)) * float(scale)
                assert (p[0], p[1]) == (wx, wy)


def test_rounded_mirror_points_equal_the_oracle_projection(oracle):
    """both sides use the host's libm: Point::from_node is round() of what nodes_to_points leaves unrounded"""
    rng = np.random.default_rng(33)
    tx, ty = A.T18
    for zoom, x, y in _tiles_of_zooms():
        n = 1 << zoom
        # around the tile where that keeps the i32 conversion in range; anywhere for the small zooms
        if zoom >= 10:
            ll = np.array([A.latlon_of_px(px, py, ((x << (18 - zoom)), (y << (18 - zoom)))) for px, py in rng.uniform(-600, 900, (400, 2)) * (1 << (18 - zoom))])
            ll[:, 0], ll[:, 1] = np.clip(ll[:, 0], -85.0, 85.0), np.clip(ll[:, 1], -180.0, 180.0)
        else:
            ll = np.stack([rng.uniform(-85.0, 85.0, 400), rng.uniform(-180.0, 180.0, 400)], 1)
        f = A.mercator_factors(ll)
        for scale in (1, 2, 4):
            got = A.round_half_away(A.np_project(f, zoom, x, y, scale))
            want = oracle.project_points(ll, zoom, x, y, float(scale))
            assert np.array_equal(got, want.astype(np.int64)), (zoom, scale, n, tx, ty)


def test_mirror_position_over_tile_requests_matches_the_point_form():
    """get_label_position over label_rings_of is the mirror of the point form fed the same points"""
    from tests import _polylabel_shim as S

    w = A.World()
    sq = w.way(w.shape([[10.5, 20.25], [50.5, 20.25], [50.5, 60.25], [10.5, 60.25], [10.5, 20.25]]))
    empty = w.way([])
    g = w.geodata()
    f = A.mercator_factors(g.nodes)
    tx, ty = A.T18
    for scale in (1, 2, 4):
        tiles = [(18, tx, ty), (15, tx >> 3, ty >> 3)]
        reqs = [(sq, 0), (sq, 1), (empty, 0)]
        rings, pts = A.expected_expansion(g, f, tiles, reqs, scale)
        want, _, _ = S.mirror(rings, pts, A.as_label_requests(g, reqs, scale), capped=False)
        for (e, t), wnt in zip(reqs, want):
            got = A.mirror_position(g, f, e, *tiles[t], scale)
            assert (got["status"], got["x"], got["y"]) == (wnt["status"], wnt["x"], wnt["y"])
        assert want["status"].tolist() == [abi.LABEL_OK, abi.LABEL_OK, abi.LABEL_NONE]


def test_mirror_under_sanitizers():
    out = subprocess.run([A.build_host_main()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 5000
