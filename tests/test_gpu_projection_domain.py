"""The projection on the device over its whole admitted domain, against the bounded model.

project_point (csrc/osmt_project.h) is the one function of the library that is not exact by construction: its y passes through
the device's tan and log.  tests/golden/projection_cases.json (made by tests/golden/make_projection_cases.py from
tests/_projection_model.py; tests/test_projection_model_cpu.py holds the oracle and the factor-built projection against it)
gives per case ONE integer x — the longitude path is IEEE arithmetic alone — and the interval [y_lo, y_hi] an
implementation may answer whose tan is within 5 ulp and whose log is within 3 ulp of the correctly rounded value.  So:

  * x is asserted bit for bit, y inside its interval; where the interval is one integer (families A, B, C, E) that is also the
    oracle's answer.  Device == glibc is asserted nowhere else: over the near-tie family D the disagreement is counted and
    printed, not asserted.
  * every device route to project_point (k_project with and without node references, the tile-built scene, k_tl_emit,
    k_al_project) is compared with osmt_project element by element: device against device, exact.
  * tiles at the corners of the world render as the oracle renders them and as the device renders the fixture's integers.
  * the validator's edge: the limits are admitted, one double outside them is refused, and the context goes on working."""
import ctypes as C
import math

import numpy as np
import pytest

from osm_renderer_amd import abi, display_list, labels, lib, styled
from osm_renderer_amd.display_list import JOB_DTYPE, OP_DTYPE, RING_DTYPE, DisplayList, TileBuilder
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as A
from tests import _projection_cases as PC
from tests import _tilelabels as tl

pytestmark = pytest.mark.gpu

CS = PC.load()
LL = PC.latlon(CS)
GROUPS = PC.groups(CS)
M18 = (1 << 18) - 1
MAX_LAT, SQUARE_LAT = 85.06, 85.0511287798066
PAD_SIZES = (63, 64, 65, 255, 256, 257)


def _bits(v):
    return np.float64(v).view(np.uint64)


# ---- osmt_project against the fixture ---------------------------------------------------------------------------------------
def test_osmt_project_x_is_exact_and_y_lies_in_its_interval(gpu_ctx):
    """k_project_single over every family, one call per (zoom, tile, scale); groups of 1 point (family A), of the sizes the
    fixture has, and six groups padded by repetition to the wave and block edges"""
    padded = [k for k, idx in GROUPS.items() if 20 <= len(idx) <= PAD_SIZES[0]][: len(PAD_SIZES)]
    assert len(padded) == len(PAD_SIZES)
    sizes, bad_x, bad_y, n = set(), [], [], 0
    for k, idx in GROUPS.items():
        if k in padded:
            idx = np.resize(idx, PAD_SIZES[padded.index(k)])  # repeats the group's cases
        sizes.add(len(idx))
        zoom, tx, ty, scale = k
        got = gpu_ctx.project(LL[idx], zoom, tx, ty, float(scale))
        c = CS[idx]
        for i in np.nonzero(got[:, 0] != c["x"])[0]:
            bad_x.append((k, str(c["family"][i]), float(c["lon"][i]), int(got[i, 0]), int(c["x"][i])))
        for i in np.nonzero((got[:, 1] < c["y_lo"]) | (got[:, 1] > c["y_hi"]))[0]:
            bad_y.append((k, str(c["family"][i]), float(c["lat"][i]).hex(), int(got[i, 1]), int(c["y_lo"][i]), int(c["y_hi"][i])))
        n += len(idx)
    assert sizes >= {1, *PAD_SIZES}, sorted(sizes)
    assert n >= len(CS)
    assert not bad_x, f"{len(bad_x)} x differ from the model (tile, family, lon, got, want): {bad_x[:8]}"
    assert not bad_y, f"{len(bad_y)} y outside the interval (tile, family, lat, got, lo, hi): {bad_y[:8]}"


def test_near_ties_stay_in_the_interval_and_the_disagreement_is_counted(gpu_ctx, oracle):
    """Family D: latitudes within 2 ulp of a round() tie.  The assertion is the interval; how often the device, the oracle
    (glibc) and the factor-built projection of the anchors (host tan / log) part inside it is printed — a
    measurement that DESIGN 3.1 and 3.8 quote, not a property."""
    d = np.nonzero(CS["family"] == "D")[0]
    fac = A.mercator_factors(LL[d])
    dev = np.zeros((len(d), 2), np.int32)
    orc, fct = np.zeros_like(dev), np.zeros((len(d), 2), np.int64)
    for k, idx in PC.groups(CS[d]).items():
        zoom, tx, ty, scale = k
        dev[idx] = gpu_ctx.project(LL[d][idx], zoom, tx, ty, float(scale))
        orc[idx] = oracle.project_points(LL[d][idx], zoom, tx, ty, float(scale))
        fct[idx] = A.round_half_away(A.np_project(fac[idx], zoom, tx, ty, scale))
    c = CS[d]
    undecided = int((c["y_lo"] < c["y_hi"]).sum())
    print(f"\nfamily D: {len(d)} near-tie points, {undecided} with two admitted integers; device != oracle at "
          f"{int((dev != orc).any(1).sum())}, device != project_from_factors at {int((dev != fct).any(1).sum())}, "
          f"oracle != project_from_factors at {int((orc != fct).any(1).sum())}")
    assert np.array_equal(dev[:, 0], c["x"])
    assert ((c["y_lo"] <= dev[:, 1]) & (dev[:, 1] <= c["y_hi"])).all()
    decided = c["y_lo"] == c["y_hi"]
    assert np.array_equal(dev[decided], orc[decided])  # one admitted integer: also the oracle's


def test_osmt_project_refuses_a_zoom_past_max_zoom(gpu_ctx):
    ll = np.array([[55.75, 37.61], [0.0, 0.0]])
    want = gpu_ctx.project(ll, 18, 3, 4, 2.0)
    for zoom in (19, 23, 24, 31, 32, 255):  # 256 << zoom wraps to 0 at 24; 1u << zoom is undefined from 32
        out = np.full((2, 2), 77, np.int32)
        rc = lib.load().osmt_project(gpu_ctx._h, ll.ctypes.data_as(C.POINTER(C.c_double)), 2, zoom, 3, 4, 2.0, out.ctypes.data_as(C.POINTER(C.c_int32)))
        err = lib.load().osmt_last_error().decode()
        assert rc == abi.INVALID_ARG and f"zoom {zoom} > MAX_ZOOM" in err, (zoom, rc, err)
        assert (out == 77).all()
        assert np.array_equal(gpu_ctx.project(ll, 18, 3, 4, 2.0), want)  # the context goes on working
    with pytest.raises(OsmtError):
        gpu_ctx.project(ll, 19, 0, 0, 1.0)
    assert np.array_equal(gpu_ctx.project(ll, abi.MAX_ZOOM, 3, 4, 2.0), want)


# ---- every device route gives the same integers -----------------------------------------------------------------------------
CORNERS = [(18, 0, 0), (18, M18, M18), (0, 0, 0), (18, M18, 0), (18, 0, M18), (17, 0, (1 << 17) - 1), (1, 1, 0)]


def _node_cases():
    """the cases whose (lat, lon) make the node set: the edge groups of both far corners of zoom 18 and of the zoom 0 tile, and
    random, x-tie and near-y-tie cases (every family that lies in the admitted domain)"""
    idx = [GROUPS[(18, 0, 0, 1)], GROUPS[(18, M18, M18, 4)], GROUPS[(0, 0, 0, 1)]]
    idx += [np.nonzero(CS["family"] == f)[0][:n] for f, n in (("A", 60), ("C", 40), ("D", 60))]
    idx = np.concatenate(idx)
    return idx[CS["family"][idx] != "E"]  # family E shares these tiles and lies outside what a batch or a geodata file admits


NODE_CASES = _node_cases()
NODES = LL[NODE_CASES]


def _tiles(n):
    """n tiles: the corners first, then the tiles of the tie cases of the node set (their ties are those tiles'), then others"""
    out = list(CORNERS)
    for c in list(CS[NODE_CASES][::-1]) + list(CS[CS["family"] == "A"]):
        t = (int(c["zoom"]), int(c["tx"]), int(c["ty"]))
        if t not in out:
            out.append(t)
    return out[:n]


class _Expected:
    """osmt_project of a node set under a tile, once per tile"""

    def __init__(self, ctx, scale, nodes=None):
        self.ctx, self.scale, self.nodes, self.memo = ctx, scale, NODES if nodes is None else nodes, {}

    def __call__(self, tile):
        if tile not in self.memo:
            self.memo[tile] = self.ctx.project(self.nodes, *tile, float(self.scale))
        return self.memo[tile]


def _point_batch(tiles, scale, kind, rng):
    """A batch of jobs without ops whose points are the node set in a shuffled, repeating order: nothing to rasterise, every
    point projected.  With several jobs, job 7 has no points; behind every third job lie points of no job.  Returns (display
    list, [(job or -1, node)] per point)."""
    n = len(NODES)
    jobs = np.zeros(len(tiles), JOB_DTYPE)
    owner = []
    for j, (zoom, x, y) in enumerate(tiles):
        jobs[j]["zoom"], jobs[j]["x"], jobs[j]["y"], jobs[j]["has_canvas"] = zoom, x, y, 1
        order = [] if j == 7 else np.concatenate([rng.permutation(n), rng.integers(0, n, 9)]).tolist()
        jobs[j]["pt_off"], jobs[j]["n_pts"] = len(owner), len(order)
        owner += [(j, k) for k in order]
        if j % 3 == 0:
            owner += [(-1, int(k)) for k in rng.integers(0, n, 5)]
    refs = np.array([k for _, k in owner], np.uint32)
    empty = (np.zeros(0, OP_DTYPE), np.zeros(0, RING_DTYPE))
    if kind == abi.COORD_NODE_REF:
        return DisplayList(jobs, *empty, refs, [], kind, scale, nodes=NODES), owner
    return DisplayList(jobs, *empty, NODES[refs], [], kind, scale), owner


@pytest.mark.parametrize("n_jobs,scale", [(1, 4), (65, 1), (65, 4)])
@pytest.mark.parametrize("kind", [abi.COORD_LATLON_F64, abi.COORD_NODE_REF], ids=["latlon", "node_ref"])
def test_k_project_equals_osmt_project(gpu_ctx, kind, n_jobs, scale):
    tiles = [(18, M18, M18)] if n_jobs == 1 else _tiles(n_jobs)
    assert len(tiles) == n_jobs
    dl, owner = _point_batch(tiles, scale, kind, np.random.default_rng(5 * n_jobs + scale))
    exp = _Expected(gpu_ctx, scale)
    want = np.array([exp(tiles[j])[k] if j >= 0 else (0, 0) for j, k in owner], np.int32)
    sc = gpu_ctx.upload(dl)
    gpu_ctx.render_stages(sc, 1)  # the projection stage alone
    got = gpu_ctx.read_points(sc)
    sc.free()
    assert sum(j < 0 for j, _ in owner) >= 5 and (n_jobs == 1 or dl.jobs[7]["n_pts"] == 0)
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} points differ, first {bad[0]}: owner {owner[bad[0]]}, {got[bad[0]]} != {want[bad[0]]}"


def _register_world(ctx, nodes):
    """`nodes` as a registered geodata file: two ways over all of them (in order; shuffled and repeating), listed with every
    node under the z18 index tile of every tile the cases ask for, and one draw style bound to both ways"""
    n = len(nodes)
    rng = np.random.default_rng(77)
    ways = [(5000, list(range(n))), (5001, np.concatenate([rng.permutation(n), rng.integers(0, n, 17)]).tolist())]
    keys = sorted({(x << (18 - z), y << (18 - z)) for z, x, y in _tiles(65)})
    w = type("World", (), {})()
    w.nodes, w.ways = nodes, [np.array(v) for _, v in ways]
    w.gid = ctx.register_geodata(styled.Geodata(nodes, ways))
    ctx.register_tile_index(w.gid, styled.TileIndex([(k, [0, 1], []) for k in keys]))
    ctx.register_node_index(w.gid, styled.NodeIndex(np.arange(1, n + 1), [list(range(n))] * len(keys)))  # global ids rise with the node
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_color"], st["color"], st["has_width"], st["width"] = 1, (40, 60, 200), 1, 1.0
    first = ctx.register_styles(st)
    w.draw = ctx.register_style_bindings(styled.StyleBindings(w.gid, 0, 18, [[first], [first]], []))
    return w


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """the whole node set, with a label style without icon or text bound to every node"""
    w = _register_world(gpu_ctx, NODES)
    ls = gpu_ctx.register_label_styles(tl.label_styles([dict()]))
    w.node_bind = gpu_ctx.register_label_bindings(styled.LabelBindings(w.gid, 0, 18, [[(ls, None)]] * len(NODES), [""]))
    return w


@pytest.fixture(scope="module")
def inner_world(gpu_ctx):
    """The nodes inside the Mercator square — area label bindings need the file's Mercator factors, and
    osmt_register_node_mercator admits factors in [0, 1] only, which the band 85.0511 < |lat| <= 85.06 leaves — with a text
    style (a way's default position: Line) and an empty text bound to both ways."""
    f = A.mercator_factors(NODES)
    keep = ((f >= 0.0) & (f <= 1.0)).all(1)
    assert 200 <= int(keep.sum()) < len(NODES) and (np.abs(NODES[keep][:, 1]) == 180.0).any()
    w = _register_world(gpu_ctx, np.ascontiguousarray(NODES[keep]))
    gpu_ctx.register_node_mercator(w.gid, np.ascontiguousarray(f[keep]))
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    font = labels.FontTable([(0x41, 0)], [labels.SYNTH_GLYPHS[0][0]], [syn.first_id])
    gpu_ctx.register_font(font)
    ls = gpu_ctx.register_label_styles(tl.label_styles([dict(font_size=9.0, font_id=font.font_id)]))
    w.area_bind = gpu_ctx.register_area_label_bindings(styled.AreaLabelBindings(w.gid, 0, 18, [[(ls, 0)], [(ls, 0)]], [], [""]))
    return w


def _scene(ctx, w, tiles, scale):
    return ctx.build_tiles(styled.TileBatch(w.gid, tiles, {z: w.draw for z in range(19)}, scale=scale))


# scale 4 under the zoom 0 tile only: at zoom 18 and scale 4 a node of the band |lat| > 85.0511 lies up to 76 748 px past
# 2^28 under a tile of the opposite edge, which these scenes' ops would carry into the pre-pass
GEO_PARAMS = [(1, 4), (65, 1), (65, 3)]


@pytest.mark.parametrize("n_jobs,scale", GEO_PARAMS)
def test_tile_built_scene_points_equal_osmt_project(gpu_ctx, world, n_jobs, scale):
    tiles = [(0, 0, 0)] if n_jobs == 1 else _tiles(n_jobs)
    exp = _Expected(gpu_ctx, scale)
    sc = _scene(gpu_ctx, world, tiles, scale)
    gpu_ctx.render_stages(sc, 1)
    dl, got = sc.dl, gpu_ctx.read_points(sc)
    assert dl.coord_kind == abi.COORD_NODE_REF and len(dl.jobs) == n_jobs
    for j, tile in enumerate(tiles):
        a, m = int(dl.jobs[j]["pt_off"]), int(dl.jobs[j]["n_pts"])
        assert m == sum(len(v) for v in world.ways)  # both ways, once each
        assert np.array_equal(got[a : a + m], exp(tile)[dl.coords[a : a + m]]), (j, tile)
    sc.free()


@pytest.mark.parametrize("n_jobs,scale", GEO_PARAMS)
def test_node_label_anchors_equal_osmt_project(gpu_ctx, world, n_jobs, scale):
    """k_tl_emit: one label per node (a style without icon or text), ordered by global id = node number"""
    tiles = [(0, 0, 0)] if n_jobs == 1 else _tiles(n_jobs)
    exp = _Expected(gpu_ctx, scale)
    sc = _scene(gpu_ctx, world, tiles, scale)
    node = sc.build_tile_labels({z: world.node_bind for z in range(19)})
    off = node.job_label_off
    assert off.tolist() == [len(NODES) * j for j in range(n_jobs + 1)]
    for j, tile in enumerate(tiles):
        lab, run = node.labels[off[j] : off[j + 1]], node.runs[off[j] : off[j + 1]]
        want = exp(tile).astype(np.float64)
        assert np.array_equal(np.stack([lab["icon_center_x"], lab["icon_center_y"]], 1), want), (j, tile)
        assert np.array_equal(np.stack([run["center_x"], run["center_y"]], 1), want), (j, tile)
    sc.free()


@pytest.mark.parametrize("n_jobs,scale", GEO_PARAMS)
def test_way_text_points_equal_osmt_project(gpu_ctx, inner_world, n_jobs, scale):
    """k_al_project: the points of a text along a way, walked from the end with the smaller x (text_placer.rs:65-67)"""
    tiles = [(0, 0, 0)] if n_jobs == 1 else _tiles(n_jobs)
    world = inner_world
    exp = _Expected(gpu_ctx, scale, world.nodes)
    sc = _scene(gpu_ctx, world, tiles, scale)
    area, node = sc.build_tile_labels_all({z: world.area_bind for z in range(19)}, None)
    off = area.job_label_off
    assert off.tolist() == [2 * j for j in range(n_jobs + 1)] and len(node.labels) == 0
    for j, tile in enumerate(tiles):
        for k, nodes in enumerate(world.ways):  # global ids 5000, 5001: the label order
            r = area.runs[off[j] + k]
            assert r["position"] == abi.TEXT_LINE and r["n_pts"] == len(nodes) and area.labels[off[j] + k]["has_text"] == 1
            want = exp(tile)[nodes]
            if want[0][0] > want[-1][0]:
                want = want[::-1]
            assert np.array_equal(area.way_pts[int(r["pt_off"]) : int(r["pt_off"]) + len(nodes)], want), (j, tile, k)
    sc.free()


# ---- rendering at the corners of the world ------------------------------------------------------------------------------------
def _fixture_point(lat, lon, zoom, tx, ty, scale):
    """the fixture's integers for exactly this double pair under this tile; only cases with one admitted y serve"""
    m = ((CS["zoom"] == zoom) & (CS["tx"] == tx) & (CS["ty"] == ty) & (CS["scale"] == scale) & (CS["lat"].view(np.uint64) == _bits(lat))
         & (CS["lon"].view(np.uint64) == _bits(lon)) & ((CS["family"] == "A") | (CS["family"] == "B")))
    c = CS[m]
    assert len(c) >= 1 and c["y_lo"][0] == c["y_hi"][0], (lat, lon, zoom, tx, ty, scale)
    return int(c["x"][0]), int(c["y_lo"][0])


def _corner_geometry(zoom, tx, ty, scale):
    """(polygon ring, way) in (lat, lon).  Zoom 18: the vertices of family B nearest the tile — the polygon's edge from the
    square's corner to (0, 0) crosses the tile on its diagonal, the way runs from the admitted limit to the square's corner
    along the meridian +-180 and ends in the tile's corner.  Zoom 0: the world's corners and family A's points of that tile."""
    if zoom == 0:
        a = CS[(CS["family"] == "A") & (CS["zoom"] == 0) & (CS["scale"] == scale)]
        inner = [(float(c["lat"]), float(c["lon"])) for c in a]
        assert len(inner) >= 10
        ring = [(SQUARE_LAT, -180.0)] + inner[:6] + [(-SQUARE_LAT, 180.0), (0.0, 0.0), (SQUARE_LAT, -180.0)]
        way = [(MAX_LAT, -180.0), inner[6], (-MAX_LAT, 180.0), inner[7], (MAX_LAT, 180.0), inner[8], (-MAX_LAT, -180.0)]
        return ring, way
    lon = -180.0 if tx == 0 else 180.0
    s = 1.0 if ty == 0 else -1.0
    ring = [(s * SQUARE_LAT, lon), (0.0, 0.0), (0.0, lon), (s * SQUARE_LAT, lon)]
    return ring, [(s * MAX_LAT, lon), (s * SQUARE_LAT, lon)]


@pytest.mark.parametrize("scale", [1, 4])
def test_tiles_at_the_corners_of_the_world_render_as_the_oracle(gpu_ctx, oracle, scale):
    tiles = [(18, 0, 0), (18, M18, 0), (18, 0, M18), (18, M18, M18), (0, 0, 0)]
    as_ll, as_i32 = [], []
    for zoom, tx, ty in tiles:
        ring, way = _corner_geometry(zoom, tx, ty, scale)
        for kind, out in ((abi.COORD_LATLON_F64, as_ll), (abi.COORD_POINT_I32, as_i32)):
            conv = (lambda p: p) if kind == abi.COORD_LATLON_F64 else (lambda p: _fixture_point(p[0], p[1], zoom, tx, ty, scale))
            tb = TileBuilder(zoom, tx, ty, scale, coord_kind=kind)
            tb.fill([[conv(p) for p in ring]], (200, 120, 40), 0.75)
            tb.stroke([conv(p) for p in way], 24.0 * scale, (20, 40, 200), 0.9, dashes=[30.0 * scale, 10.0 * scale], cap=abi.CAP_ROUND,
                      use_caps_for_dashes=True)
            out.append(tb.build())
    dl_ll, dl_i32 = display_list.concat(as_ll), display_list.concat(as_i32)
    flat = dl_ll.coords
    assert (np.abs(flat[:, 1]) == 180.0).any() and (np.abs(flat[:, 0]) == MAX_LAT).any()
    assert int(np.abs(dl_i32.coords).max()) <= 1 << 28
    want = oracle.render_batch(dl_ll, threads=len(tiles))  # glibc's projection: the same integers where one is admitted
    sa, sb = gpu_ctx.upload(dl_ll), gpu_ctx.upload(dl_i32)
    got, twin = gpu_ctx.render(sa).cpu().numpy(), gpu_ctx.render(sb).cpu().numpy()
    assert np.array_equal(gpu_ctx.read_points(sa), dl_i32.coords)
    sa.check(), sb.check()
    sa.free(), sb.free()
    for j, tile in enumerate(tiles):
        colours = len(np.unique(np.ascontiguousarray(want[j]).view(np.uint32)))
        assert colours >= 3, (tile, colours)  # canvas, polygon and way are all in the picture
        assert np.array_equal(got[j], want[j]), f"{tile}: {int((got[j] != want[j]).any(-1).sum())} pixels differ from the oracle"
        assert np.array_equal(got[j], twin[j]), f"{tile}: {int((got[j] != twin[j]).any(-1).sum())} pixels differ from the i32 batch"


# ---- the validator's edge -----------------------------------------------------------------------------------------------------
def _edge_tile(kind, bad=None):
    """A zoom 0 tile of one triangle whose vertices are the admitted limits; bad = (lat, lon) replaces vertex 2"""
    ring = [(MAX_LAT, -180.0), (MAX_LAT, 180.0), (-MAX_LAT, 180.0), (MAX_LAT, -180.0)]
    if bad is not None:
        ring[2] = bad
    tb = TileBuilder(0, 0, 0, 1, coord_kind=abi.COORD_LATLON_F64)
    tb.fill([ring], (10, 200, 90), 0.5)
    dl = tb.build()
    if kind == abi.COORD_NODE_REF:  # the node table in the ring's order: vertex 2 is node 2
        dl = DisplayList(dl.jobs, dl.ops, dl.rings, np.arange(len(ring), dtype=np.uint32), dl.dashes, kind, 1, nodes=dl.coords)
    return dl


def _outside():
    up, inf, nan = math.nextafter, math.inf, math.nan
    lats = [up(MAX_LAT, inf), up(-MAX_LAT, -inf), nan, inf, -inf]
    lons = [up(180.0, inf), up(-180.0, -inf), nan, inf, -inf]
    return [(v, 180.0) for v in lats] + [(-MAX_LAT, v) for v in lons]


@pytest.mark.parametrize("kind", [abi.COORD_LATLON_F64, abi.COORD_NODE_REF], ids=["latlon", "node_ref"])
def test_batches_admit_the_limits_and_refuse_one_double_past_them(gpu_ctx, oracle, kind):
    L = lib.load()
    good = _edge_tile(kind)
    want = oracle.render_batch(good)
    b = good.as_batch()
    assert L.osmt_validate_batch(C.byref(b)) == abi.OK
    sc = gpu_ctx.upload(good)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), want) and len(np.unique(np.ascontiguousarray(want).view(np.uint32))) >= 2
    sc.free()
    probe = gpu_ctx.project(good.nodes if kind == abi.COORD_NODE_REF else good.coords, 0, 0, 0, 1.0)
    for lat, lon in _outside():
        dl = _edge_tile(kind, (lat, lon))
        b = dl.as_batch()
        assert L.osmt_validate_batch(C.byref(b)) == abi.UNSUPPORTED
        err = L.osmt_last_error().decode()
        assert "point 2:" in err and "outside the Web-Mercator square" in err, err
        with pytest.raises(OsmtError) as e:
            gpu_ctx.upload(dl)
        assert e.value.code == abi.UNSUPPORTED and "point 2:" in str(e.value), str(e.value)
        # a correct call on the same context
        sc = gpu_ctx.upload(good)
        gpu_ctx.render_stages(sc, 1)
        assert np.array_equal(gpu_ctx.read_points(sc), probe[good.coords] if kind == abi.COORD_NODE_REF else probe)
        sc.free()
    sc = gpu_ctx.upload(good)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), want)
    sc.free()


def test_geodata_registration_admits_the_limits_and_refuses_one_double_past_them(gpu_ctx, oracle):
    nodes = np.array([(MAX_LAT, -180.0), (MAX_LAT, 180.0), (-MAX_LAT, 180.0)])
    way = [(7, [0, 1, 2, 0])]
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["has_fill_opacity"], st["fill_opacity"] = 1, (10, 200, 90), 1, 0.5
    first = gpu_ctx.register_styles(st)

    def render(gid):
        """accepted means it renders: the zoom 0 tile of a scene built over the registration, against the oracle"""
        gpu_ctx.register_tile_index(gid, styled.TileIndex([((0, 0), [0], [])]))
        bind = gpu_ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[first]], []))
        sc = gpu_ctx.build_tiles(styled.TileBatch(gid, [(0, 0, 0)], {0: bind}))
        px = gpu_ctx.render(sc).cpu().numpy()
        twin = sc.dl
        sc.free()
        want = oracle.render_batch(twin)
        assert np.array_equal(px, want) and len(np.unique(np.ascontiguousarray(want).view(np.uint32))) >= 2

    render(gpu_ctx.register_geodata(styled.Geodata(nodes, way)))
    probe = gpu_ctx.project(nodes, 0, 0, 0, 1.0)
    assert probe.tolist() == [[0, 0], [256, 0], [256, 256]]
    for lat, lon in _outside():
        bad = nodes.copy()
        bad[2] = (lat, lon)
        with pytest.raises(OsmtError) as e:
            gpu_ctx.register_geodata(styled.Geodata(bad, way))
        assert e.value.code == abi.INVALID_ARG and "geodata: node 2:" in str(e.value) and "outside the Web-Mercator square" in str(e.value)
        assert np.array_equal(gpu_ctx.project(nodes, 0, 0, 0, 1.0), probe)  # a correct call on the same context
    render(gpu_ctx.register_geodata(styled.Geodata(nodes, way)))  # the context registers and renders as before
