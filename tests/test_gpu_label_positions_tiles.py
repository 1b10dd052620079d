"""Label anchors from tile coordinates on the GPU (osmt_label_positions_tiles): the rings and points the device projects from
registered Mercator factors compared BIT FOR BIT with a numpy restatement of the three operations over the same factors, and
the positions compared bit for bit with osmt_label_positions fed those points and with the host mirror.  Runs on poisoned
device memory like the rest of the GPU suite (tests/conftest.py)."""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as A
from tests import _polylabel_shim as S

pytestmark = pytest.mark.gpu

MP = abi.STYLED_MULTIPOLYGON
LDS_TIER_CELLS = 256  # PL_LDS_CELLS of csrc/osmt_polylabel.hip
RING_LENGTHS = (0, 1, 2, 63, 64, 65, 300)
BIG = 65536


def _star(n, seed, cx=128.3, cy=77.7, r=100.0):
    """a closed star-shaped ring of n points in all (n >= 4), or n arbitrary points below that"""
    rng = np.random.default_rng(seed)
    if n < 4:
        return rng.uniform(0, 256, (n, 2))
    ang = np.sort(rng.uniform(0, 2 * np.pi, n - 1))
    rad = r * rng.uniform(0.5, 1.0, n - 1)
    p = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return np.concatenate([p, p[:1]])


def _rect(x0, y0, w, h):
    return [[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h], [x0, y0]]


def _build_world():
    w = A.World()
    e = types.SimpleNamespace()
    e.len = {n: w.way(w.shape(_star(n, 100 + n))) for n in RING_LENGTHS}
    e.sq = w.way(w.shape(_rect(10.5, 20.25, 40.0, 40.0)))
    e.ell = w.way(w.shape([[1.5, 2.5], [81.5, 2.5], [81.5, 32.25], [31.75, 32.25], [31.75, 92.5], [1.5, 92.5], [1.5, 2.5]]))
    e.strip_lds = w.way(w.shape(_rect(3.25, -7.5, 1000.0, 1.0)))     # 1000 cells in the first grid: past the LDS tier
    e.strip_big = w.way(w.shape(_rect(0.0, 0.0, 5000.0, 0.01)))      # 500 000 cells in the first grid: TOO_LARGE
    planted = w.shape(_rect(1.0, 1.0, 2.0, 2.0))                      # their factors are replaced below by exact 0.0 and 1.0
    e.planted = w.way(planted)
    e.big = w.way([0] * BIG)                                          # 65 536 references to one node: the limit test
    p_empty, p_one = w.polygon([]), w.polygon(w.shape([[5.5, 6.5]]))
    p_a = w.polygon(w.shape(_rect(300.0, 300.0, 10.0, 10.0)))
    p_big = w.polygon(w.shape(_rect(20.0, 20.0, 180.0, 180.0)))
    p_hole = w.polygon(w.shape(_rect(60.0, 60.0, 40.0, 40.0))[::-1])
    small = [w.polygon(w.shape(_star(4 + k % 5, 900 + k, cx=20.0 + 30.0 * (k % 10), cy=20.0 + 30.0 * (k // 10), r=12.0))) for k in range(70)]
    e.mp1, e.mp2, e.mp70 = w.mp([p_big]), w.mp([p_big, p_hole]), w.mp(small)
    e.mp_first_empty = w.mp([p_empty, p_big])
    e.mp_mid_one = w.mp([p_big, p_one, p_hole])
    e.mp_order = w.mp([p_a, p_big, p_hole])  # the largest ring is not the first, and it has a hole
    e.mp_none = w.mp([])
    g = w.geodata()
    f = A.mercator_factors(g.nodes)
    f[planted[:4]] = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    f[planted[4]] = [0.0, 0.0]
    e.ordinary = [e.len[n] for n in RING_LENGTHS] + [e.sq, e.ell, e.planted, e.mp1, e.mp2, e.mp70, e.mp_first_empty, e.mp_mid_one, e.mp_order, e.mp_none]
    tx, ty = A.T18
    last = (1 << 18) - 1
    e.tiles = [(15, tx >> 3, ty >> 3), (18, tx, ty), (0, 0, 0), (18, 0, 0), (18, last, last), (10, tx >> 8, ty >> 8), (18, 0, last)]
    return types.SimpleNamespace(g=g, f=f, gid=None, e=e)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    W = _build_world()
    W.gid = gpu_ctx.register_geodata(W.g)
    gpu_ctx.register_node_mercator(W.gid, W.f)
    return W


def _check_expansion(ctx, W, tiles, reqs, scale):
    rings, pts = ctx.label_tile_batch_expand(W.gid, tiles, reqs, scale)
    want_rings, want_pts = A.expected_expansion(W.g, W.f, tiles, reqs, scale)
    assert np.array_equal(rings, want_rings)
    assert pts.shape == want_pts.shape
    bad = np.nonzero((A.bits(pts) != A.bits(want_pts)).any(axis=1))[0]
    assert not len(bad), (len(bad), int(bad[0]), pts[bad[0]], want_pts[bad[0]])
    return rings, pts


def _same(got, want):
    bad = np.nonzero((got["x"].view(np.uint64) != want["x"].view(np.uint64)) | (got["y"].view(np.uint64) != want["y"].view(np.uint64))
                     | (got["status"] != want["status"]))[0]
    assert not len(bad), (len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("scale", [1, 2, 4])
def test_expanded_rings_and_points_bit_for_bit(gpu_ctx, world, scale):
    """every ring length, every multipolygon shape, every tile (zoom 0, both far corners of zoom 18, mixed zooms), exact 0.0 and
    1.0 factors; the same entity under two tiles and the same (entity, tile) twice"""
    W, e = world, world.e
    reqs = [(ent, (i + k) % len(e.tiles)) for k in range(len(e.tiles)) for i, ent in enumerate(e.ordinary)]
    reqs += [(e.sq, 0), (e.sq, 1), (e.mp_order, 3), (e.mp_order, 3), (e.planted, 2), (e.planted, 4), (e.planted, 3)]
    rings, pts = _check_expansion(gpu_ctx, W, e.tiles, reqs, scale)
    assert len(rings) > len(reqs) and (np.abs(pts) <= 2.0 ** 28).all()
    # the planted way under the far corner of zoom 18: 1.0 * 2^26 minus the largest offset, times scale — exact
    r, p = gpu_ctx.label_tile_batch_expand(W.gid, [e.tiles[4]], [(e.planted, 0)], scale)
    off = float(((1 << 18) - 1) * 256)
    assert p.tolist() == [[-off * scale, -off * scale], [256.0 * scale, -off * scale], [256.0 * scale, 256.0 * scale], [-off * scale, 256.0 * scale],
                          [-off * scale, -off * scale]]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_request_counts_around_the_scan_blocks(gpu_ctx, world, n):
    """requests without nodes at the start, in the middle and at the end; expansion and positions"""
    W, e = world, world.e
    reqs = [(e.ordinary[(3 * i) % len(e.ordinary)], i % len(e.tiles)) for i in range(n)]
    reqs[0] = (e.len[0], 0)
    reqs[n // 2] = (e.mp_none, 1) if n > 1 else reqs[0]
    reqs[-1] = (e.len[0], 2) if n > 1 else reqs[0]
    scale = 2
    rings, pts = _check_expansion(gpu_ctx, W, e.tiles, reqs, scale)
    got = gpu_ctx.label_positions_tiles(W.gid, e.tiles, reqs, scale)
    assert gpu_ctx.label_positions_stats()[0] == n
    rq = A.as_label_requests(W.g, reqs, scale)
    _same(got, gpu_ctx.label_positions(rings, pts, rq))
    want, _, _ = S.mirror(rings, pts, rq)
    _same(got, want)
    assert got["status"][0] == got["status"][-1] == abi.LABEL_NONE


@pytest.mark.parametrize("scale", [1, 2])
def test_positions_and_statuses_bit_for_bit(gpu_ctx, world, scale):
    W, e = world, world.e
    ents = [e.sq, e.ell, e.strip_lds, e.strip_big, e.mp_order, e.mp2, e.mp_first_empty, e.len[0], e.mp_none, e.len[1], e.len[2], e.len[65], e.len[300],
            e.mp70, e.mp_mid_one]
    tiles = e.tiles[:2]
    reqs = [(ent, t) for t in range(2) for ent in ents]
    rings, pts = A.expected_expansion(W.g, W.f, tiles, reqs, scale)
    rq = A.as_label_requests(W.g, reqs, scale)
    want, peak, pops = S.mirror(rings, pts, rq, capped=True)
    got = gpu_ctx.label_positions_tiles(W.gid, tiles, reqs, scale)
    stats = gpu_ctx.label_positions_stats()
    _same(got, want)
    _same(got, gpu_ctx.label_positions(rings, pts, rq))
    st = dict(zip(ents, want["status"][:len(ents)].tolist()))
    assert st[e.strip_big] == abi.LABEL_TOO_LARGE and st[e.strip_lds] == abi.LABEL_OK and st[e.mp_order] == abi.LABEL_OK
    assert st[e.mp_first_empty] == st[e.len[0]] == st[e.mp_none] == abi.LABEL_NONE
    left_lds = int(((peak > LDS_TIER_CELLS) & (want["status"] == abi.LABEL_OK)).sum())
    assert left_lds >= 2 and stats[0] == len(reqs) and stats[2] == int((want["status"] == abi.LABEL_TOO_LARGE).sum()) == 2
    assert left_lds <= stats[1] <= int((peak > LDS_TIER_CELLS).sum())  # a request the second tier declines has left the first one too
    # the largest ring of mp_order is its second polygon and the hole counts: the answer is not the plain square's
    i_order = ents.index(e.mp_order)
    plain = gpu_ctx.label_positions_tiles(W.gid, tiles, [(e.mp1, 0)], scale)[0]
    assert (got["x"][i_order], got["y"][i_order]) != (plain["x"], plain["y"])
    # the host fallback of osmt::TileLabelPositions for the declined strip: the uncapped mirror from the same factors
    k = ents.index(e.strip_big)
    fb = A.mirror_position(W.g, W.f, e.strip_big, *tiles[0], scale)
    assert fb["status"] == abi.LABEL_OK and got["status"][k] == abi.LABEL_TOO_LARGE and (got["x"][k], got["y"][k]) == (0.0, 0.0)


def test_tile_label_positions_collector_falls_back():
    """osmt::TileLabelPositions in a program of its own: the strip stated in degrees is declined by the device and computed on the host"""
    out = subprocess.run([A.build_demo()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "fallbacks 2" and len(lines) == 6
    for ln in lines[:-1]:
        i, gs, gx, gy, ws, wx, wy = ln.split()
        assert (gs, gx, gy) == (ws, wx, wy), ln
        assert int(gs) == abi.LABEL_OK


def _sentinel(n):
    out = np.zeros(n, labels.LABEL_POSITION_DTYPE)
    out.view(np.uint8)[:] = 0xEE
    return out


def _refused(ctx, code, needle, *args, n_out=None, **kw):
    reqs = args[2]
    out = _sentinel(len(reqs) if n_out is None else n_out)
    with pytest.raises(OsmtError) as ei:
        ctx.label_positions_tiles(*args, out=out, **kw)
    assert ei.value.code == code and needle in str(ei.value), str(ei.value)
    assert (out.view(np.uint8) == 0xEE).all()  # a refusal leaves `out` untouched


def test_limits_and_refusals(gpu_ctx, world):
    W, e = world, world.e
    tiles = e.tiles[:2]
    # 65 536 requests for one way of 65 536 nodes: 2^32 points, refused with the figure, before anything is allocated for them
    many = np.zeros(BIG, labels.LABEL_TILE_REQUEST_DTYPE)
    many["entity"] = e.big
    _refused(gpu_ctx, abi.UNSUPPORTED, "4294967296", W.gid, tiles, many, 1)
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.label_tile_batch_expand(W.gid, tiles, many, 1)
    assert ei.value.code == abi.UNSUPPORTED and "4294967296" in str(ei.value)
    # a correct call on the same context follows
    reqs = [(e.sq, 0), (e.mp_order, 1)]
    rings, pts = A.expected_expansion(W.g, W.f, tiles, reqs, 1)
    _same(gpu_ctx.label_positions_tiles(W.gid, tiles, reqs, 1), S.mirror(rings, pts, A.as_label_requests(W.g, reqs, 1))[0])
    # the same way in one request is an ordinary batch
    rings, pts = gpu_ctx.label_tile_batch_expand(W.gid, tiles, [(e.big, 0)], 1)
    assert rings.tolist() == [[0, BIG]] and (A.bits(pts) == A.bits(A.np_project(W.f[[0]], *tiles[0], 1))).all()

    n_ways, n_mps = len(W.g.way_ids), len(W.g.multipolygon_ids)
    I = abi.INVALID_ARG
    _refused(gpu_ctx, I, "not a tile", W.gid, tiles, [(e.sq, 0), (e.sq, 2)], 1)
    _refused(gpu_ctx, I, "way %d out of range" % n_ways, W.gid, tiles, [(e.sq, 0), (n_ways, 0)], 1)
    _refused(gpu_ctx, I, "multipolygon %d out of range" % n_mps, W.gid, tiles, [(n_mps | MP, 0)], 1)
    _refused(gpu_ctx, I, "way", W.gid, tiles, [(0x7FFFFFFF, 0)], 1)
    _refused(gpu_ctx, I, "zoom", W.gid, [(19, 0, 0)], [(e.sq, 0)], 1)
    _refused(gpu_ctx, I, "outside zoom", W.gid, tiles + [(18, 1 << 18, 0)], [(e.sq, 0)], 1)  # a tile no request names is checked too
    _refused(gpu_ctx, I, "outside zoom", W.gid, [(15, 0, 1 << 15)], [(e.sq, 0)], 1)
    _refused(gpu_ctx, I, "scale", W.gid, tiles, [(e.sq, 0)], 0)
    _refused(gpu_ctx, I, "scale", W.gid, tiles, [(e.sq, 0)], abi.MAX_SCALE + 1)
    _refused(gpu_ctx, I, "not registered", 10 ** 6, tiles, [(e.sq, 0)], 1)
    # a geodata file without factors; then with: the second registration, a wrong count and a bad factor are refused
    g2 = styled.Geodata([[55.0, 37.0], [55.1, 37.1], [55.0, 37.2]], [(1, [0, 1, 2, 0])])
    gid2 = gpu_ctx.register_geodata(g2)
    _refused(gpu_ctx, I, "no Mercator factors", gid2, tiles, [(0, 0)], 1)
    f2 = A.mercator_factors(g2.nodes)
    for bad, needle in ((f2[:1], "n_nodes = 1"), (np.array([[0.5, np.nan], [0.5, 0.5], [0.5, 0.5]]), "node 0: y"),
                        (np.array([[0.5, 0.5], [1.25, 0.5], [0.5, 0.5]]), "node 1: x")):
        with pytest.raises(OsmtError) as ei:
            gpu_ctx.register_node_mercator(gid2, bad)
        assert ei.value.code == I and needle in str(ei.value), str(ei.value)
    gpu_ctx.register_node_mercator(gid2, f2)
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.register_node_mercator(gid2, f2)
    assert ei.value.code == I and "already" in str(ei.value)
    got = gpu_ctx.label_positions_tiles(gid2, tiles, [(0, 0)], 1)
    assert got["status"][0] == abi.LABEL_OK
    # NULL pools with a count
    L = lib.load()
    b, _keep = gpu_ctx._label_tile_batch(W.gid, tiles, [(e.sq, 0)], 1)
    out = _sentinel(1)
    b.requests = None
    assert L.osmt_label_positions_tiles(gpu_ctx._h, C.byref(b), out.ctypes.data_as(C.c_void_p)) == I
    b, _keep = gpu_ctx._label_tile_batch(W.gid, tiles, [(e.sq, 0)], 1)
    b.tiles = None
    assert L.osmt_label_positions_tiles(gpu_ctx._h, C.byref(b), out.ctypes.data_as(C.c_void_p)) == I
    b, _keep = gpu_ctx._label_tile_batch(W.gid, tiles, [(e.sq, 0)], 1)
    assert L.osmt_label_positions_tiles(gpu_ctx._h, C.byref(b), None) == I
    assert (out.view(np.uint8) == 0xEE).all()
    # zero requests: OSMT_OK, with or without tiles
    assert len(gpu_ctx.label_positions_tiles(W.gid, tiles, [], 1)) == 0 and len(gpu_ctx.label_positions_tiles(W.gid, [], [], 1)) == 0
    r, p = gpu_ctx.label_tile_batch_expand(W.gid, tiles, [], 1)
    assert r.shape == (0, 2) and p.shape == (0, 2)


def test_two_jobs_in_flight(gpu_ctx, world):
    W, e = world, world.e
    a = [(ent, i % 2) for i, ent in enumerate(e.ordinary)]
    b = [(e.strip_lds, 1), (e.sq, 0), (e.mp_order, 1), (e.len[300], 0)]
    one_a = gpu_ctx.label_positions_tiles(W.gid, e.tiles, a, 2)
    one_b = gpu_ctx.label_positions_tiles(W.gid, e.tiles, b, 1)
    ja = gpu_ctx.label_positions_tiles_begin(W.gid, e.tiles, a, 2)
    jb = gpu_ctx.label_positions_tiles_begin(W.gid, e.tiles, b, 1)
    got_b = gpu_ctx.label_positions_end(jb)
    assert gpu_ctx.label_positions_stats()[0] == len(b)
    got_a = gpu_ctx.label_positions_end(ja)
    assert got_a.tobytes() == one_a.tobytes() and got_b.tobytes() == one_b.tobytes()
    j0 = gpu_ctx.label_positions_tiles_begin(W.gid, e.tiles, [], 1)
    assert len(gpu_ctx.label_positions_end(j0)) == 0


def test_rounding_agrees_with_osmt_project(gpu_ctx, world):
    """round() of the unrounded points equals the i32 points of osmt_project for the nodes of a 5-tile batch: the two paths use
    different tan / log (the host's in the factors, the device's in k_project), so equality here is an observation on these
    inputs, not a theorem"""
    W, e = world, world.e
    tx, ty = A.T18
    tiles = [(18, tx, ty), (18, tx + 1, ty), (17, tx >> 1, ty >> 1), (15, tx >> 3, ty >> 3), (12, tx >> 6, ty >> 6)]
    ents = [e.len[300], e.len[65], e.sq, e.ell, e.mp70, e.mp_order]
    for scale in (1, 2):
        for t, tile in enumerate(tiles):
            reqs = [(ent, t) for ent in ents]
            _, pts = gpu_ctx.label_tile_batch_expand(W.gid, tiles, reqs, scale)
            nodes = np.concatenate([r for ent in ents for r in A.entity_rings(W.g, ent)])
            want = gpu_ctx.project(W.g.nodes[nodes], *tile, float(scale))
            got = A.round_half_away(pts)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert not len(bad), (tile, scale, len(bad), pts[bad[0]], want[bad[0]])
