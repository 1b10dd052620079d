"""Display lists built on the GPU (osm_renderer_amd/csrc/osmt_styled.hip) at the sizes of the workload and at the limits of
the kernels: more than 1024 tiles (the second and later blocks of the one-lane-per-tile kernels, find_tile over long flat
stretches), more than 65 536 elements (the second chunk of k_styled_scan_blocks), 64-bit totals at and far above 2^32, the
device-memory tier of the sort up to the tile limit of 65 536 areas, global ids with bit 63 set, ranks that move under an
old batch, the list-kernel switch at 128 ops, and built scenes rendered on the paths above 64 and above 256 tiles.

Yardsticks, none of them under test here: osmt::SceneBuilder (byte for byte, tests/test_gpu_styled_feed.py) and the numpy
order model of tests/_styled_order_model.py.  Every test asserts the shape that makes it cross its boundary."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, lib
from tests import _styled_order_model as model
from tests._geodata import Reader, write_geodata
from tests._styled_feed import (LAT0, LON0, _center_tile, _file, extreme_id_world, fill_only_styles, geodata_of, random_pairs, recs_of)
from tests.test_gpu_styled_feed import _assert_same_list, _batch, _build_both, _cycled_tile, _small_world, _validates
from tests.test_styled_builder import STYLE_DTYPE, _build_cpp, _lib, _random_styles

pytestmark = pytest.mark.gpu

WG = 256  # lanes per block of k_styled_jobs / k_styled_tilemax / k_styled_count; blocks per chunk of k_styled_scan_blocks
CANVAS = np.array([241, 238, 232, 255], np.uint8)


def _with_a_long_way(tmp_path, oracle, r):
    """the world of Reader r again, plus an open way of 130 nodes (way r.n_ways): an op of more than 64 edges"""
    nodes = [(1000 + i, float(lat), float(lon), {}) for i, (lat, lon) in enumerate(r.node_table())]
    ways = [(r.global_id(1, i), r.way_nodes(i), {}) for i in range(r.n_ways)]
    polygons = [r.polygon_nodes(i) for i in range(r.n_polygons)]
    multis = [(r.global_id(2, i), r.multipolygon_polygons(i), {}) for i in range(r.n_multipolygons)]
    zig = []
    for i in range(130):
        nodes.append((1000 + len(nodes), LAT0 - 0.003 + 0.00005 * i, LON0 - 0.0019 + (0.0004 if i % 2 else 0.0), {}))
        zig.append(len(nodes) - 1)
    return _file(tmp_path, oracle, nodes, ways + [(7005, zig, {})], polygons, multis, name="long.bin")


class _World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory, gpu_ctx, oracle):
    """_small_world plus a 130-node way, 40 random styles and the batch of the workload's shape (test a; f cuts from it)"""
    tmp = tmp_path_factory.mktemp("styled_scale")
    small = _small_world(tmp, oracle)
    w = _World()
    w.r = _with_a_long_way(tmp, oracle, small)
    assert w.r.n_ways == small.n_ways + 1 == 11 and len(w.r.way_nodes(10)) == 130
    small.close()
    rng = np.random.default_rng(1)
    w.st, w.pool = _random_styles(rng, 40)
    w.gid = gpu_ctx.register_geodata(geodata_of(w.r))
    w.first = gpu_ctx.register_styles(recs_of(w.st), w.pool)
    tx, ty = _center_tile(oracle)
    # 300 empty | 468 drawn | 300 empty from tile 768 = 3 * 256 on | 632 drawn | 300 empty: blocks 0, 3 and 7 of the
    # one-lane-per-tile kernels hold empty tiles only
    counts = []
    for run, drawn in ((300, 468), (300, 632), (300, 0)):
        counts += [0] * run
        counts += [0 if k % 7 == 0 else int(rng.integers(1, 151)) for k in range(drawn)]
    w.tiles = [_cycled_tile(rng, 15, tx + (k % 2), ty, n, w.r.n_ways, w.r.n_multipolygons, len(w.st)) for k, n in enumerate(counts)]
    w.counts = counts
    w.want = _build_cpp(_lib(), w.r, w.tiles, w.st, w.pool, 1, True)
    yield w
    w.r.close()


def test_a_batch_of_the_workloads_shape(gpu_ctx, world):
    """a: 2000 tiles, 1100 of them the workload's (0..150 areas, every seventh empty), whole 256-lane blocks of empty tiles,
    more than 65 536 elements; then the same tiles in another order over the same areas array"""
    w = world
    counts, n_tiles, total = w.counts, len(w.tiles), sum(w.counts)
    assert n_tiles > 1024 and sum(1 for n in counts if n) > 900
    assert 3 * total > 65536 and (3 * total + WG - 1) // WG > WG  # the block scan's second chunk
    for blk in (0, 3, 7):
        assert not any(counts[blk * WG : (blk + 1) * WG]) and len(counts) > blk * WG
    assert max(counts) <= 150 and counts[-1] == 0 and counts[0] == 0
    scene = gpu_ctx.build_styled(_batch(w.gid, w.tiles, w.first))
    got = scene.read_display_list()
    _assert_same_list(got, w.want)
    assert _validates(got)[0] == abi.OK
    # the fullest tile lies beyond the first block of k_styled_tilemax (for a batch of this size the renderer does not look)
    fullest = int(np.argmax(w.want.jobs["n_ops"]))
    assert fullest >= WG and scene.max_tile_ops() == int(w.want.jobs["n_ops"][fullest]) > 128
    assert len(got.ops) > total / 2 and (got.rings["n_pts"] == 130).any() and len(got.dashes) > 0
    scene.free()
    perm = np.random.default_rng(2).permutation(n_tiles)
    sb = _batch(w.gid, w.tiles, w.first)
    areas_before = sb.areas.copy()
    sb.tiles = sb.tiles[perm].copy()
    assert np.array_equal(sb.areas, areas_before) and not np.array_equal(perm, np.arange(n_tiles))
    scene = gpu_ctx.build_styled(sb)
    got = scene.read_display_list()
    _assert_same_list(got, _build_cpp(_lib(), w.r, [w.tiles[k] for k in perm], w.st, w.pool, 1, True))
    assert _validates(got)[0] == abi.OK and scene.max_tile_ops() == int(got.jobs["n_ops"].max())
    scene.free()


def test_b_the_sort_large_and_at_the_limit(tmp_path, gpu_ctx, oracle):
    """b: the device-memory tier of k_styled_sort at 2 049 .. 65 536 areas (N == n at the limit: no virtual padding, the
    position field of the key full), over global ids at both ends of 32, 63 and 64 bits and 200 styles with many equal keys"""
    r = extreme_id_world(tmp_path, oracle)
    way_gids, mp_gids = model.gids(r)
    assert {0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 1} <= set(way_gids) and {2**63, 2**64 - 1} <= set(way_gids) & set(mp_gids)
    rng = np.random.default_rng(43)
    st, pool = fill_only_styles(rng)
    counts = [2049, 4097, 8191, 32769, 65535, 65536]
    pow2 = lambda n: 1 << (n - 1).bit_length()
    assert [pow2(n) for n in counts] == [4096, 8192, 8192, 65536, 65536, 65536] and counts[-1] == abi.STYLED_MAX_TILE_AREAS
    assert min(counts) > abi.STYLED_LDS_AREAS and len(st) == 200
    tx, ty = _center_tile(oracle)
    tiles = []
    for n in counts:
        n_w = int(0.8 * n)
        tiles.append((15, tx, ty, random_pairs(rng, n_w, r.n_ways, len(st)), random_pairs(rng, n - n_w, r.n_multipolygons, len(st))))
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    scene, got, want = _build_both(gpu_ctx, r, gid, tiles, st, pool, first)
    assert [int(n) for n in want.jobs["n_ops"]] == counts  # every area is one op
    _assert_same_list(got, want)
    assert [int(n) for n in got.jobs["n_ops"]] == counts and int(got.jobs["n_ops"][-1]) == 65536
    assert _validates(got)[0] == abi.OK
    firsts = model.first_nodes(r)
    for j, (_, _, _, ways, mps) in enumerate(tiles):
        assert np.array_equal(model.seen_marks(got, j), model.expected_marks(ways, mps, st, way_gids, mp_gids, *firsts)), j
    scene.free()
    r.close()


def _coloured(n, base):
    """n styles that draw nothing yet; style k of the table gets colours that name it and the pass"""
    st = np.zeros(n, STYLE_DTYPE)
    st["is_foreground_fill"] = 1
    for k in range(n):
        st[k]["fill_color"], st[k]["casing_color"], st[k]["color"] = (base + k, 1, 0), (base + k, 2, 0), (base + k, 3, 0)
    return st


def test_c_ranks_that_move_under_an_old_batch(gpu_ctx, world):
    """c: registering styles whose keys interleave the old ones re-ranks every old style (sync_styles); an old batch rebuilt
    afterwards is the same bytes, and a batch that mixes both tables is ordered as if they had been one from the start"""
    r = world.r
    rng = np.random.default_rng(47)
    A = _coloured(6, 0)
    A["has_fill_color"], A["z_index"] = 1, [1.0, 3.0, 5.0, 1.0, 3.0, 5.0]
    A["has_layer"], A["layer"] = [0, 0, 0, 1, 1, 1], [0, 0, 0, -2, 2, 2]
    A["has_color"][[1, 4]], A["has_width"][[1, 4]], A["width"][[1, 4]] = 1, 1, 2.0
    A[4]["has_dashes"], A[4]["dashes_off"], A[4]["n_dashes"] = 1, 0, 2
    pool_a = np.array([4.0, 2.0, 0.0])
    first_a = gpu_ctx.register_styles(recs_of(A), pool_a)
    tx, ty = world.tiles[0][1], world.tiles[0][2]
    X = [_cycled_tile(rng, 15, tx, ty, n, r.n_ways, r.n_multipolygons, len(A)) for n in (0, 200, 37, 2100)]
    scene, got_x, want_x = _build_both(gpu_ctx, r, world.gid, X, A, pool_a, first_a)
    _assert_same_list(got_x, want_x)
    scene.free()
    B = _coloured(9, len(A))
    B["has_fill_color"], B["z_index"] = 1, [0.0, 2.0, 4.0, 6.0, 0.0, 2.0, 4.0, 6.0, 2.0]
    B["has_layer"], B["layer"] = [0, 0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 0, -3, -1, 2, 3, 0]
    B["is_foreground_fill"][8] = 0
    for k, (off, cnt) in ((1, (0, 3)), (5, (3, 1)), (7, (0, 3))):
        B[k]["has_color"], B[k]["has_width"], B[k]["width"], B[k]["line_cap"] = 1, 1, 1.5, abi.CAP_ROUND
        B[k]["has_dashes"], B[k]["dashes_off"], B[k]["n_dashes"] = 1, off, cnt
    B[3]["has_casing_color"], B[3]["has_casing_width"], B[3]["casing_width"] = 1, 1, 5.0
    B[3]["has_casing_dashes"], B[3]["casing_dashes_off"], B[3]["n_casing_dashes"] = 1, 1, 2
    pool_b = np.array([6.0, 1.0, 2.5, 3.0, 0.0])
    first_b = gpu_ctx.register_styles(recs_of(B), pool_b)
    assert first_b == first_a + len(A)
    # every rank of A moved: B has a key below A's lowest, and keys between each two neighbours of A's
    both = np.concatenate([A, B])
    both["dashes_off"][len(A):] += np.where(B["has_dashes"] != 0, len(pool_a), 0).astype(np.uint32)
    both["casing_dashes_off"][len(A):] += np.where(B["has_casing_dashes"] != 0, len(pool_a), 0).astype(np.uint32)
    pool_both = np.concatenate([pool_a, pool_b])
    key = lambda s: (int(s["layer"]) if s["has_layer"] else 0, int(s["is_foreground_fill"]), float(s["z_index"]))
    keys_a, keys_b = sorted({key(s) for s in A}), sorted({key(s) for s in B})
    assert not set(keys_a) & set(keys_b) and keys_b[0] < keys_a[0] and keys_b[-1] > keys_a[-1]
    assert all(any(lo < k < hi for k in keys_b) for lo, hi in zip(keys_a, keys_a[1:]))
    again = gpu_ctx.build_styled(_batch(world.gid, X, first_a))
    _assert_same_list(again.read_display_list(), got_x)
    again.free()
    Y = [_cycled_tile(rng, 15, tx, ty, n, r.n_ways, r.n_multipolygons, len(both)) for n in (300, 0, 2500)]
    scene, got_y, want_y = _build_both(gpu_ctx, r, world.gid, Y, both, pool_both, first_a)
    _assert_same_list(got_y, want_y)
    assert _validates(got_y)[0] == abi.OK and len(got_y.dashes) > 0 and (got_y.ops["has_dashes"] != 0).any()
    way_gids, mp_gids = model.gids(r)
    firsts = model.first_nodes(r)
    for j, (_, _, _, ways, mps) in enumerate(Y):
        styles_seen = {s for _, s in ways + mps}
        assert j == 1 or (min(styles_seen) < len(A) <= max(styles_seen))
        assert np.array_equal(model.seen_marks(got_y, j), model.expected_marks(ways, mps, both, way_gids, mp_gids, *firsts)), j
    scene.free()


def _refused(gpu_ctx, sb):
    b, h = sb.as_batch(), C.c_void_p(1)
    rc = lib.load().osmt_scene_build_styled(gpu_ctx._h, C.byref(b), C.byref(h))
    return rc, h.value, lib.load().osmt_last_error().decode()


def test_d_totals_beyond_32_bits_are_refused_with_the_exact_figure(tmp_path, gpu_ctx):
    """d: the scans are 32-bit and wrap; what makes that safe is that the block totals and their scan are 64-bit and that the
    host refuses a total of 2^32 or more before anything is emitted.  Nothing is drawn and nothing is allocated for the list:
    the refusal names the total, and the figure must be the arithmetic one.

    One way of 70 000 nodes, 65 536 areas: 65 536 x 70 000 = 4 587 520 000 node references (every partial sum inside a wave
    still fits 32 bits).  One multipolygon that lists a 70 000-node polygon 2 048 times has 143 360 000 nodes; 65 536 areas
    of it need 65 536 x 143 360 000 = 9 395 240 960 000 references: 32 lanes of a wave already sum to more than 2^32, so the
    high words of wave_sum64 and of the block scan's shuffles carry information, over three chunks of the block scan."""
    N, K, AREAS = 70000, 2048, abi.STYLED_MAX_TILE_AREAS
    nodes = [(1000 + i, LAT0 + 1e-7 * i, LON0 + (1e-4 if i % 2 else 0.0), {}) for i in range(N)]
    ring = list(range(N))
    p = str(tmp_path / "long.bin")
    write_geodata(p, nodes, [(1, ring, {}), (2, ring[:3], {})], [ring], [(3, [0] * K, {})], tile_refs={})
    r = Reader(p)
    assert len(r.way_nodes(0)) == N and len(r.multipolygon_polygons(0)) == K
    st = np.zeros(3, STYLE_DTYPE)
    st["is_foreground_fill"] = 1
    st[0]["has_fill_color"], st[0]["fill_color"] = 1, (1, 2, 3)
    st[1]["has_color"], st[1]["has_width"], st[1]["width"], st[1]["line_cap"] = 1, 1, 2.0, abi.CAP_ROUND
    st[2]["has_fill_color"], st[2]["has_color"] = 1, 1
    pool = np.zeros(1)
    gid = gpu_ctx.register_geodata(geodata_of(r))
    first = gpu_ctx.register_styles(recs_of(st), pool)
    small = [(15, 1, 2, [(1, 2), (0, 0), (1, 1)], []), (15, 1, 3, [], []), (15, 2, 2, [(0, 1), (1, 0)], [])]

    def small_build_is_right():
        scene, got, want = _build_both(gpu_ctx, r, gid, small, st, pool, first)
        assert len(want.coords) == 2 * N + 4 * 3
        _assert_same_list(got, want)
        scene.free()

    small_build_is_right()
    # (what, tile, the total the refusal must name): node references come before virtual stroke segments in the host's order,
    # and the stroke-only tile has 65 536 x 70 000 of the former (and 65 536 x 70 001 of the latter)
    cases = (("fill", ([(0, 0)] * AREAS, []), AREAS * N), ("round-capped stroke", ([(0, 1)] * AREAS, []), AREAS * N),
             ("multipolygon", ([], [(0, 0)] * AREAS), AREAS * K * N))
    assert cases[0][2] == 4587520000 and cases[2][2] == 9395240960000 and 32 * K * N > 2**32 and (3 * AREAS) // WG > 2 * WG
    for what, (ways, mps), total in cases:
        rc, handle, msg = _refused(gpu_ctx, _batch(gid, [(15, 1, 2, ways, mps)], first))
        print(what, rc, msg)
        assert rc == abi.UNSUPPORTED and not handle, (what, rc, msg)
        assert "node references" in msg and f"needs {total} node references" in msg, (what, msg)
        small_build_is_right()
    r.close()


@pytest.mark.parametrize("most,where", [(128, "first"), (128, "last"), (129, "first"), (129, "last")])
def test_e_the_list_kernel_switch(gpu_ctx, world, most, where):
    """e: batches of 64 tiles take k_raster<FOLD>, and k_sublist runs only if s->max_job_ops (k_styled_tilemax) says that a
    tile has more than OSMT_FOLD_MAX_OPS = 128 ops; fill-only styles on entities with rings: ops == areas"""
    r = world.r
    rng = np.random.default_rng(53 + most)
    st, pool = fill_only_styles(rng, 24)
    first = gpu_ctx.register_styles(recs_of(st), pool)
    counts = [0 if k % 9 == 4 else int(rng.integers(1, 41)) for k in range(64)]
    counts[0 if where == "first" else 63] = most
    tx, ty = world.tiles[0][1], world.tiles[0][2]
    # the world lies in tile (tx, ty): the fullest tile is that one wherever it stands in the batch, so that its ops show
    tiles = [_cycled_tile(rng, 15, tx + (k % 2 if n != most else 0), ty, n, r.n_ways, r.n_multipolygons, len(st)) for k, n in enumerate(counts)]
    scene, got, want = _build_both(gpu_ctx, r, world.gid, tiles, st, pool, first)
    n_ops = [int(n) for n in got.jobs["n_ops"]]
    assert n_ops == counts and len(n_ops) == 64 and max(n_ops) == most and n_ops.index(most) == (0 if where == "first" else 63)
    assert sorted(n_ops)[-2] <= 40 and 0 in n_ops
    _assert_same_list(got, want)
    assert scene.max_tile_ops() == most
    px = gpu_ctx.render(scene).cpu().numpy()
    scene.check()
    assert np.array_equal(px, gpu_ctx.render_batch_host(want))
    k = n_ops.index(most)
    assert not (px[k] == CANVAS).all() and (px[n_ops.index(0)] == CANVAS).all()
    scene.free()


@pytest.mark.parametrize("lo,hi,scale", [(600, 900, 1), (700, 770, 2)])
def test_f_built_scenes_above_64_and_above_256_tiles(gpu_ctx, world, lo, hi, scale):
    """f: tiles cut from batch a, rendered: above 64 tiles every tile's list comes from k_sublist, and the pre-pass reads the
    op tables the build wrote (op_job, op_aux, op_blk, op_vseg); pixels and projected points against the host-built twin"""
    w = world
    tiles = w.tiles[lo:hi]
    n = len(tiles)
    assert (n > 256 if scale == 1 else 64 < n <= 256)
    scene, got, want = _build_both(gpu_ctx, w.r, w.gid, tiles, w.st, w.pool, w.first, scale=scale)
    _assert_same_list(got, want)
    assert _validates(got)[0] == abi.OK
    n_ops = want.jobs["n_ops"]
    assert (n_ops == 0).any() and int(n_ops.max()) > 128
    strokes = want.ops[want.ops["kind"] == abi.OP_STROKE]
    assert (strokes["has_dashes"] != 0).any() and {abi.CAP_ROUND, abi.CAP_SQUARE, abi.CAP_BUTT} <= set(strokes["cap"].tolist())
    assert (want.rings["n_pts"][want.ops["ring_off"][want.ops["n_rings"] == 1]] == 130).any()  # an op with a block table
    px = gpu_ctx.render(scene).cpu().numpy()
    scene.check()
    assert px.shape == (n, 256 * scale, 256 * scale, 4)
    assert np.array_equal(px, gpu_ctx.render_batch_host(want))
    empty = int(np.nonzero(n_ops == 0)[0][0])
    drawn = int(np.argmax(np.where(np.arange(n) % 2 == 0, n_ops, 0)))  # lo is even: the even tiles of the cut are the world's tile
    assert lo % 2 == 0 and (px[empty] == CANVAS).all() and not (px[drawn] == CANVAS).all()
    twin = gpu_ctx.upload(want)
    assert scene.max_tile_ops() == twin.max_tile_ops() == int(n_ops.max())
    assert np.array_equal(gpu_ctx.render(twin).cpu().numpy(), px)
    pts = gpu_ctx.read_points(scene)
    assert len(pts) == len(want.coords) and np.array_equal(pts, gpu_ctx.read_points(twin))
    twin.free()
    scene.free()
