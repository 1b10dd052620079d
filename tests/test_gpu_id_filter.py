"""The osm_ids filter on the GPU (osmt_register_id_filter, osmt_read_id_filter, osmt_scene_build_tiles_filtered;
k_idf_plane in osm_renderer_amd/csrc/osmt_idfilter.hip, the keep planes of k_tq_mark / k_tq_emit and k_tl_mark).

The yardsticks are not under test: np.isin for the planes; the UNFILTERED styled batch of the same tiles with the areas of
unlisted entities deleted by numpy; the host twins with their osm_ids argument (tests/_idfilter.py), which
tests/test_idfilter_cpu.py holds against Python restatements; osmt_scene_build_styled over the twin's areas for the display
list; the oracle for pixels and label statuses.  The suite runs on poisoned device memory (tests/conftest.py): a word of a plane
the kernel did not write reads 0xA5A5A5A5."""
import numpy as np
import pytest

from osm_renderer_amd import abi, labels, styled
from tests import _arealabels as al
from tests import _idfilter as idf
from tests import _tilelabels as tl
from tests import _tilequery as tq
from tests._tilequery import center_z18
from tests.test_gpu_area_labels import CANVAS, TEXTS, TX, TY, World, Z, _err, _images, _latlon, _oracle_labels, _same, tables, town  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

A = abi
MP = al.MP
CX, CY = center_z18()
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]  # the word, wave and workgroup edges
EDGE_IDS = [0, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, (7 << 32) | 5, (7 << 32) | 6, (8 << 32) | 5]  # low word apart, high word apart


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(COUNTS)))
def test_planes_equal_isin(gpu_ctx, k):
    """ways, multipolygons and nodes take three different counts of COUNTS per case, every count once per kind over the cases"""
    rng = np.random.default_rng(100 + k)
    n_w, n_m, n_n = COUNTS[k], COUNTS[(k + 3) % len(COUNTS)], COUNTS[(k + 6) % len(COUNTS)]
    pool = np.array(EDGE_IDS + rng.integers(0, 1 << 63, 4000, dtype=np.uint64).tolist(), dtype=np.uint64)
    pick = lambda n: np.concatenate([pool[: min(n, len(EDGE_IDS))], rng.choice(pool, max(n - len(EDGE_IDS), 0))])[:n] if n else np.zeros(0, np.uint64)
    wg, mg, ng = pick(n_w), pick(n_m), rng.permutation(pick(n_n))
    nodes = np.stack([55.0 + 1e-5 * np.arange(n_n), 37.0 + np.zeros(n_n)], axis=1) if n_n else np.zeros((0, 2))
    gid = gpu_ctx.register_geodata(styled.Geodata(nodes, [(int(g), []) for g in wg], [], [(int(g), []) for g in mg]))
    gpu_ctx.register_tile_index(gid, styled.TileIndex([((CX, CY), [], [])]))
    sets = {0: [], 1: [int(pool[5])], 2: [(7 << 32) | 5, 1 << 63], 1000: rng.choice(pool, 1000).tolist() + EDGE_IDS[:5]}  # any order, repeats
    before = gpu_ctx.register_id_filter(gid, sets[1000])  # no node index yet: no node plane
    gpu_ctx.register_node_index(gid, styled.NodeIndex(ng, [list(range(n_n))]))
    for n_ids, ids in sets.items():
        f = gpu_ctx.register_id_filter(gid, ids)
        for got, gids, name in zip(gpu_ctx.read_id_filter(f), (wg, mg, ng), ("ways", "multipolygons", "nodes")):
            want = idf.numpy_plane(gids, ids)
            assert len(got) == (len(gids) + 63) // 64 * 2 and np.array_equal(got, want), (name, len(gids), n_ids)
            assert np.array_equal(got, idf.host_plane(gids, ids))
            bits = np.unpackbits(got.view(np.uint8), bitorder="little")
            assert not bits[len(gids) :].any()  # the bits past the entity count, on poisoned memory
            if n_ids == 1000 and len(gids) > 8:
                assert 0 < bits.sum() < len(gids)
    w, m, n = gpu_ctx.read_id_filter(before)
    assert len(n) == 0 and np.array_equal(w, idf.numpy_plane(wg, sets[1000])) and np.array_equal(m, idf.numpy_plane(mg, sets[1000]))


# ---- filtered scenes ---------------------------------------------------------------------------------------------------------
FAR, TILES = idf.far_and_tiles(Z, TX, TY)  # no index tile near FAR: plain canvas, in the middle and at the end
Feed, _half = idf.Feed, idf.half_of_the_ids


@pytest.fixture(scope="module")
def feed(gpu_ctx, tables, town, tmp_path_factory):  # noqa: F811
    f = Feed(gpu_ctx, town, tmp_path_factory.mktemp("idf") / "town_nodes.bin", TEXTS, CANVAS)
    yield f
    f.close()


def _same_nodes(got, want):
    assert got.job_label_off.tolist() == want.job_label_off.tolist()
    for name in ("labels", "runs", "chars"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(_u8(g), _u8(w)), name


def _dl_bytes(dl):
    return [_u8(a).tobytes() for a in (dl.jobs, dl.ops, dl.rings, dl.coords, dl.dashes)]


def test_styled_batch_is_the_unfiltered_one_with_unlisted_areas_deleted(gpu_ctx, feed):
    ids = _half(feed)
    f = gpu_ctx.register_id_filter(feed.W.gid, ids)
    tiles = TILES + [(Z - 2, TX >> 2, TY >> 2), (0, 0, 0)]  # mixed zooms: the whole town in one tile
    plain, flt = feed.scene(tiles), feed.scene(tiles, flt=f)
    t0, a0 = plain.read_styled_areas()
    t1, a1 = flt.read_styled_areas()
    keep = np.isin(feed.gid_of(a0["entity"]), ids)
    assert 0 < keep.sum() < len(keep)  # something was filtered out, something stays
    assert np.array_equal(_u8(a1), _u8(a0[keep]))
    n = [int(keep[int(t["area_off"]) : int(t["area_off"]) + int(t["n_areas"])].sum()) for t in t0]
    want_t = t0.copy()
    want_t["n_areas"], want_t["area_off"] = n, np.concatenate([[0], np.cumsum(n)[:-1]])
    assert np.array_equal(_u8(t1), _u8(want_t))
    # the filtered mirror, and the display list osmt_scene_build_styled makes of the mirror's areas
    mirror = [idf.areas(feed.tqm, z, x, y, ids) for z, x, y in tiles]
    assert np.array_equal(_u8(a1), _u8(np.concatenate(mirror)))
    split = lambda a: ([(int(e), int(s)) for e, s in zip(a["entity"], a["style"]) if not e & MP], [(int(e) & ~MP, int(s)) for e, s in zip(a["entity"], a["style"]) if e & MP])
    built = gpu_ctx.build_styled(styled.StyledBatch(feed.W.gid, [(z, x, y) + split(a) for (z, x, y), a in zip(tiles, mirror)], canvas=CANVAS))
    assert _dl_bytes(flt.read_display_list()) == _dl_bytes(built.read_display_list())
    assert _dl_bytes(flt.read_display_list()) != _dl_bytes(plain.read_display_list())
    for s in (plain, flt, built):
        s.free()


def test_a_filter_of_every_id_and_the_empty_filter(gpu_ctx, feed):
    W = feed.W
    every = gpu_ctx.register_id_filter(W.gid, np.concatenate([feed.node_gid, feed.mp_gid, feed.way_gid]))
    empty = gpu_ctx.register_id_filter(W.gid, [])
    plain, full, none = feed.scene(TILES), feed.scene(TILES, flt=every), feed.scene(TILES, flt=empty)
    assert _dl_bytes(full.read_display_list()) == _dl_bytes(plain.read_display_list())  # byte for byte
    for a, b in zip(full.read_styled_areas(), plain.read_styled_areas()):
        assert np.array_equal(_u8(a), _u8(b))
    binds = ({Z: W.all[0]}, {Z: feed.node_bind})
    area_f, node_f = full.build_tile_labels_all(*binds)
    area_p, node_p = plain.build_tile_labels_all(*binds)
    _same(area_f, area_p)
    _same_nodes(node_f, node_p)
    assert len(area_p.labels) > 20 and len(node_p.labels) > 5
    assert np.array_equal(gpu_ctx.render(full).cpu().numpy(), gpu_ctx.render(plain).cpu().numpy())
    # Some(empty) keeps nothing: plain canvas in every tile, no labels of either kind
    assert none.read_styled_areas()[0]["n_areas"].tolist() == [0] * len(TILES) and len(none.read_styled_areas()[1]) == 0
    area_n, node_n = none.build_tile_labels_all(*binds)
    assert len(area_n.labels) == 0 and len(node_n.labels) == 0 and area_n.job_label_off.tolist() == [0] * (len(TILES) + 1)
    assert node_n.job_label_off.tolist() == [0] * (len(TILES) + 1) and len(none.label_status()) == 0
    px = gpu_ctx.render(none).cpu().numpy()
    assert (px[..., :3] == np.array(CANVAS, np.uint8)).all() and (px[..., 3] == 255).all()
    assert len(np.unique(gpu_ctx.render(plain).cpu().numpy()[0].reshape(-1, 4), axis=0)) > 3
    for s in (plain, full, none):
        s.free()


@pytest.mark.parametrize("scale", [1, 2])
def test_labels_and_pixels_of_a_filtered_scene(gpu_ctx, oracle, tables, feed, scale):  # noqa: F811
    W = feed.W
    ids = _half(feed, seed=7)
    f = gpu_ctx.register_id_filter(W.gid, ids)
    sc, plain = feed.scene(TILES, scale, flt=f), feed.scene(TILES, scale)
    binds = ({Z: W.all[0]}, {Z: feed.node_bind})
    area, node = sc.build_tile_labels_all(*binds)
    want_area, want_node = feed.want_labels(TILES, scale, ids)
    _same(area, want_area)  # byte for byte the filtered mirrors
    _same_nodes(node, want_node)
    alone = sc.build_tile_labels(binds[1])  # the node-only call applies the scene's filter too
    _same_nodes(alone, want_node)
    area, node = sc.build_tile_labels_all(*binds)
    all_area, all_node = plain.build_tile_labels_all(*binds)
    assert 0 < len(area.labels) < len(all_area.labels) and 0 < len(node.labels) < len(all_node.labels)  # something was filtered out
    n = np.diff(area.job_label_off).tolist()
    assert n[2] == 0 and n[4] == 0 and min(n[0], n[1], n[3]) >= 2
    out, st = gpu_ctx.render(sc).cpu().numpy(), sc.label_status()
    both = labels.splice_string_labels(want_area, want_node)
    assert len(st) == len(both.labels)
    ref, rst = oracle.render_batch(_latlon(sc.dl), images=_images(tables), threads=5, labels=_oracle_labels(both, tables), want_status=True)
    assert np.array_equal(st, rst) and 1 in rst.tolist()
    assert np.array_equal(out, ref)
    bare = feed.scene(TILES, scale, flt=f)
    bare_px = gpu_ctx.render(bare).cpu().numpy()
    assert not np.array_equal(bare_px[0], out[0])  # the labels are in the pixels
    assert not np.array_equal(bare_px[0], gpu_ctx.render(plain).cpu().numpy()[0])  # and the unlisted areas are not (plain carries labels too)
    assert len(np.unique(out[2].reshape(-1, 4), axis=0)) == 1
    for s in (sc, plain, bare):
        s.free()


# ---- refusals, snapshots -----------------------------------------------------------------------------------------------------
def test_refusals_each_followed_by_a_correct_call(gpu_ctx, tables, feed, tmp_path):  # noqa: F811
    W = feed.W
    f = gpu_ctx.register_id_filter(W.gid, feed.way_gid[:10])
    _err(lambda: feed.scene(TILES, flt=f + 1000), A.INVALID_ARG, f"id filter {f + 1000}", "not registered")
    _err(lambda: gpu_ctx.read_id_filter(f + 1000), A.INVALID_ARG, f"id filter {f + 1000}", "not registered")
    _err(lambda: gpu_ctx.register_id_filter(1 << 20, [1]), A.INVALID_ARG, f"geodata id {1 << 20}", "not registered")
    feed.scene(TILES, flt=f).free()
    # a filter of another geodata id; the node index of that file comes after its first filter
    V = World(gpu_ctx, tables, tmp_path / "other.bin", al.feature_world((CX, CY), [0, 1 << 32, (1 << 64) - 1, 77, 78]),
              [[0], [0], [], [], [0], [0], [0], [0]])  # every way of two nodes and more is drawn
    early = gpu_ctx.register_id_filter(V.gid, [77, 0, 5])
    _err(lambda: feed.scene(TILES, flt=early), A.INVALID_ARG, f"id filter {early}", f"belongs to geodata id {V.gid}, not {W.gid}")
    near = [(18, CX, CY)]
    batch = styled.TileBatch(V.gid, near, {18: V.draw_bind}, canvas=CANVAS)
    sc = gpu_ctx.build_tiles(batch, id_filter=early)
    assert set(sc.read_styled_areas()[1]["entity"].tolist()) == {0, 4}  # the ways of global ids 0 and 77 (5 is a way without nodes: not drawn)
    node_refs = {k: (list(range(6)) if k == (CX, CY) else [], v[1], v[2]) for k, v in V.refs.items()}
    gpu_ctx.register_node_index(V.gid, tl.node_index_of(V.r, node_refs))
    nid = gpu_ctx.register_label_bindings(styled.LabelBindings(V.gid, 0, 18, [[(V.first + 4, 4)]] * 6 + [[]] * (V.r.n_nodes - 6), TEXTS))
    _err(lambda: sc.build_tile_labels_all(None, {18: nid}), A.INVALID_ARG, "no node plane", "register the node index first")
    _err(lambda: sc.build_tile_labels({18: nid}), A.INVALID_ARG, "no node plane", "osmt_register_node_index")
    assert len(gpu_ctx.read_id_filter(early)[2]) == 0
    sc.free()
    node_gids = [V.r.global_id(0, i) for i in range(V.r.n_nodes)]
    late = gpu_ctx.register_id_filter(V.gid, [77, 0, 5, node_gids[1], node_gids[4], node_gids[9]])  # node 9 is listed by no tile
    sc = gpu_ctx.build_tiles(batch, id_filter=late)
    _, node = sc.build_tile_labels_all(None, {18: nid})
    assert len(node.labels) == 2 and len(sc.label_status()) == 2
    pts = gpu_ctx.project(V.ll, 18, CX, CY, 1.0)  # the two listed nodes of the tile, at their projected points
    want_xy = sorted((float(pts[i][0]), float(pts[i][1])) for i in (1, 4))
    assert sorted(zip(node.labels["icon_center_x"].tolist(), node.labels["icon_center_y"].tolist())) == want_xy
    sc.free()
    V.close()


def test_a_later_registration_does_not_disturb_a_built_scene(gpu_ctx, feed):
    W = feed.W
    ids = _half(feed, seed=9)
    f = gpu_ctx.register_id_filter(W.gid, ids)
    sc = feed.scene(TILES, flt=f)
    binds = ({Z: W.all[0]}, {Z: feed.node_bind})
    area0, node0 = sc.build_tile_labels_all(*binds)
    px0, plane0 = gpu_ctx.render(sc).cpu().numpy(), gpu_ctx.read_id_filter(f)
    later = [gpu_ctx.register_id_filter(W.gid, _half(feed, seed=20 + k)[: 1 + 37 * k]) for k in range(6)]
    later.append(gpu_ctx.register_id_filter(W.gid, np.arange(200000, dtype=np.uint64)))
    assert later == list(range(f + 1, f + 8))
    area1, node1 = sc.build_tile_labels_all(*binds)  # the scene's snapshot, not the newest filter
    _same(area1, area0)
    _same_nodes(node1, node0)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), px0)
    assert all(np.array_equal(a, b) for a, b in zip(gpu_ctx.read_id_filter(f), plane0))
    sc.free()
