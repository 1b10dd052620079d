"""Tile requests: (z, x, y, scale) in, PNG out (osmt_tile_server_create, osmt_tile_server_render_png,
osmt_last_declined_anchors, osmt_worker_render_tile_png, osmt_worker_tile_stats).

The yardstick is the three-call chain the entries replace — osmt_scene_build_tiles[_filtered], osmt_scene_build_tile_labels_all,
osmt_render_scene_png — whose files the entries must repeat byte for byte, whatever group a request rode in; the chain's own
parts are held against mirrors and the oracle elsewhere (tests/test_gpu_id_filter.py, tests/test_gpu_scene_png.py), and for
small batches the decoded files are compared with the oracle's pixels here once more."""
import ctypes as C
import io
import subprocess
import threading

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled, synth
from osm_renderer_amd.lib import OsmtError
from osm_renderer_amd.renderer import TileServer, last_declined_anchors
from tests import _anchors as an
from tests import _arealabels as al
from tests import _idfilter as idf
from tests import _tilelabels as tl
from tests import _tilerequests
from tests._styled_feed import geodata_of
from tests._tilequery import center_z18
from tests.test_gpu_area_labels import CANVAS, TEXTS, TX, TY, World, Z, _err, _images, _latlon, _oracle_labels, tables, town  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

A = abi
CX, CY = center_z18()
FAR, TILES = idf.far_and_tiles(Z, TX, TY)
_half = idf.half_of_the_ids


def _decode(png):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png)).convert("RGB"))


class Servers:
    """the labelled town of tests/_idfilter.Feed behind two tile servers, one of them filtered, and the chain they replace"""

    def __init__(self, ctx, feed):
        self.ctx, self.feed = ctx, feed
        W = feed.W
        self.flt = ctx.register_id_filter(W.gid, _half(feed, seed=13))
        self.binds = ({z: W.all[0] for z in range(19)}, {z: feed.node_bind for z in range(19)})
        kw = dict(area_label_bindings=self.binds[0], node_label_bindings=self.binds[1], canvas=CANVAS)
        self.plain = ctx.tile_server(W.gid, {z: feed.draw for z in range(19)}, **kw)
        self.filtered = ctx.tile_server(W.gid, {z: feed.draw for z in range(19)}, id_filter=self.flt, **kw)
        self._memo = {}

    def of(self, filtered):
        return self.filtered if filtered else self.plain

    def chain(self, tiles, scale, filtered, want_scene=False):
        """build -> label -> files, by the three calls; with want_scene also (scene, area batch, node batch): the caller frees it"""
        sc = self.feed.scene(tiles, scale, flt=self.flt if filtered else None)
        area, node = sc.build_tile_labels_all(*self.binds)
        files = self.ctx.render_scene_png(sc) if tiles else []
        if want_scene:
            return files, sc, area, node
        sc.free()
        return files

    def chain_one(self, tile, scale, filtered):
        key = (tile, scale, filtered)
        if key not in self._memo:
            self._memo[key] = self.chain([tile], scale, filtered)[0]
        return self._memo[key]

    def close(self):
        self.plain.close(), self.filtered.close()


@pytest.fixture(scope="module")
def feed(gpu_ctx, tables, town, tmp_path_factory):  # noqa: F811
    f = idf.Feed(gpu_ctx, town, tmp_path_factory.mktemp("req") / "town_nodes.bin", TEXTS, CANVAS)
    yield f
    f.close()


@pytest.fixture(scope="module")
def servers(gpu_ctx, feed):
    s = Servers(gpu_ctx, feed)
    yield s
    s.close()


def _tiles_of(n):
    if n <= 1:
        return TILES[:n]
    if n == 5:
        return list(TILES)  # far tiles in the middle and at the end
    town_tiles = [(Z, TX + k % 10, TY + k // 10) for k in range(n - 2)]
    return town_tiles[:30] + [FAR[0]] + town_tiles[30:] + [FAR[1]]


# ---- the server ----------------------------------------------------------------------------------------------------------------
def test_server_refusals_name_their_offender(gpu_ctx, feed, servers):
    W, L, h = feed.W, lib.load(), gpu_ctx._h
    draw = {z: feed.draw for z in range(19)}

    def refused(words, *a, ctx=h, **kw):
        d = TileServer.describe(*a, **kw)
        rc = L.osmt_validate_tile_server(C.byref(d), ctx)
        msg = L.osmt_last_error().decode()
        assert rc == A.INVALID_ARG and all(w in msg for w in words), (rc, msg)
        if ctx:  # and no server comes of it
            with pytest.raises(OsmtError):
                gpu_ctx.tile_server(*a, **kw)

    refused(["geodata id", "no context"], W.gid, draw, ctx=None)
    assert L.osmt_validate_tile_server(None, h) == A.INVALID_ARG and "NULL" in L.osmt_last_error().decode()
    refused([f"geodata id {1 << 20}", "not registered"], 1 << 20, draw)
    refused(["bindings id 99999 of zoom 7", "not registered"], W.gid, {**draw, 7: 99999})
    refused(["area label bindings id 99999 of zoom 0", "not registered"], W.gid, draw, area_label_bindings={0: 99999})
    refused(["node label bindings id 99999 of zoom 18", "not registered"], W.gid, draw, node_label_bindings={18: 99999})
    refused(["id filter 99999", "not registered"], W.gid, draw, id_filter=99999)
    narrow, _ = W.bind([[(0, 0)]], [], 16, 18)
    refused([f"area label bindings id {narrow}", "covers zooms 16..18, not zoom 3"], W.gid, draw, area_label_bindings={3: narrow, 16: narrow})
    # tables and a filter of another file
    other = gpu_ctx.register_geodata(W.g)
    gpu_ctx.register_tile_index(other, styled.TileIndex([(k, W.refs[k][1], W.refs[k][2]) for k in sorted(W.refs)]))
    refused([f"bindings id {feed.draw} of zoom 0", f"belongs to geodata id {W.gid}, not {other}"], other, draw)
    theirs = gpu_ctx.register_id_filter(other, [1, 2, 3])
    refused([f"id filter {theirs}", f"belongs to geodata id {other}, not {W.gid}"], W.gid, draw, id_filter=theirs)
    nb_other = gpu_ctx.register_label_bindings(styled.LabelBindings(other, 0, 18, [[] for _ in range(W.r.n_nodes)], []))
    refused([f"geodata id {other}", "no node index"], other, {}, node_label_bindings={16: nb_other})
    # a filter registered before the node index has no node plane: nodes cannot be labelled under it
    fresh = gpu_ctx.register_geodata(W.g)
    gpu_ctx.register_tile_index(fresh, styled.TileIndex([(k, W.refs[k][1], W.refs[k][2]) for k in sorted(W.refs)]))
    early = gpu_ctx.register_id_filter(fresh, [1])
    gpu_ctx.register_node_index(fresh, styled.NodeIndex(feed.node_gid, [[] for _ in W.refs]))
    nb = gpu_ctx.register_label_bindings(styled.LabelBindings(fresh, 0, 18, [[] for _ in range(W.r.n_nodes)], []))
    refused([f"id filter {early}", "no node plane", "register the node index first"], fresh, {}, node_label_bindings={16: nb}, id_filter=early)
    gpu_ctx.tile_server(fresh, {}, node_label_bindings={16: nb}, id_filter=gpu_ctx.register_id_filter(fresh, [1])).close()  # and a correct one
    # per request: a zoom without bindings, a zoom with NONE in a label array that is not all-NONE, a tile outside its zoom
    only16 = gpu_ctx.tile_server(W.gid, {16: feed.draw}, canvas=CANVAS)
    _err(lambda: only16.render_png([TILES[0], (15, 3, 3)]), A.INVALID_ARG, "tile 1", "zoom 15 has no bindings")
    assert len(only16.render_png([TILES[0]])) == 1
    only16.close()
    gap = gpu_ctx.tile_server(W.gid, draw, area_label_bindings={16: W.all[0]}, canvas=CANVAS)
    _err(lambda: gap.render_png([TILES[0], (15, 3, 3)]), A.INVALID_ARG, "tile 1", "zoom 15 has no area label bindings")
    _err(lambda: gap.render_png([(16, 1 << 16, 0)]), A.INVALID_ARG, "tile 0", "outside")
    _err(lambda: gap.render_png([(19, 0, 0)]), A.INVALID_ARG, "tile 0", "zoom 19")
    _err(lambda: gap.render_png([TILES[0]], scale=5), A.INVALID_ARG, "scale 5")
    assert len(gap.render_png([TILES[0]])) == 1
    gap.close()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("n", [0, 1, 5, 65])
def test_render_png_equals_the_three_call_chain(gpu_ctx, oracle, tables, servers, n, scale, filtered):  # noqa: F811
    tiles = _tiles_of(n)
    assert len(tiles) == n
    files = servers.of(filtered).render_png(tiles, scale)
    want, sc, area, node = servers.chain(tiles, scale, filtered, want_scene=True)
    assert files == want and len(files) == n  # byte for byte
    assert servers.of(filtered).last_offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in want])]).astype(np.uint64).tolist()
    if 0 < n <= 5:
        both = labels.splice_string_labels(area, node) if len(area.labels) else node
        ref = oracle.render_batch(_latlon(sc.dl), images=_images(tables), threads=5, labels=_oracle_labels(both, tables))
        for i, png in enumerate(files):
            assert np.array_equal(_decode(png), ref[i][..., :3]), f"tile {i}: decoded pixels differ from the oracle"
        assert len(both.labels) > 0
    if n >= 5:
        assert files[0] != servers.of(not filtered).render_png(tiles[:1], scale)[0]  # the filter is in the files
        far = [i for i, t in enumerate(tiles) if t in FAR]
        assert len({files[i] for i in far}) == 1 and files[far[0]] != files[0]  # plain canvas, in the middle and at the end
    sc.free()


def test_a_capacity_one_byte_short_fills_the_offsets(gpu_ctx, servers):
    want = servers.chain(TILES, 1, True)
    total = sum(len(f) for f in want)
    off = np.concatenate([[0], np.cumsum([len(f) for f in want])]).tolist()
    s = servers.filtered
    _err(lambda: s.render_png(TILES, 1, out=np.empty(total - 1, np.uint8)), A.INVALID_ARG, "out_capacity", str(total))
    assert s.last_offsets.tolist() == off
    assert s.render_png(TILES, 1, out=np.empty(total, np.uint8)) == want  # the repeated call, with exactly the size reported


def _strip_world(ctx, tables, path):  # noqa: F811
    """the world of test_too_large_is_refused_read_and_rebuilt_with_the_callers_anchor: a strip the anchor search declines"""
    w = al.World((CX, CY))
    rect = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    near, east = (CX, CY), (CX + 1, CY)
    w.way(w.shape(rect(20, 20, 60, 60)), 5, [near])
    strip = w.way(w.shape(rect(0.0, 0.0, 5000.0, 0.01)), 6, [near, east])
    w.mp([w.polygon(w.shape(rect(100, 100, 30, 30)))], 7, [near])
    W = World(ctx, tables, path, w, [[0], [], []])
    bid, _ = W.bind([[(2, 0)], [(2, 0), (7, 4), (1, None)], []], [[(0, 0)]])
    return W, bid, strip, [(18, CX + 9, CY + 9), (18, *near), (18, *east)]


def _computed(W, dec, tiles):
    dec = dec.copy()
    for d in dec:
        p = an.mirror_position(W.g, W.f, int(d["entity"]), *tiles[int(d["tile"])], 1)
        assert p["status"] == A.LABEL_OK
        d["x"], d["y"], d["status"] = p["x"], p["y"], p["status"]
    return dec


@pytest.fixture(scope="module")
def strip(gpu_ctx, tables, tmp_path_factory):  # noqa: F811
    W, bid, way, tiles = _strip_world(gpu_ctx, tables, tmp_path_factory.mktemp("req") / "strip.bin")
    server = gpu_ctx.tile_server(W.gid, {18: W.draw_bind}, area_label_bindings={18: bid}, canvas=CANVAS)

    def chain(tl, anchors):
        sc = W.scene(tl)
        sc.build_tile_labels_all({18: bid}, None, anchors)
        files = gpu_ctx.render_scene_png(sc)
        sc.free()
        return files

    yield W, server, way, tiles, chain
    server.close()
    W.close()


def test_too_large_is_refused_listed_for_the_thread_and_repeated_with_anchors(gpu_ctx, strip):
    W, server, way, tiles, chain = strip
    _err(lambda: server.render_png(tiles), A.UNSUPPORTED, "declined 2", "tile 1", f"way {way}")
    dec = last_declined_anchors()
    assert [(int(d["tile"]), int(d["entity"]), int(d["status"])) for d in dec] == [(1, way, A.LABEL_TOO_LARGE), (2, way, A.LABEL_TOO_LARGE)]
    seen = []
    t = threading.Thread(target=lambda: seen.append(len(last_declined_anchors())))  # thread-local like osmt_last_error
    t.start(), t.join()
    assert seen == [0]
    dec = _computed(W, dec, tiles)
    _err(lambda: server.render_png(tiles, anchors=dec[:1]), A.UNSUPPORTED, "declined 1", "tile 2")
    assert [(int(d["tile"]), int(d["entity"])) for d in last_declined_anchors()] == [(2, way)]
    files = server.render_png(tiles, anchors=dec)
    assert len(last_declined_anchors()) == 0  # a call that declined nothing leaves nothing
    assert files == chain(tiles, dec)
    assert files[1] != files[0]


# ---- the per-request entry -----------------------------------------------------------------------------------------------------
def test_one_request_alone_is_the_one_tile_chain(gpu_ctx, servers):
    w = gpu_ctx.worker()
    before = gpu_ctx.worker_tile_stats()
    for tile, scale, filtered in ((TILES[0], 1, False), (TILES[3], 2, True), (FAR[0], 1, True)):
        assert w.render_tile_png(servers.of(filtered), tile, scale) == servers.chain_one(tile, scale, filtered)
    after = gpu_ctx.worker_tile_stats()
    assert after[0] - before[0] == 3 and after[1] - before[1] == 3 and after[2] >= 1  # a lone request is a group of one: it never waits
    # a buffer one byte short: the size needed, nothing written
    want = servers.chain_one(TILES[0], 1, False)
    out = np.full(len(want) - 1, 0x5A, np.uint8)
    _err(lambda: w.render_tile_png(servers.plain, TILES[0], 1, out=out), A.INVALID_ARG, "out_capacity", str(len(want)))
    assert w.last_len == len(want) and (out == 0x5A).all()
    assert w.render_tile_png(servers.plain, TILES[0], 1, out=np.empty(len(want), np.uint8)) == want
    other = __import__("osm_renderer_amd.renderer", fromlist=["Context"]).Context(0)
    theirs = other.worker()
    try:
        _err(lambda: theirs.render_tile_png(servers.plain, TILES[0]), A.INVALID_ARG, "another context")
    finally:
        theirs.close()
        other.close()
    _err(lambda: w.render_tile_png(servers.plain, TILES[0], anchors=np.array([(1, 0, 1.0, 1.0, A.LABEL_OK, 0)], labels.AREA_ANCHOR_DTYPE)),
         A.INVALID_ARG, "anchor 0", "tile 1")
    w.close()


def test_sixteen_threads_over_two_servers_scales_and_zooms(gpu_ctx, servers):
    tiles = [TILES[0], TILES[1], TILES[3], FAR[0], (Z, TX + 4, TY + 2), (Z - 1, TX >> 1, TY >> 1), (Z + 1, 2 * TX + 1, 2 * TY), FAR[1]]
    kinds = [(t, scale, filtered) for t in tiles for scale in (1, 2) for filtered in (False, True)]
    want = {k: servers.chain_one(*k) for k in kinds}
    assert len(set(want.values())) > len(tiles)
    n_threads, calls = 16, 12
    errors, counts = [], [0] * n_threads
    start = threading.Barrier(n_threads)
    before = gpu_ctx.worker_tile_stats()

    def body(t):
        try:
            w = gpu_ctx.worker()
            start.wait()
            for c in range(calls):
                tile, scale, filtered = k = kinds[(t * 7 + c * 13) % len(kinds)]
                got = w.render_tile_png(servers.of(filtered), tile, scale)
                if got != want[k]:
                    raise AssertionError(f"thread {t} call {c}: the file of {k} differs from the chain's")
                counts[t] += 1
            w.close()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:4]
    assert counts == [calls] * n_threads
    after = gpu_ctx.worker_tile_stats()
    assert after[0] - before[0] == 192 and 0 < after[1] - before[1] <= 192 and 1 <= after[2] <= 64


def test_bad_requests_fail_alone_among_good_ones_and_batch_requests_go_on(gpu_ctx, oracle, strip, servers):
    W, server, way, tiles, chain = strip
    far, near = tiles[0], tiles[1]
    good = {far: chain([far], None)[0], TILES[0]: servers.chain_one(TILES[0], 1, False)}
    dl = synth.make_tiles(synth.config_tiles(4, x0=19300, y0=10070))
    want_rgb = [np.ascontiguousarray(oracle.render_batch(dl, threads=4)[i : i + 1][..., :3]).reshape(1, -1) for i in range(4)]
    singles = [dl.subset([i]) for i in range(4)]
    n_threads = 12
    errors, done = [], []
    start = threading.Barrier(n_threads)

    def body(t):
        try:
            w = gpu_ctx.worker()
            start.wait()
            for c in range(6):
                if t == 0:  # a zoom the server has no bindings for: refused on its own thread, never queued
                    _err(lambda: w.render_tile_png(server, (17, CX >> 1, CY >> 1)), A.INVALID_ARG, "zoom 17 has no bindings")
                elif t == 1:  # needs an anchor: fails alone, its declined list is left for THIS thread, tile 0
                    _err(lambda: w.render_tile_png(server, near), A.UNSUPPORTED, "declined 1", f"way {way}")
                    dec = last_declined_anchors()
                    assert [(int(d["tile"]), int(d["entity"])) for d in dec] == [(0, way)], dec
                    anchors = _computed(W, dec, [near])
                    assert w.render_tile_png(server, near, anchors=anchors) == chain([near], anchors)[0]
                    assert len(last_declined_anchors()) == 0
                elif t < 6:  # good requests of the same server, in flight beside the bad ones
                    assert w.render_tile_png(server, far) == good[far]
                elif t < 9:  # another server
                    assert w.render_tile_png(servers.plain, TILES[0]) == good[TILES[0]]
                else:  # the batch entry shares the cap on groups in flight
                    i = (t + c) % 4
                    assert np.array_equal(w.render(singles[i]), want_rgb[i])
            w.close()
            done.append(t)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:4]
    assert sorted(done) == list(range(n_threads))


# ---- the C++ binding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale, filtered", [(1, False), (2, True)])
def test_cpp_demo_files_decode_to_the_python_paths_pixels(gpu_ctx, tmp_path, scale, filtered):
    """tests/tile_server_host_demo.cpp (TileServer::render_png, Worker::render_tile_png, the retry loop over
    osmt_last_declined_anchors) in a process of its own; the same world, styles, bindings and filter registered here give the
    files it must write and the pixels they must decode to"""
    w = al.World((CX, CY))
    rect = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    near, east = (CX, CY), (CX + 1, CY)
    w.way(w.shape(rect(20, 20, 60, 60)), 5, [near])
    strip = w.way(w.shape(rect(0.0, 0.0, 5000.0, 0.01)), 6, [near, east])  # an odd way: labelled, and its anchor is declined
    w.way(w.shape(rect(30, 150, 80, 40)), 7, [near])
    w.way(w.shape(rect(150, 150, 60, 60), east), 8, [east])
    w.mp([w.polygon(w.shape(rect(100, 100, 30, 30)))], 9, [near])
    path = tmp_path / "w.bin"
    r, refs = w.write(path)
    tiles = [(18, CX, CY), (18, CX + 9, CY + 9), (18, CX + 1, CY), (17, CX >> 1, CY >> 1)]
    ids = [8, 6, 9, 6, 12345] if filtered else None
    args = ["-1"] if ids is None else [str(len(ids))] + [str(v) for v in ids]
    out = subprocess.run([_tilerequests.build_demo(), str(path), str(scale), str(tmp_path)] + args + [str(v) for t in tiles for v in t],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    word, n_files, n_bytes, on_host = out.stdout.split()
    files = [(tmp_path / f"tile_{i}.png").read_bytes() for i in range(len(tiles))]
    assert word == "OK" and int(n_files) == len(tiles) and int(n_bytes) == sum(len(f) for f in files)
    assert int(on_host) == 2 * 3  # the strip under three of the four tiles, once in the batch call and once per request
    # the Python path
    g = geodata_of(r)
    gid = gpu_ctx.register_geodata(g)
    gpu_ctx.register_tile_index(gid, styled.TileIndex([(k, refs[k][1], refs[k][2]) for k in sorted(refs)]))
    f = an.mercator_factors(r.node_table())
    gpu_ctx.register_node_mercator(gid, f)
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
    draw = gpu_ctx.register_styles(st)
    bind = gpu_ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[draw]] * r.n_ways, [[draw]] * r.n_multipolygons))
    icon = ((37 * np.arange(7 * 3 * 4) + 11) % 256).astype(np.uint8).reshape(7, 3, 4)
    icon[..., 3] = 255
    ls = gpu_ctx.register_label_styles(tl.label_styles([dict(icon=gpu_ctx.register_image(icon))]))
    lb = gpu_ctx.register_area_label_bindings(styled.AreaLabelBindings(gid, 0, 18, [[(ls, None)] if i % 2 else [] for i in range(r.n_ways)],
                                                                       [[(ls, None)]] * r.n_multipolygons))
    flt = gpu_ctx.register_id_filter(gid, ids) if filtered else None
    sc = gpu_ctx.build_tiles(styled.TileBatch(gid, tiles, {z: bind for z in range(19)}, scale=scale, canvas=(241, 238, 232)), id_filter=flt)
    _err(lambda: sc.build_tile_labels_all({z: lb for z in range(19)}, None), A.UNSUPPORTED, "declined 3", f"way {strip}")
    dec = sc.read_declined_anchors()
    for d in dec:
        p = an.mirror_position(g, f, int(d["entity"]), *tiles[int(d["tile"])], scale)
        d["x"], d["y"], d["status"] = p["x"], p["y"], p["status"]
    area, _ = sc.build_tile_labels_all({z: lb for z in range(19)}, None, dec)
    assert (area.labels["has_icon"] == 1).sum() >= 4
    want = gpu_ctx.render(sc).cpu().numpy()
    assert gpu_ctx.render_scene_png(sc) == files
    for i, png in enumerate(files):
        assert np.array_equal(_decode(png), want[i][..., :3]), f"tile {i}"
    if filtered:  # the first square (global id 5) is not listed: its place is canvas
        assert (want[0][40, 40, :3] == np.array((241, 238, 232), np.uint8)).all() and len(np.unique(want[3].reshape(-1, 4), axis=0)) > 1
    sc.free()
    r.close()
