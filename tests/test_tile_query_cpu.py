"""The host side of scenes built from tile coordinates (include/osmtile.h, osmt_scene_build_tiles): the three validations,
none of which needs a device, and the helpers of host/osmt_tilequery.hpp — osmt::TileIndexDesc, osmt::StyleBindings and the
mirror osmt::styled_areas_of_tile, the yardstick of tests/test_gpu_tile_query.py.  The rules that compare a batch or a
bindings table with what a context has registered need a context and are checked there."""
import ctypes as C
import subprocess

import numpy as np

from osm_renderer_amd import abi, lib, styled
from tests import _tilequery as tq


def test_struct_layouts_match_the_header():
    s = tq.shim().tq_sizeof
    assert s(0) == C.sizeof(abi.TileIndexDesc)
    assert s(1) == C.sizeof(abi.StyleBindingsDesc)
    assert s(2) == C.sizeof(abi.QueryTile) == styled.QUERY_TILE_DTYPE.itemsize == 16
    assert s(3) == C.sizeof(abi.TileBatch)
    assert s(10) == abi.TileIndexDesc.n_multipolygon_refs.offset
    assert s(11) == abi.StyleBindingsDesc.way_style_off.offset
    assert s(12) == abi.StyleBindingsDesc.n_multipolygon_styles.offset
    assert s(13) == abi.QueryTile.canvas_rgb.offset == styled.QUERY_TILE_DTYPE.fields["canvas_rgb"][1]
    assert s(14) == abi.TileBatch.bindings_of_zoom.offset
    for name in ("osmt_register_tile_index", "osmt_register_style_bindings", "osmt_scene_build_tiles", "osmt_scene_read_styled_areas"):
        assert name in lib.EXPORTS and hasattr(lib.load(), name)
    assert (abi.QUERY_MAX_TILE_CANDIDATES, abi.QUERY_LDS_CANDIDATES, abi.BINDINGS_NONE) == (1 << 20, 8192, 0xFFFFFFFF)


def _index():
    return styled.TileIndex({(10, 5): ([0, 1], [0]), (10, 7): ([2], []), (12, 0): ([1, 1, 0], [1, 0])})


def _validate_index(ix, n_ways=3, n_mps=2):
    L = lib.load()
    d = ix.as_desc()
    rc = L.osmt_validate_tile_index(C.byref(d), n_ways, n_mps)
    return rc, L.osmt_last_error().decode()


def test_validate_tile_index_refusals():
    assert _validate_index(_index())[0] == abi.OK
    assert _validate_index(styled.TileIndex({}))[0] == abi.OK  # an index of no tiles
    cases = []

    def case(name, edit, word, **kw):
        ix = _index()
        edit(ix)
        cases.append(name)
        rc, msg = _validate_index(ix, **kw)
        assert rc == abi.INVALID_ARG and word in msg, (name, rc, msg)

    case("first offset not 0", lambda ix: ix.way_off.__setitem__(0, 1), "way_off[0]")
    case("decreasing offsets", lambda ix: ix.multipolygon_off.__setitem__(1, 4), "multipolygon_off[2]")
    case("offsets that stop short", lambda ix: ix.way_off.__setitem__(3, 5), "way_off[3]")
    case("equal tiles", lambda ix: ix.tile_xy.__setitem__(1, (10, 5)), "tile 1")
    case("y descending in a column", lambda ix: ix.tile_xy.__setitem__(1, (10, 4)), "tile 1")
    case("x descending", lambda ix: ix.tile_xy.__setitem__(2, (9, 9)), "tile 2")
    case("x outside the world", lambda ix: ix.tile_xy.__setitem__(2, (1 << 18, 0)), "tile 2")
    case("y outside the world", lambda ix: ix.tile_xy.__setitem__(2, (12, 1 << 18)), "tile 2")
    case("way id out of range", lambda ix: ix.ways.__setitem__(4, 3), "ways[4] = 3")
    case("multipolygon id out of range", lambda ix: None, "multipolygons[0] = 0", n_mps=0)
    assert len(cases) == 10
    # a NULL array with a non-zero count
    L, d = lib.load(), _index().as_desc()
    d.ways = None
    assert L.osmt_validate_tile_index(C.byref(d), 3, 2) == abi.INVALID_ARG and "NULL" in L.osmt_last_error().decode()
    d = _index().as_desc()
    d.tile_xy = None
    assert L.osmt_validate_tile_index(C.byref(d), 3, 2) == abi.INVALID_ARG and "NULL" in L.osmt_last_error().decode()
    assert L.osmt_validate_tile_index(None, 0, 0) == abi.INVALID_ARG
    # the largest coordinate is fine
    ix = _index()
    ix.tile_xy[2] = ((1 << 18) - 1, (1 << 18) - 1)
    assert _validate_index(ix)[0] == abi.OK


def test_validate_style_bindings_refusals_that_need_no_registration():
    """the zoom range is checked first, the geodata id next; offsets and style ids are compared with the context's tables (GPU tests)"""
    L = lib.load()

    def validate(b):
        d = b.as_desc()
        return L.osmt_validate_style_bindings(C.byref(d), None), L.osmt_last_error().decode()

    rc, msg = validate(styled.StyleBindings(0, 3, 2, [[0]], []))
    assert rc == abi.INVALID_ARG and "zoom range 3..2" in msg
    rc, msg = validate(styled.StyleBindings(0, 0, abi.MAX_ZOOM + 1, [[0]], []))
    assert rc == abi.INVALID_ARG and "zoom range 0..19" in msg
    rc, msg = validate(styled.StyleBindings(4, 0, 18, [[0]], []))
    assert rc == abi.INVALID_ARG and "geodata id 4 is not registered" in msg
    assert L.osmt_validate_style_bindings(None, None) == abi.INVALID_ARG


def test_validate_tile_batch_refusals_that_need_no_registration():
    L = lib.load()

    def validate(tb):
        b = tb.as_batch()
        return L.osmt_validate_tile_batch(C.byref(b), None), L.osmt_last_error().decode()

    tiles = [(15, 1, 2), (0, 0, 0), (18, (1 << 18) - 1, 0)]
    rc, msg = validate(styled.TileBatch(0, tiles, {}))
    assert rc == abi.INVALID_ARG and "geodata id 0 is not registered" in msg  # nothing else to object to
    for scale in (0, abi.MAX_SCALE + 1):
        rc, msg = validate(styled.TileBatch(0, tiles, {}, scale=scale))
        assert rc == abi.INVALID_ARG and "scale" in msg
    rc, msg = validate(styled.TileBatch(0, tiles + [(19, 0, 0)], {}))
    assert rc == abi.INVALID_ARG and "tile 3" in msg and "zoom 19" in msg
    rc, msg = validate(styled.TileBatch(0, tiles + [(15, 1 << 15, 0)], {}))
    assert rc == abi.INVALID_ARG and "tile 3" in msg and "32768" in msg
    rc, msg = validate(styled.TileBatch(0, [(0, 0, 1)], {}))
    assert rc == abi.INVALID_ARG and "tile 0" in msg
    assert L.osmt_validate_tile_batch(None, None) == abi.INVALID_ARG
    b = styled.TileBatch(0, tiles, {}).as_batch()
    b.tiles = None
    assert L.osmt_validate_tile_batch(C.byref(b), None) == abi.INVALID_ARG and "NULL" in L.osmt_last_error().decode()


def _sparse_world(tmp_path, rng, name="s.bin", n_ways=40, mp_polygons=(1, 0, 3, 2, 0, 1)):
    """index tiles scattered over the world's corners, edges and the middle, with lists that repeat ids"""
    refs = {}
    hi = tq.WORLD - 1
    spots = [(0, 0), (0, hi), (hi, 0), (hi, hi), (0, 1000), (1000, 0), (hi, 77), (77, hi), (131072, 131072), (131071, 131071), (131072, 131071),
             (131080, 131090), (70000, 70000), (70001, 70000), (70000, 70003)]
    for _ in range(60):
        cx, cy = spots[int(rng.integers(0, len(spots)))]
        x, y = min(hi, max(0, cx + int(rng.integers(-20, 21)))), min(hi, max(0, cy + int(rng.integers(-20, 21))))
        spots.append((x, y))
    for x, y in spots:
        w = rng.integers(0, n_ways, int(rng.integers(0, 6))).tolist()
        m = rng.integers(0, len(mp_polygons), int(rng.integers(0, 3))).tolist()
        refs[(x, y)] = ([], w + w[:1], m)
    r, refs = tq.make_world(str(tmp_path / name), n_ways, mp_polygons, tile_refs=refs, shared_nodes=True)
    return r, refs, list(mp_polygons)


def _random_bindings(rng, n_ways, n_mps, n_styles=30):
    def one():
        k = int(rng.choice([0, 1, 1, 2, 3]))
        return sorted(rng.integers(0, n_styles, k).tolist(), reverse=True)  # falling ids: binding order is not id order

    return [one() for _ in range(n_ways)], [one() for _ in range(n_mps)]


def _probe_tiles(zoom):
    n = 1 << zoom
    f = 1 << (18 - zoom)
    picks = {(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (131072 // f, 131072 // f), (70000 // f, 70000 // f), (1000 // f, 0), (0, 1000 // f),
             (min(n - 1, 131072 // f + 1), 131072 // f), (max(0, 70000 // f - 1), 70000 // f), (min(n - 1, 70000 // f + 2), 70000 // f)}
    return sorted(picks)


def test_tile_index_desc_equals_what_was_written(tmp_path):
    rng = np.random.default_rng(3)
    r, refs, _ = _sparse_world(tmp_path, rng)
    S = tq.shim()
    h = S.tq_index_new(r.h)
    d = S.tq_index_get(h).contents
    arr = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].copy()
    keys = sorted(refs)
    assert d.n_tiles == len(keys) == r.n_tiles
    assert arr(d.tile_xy, 2 * d.n_tiles).reshape(-1, 2).tolist() == [list(k) for k in keys]
    woff, w = arr(d.way_off, d.n_tiles + 1), arr(d.ways, d.n_way_refs)
    moff, m = arr(d.multipolygon_off, d.n_tiles + 1), arr(d.multipolygons, d.n_multipolygon_refs)
    for i, k in enumerate(keys):
        assert w[woff[i] : woff[i + 1]].tolist() == sorted(refs[k][1]) and m[moff[i] : moff[i + 1]].tolist() == sorted(refs[k][2])
    assert any(len(set(refs[k][1])) < len(refs[k][1]) for k in keys)  # ids repeat inside a list
    L = lib.load()
    assert L.osmt_validate_tile_index(S.tq_index_get(h), r.n_ways, r.n_multipolygons) == abi.OK, L.osmt_last_error()
    S.tq_index_free(h)
    r.close()


def test_mirror_equals_the_restatement(tmp_path):
    """osmt::styled_areas_of_tile — GeodataReader's column walk — against the clipped rectangle over the dict"""
    seen_dedup = seen_nonempty = seen_empty = seen_dropped = 0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        r, refs, n_polys = _sparse_world(tmp_path, rng, name=f"s{seed}.bin")
        ws, ms = _random_bindings(rng, r.n_ways, r.n_multipolygons)
        mir = tq.Mirror(r, ws, ms)
        d = mir.desc()
        assert d.n_way_styles == sum(map(len, ws)) and d.n_multipolygon_styles == sum(map(len, ms))
        assert [d.way_style_off[i] for i in range(r.n_ways + 1)] == np.concatenate([[0], np.cumsum([len(v) for v in ws])]).tolist()
        for zoom in (0, 10, 15, 17, 18):
            tiles = _probe_tiles(zoom)
            if zoom == 18:
                tiles += [k for k in list(refs)[:12]] + [(min(tq.WORLD - 1, x + 1), y) for x, y in list(refs)[:6]]
            for x, y in tiles:
                want, raw, distinct = tq.restate(refs, n_polys, ws, ms, zoom, x, y)
                got = tq.pairs(mir.areas(zoom, x, y))
                assert got == want, (seed, zoom, x, y)
                seen_dedup += raw > distinct
                seen_nonempty += bool(want)
                seen_empty += not want
        seen_dropped += any(n_polys[m] == 0 and ms[m] for m in range(len(ms)))
        mir.close()
        r.close()
    assert seen_dedup > 20 and seen_nonempty > 60 and seen_empty > 5 and seen_dropped


def test_host_program_under_the_sanitizers(tmp_path):
    """the mirror in a program of its own, built with -fsanitize=address,undefined: clean, and the numbers of the restatement"""
    rng = np.random.default_rng(9)
    r, refs, n_polys = _sparse_world(tmp_path, rng, name="h.bin")
    ws = [[7 * i + 5 - k for k in range(i % 3)] for i in range(r.n_ways)]
    ms = [[11 * m + 9 - k for k in range((m + 1) % 3)] for m in range(r.n_multipolygons)]
    tiles = [(z, x, y) for z in (0, 10, 15, 18) for x, y in _probe_tiles(z)]
    exe = tq.build_host_main()
    args = [str(v) for t in tiles for v in t]
    p = subprocess.run([exe, str(tmp_path / "h.bin")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    n_w, n_m = sum(len(v[1]) for v in refs.values()), sum(len(v[2]) for v in refs.values())
    assert lines[0] == f"index {len(refs)} {n_w} {n_m} bindings {sum(map(len, ws))} {sum(map(len, ms))}"
    for (z, x, y), line in zip(tiles, lines[1:]):
        want, _, _ = tq.restate(refs, n_polys, ws, ms, z, x, y)
        s = 0
        for e, st in want:
            s = (s * 1000003 + e * 31 + st) % (1 << 64)
        assert line == f"{len(want)} {s}", (z, x, y)
    assert sum(int(l.split()[0]) > 0 for l in lines[1 : 1 + len(tiles)]) > 10
    r.close()
