"""The host side of the tile index pyramid (include/osmtile.h, osmt_register_tile_pyramid): the validator rules that need no
context; the host twin osmt::tile_pyramid_level (host/osmt_tilequery.hpp), the yardstick of tests/test_gpu_tile_pyramid.py,
against a Python restatement of a level's definition; the mirror queries, which must not depend on the pyramid they are given;
and the twin once more in a program of its own under the sanitizers."""
import ctypes as C
import subprocess

import numpy as np

from osm_renderer_amd import abi, lib, styled
from tests import _tilepyramid as tp
from tests import _tilequery as tq

HI = tq.WORLD - 1
LEVELS = (0, 1, 9, 17, 18)


def test_validator_rules_that_need_no_context():
    L = lib.load()

    def refused(mask, *words, gid=0):
        rc = L.osmt_validate_tile_pyramid(gid, mask, None)
        msg = L.osmt_last_error().decode()
        assert rc == abi.INVALID_ARG and all(w in msg for w in words), (rc, msg)

    refused(0, "mask 0")
    refused(1 << 19, "0x80000", "above level 18")
    refused(abi.PYRAMID_ALL_LEVELS | (1 << 31), "above level 18")
    refused(abi.PYRAMID_ALL_LEVELS, "geodata id 7", "no context", gid=7)  # a mask nothing is wrong with: the id has no context
    refused(1 << 18, "geodata id 0", "no context")
    assert abi.PYRAMID_ALL_LEVELS == (1 << 19) - 1
    assert L.osmt_register_tile_pyramid(None, 0, 1) == abi.INVALID_ARG
    out = (C.c_uint64 * 4)()
    assert L.osmt_tile_query_stats(None, out) == abi.INVALID_ARG
    for name in ("osmt_validate_tile_pyramid", "osmt_register_tile_pyramid", "osmt_tile_pyramid_levels", "osmt_read_tile_pyramid", "osmt_tile_query_stats"):
        assert name in lib.EXPORTS and hasattr(L, name)


def _lists(rng, n_ways=50, n_mps=6, n_nodes=30):
    """three lists in any order, with repeats, sometimes empty"""
    def one(n, most):
        v = rng.integers(0, n, int(rng.integers(0, most))).tolist()
        return v + v[:2] if rng.random() < 0.6 else v

    return one(n_ways, 7), one(n_mps, 3), one(n_nodes, 5)


def sparse_tiles(rng):
    """a sparse index: clusters with absent columns, runs of one column, and tiles without any list"""
    tiles = {}
    for cx, cy in ((70000, 70000), (131072, 131072), (131071, 131071), (512, 200000), (200000, 512)):
        for _ in range(14):
            x, y = cx + 2 * int(rng.integers(-6, 7)), cy + int(rng.integers(-9, 10))  # only every second column exists
            tiles[(x, y)] = _lists(rng)
    for y in range(300, 340, 3):
        tiles[(99999, y)] = _lists(rng)
    for k in ((70000, 70001), (131072, 131080), (99999, 301)):
        tiles[k] = ([], [], [])
    return [(k, *tiles[k]) for k in sorted(tiles)]


def corner_tiles(rng):
    """all four world corners in one index: keys that differ only in their top bits, and neighbours that share every parent"""
    tiles = {}
    for x, y in [(0, 0), (0, HI), (HI, 0), (HI, HI), (1, 0), (0, 1), (HI - 1, HI), (HI, HI - 1), (HI - 1, 0), (0, HI - 1), (1 << 17, 1 << 17), ((1 << 17) - 1, (1 << 17) - 1),
                 (1 << 17, (1 << 17) - 1)]:
        tiles[(x, y)] = _lists(rng)
    tiles[(0, 0)] = ([49, 0, 49, 7, 0], [5, 5], [29, 0])
    return [(k, *tiles[k]) for k in sorted(tiles)]


INDICES = {"sparse": sparse_tiles, "corners": corner_tiles, "no tile": lambda rng: [], "one tile": lambda rng: [((77, 200001), [3, 1, 3], [], [4, 4])],
           "one empty tile": lambda rng: [((HI, 0), [], [], [])]}


def test_twin_equals_the_restatement():
    seen_repeat = seen_empty_list = seen_merge = 0
    for name, make in INDICES.items():
        tiles = make(np.random.default_rng(len(name)))
        index, node_lists = tp.index_of(tiles)
        for level in LEVELS:
            for with_nodes in (True, False):
                got = tp.twin_level(index, level, node_lists if with_nodes else None)
                want = tp.restate_level(tiles, level, with_nodes)
                tp.same_level(got, want)
                assert len(got["nodes"]) > 0 or not with_nodes or name in ("no tile", "one empty tile")
                # strictly ascending tiles, strictly ascending lists
                xy = got["tile_xy"].astype(np.int64)
                key = xy[:, 0] * (1 << 18) + xy[:, 1]
                assert (np.diff(key) > 0).all()
                for off, pool in (("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes")):
                    for i in range(len(xy)):
                        assert (np.diff(got[pool][got[off][i] : got[off][i + 1]].astype(np.int64)) > 0).all()
                seen_merge += len(got["tile_xy"]) < len(tiles)
        seen_repeat += any(len(set(w)) < len(w) for _, w, _, _ in tiles)
        seen_empty_list += any(not w and not m for _, w, m, _ in tiles)
        # a level of 0 tiles for 0 tiles, of 1 tile for 1 tile; level 18 keeps every tile, level 0 has at most one
        assert len(tp.twin_level(index, 18)["tile_xy"]) == len(tiles) and len(tp.twin_level(index, 0)["tile_xy"]) == min(len(tiles), 1)
    assert seen_repeat >= 3 and seen_empty_list >= 2 and seen_merge >= 10
    # the corners: four tiles at level 1, one per quadrant, and level 17 keeps (0, 0) and (1, 0) together
    index, _ = tp.index_of(corner_tiles(np.random.default_rng(1)))
    assert tp.twin_level(index, 1)["tile_xy"].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    l17 = tp.twin_level(index, 17)
    assert l17["tile_xy"][0].tolist() == [0, 0] and l17["ways"][: l17["way_off"][1]].tolist() == sorted(
        {49, 0, 7} | {w for k, ws, _, _ in corner_tiles(np.random.default_rng(1)) if k in ((1, 0), (0, 1)) for w in ws})


def _world(tmp_path, rng, name):
    """the sparse world of tests/test_tile_query_cpu.py with node lists: index tiles scattered over corners, edges and the middle"""
    mp_polygons = (1, 0, 3, 2, 0, 1)
    n_nodes = 2 + 4 * sum(mp_polygons)
    spots = [(0, 0), (0, HI), (HI, 0), (HI, HI), (0, 1000), (1000, 0), (HI, 77), (77, HI), (131072, 131072), (131071, 131071), (131072, 131071), (131080, 131090),
             (70000, 70000), (70001, 70000), (70000, 70003)]
    for _ in range(60):
        cx, cy = spots[int(rng.integers(0, len(spots)))]
        spots.append((min(HI, max(0, cx + int(rng.integers(-20, 21)))), min(HI, max(0, cy + int(rng.integers(-20, 21))))))
    refs = {}
    for x, y in spots:
        w, m, n = _lists(rng, 40, len(mp_polygons), n_nodes)
        refs[(x, y)] = (n, w, m)
    r, refs = tq.make_world(str(tmp_path / name), 40, mp_polygons, tile_refs=refs, shared_nodes=True)
    assert r.n_nodes == n_nodes
    tiles = [(k, refs[k][1], refs[k][2], refs[k][0]) for k in sorted(refs)]
    return r, tiles


def _probe_tiles(zoom, tiles):
    n, f = 1 << zoom, 1 << (18 - zoom)
    picks = {(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (131072 // f, 131072 // f), (70000 // f, 70000 // f), (1000 // f, 0), (0, 1000 // f),
             (min(n - 1, 131072 // f + 1), 131072 // f), (max(0, 70000 // f - 1), 70000 // f), (min(n - 1, 70000 // f + 2), 70000 // f)}
    if zoom == 18:
        picks |= {k for k, _, _, _ in tiles[:10]} | {(min(HI, x + 1), y) for (x, y), _, _, _ in tiles[:5]}
    return sorted(picks)


def test_mirror_query_does_not_depend_on_the_pyramid(tmp_path):
    """tile for tile, at zooms 0, 10, 15, 17 and 18, for ways, multipolygons and nodes, with and without an id filter: the
    entities and the areas of the mirror with a pyramid are those of the mirror without one"""
    seen = {"level above the zoom": 0, "z18 fallback": 0, "nodes from z18": 0, "non-empty": 0, "filtered away": 0}
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        r, tiles = _world(tmp_path, rng, f"p{seed}.bin")
        index, node_lists = tp.index_of(tiles)
        ws = [sorted(rng.integers(0, 30, int(rng.choice([0, 1, 1, 3]))).tolist(), reverse=True) for _ in range(r.n_ways)]
        ms = [sorted(rng.integers(0, 30, int(rng.choice([0, 1, 2]))).tolist(), reverse=True) for _ in range(r.n_multipolygons)]
        mir = tq.Mirror(r, ws, ms)
        every = [r.global_id(1, i) for i in range(r.n_ways)] + [r.global_id(3, i) for i in range(r.n_multipolygons)] + [r.global_id(0, i) for i in range(r.n_nodes)]
        some = rng.choice(np.array(every, dtype=np.uint64), len(every) // 2, replace=False)
        pyramids = [tp.Pyramid(index, range(19), node_lists), tp.Pyramid(index, (18, 12, 8), node_lists), tp.Pyramid(index, (16, 11), None),
                    tp.Pyramid(index, (3,), node_lists)]
        assert [pyramids[1].level_for(z) for z in (0, 8, 9, 12, 13, 18)] == [8, 8, 12, 12, 18, 18] and pyramids[3].level_for(4) == -1
        for zoom in (0, 10, 15, 17, 18):
            for x, y in _probe_tiles(zoom, tiles):
                for ids in (None, some, np.zeros(0, np.uint64)):
                    want = tp.entities(r, None, zoom, x, y, ids)
                    want_areas = tp.areas(mir, None, zoom, x, y, ids)
                    if ids is None:
                        assert want_areas.tobytes() == mir.areas(zoom, x, y).tobytes()  # the mirror the GPU tests know
                        assert want == r.query(zoom, x, y, neighbours=True)  # and GeodataReader's own walk
                    for p in pyramids:
                        assert tp.entities(r, p, zoom, x, y, ids) == want, (seed, zoom, x, y)
                        assert tp.areas(mir, p, zoom, x, y, ids).tobytes() == want_areas.tobytes(), (seed, zoom, x, y)
                        lv = p.level_for(zoom)
                        seen["level above the zoom"] += lv > zoom
                        seen["z18 fallback"] += lv == -1
                    seen["nodes from z18"] += bool(want[0])
                    seen["non-empty"] += ids is None and bool(want[1]) and bool(want[2]) and bool(want[0])
                    seen["filtered away"] += ids is some and len(want[1]) < len(tp.entities(r, None, zoom, x, y)[1])
        for p in pyramids:
            p.close()
        mir.close()
        r.close()
    assert all(v >= 10 for v in seen.values()), seen


def _mix(h, v):
    for x in v:
        h = (h * 1000003 + int(x)) % (1 << 64)
    return (h * 1000003 + len(v)) % (1 << 64)


def test_host_program_under_the_sanitizers(tmp_path):
    """the twin and the mirror query in a program of their own, built with -fsanitize=address,undefined: clean, the numbers of
    the restatement, and every tile the same with and without the pyramid"""
    rng = np.random.default_rng(9)
    r, tiles = _world(tmp_path, rng, "h.bin")
    probes = [(z, x, y) for z in (0, 10, 15, 17, 18) for x, y in _probe_tiles(z, tiles)]
    exe = tp.build_host_main()
    args = [str(len(LEVELS))] + [str(v) for v in LEVELS] + [str(v) for t in probes for v in t]
    p = subprocess.run([exe, str(tmp_path / "h.bin")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    for level, line in zip(LEVELS, lines):
        want = tp.restate_level(tiles, level, True)
        h = 0
        for name in tp.ARRAYS:
            h = _mix(h, want[name].reshape(-1))
        assert line == f"level {level} {len(want['tile_xy'])} {len(want['ways'])} {len(want['mps'])} {len(want['nodes'])} {h}", level
    got = lines[len(LEVELS) : len(LEVELS) + len(probes)]
    assert len(got) == len(probes) and all(l.endswith(" same") for l in got)
    for (z, x, y), line in zip(probes, got):
        nodes, ways, mps = tp.entities(r, None, z, x, y)
        assert line == f"{len(nodes)} {len(ways)} {len(mps)} {_mix(_mix(_mix(0, nodes), ways), mps)} same", (z, x, y)
    assert sum(int(l.split()[1]) > 0 for l in got) > 10 and sum(int(l.split()[0]) > 0 for l in got) > 10
    r.close()
