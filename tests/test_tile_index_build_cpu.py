"""The host side of the z18 tile index build (include/osmtile.h, osmt_build_tile_index): the refusals that need no context; the
host twin osmt::tile_index_of (host/osmt_tilequery.hpp), the yardstick of tests/test_gpu_tile_index_build.py, against
tests/_geodata.get_tile_references — the Python restatement of saver.rs:167-226 — with the nodes' tiles computed from the same
factors; the node-tile formula over osmt::mercator_factors against the reference's known tiles; and the twin once more in a
program of its own under the sanitizers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, lib
from tests import _tileindexbuild as tib
from tests._geodata import ROOT

HI = tib.HI


def test_refusals_that_need_no_context():
    L = lib.load()
    ids = (C.c_uint64 * 2)(1, 2)
    for node_ids, n in ((None, 0), (ids, 2)):
        rc = L.osmt_validate_tile_index_build(7, node_ids, n, None)
        msg = L.osmt_last_error().decode()
        assert rc == abi.INVALID_ARG and "geodata id 7" in msg and "no context" in msg, (rc, msg)
    assert L.osmt_build_tile_index(None, 0, None, 0) == abi.INVALID_ARG
    counts = (C.c_size_t * 4)()
    assert L.osmt_read_tile_index(None, 0, None, None, None, None, None, None, None, None, counts) == abi.INVALID_ARG
    for name in ("osmt_validate_tile_index_build", "osmt_build_tile_index", "osmt_read_tile_index"):
        assert name in lib.EXPORTS and hasattr(L, name)


def _ascending(got):
    xy = got["tile_xy"].astype(np.int64)
    assert (np.diff(xy[:, 0] * (1 << 18) + xy[:, 1]) > 0).all()
    for off, pool in (("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes")):
        assert got[off][0] == 0 and got[off][-1] == len(got[pool]) and len(got[off]) == len(xy) + 1
        for i in range(len(xy)):
            assert (np.diff(got[pool][got[off][i] : got[off][i + 1]].astype(np.int64)) > 0).all()
    # a tile exists iff something is listed in it
    assert ((np.diff(got["way_off"]) + np.diff(got["mp_off"]) + np.diff(got["node_off"])) > 0).all()


def test_twin_equals_the_restatement_on_random_worlds():
    for seed in (1, 2, 3):
        w = tib.random_world(seed)
        got = tib.twin(w)
        tib.same(got, tib.restate(w))
        _ascending(got)
        assert len(got["tile_xy"]) > 100 and len(got["ways"]) > len(w.ways) and len(got["mps"]) > 10 and len(got["nodes"]) == len(w.factors)
        assert any(not x for x in w.ways) and any(not m for m in w.mps) and any(not p for p in w.polygons)


def test_twin_equals_the_restatement_on_the_edge_worlds():
    for name, make in tib.EDGE_WORLDS.items():
        w = make()
        got = tib.twin(w)
        tib.same(got, tib.restate(w))
        _ascending(got)
    assert len(tib.twin(tib.EDGE_WORLDS["nothing"]())["tile_xy"]) == 0
    one = tib.twin(tib.EDGE_WORLDS["one node"]())
    assert one["tile_xy"].tolist() == [[HI, 0]] and one["nodes"].tolist() == [0] and len(one["ways"]) == 0
    assert tib.twin(tib.EDGE_WORLDS["ways without nodes"]())["tile_xy"].tolist() == [[3, 4]]


def _tile(got, x, y):
    i = got["tile_xy"].tolist().index([x, y])
    return tuple(got[p][got[o][i] : got[o][i + 1]].tolist() for o, p in (("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes")))


def test_shapes_of_entities():
    got = tib.twin(tib.shapes_world())
    X, Y = 1000, 2000
    listed = lambda pool: set(got[pool].tolist())
    assert listed("ways") == {2, 3, 6, 7}  # the ways without nodes are listed nowhere
    assert listed("mps") == {3, 4, 5, 6}   # nor a multipolygon without polygons, or with empty polygons only
    assert _tile(got, X, Y) == ([2, 3, 7], [3, 5], [0])
    assert _tile(got, X + 1, Y + 1) == ([3, 7], [3, 5], [])  # inside the rectangles, no node of its own
    assert _tile(got, X + 30, Y + 5)[1] == [4, 5] and _tile(got, X + 25, Y + 6)[1] == [5]  # polygon 3 belongs to both
    assert _tile(got, X + 9, Y + 9) == ([], [], [3])  # polygon 4 is named by no multipolygon: its node lists only itself
    assert _tile(got, X + 20, Y)[1] == [3, 5, 6]


def test_rectangles():
    got = tib.twin(tib.rectangles_world())
    X, Y = 5000, 7000
    n = {w: int((got["ways"] == w).sum()) for w in range(7)}
    assert n == {0: 1, 1: 7, 2: 7, 3: 1600, 4: 20, 5: 20, 6: 49}
    assert _tile(got, X + 101, Y + 102) == ([4, 5], [0], [])  # an interior tile of the diagonal: the ways and the multipolygon, no node
    assert _tile(got, X + 200, Y) == ([], [], [6])  # a node and nothing else
    assert _tile(got, X + 300, Y + 1) == ([], [1], [7])


def test_tile_edges():
    w = tib.edges_world()
    k = 77777
    assert w.node_tiles().tolist() == [[k, k], [k - 1, k], [k, k - 1], [0, 0], [HI, HI], [0, HI], [HI, 0], [0, 131072], [131072, 131071], [1, 0]]
    for f, axis, node in (((1.0, 0.5), "x", 1), ((0.5, 1.0), "y", 1), ((1.0, 1.0), "x", 1)):
        bad = tib.World([(0.25, 0.25), f, (1.0, 0.1)], [[0, 1]])
        try:
            tib.twin(bad)
            assert False, "a factor of 1.0 was accepted"
        except tib.Refused as e:
            assert (e.node, e.axis) == (node, axis)


def test_the_twin_refuses_factors_outside_the_unit_interval():
    for bad in (-1e-9, 1.0000001, 65.0, float("nan"), float("inf")):
        try:
            tib.twin(tib.World([(0.5, 0.5), (0.5, bad)]))
            assert False, bad
        except ValueError:
            pass


def test_node_tiles_of_the_references_known_points():
    """(u32)(f * 2^26) >> 8 over osmt::mercator_factors is the reference's coords_to_max_zoom_tile on its own test points"""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))["projection_max_zoom_tile"]
    assert len(kat) >= 3
    f = tib.mercator_factors([(k["lat"], k["lon"]) for k in kat])
    assert tib.World(f).node_tiles().tolist() == [[k["x"], k["y"]] for k in kat]


def _mix(h, v):
    for x in v:
        h = (h * 1000003 + int(x)) % (1 << 64)
    return (h * 1000003 + len(v)) % (1 << 64)


def test_host_program_under_the_sanitizers(tmp_path):
    """the twin in a program of its own, built with -fsanitize=address,undefined: clean, and the numbers of the restatement"""
    exe = tib.build_host_main()
    worlds = [tib.random_world(4)] + [make() for make in tib.EDGE_WORLDS.values()] + [tib.World([(0.5, 0.5), (0.5, 1.0)], [[0, 1]])]
    for i, w in enumerate(worlds):
        path = tmp_path / f"w{i}.txt"
        w.write_text(path)
        p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        if i == len(worlds) - 1:
            assert p.stdout == "refused 1 y\n"
            continue
        want = tib.restate(w)
        h = 0
        for name in tib.ARRAYS:
            h = _mix(h, want[name].reshape(-1))
        assert p.stdout == f"index {len(want['tile_xy'])} {len(want['ways'])} {len(want['mps'])} {len(want['nodes'])} {h}\n", i
