"""The host side of the multipolygon assembly (include/osmtile.h, osmt_assemble_multipolygons): the host twin
osmt::assemble_multipolygons_host (host/osmt_polygons.hpp), the yardstick of tests/test_gpu_polygons.py, against the Python
restatement of find_polygons_in_multipolygon in tests/_polygons.py — on the table of known results, on random worlds and on
positions that differ only in their bits; the refusals of osmt_validate_relations; the exports; and the twin once more in a
program of its own under the sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from tests import _polygons as mp


@pytest.mark.parametrize("row", mp.TABLE, ids=[r[0] for r in mp.TABLE])
def test_table_rows(row):
    w = mp.table_world(row)
    want = mp.table_arrays(row)
    mp.same(mp.restate(w), want)
    mp.same(mp.twin(w), want)


def test_table_rows_together():
    w = mp.concat([mp.table_world(r) for r in mp.TABLE])
    got = mp.twin(w)
    mp.same(got, mp.restate(w))
    assert got["status"]["accepted"].tolist() == [0 if isinstance(r[4], tuple) else 1 for r in mp.TABLE]
    assert mp.polygons_of(got)[0] == [[0, 1, 2, 0]] and got["multipolygon_relation"].tolist() == [i for i, r in enumerate(mp.TABLE) if not isinstance(r[4], tuple)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_equals_the_restatement_on_random_worlds(seed):
    w = mp.random_world(seed, 400)
    want = mp.restate(w)
    # over the restatement alone: a generator that drifts to all-rejected (or all-accepted) would test nothing
    acc = want["status"]["accepted"]
    assert acc.sum() >= len(acc) / 2 and (acc == 0).sum() >= len(acc) / 10, (int(acc.sum()), len(acc))
    counts = w.segment_counts()
    assert min(counts) == 0 and 30 <= max(counts) <= 40
    assert len({int(x) for x in want["status"]["rings_built"]}) >= 3
    mp.same(mp.twin(w), want)


def test_positions_are_compared_by_their_bits():
    nan_a = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    nan_b = np.array([0x7FF8000000000002], dtype=np.uint64).view(np.float64)[0]
    # -0.0 and 0.0 are two vertices: the ring 0-1-2 does not close through node 3 at (-0.0, 0)
    open_ring = mp.World([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (-0.0, 0.0)], [[0, 1], [1, 2], [2, 3]], [[(0, 0), (1, 0), (2, 0)]])
    got = mp.twin(open_ring)
    mp.same(got, mp.restate(open_ring))
    assert got["status"].tolist() == [(0, 0, 3)]
    # two NaNs of equal bits are one vertex, of different bits two
    for last, accepted in ((nan_a, 1), (nan_b, 0)):
        w = mp.World([(nan_a, 5.0), (1.0, 0.0), (2.0, 0.0), (last, 5.0)], [[0, 1], [1, 2], [2, 3]], [[(0, 0), (1, 0), (2, 0)]])
        got = mp.twin(w)
        mp.same(got, mp.restate(w))
        assert got["status"]["accepted"].tolist() == [accepted]
        if accepted:
            assert mp.polygons_of(got) == [[[0, 1, 2, 3]]]


def _refused(world_or_desc, code, *words):
    L = lib.load()
    d = world_or_desc if isinstance(world_or_desc, abi.RelationsDesc) else world_or_desc.r.as_desc()
    rc = L.osmt_validate_relations(C.byref(d))
    msg = L.osmt_last_error().decode()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_validate_relations_refusals():
    L = lib.load()
    ok = mp.table_world(mp.TABLE[0])
    assert L.osmt_validate_relations(C.byref(ok.r.as_desc())) == abi.OK
    assert L.osmt_validate_relations(C.byref(mp.World(np.zeros((0, 2)), [], []).r.as_desc())) == abi.OK
    assert L.osmt_validate_relations(None) == abi.INVALID_ARG
    for name in ("nodes", "way_node_off", "way_nodes", "relation_ids", "relation_way_off", "relation_ways", "relation_way_inner"):
        d = ok.r.as_desc()
        setattr(d, name, None)
        _refused(d, abi.INVALID_ARG, name, "NULL")
    w = mp.table_world(mp.TABLE[0])
    w.r.way_node_off[1] = 5
    _refused(w, abi.INVALID_ARG, "way_node_off")
    w = mp.table_world(mp.TABLE[0])
    w.r.relation_way_off[-1] = 2
    _refused(w, abi.INVALID_ARG, "relation_way_off")
    w = mp.table_world(mp.TABLE[0])
    w.r.way_nodes[3] = 3
    _refused(w, abi.INVALID_ARG, "way_nodes[3] = 3", "3 nodes")
    w = mp.table_world(mp.TABLE[0])
    w.r.relation_ways[1] = 9
    _refused(w, abi.INVALID_ARG, "relation_ways[1] = 9", "3 ways")
    w = mp.table_world(mp.TABLE[0])
    w.r.relation_way_inner[2] = 2
    _refused(w, abi.INVALID_ARG, "relation_way_inner[2] = 2")
    d = ok.r.as_desc()
    d.n_nodes = 2**32 - 1
    _refused(d, abi.UNSUPPORTED, str(2**32 - 1), "nodes")
    # 2^31 segments: a way of 2^16 + 1 nodes named 2^15 times; one less is accepted
    n = 2**16 + 1
    for refs, code in ((2**15, abi.UNSUPPORTED), (2**15 - 1, abi.OK)):
        r = styled.Relations(np.zeros((1, 2)), [], [])
        r.way_node_off, r.way_nodes = np.array([0, n], np.uint32), np.zeros(n, np.uint32)
        r.relation_ids, r.relation_way_off = np.array([1], np.uint64), np.array([0, refs], np.uint32)
        r.relation_ways, r.relation_way_inner = np.zeros(refs, np.uint32), np.zeros(refs, np.uint8)
        d = r.as_desc()
        if code == abi.OK:
            assert L.osmt_validate_relations(C.byref(d)) == abi.OK
        else:
            _refused(d, code, str(2**31), "segments")


def test_exports_and_null_arguments():
    L = lib.load()
    for name in ("osmt_validate_relations", "osmt_assemble_multipolygons", "osmt_polygons_counts", "osmt_polygons_read", "osmt_polygons_free",
                 "osmt_debug_vertex_hash_bits"):
        assert name in lib.EXPORTS and hasattr(L, name)
    d = mp.table_world(mp.TABLE[0]).r.as_desc()
    h = C.c_void_p()
    assert L.osmt_assemble_multipolygons(None, C.byref(d), C.byref(h)) == abi.INVALID_ARG and not h.value
    counts = (C.c_size_t * 4)()
    assert L.osmt_polygons_counts(None, counts) == abi.INVALID_ARG
    assert L.osmt_polygons_read(None, None, None, None, None, None, None, None, None) == abi.INVALID_ARG
    assert L.osmt_debug_vertex_hash_bits(None, 4) == abi.INVALID_ARG
    L.osmt_polygons_free(None)
    assert C.sizeof(abi.RelationsDesc) == 12 * 8 and styled.RELATION_STATUS_DTYPE.itemsize == 12


def _mix(h, v):
    for x in v:
        h = (h * 1000003 + int(x)) % (1 << 64)
    return (h * 1000003 + len(v)) % (1 << 64)


def test_host_program_under_the_sanitizers(tmp_path):
    """the twin in a program of its own, built with -fsanitize=address,undefined: clean, and the numbers of the restatement"""
    exe = mp.build_host_main()
    nan = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    worlds = [mp.random_world(4, 200), mp.concat([mp.table_world(r) for r in mp.TABLE]), mp.World(np.zeros((0, 2)), [], []), mp.star_world(65, 2),
              mp.World([(nan, 5.0), (1.0, -0.0), (2.0, 0.0), (nan, 5.0)], [[0, 1], [1, 2], [2, 3], [], [1]], [[(0, 0), (1, 0), (2, 0), (3, 1), (4, 0)], []])]
    for i, w in enumerate(worlds):
        path = tmp_path / f"w{i}.txt"
        w.write_text(path)
        p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        want = mp.restate(w)
        h = 0
        for name in mp.ARRAYS:
            a = want[name]
            h = _mix(h, np.array(a.tolist(), dtype=np.uint64).reshape(-1) if name == "status" else a)
        assert p.stdout == f"polygons {len(want['polygon_node_off']) - 1} {len(want['polygon_nodes'])} {len(want['multipolygon_ids'])} {h}\n", i
