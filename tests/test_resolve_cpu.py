"""The host side of the id resolution (include/osmtile.h, osmt_resolve_refs): the host twin osmt::resolve_refs_host
(host/osmt_resolve.hpp), the yardstick of tests/test_gpu_resolve.py, against the Python model of the three importer steps in
tests/_resolve.py — on the table of known results, on duplicate ids with and without `seen`, on empty shapes and on a few
hundred random worlds; the refusals of osmt_validate_resolve with their messages; the exports and the Python surfaces; and the
twin once more in a program of its own under the sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from tests import _resolve as rs


@pytest.mark.parametrize("row", rs.TABLE, ids=[r[0] for r in rs.TABLE])
def test_table_rows(row):
    w = rs.table_world(row)
    want = rs.table_arrays(row)
    rs.same(rs.model(w), want)
    rs.same(rs.twin(w), want)


def test_table_rows_together():
    w = rs.table_world_all()
    got = rs.twin(w)
    rs.same(got, rs.model(w))
    assert rs.ways_of(got) == [r[2] for r in rs.TABLE]
    assert got["relation_ways"].tolist() == list(range(len(rs.TABLE))) and got["relation_way_inner"].tolist() == [i & 1 for i in range(len(rs.TABLE))]


def test_a_later_element_of_an_id_wins_and_an_unread_one_does_not_exist():
    for seen, want in ((None, [2]), ([3], [2]), ([2], [0]), ([1], [0]), ([0], [])):
        w = rs.World([5, 7, 5], [(1, [5])], [], seen, None if seen is None else [])
        got = rs.twin(w)
        rs.same(got, rs.model(w))
        assert got["way_nodes"].tolist() == want and got["counts"] == (len(want), 0, 1 - len(want), 0, 0)
    # a way id shadowed the same way; the member keeps its role
    for seen, want in ((None, [2]), ([3], [2]), ([1], [0]), ([0], [])):
        w = rs.World([1], [(5, [1]), (7, []), (5, [1, 1])], [[(5, 1), (7, 0)]], None if seen is None else [1, 1, 1], seen)
        got = rs.twin(w)
        rs.same(got, rs.model(w))
        assert got["relation_ways"].tolist() == want + ([1] if seen is None or seen[0] >= 2 else [])
        assert got["relation_way_inner"].tolist()[:len(want)] == [1] * len(want)
        assert rs.ways_of(got) == [[0], [], [0, 0]]  # every way stays stored


def test_empty_shapes():
    for w in (rs.World([], [], []), rs.World([1, 2], [], []), rs.World([], [(1, [])], [[]]), rs.World([4], [(1, [9, 9]), (2, [])], [[], [(3, 1)], []]),
              rs.World([], [], [], [], [])):
        got = rs.twin(w)
        rs.same(got, rs.model(w))
        assert got["counts"][:2] == (0, 0) and not got["way_node_off"].any() and not got["relation_way_off"].any()
        assert len(got["way_node_off"]) == len(w.ways) + 1 and len(got["relation_way_off"]) == len(w.relations) + 1


@pytest.mark.parametrize("block", range(6))
def test_twin_equals_the_model_on_random_worlds(block):
    resolved = dropped = repeats = big = 0
    for seed in range(60 * block, 60 * block + 60):
        w = rs.random_world(seed)
        want = rs.model(w)
        rs.same(rs.twin(w), want)
        c = want["counts"]
        resolved, dropped, repeats = resolved + c[0] + c[1], dropped + c[2] + c[4], repeats + c[3]
        big += sum(1 for g in w.node_ids if g >= 1 << 36)
    # over the model alone: a generator that drifts to all-resolved (or all-dropped) would test nothing
    assert resolved > 200 and dropped > 200 and repeats > 30 and big > 30, (resolved, dropped, repeats, big)


def test_ids_of_all_64_bits():
    top = (1 << 64) - 1
    w = rs.World([top, 0, 1 << 36, (1 << 36) + 1, top], [(top, [top, 0, (1 << 36) + 1, 1 << 36, top - 1, top])], [[(top, 1), (top - 1, 0)]])
    got = rs.twin(w)
    rs.same(got, rs.model(w))
    assert got["way_nodes"].tolist() == [4, 1, 3, 2, 4] and got["relation_ways"].tolist() == [0] and got["counts"] == (5, 1, 1, 0, 1)


def test_counted_and_run_worlds_agree_with_the_model():
    """the generators of the GPU tests, at small sizes"""
    for w in (rs.counted_world(1, 40, 9, 70, 5, 30), rs.counted_world(2, 40, 9, 70, 5, 30, with_seen=True), rs.run_world(5, False), rs.run_world(5, True),
              rs.key_byte_world([40, 48, 56]), rs.key_byte_world([0]), rs.way_length_world([0, 1, 2, 9, 10], True, miss_every=3)):
        rs.same(rs.twin(w), rs.model(w))
    got = rs.twin(rs.way_length_world([64], True))
    assert got["counts"] == (33, 1, 0, 31, 0)  # there and back over 33 nodes: the way back repeats every pair
    got = rs.twin(rs.run_world(5, True))
    assert rs.ways_of(got)[:4] == [[], [0], [1, 0], [1, 2, 2, 0]]  # sees nothing; node 3; 776 and 3; the first 777, and {2, 0} a second time


def _refused(d, code, *words):
    L = lib.load()
    rc = L.osmt_validate_resolve(C.byref(d))
    msg = L.osmt_last_error().decode()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_validate_resolve_refusals():
    L = lib.load()
    ok = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]], [3, 3], [2])
    assert L.osmt_validate_resolve(C.byref(ok.r.as_desc())) == abi.OK
    assert L.osmt_validate_resolve(C.byref(rs.World([], [], []).r.as_desc())) == abi.OK
    assert L.osmt_validate_resolve(C.byref(abi.RawOsmDesc())) == abi.OK  # nothing at all, every pointer NULL
    assert L.osmt_validate_resolve(None) == abi.INVALID_ARG
    for name in ("node_ids", "way_ids", "way_ref_off", "way_refs", "relation_ref_off", "relation_refs", "relation_ref_inner"):
        d = ok.r.as_desc()
        setattr(d, name, None)
        _refused(d, abi.INVALID_ARG, name, "NULL")
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]])
    w.r.way_ref_off[1] = 5
    _refused(w.r.as_desc(), abi.INVALID_ARG, "way_ref_off")
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]])
    w.r.relation_ref_off[-1] = 1
    _refused(w.r.as_desc(), abi.INVALID_ARG, "relation_ref_off")
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]])
    w.r.relation_ref_inner[1] = 2
    _refused(w.r.as_desc(), abi.INVALID_ARG, "relation_ref_inner[1] = 2")
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]], [3, 4], [2])
    _refused(w.r.as_desc(), abi.INVALID_ARG, "way_nodes_seen[1] = 4", "3 nodes")
    w = rs.World([1, 2, 3], [(10, [1, 2]), (11, [3])], [[(10, 0), (11, 1)]], [3, 3], [3])
    _refused(w.r.as_desc(), abi.INVALID_ARG, "relation_ways_seen[0] = 3", "2 ways")
    for field, what in (("n_nodes", "nodes"), ("n_ways", "ways"), ("n_way_refs", "node references"), ("n_relation_refs", "way references")):
        d = ok.r.as_desc()
        setattr(d, field, 2**32 - 1)
        _refused(d, abi.UNSUPPORTED, str(2**32 - 1), what)


def test_exports_null_arguments_and_surfaces():
    L = lib.load()
    for name in ("osmt_validate_resolve", "osmt_resolve_refs", "osmt_resolved_counts", "osmt_resolved_read", "osmt_resolved_free",
                 "osmt_debug_resolve_short_way_max"):
        assert name in lib.EXPORTS and hasattr(L, name)
    d = rs.table_world(rs.TABLE[3]).r.as_desc()
    h = C.c_void_p()
    assert L.osmt_resolve_refs(None, C.byref(d), C.byref(h)) == abi.INVALID_ARG and not h.value
    counts = (C.c_size_t * 5)()
    assert L.osmt_resolved_counts(None, counts) == abi.INVALID_ARG
    assert L.osmt_resolved_read(None, None, None, None, None, None, None) == abi.INVALID_ARG
    assert L.osmt_debug_resolve_short_way_max(None, 4) == abi.INVALID_ARG
    L.osmt_resolved_free(None)
    assert C.sizeof(abi.RawOsmDesc) == 14 * 8
    # the Relations of a resolution: the chain's next link
    w = rs.table_world_all()
    nodes = np.array([(1.0, 2.0), (3.0, 4.0), (5.0, 6.0)])
    r = styled.Relations.from_resolved(nodes, w.r.relation_ids, rs.model(w))
    assert L.osmt_validate_relations(C.byref(r.as_desc())) == abi.OK, L.osmt_last_error().decode()
    assert r.relation_ids.tolist() == [7000] and len(r.way_node_off) == len(rs.TABLE) + 1
    with pytest.raises(ValueError, match="relation ids"):
        styled.Relations.from_resolved(nodes, [1, 2], rs.model(w))
    with pytest.raises(ValueError, match="nodes_seen"):
        styled.RawOsm([1], [(2, [1])], [], nodes_seen=[1, 1])


def _mix(h, v):
    for x in v:
        h = (h * 1000003 + int(x)) % (1 << 64)
    return (h * 1000003 + len(v)) % (1 << 64)


def test_host_program_under_the_sanitizers(tmp_path):
    """the twin in a program of its own, built with -fsanitize=address,undefined: clean, and the numbers of the model"""
    exe = rs.build_host_main()
    worlds = [rs.random_world(s) for s in range(1, 40)] + [rs.table_world_all(), rs.World([], [], []), rs.run_world(65, True), rs.run_world(65, False),
                                                          rs.key_byte_world([40, 48, 56]), rs.way_length_world([0, 1, 2, 63, 64, 65, 300], True, miss_every=5),
                                                          rs.counted_world(3, 300, 40, 500, 20, 90, with_seen=True)]
    for i, w in enumerate(worlds):
        if (w.nodes_seen is None) != (w.ways_seen is None):
            continue
        path = tmp_path / f"w{i}.txt"
        w.write_text(path)
        p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        want = rs.model(w)
        h = 0
        for name in rs.ARRAYS:
            h = _mix(h, want[name])
        assert p.stdout == "resolved " + " ".join(str(c) for c in want["counts"]) + f" {h}\n", i
