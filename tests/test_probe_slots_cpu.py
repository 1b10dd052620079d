"""The slot arithmetic of the importer's two open-addressing tables (osm_renderer_amd/csrc/osmt_probe_slots.h), host build.

The header's six functions are held against a plain Python restatement with 64-bit masks; the shim's two sequential players
(crossings_pairs, crossings_vertices: tests/_probe_slots.py) against a Python table filled from that restatement; and every
world tests/test_gpu_import_counts.py runs has its guard asserted here, where no device is needed: how many probes step from
the last slot of a table to slot 0, how many owners a launch has, and what the host twins make of the world.  Those counts are
the evidence that the GPU tests reach the wrap of k_mpa_vertices, k_mpa_canon and k_res_short and the 2-D grids of k_res_short,
k_mpa_walk and k_mpa_emit."""
import numpy as np
import pytest

from tests import _polygons as mp
from tests import _probe_slots as ps
from tests import _resolve as rs

COUNTS = [ps.OWNERS - 1, ps.OWNERS, ps.OWNERS + 1]


def _u64s(rng, n):
    """n 64-bit values: random bits, with the extremes and small values among them"""
    v = [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64)]
    v = [(x << 1) | (i & 1) for i, x in enumerate(v)]
    return [0, 1, ps.M64, ps.M64 - 1, 1 << 32, (1 << 32) - 1] + v


# ---- the header against the restatement ------------------------------------------------------------------------------------
def test_the_pair_key_and_its_hash_equal_the_restatement():
    L, rng = ps.shim(), np.random.default_rng(1)
    idx = [0, 1, 2, 0xFFFFFFFE, 0xFFFFFFFD, 65535, 65536] + [int(x) for x in rng.integers(0, 0xFFFFFFFF, 3000)]
    for a, b in zip(idx, idx[1:] + idx[:1]):
        k = L.shim_pair_key(a, b)
        assert k == ps.py_pair_key(a, b) == L.shim_pair_key(b, a) and k != ps.M64
        assert L.shim_pair_hash(k) == ps.py_pair_hash(k)
    assert L.shim_pair_key(7, 7) == (7 << 32) | 7
    for k in _u64s(rng, 3000):
        assert L.shim_pair_hash(k) == ps.py_pair_hash(k)


def test_the_pair_table_size_equals_the_restatement():
    L = ps.shim()
    known = {3: 64, 33: 64, 34: 128, 65: 128, 129: 256, 256: 512, 257: 512, 1024: 2048}  # "64 slots, doubled until >= 2 * (len - 1)"
    for n, slots in known.items():
        assert L.shim_pair_slots(n) == ps.py_pair_slots(n) == slots
    for n in range(1, 1100):
        s = L.shim_pair_slots(n)
        assert s == ps.py_pair_slots(n) and s >= 64 and s & (s - 1) == 0 and s >= 2 * (n - 1) and (s == 64 or s // 2 < 2 * (n - 1))
    # the launcher's LDS of slots_cap >= 2 * short_max slots holds the table of every way up to the bound
    assert L.shim_pair_slots(rs.SHORT_WAY_MAX) == 2 * rs.SHORT_WAY_MAX and L.shim_pair_slots(ps.PATH_BOUND) == 2 * ps.PATH_BOUND


def test_the_vertex_hash_and_first_slot_equal_the_restatement():
    L, rng = ps.shim(), np.random.default_rng(2)
    vals = _u64s(rng, 3000)
    rels = [0, 1, 2, 65535, 65536, 0x7FFFFFFE] + [int(x) for x in rng.integers(0, 1 << 31, 3000)]
    for i, (lat, lon) in enumerate(zip(vals, vals[7:] + vals[:7])):
        rel = rels[i % len(rels)]
        assert L.shim_vertex_hash(lat, lon, rel) == ps.py_vertex_hash(lat, lon, rel)
        bits, mask = (0, 4, 31, 32)[i % 4] if i % 3 else int(rng.integers(0, 33)), (1 << int(rng.integers(6, 33))) - 1
        assert L.shim_vertex_first_slot(lat, lon, rel, bits, mask) == ps.py_vertex_first_slot(lat, lon, rel, bits, mask) <= mask
    assert L.shim_vertex_first_slot(vals[9], vals[10], 3, 0, 63) == 0
    assert L.shim_vertex_hash(1, 2, 3) != L.shim_vertex_hash(2, 1, 3) != L.shim_vertex_hash(2, 1, 4)  # every part of the key counts


def test_the_vertex_table_size_equals_the_restatement():
    L = ps.shim()
    known = {0: 64, 1: 64, 16: 64, 17: 64, 32: 64, 33: 128}  # "64 slots, doubled until >= 2 * endpoints"
    for e, slots in known.items():
        assert L.shim_vertex_slots(e) == ps.py_vertex_slots(e) == slots
    for e in list(range(0, 300)) + [2**20, 2**20 + 1, 2**30, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2]:  # capped at 2^32
        s = L.shim_vertex_slots(e)
        assert s == ps.py_vertex_slots(e) and 64 <= s <= 2**32 and s & (s - 1) == 0 and (s >= 2 * e or s == 2**32) and s > e


# ---- the crossings helpers against a Python table --------------------------------------------------------------------------
def _py_pair_crossings(refs):
    slots = ps.py_pair_slots(len(refs))
    keys = [ps.py_pair_key(a, b) for a, b in zip(refs, refs[1:])]
    return ps.py_crossings([(k, ps.py_pair_hash(k) & (slots - 1)) for k in keys], slots)


def _py_vertex_crossings(world, hash_bits):
    bits = world.nodes.view(np.uint64).reshape(-1, 2)
    ends = [(r, int(bits[n, 0]), int(bits[n, 1])) for r, members in enumerate(world.relations) for w, _ in members
            for a, b in zip(world.ways[w], world.ways[w][1:]) for n in (a, b)]
    slots = ps.py_vertex_slots(len(ends))
    return ps.py_crossings([(e, ps.py_vertex_first_slot(e[1], e[2], e[0], hash_bits, slots - 1)) for e in ends], slots) + (slots if ends else 0, len(ends))


def test_crossings_pairs_equals_a_python_table():
    rng = np.random.default_rng(3)
    ways = [rs.walk(n, True) for n in (3, 33, 34, 200)] + [rng.integers(0, 6, n).tolist() for n in (0, 1, 2, 3, 40, 41, 256)] + ps.made("path")[0].paths
    ways += [rng.integers(0, 1 << 20, 1 + 2 * k).tolist() for k in range(120)]  # short ways over many nodes: some cross by luck
    off = np.concatenate([[0], np.cumsum([len(w) for w in ways])])
    n, per_way = ps.crossings_pairs(off, [i for w in ways for i in w], short_max=ps.PATH_BOUND)
    want = [_py_pair_crossings(w) if len(w) > 2 else (0, 0) for w in ways]
    assert per_way.tolist() == [list(c) for c in want]
    assert n == sum(1 for c in want if c[0]) and n > len(ps.PATH_LENGTHS)
    # a way above the bound has no table
    above = [len(w) > 255 for w in ways]
    assert sum(above) == 3 and not ps.crossings_pairs(off, [i for w in ways for i in w], short_max=255)[1][above].any()


@pytest.mark.parametrize("bits", [32, 4, 0])
def test_crossings_vertices_equals_a_python_table(bits):
    worlds = [b() for b, _, _ in ps.RING_WORLDS.values()] + [mp.random_world(5, 40), mp.star_world(8, relations=2), ps.no_segments_world()]
    for w in worlds:
        assert ps.crossings_vertices(w.r, bits) == _py_vertex_crossings(w, bits)


# ---- the guards of the GPU tests' worlds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.RING_WORLDS))
def test_a_wrapping_ring_world_crosses_the_end_of_its_vertex_table(name):
    build, slots, rings = ps.RING_WORLDS[name]
    w = build()
    crossings, longest, got_slots, endpoints = ps.crossings_vertices(w.r)
    print(f"{name}: {len(w.relations)} relations, {endpoints} endpoints in {got_slots} slots, {crossings} crossing steps, longest crossing probe {longest}")
    assert got_slots == slots and endpoints == 2 * sum(w.segment_counts())
    assert ps.homes_at_end(w) == (slots, [ps.AT_END * rings] * len(w.relations))
    assert crossings >= ps.RING_MIN_CROSSINGS
    want = mp.twin(w)
    mp.same(want, mp.restate(w))
    assert want["status"].tolist() == [(1, rings, 0)] * len(w.relations)


def test_the_wrapping_paths_cross_the_end_of_their_pair_tables():
    w, want, _ = ps.made("path")
    assert [ps.shim().shim_pair_slots(n) for n in ps.PATH_LENGTHS] == ps.PATH_SLOTS
    assert ps.PATH_SLOTS[3] == 2 * rs.SHORT_WAY_MAX and ps.PATH_SLOTS[4] == 2 * ps.PATH_BOUND  # the tables that fill the launch's LDS: slots == slots_cap
    assert [len(p) for p in w.paths] == ps.PATH_LENGTHS and max(max(p) for p in w.paths) < ps.PATH_NODES
    n, per_way = ps.crossings_pairs(w.resolved_off, w.resolved_refs, short_max=ps.PATH_BOUND)
    print("paths: (crossing steps, longest crossing probe) per way:", per_way.tolist())
    assert n == len(ps.PATH_LENGTHS) and (per_way[:, 1] >= ps.PATH_MIN_CHAIN).all()
    n_default, per_way_default = ps.crossings_pairs(w.resolved_off, w.resolved_refs)
    assert n_default == len(ps.PATH_LENGTHS) - 1 and per_way_default[-1].tolist() == [0, 0]  # 1024 > 256: through the sort there
    # the way back repeats every pair of the way out: the dedup keeps the way out alone
    rs.same(want, rs.model(w))
    assert np.diff(want["way_node_off"]).tolist() == w.kept == [n // 2 + 1 for n in ps.PATH_LENGTHS]
    assert rs.ways_of(want) == [p[: n // 2 + 1] for p, n in zip(w.paths, ps.PATH_LENGTHS)]


@pytest.mark.parametrize("n_ways", COUNTS)
def test_a_many_ways_world_has_its_owners_and_crossings(n_ways):
    w, want, seconds = ps.made("ways", n_ways)
    r = w.r
    assert len(r.way_ids) == n_ways and -(-len(r.node_ids) // rs.SORT_BLOCK) == 257 and len(np.unique(r.node_ids)) == len(r.node_ids)
    resolved = np.diff(w.resolved_off.astype(np.int64))
    assert resolved.min() == 0 and resolved.max() == 40 and np.diff(r.way_ref_off.astype(np.int64)).max() == 43
    pairs = int(np.maximum(resolved - 1, 0).sum())
    assert pairs > 256 * rs.SORT_BLOCK  # under bound 0 the long sort takes more than 256 blocks
    n_refs = len(r.way_refs)
    assert (r.way_refs[12::13] == ps.NO_NODE).all() and want["counts"][2] == n_refs // 13 == n_refs - len(w.resolved_refs)
    assert want["counts"][0] + want["counts"][3] == len(w.resolved_refs)
    kept = np.diff(want["way_node_off"].astype(np.int64))
    assert 2 < kept[-1] < resolved[-1]
    crossing, per_way = ps.crossings_pairs(w.resolved_off, w.resolved_refs)
    print(f"{n_ways} ways: {n_refs} references, {pairs} pairs, {crossing} ways cross their table's end, the last way keeps {kept[-1]} of {resolved[-1]}, twin {seconds:.2f} s")
    assert crossing >= ps.MANY_WAYS_MIN_CROSSING and (per_way[:, 0] > 0).sum() == crossing
    # the relations name the ways at 0, OWNERS - 1 and OWNERS where there are such ways
    named = [i for i in (0, ps.OWNERS - 1, ps.OWNERS) if i < n_ways]
    assert sorted(set(want["relation_ways"].tolist())) == named and want["counts"][1] == w.members and want["counts"][4] == 7 - w.members
    # a sample of the ways against the model's dedup
    for k in (0, 1, n_ways // 2, ps.OWNERS - 2, n_ways - 1):
        refs = w.resolved_refs[w.resolved_off[k]:w.resolved_off[k + 1]].tolist()
        assert want["way_nodes"][want["way_node_off"][k]:want["way_node_off"][k + 1]].tolist() == rs.postprocess_node_refs(refs)


@pytest.mark.parametrize("n_rels", COUNTS)
def test_a_many_relations_world_has_its_owners_and_outcomes(n_rels):
    w, want, seconds = ps.made("relations", n_rels)
    st = want["status"]
    accepted, rejected = int((st["accepted"] == 1).sum()), int((st["accepted"] == 0).sum())
    crossings, _, slots, endpoints = ps.crossings_vertices(w.r)
    print(f"{n_rels} relations: {endpoints // 2} segments in {slots} slots, {crossings} crossing steps, {accepted} accepted, {rejected} rejected, last {st[-1]}, twin {seconds:.2f} s")
    assert len(st) == n_rels == len(w.r.relation_ids) and accepted + rejected == n_rels
    assert accepted >= 2000 and rejected >= 2000
    assert st[-1]["accepted"] == 1 and st[-1]["rings_built"] >= 1
    # every copy is the base world again: what the twin makes of relation i is what it makes of relation i mod BASE_RELATIONS
    base = mp.twin(ps.base_world())["status"]
    assert st.tobytes() == np.tile(base, -(-n_rels // ps.BASE_RELATIONS))[:n_rels].tobytes()


def test_the_world_without_segments():
    w = ps.no_segments_world()
    assert w.segment_counts() == [0, 0, 0]
    want = mp.twin(w)
    mp.same(want, mp.restate(w))
    assert want["status"].tolist() == [(1, 0, 0)] * 3 and len(want["multipolygon_ids"]) == 3 and len(want["polygon_node_off"]) == 1
