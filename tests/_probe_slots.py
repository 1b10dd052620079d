"""Shared helpers of tests/test_probe_slots_cpu.py and tests/test_gpu_import_counts.py: the shim over
osm_renderer_amd/csrc/osmt_probe_slots.h (tests/probe_slots_shim.cpp), a plain Python restatement of its six functions with
64-bit masks, the crossings_* helpers that fill a world's table sequentially with the shim's slots and count the probe steps
from the last slot to slot 0, and the worlds of the GPU tests.  The builders of the wrapping worlds SEARCH their inputs through
the shim, so a changed hash or table size moves the worlds with it; every world's guard is asserted on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import styled
from tests import _polygons as mp
from tests import _resolve as rs
from tests._geodata import ROOT

SHIM = os.path.join(ROOT, "tests", "_build", "libprobe_slots_shim.so")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "csrc", "osmt_probe_slots.h")]
_lib = None
M64 = (1 << 64) - 1
OWNERS = 65536  # the widest 1-D grid of way_grid and rel_grid (csrc/osmt_resolve.hip, csrc/osmt_polygons.hip)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "probe_slots_shim.cpp")
        if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(p) for p in [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", tmp, src])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        u32, u64, vp, sz = C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t
        for name, res, args in (("shim_pair_key", u64, [u32, u32]), ("shim_pair_hash", u32, [u64]), ("shim_pair_slots", u32, [u32]),
                                ("shim_vertex_hash", u32, [u64, u64, u32]), ("shim_vertex_first_slot", u32, [u64, u64, u32, u32, u32]),
                                ("shim_vertex_slots", u64, [u64]), ("shim_pair_homes", None, [u32, vp, sz, u32, vp]),
                                ("shim_vertex_homes", None, [vp, sz, u32, u32, u32, vp]), ("shim_pair_crossings", u64, [vp, vp, sz, u32, vp]),
                                ("shim_vertex_crossings", None, [vp, vp, vp, vp, vp, sz, u32, vp])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


# ---- the restatement -------------------------------------------------------------------------------------------------------
def py_pair_key(a, b):
    return (min(a, b) << 32) | max(a, b)


def py_pair_hash(k):
    k = (k * 0x9E3779B97F4A7C15) & M64
    k ^= k >> 29
    k = (k * 0xBF58476D1CE4E5B9) & M64
    return k >> 32


def py_pair_slots(length):
    slots = 64
    while slots < 2 * (length - 1):
        slots *= 2
    return slots


def py_vertex_hash(lat, lon, rel):
    h = (lat * 0x9E3779B97F4A7C15) & M64
    h ^= h >> 29
    h = ((h + lon) * 0xBF58476D1CE4E5B9) & M64
    h ^= h >> 32
    h = ((h + rel) * 0x94D049BB133111EB) & M64
    return h >> 32


def py_vertex_first_slot(lat, lon, rel, hash_bits, table_mask):
    keep = 0xFFFFFFFF if hash_bits >= 32 else (1 << hash_bits) - 1
    return py_vertex_hash(lat, lon, rel) & keep & table_mask


def py_vertex_slots(endpoints):
    slots = 64
    while slots < 2 * endpoints and slots < 1 << 32:
        slots *= 2
    return slots


def py_crossings(keys_and_homes, slots):
    """[(key, home slot)] entered in order into a table of `slots` slots; equal keys share a slot.  (crossing steps, the steps
    of the longest probe that crossed) — the count the shim's two players make, from the definition"""
    table, crossings, longest = [None] * slots, 0, 0
    for key, slot in keys_and_homes:
        steps, crossed = 0, False
        while table[slot] is not None and table[slot] != key:
            if slot == slots - 1:
                crossings, crossed = crossings + 1, True
            slot, steps = (slot + 1) % slots, steps + 1
        table[slot] = key
        if crossed:
            longest = max(longest, steps)
    return crossings, longest


# ---- crossings of a world --------------------------------------------------------------------------------------------------
def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def crossings_pairs(way_node_off, way_nodes, short_max=rs.SHORT_WAY_MAX):
    """k_res_short's tables over RESOLVED references (before the dedup).  (ways with a crossing step, [n_ways, 2]: a way's
    crossing steps and its longest crossing probe)"""
    off, refs = _u32(way_node_off), _u32(way_nodes)
    per_way = np.zeros((len(off) - 1, 2), np.uint32)
    n = shim().shim_pair_crossings(off.ctypes.data, refs.ctypes.data, len(off) - 1, short_max, per_way.ctypes.data)
    return int(n), per_way


def crossings_vertices(relations, hash_bits=32):
    """k_mpa_vertices' table over a styled.Relations.  (crossing steps, the longest crossing probe, slots, endpoints)"""
    r, out = relations, np.zeros(4, np.uint64)
    bits = np.ascontiguousarray(r.nodes).view(np.uint64)
    shim().shim_vertex_crossings(bits.ctypes.data, r.way_node_off.ctypes.data, r.way_nodes.ctypes.data, r.relation_way_off.ctypes.data, r.relation_ways.ctypes.data,
                                 len(r.relation_ids), hash_bits, out.ctypes.data)
    return tuple(int(v) for v in out)


# ---- wrapping probes, polygons ---------------------------------------------------------------------------------------------
AT_END = 5  # vertices of a ring (per relation) whose home is one of the last two slots


def wrap_ring_world(sizes, roles=None, relations=1, way_len=3):
    """`relations` relations over the same ways: closed rings of the given sizes (segments), each cut into ways of way_len
    segments.  Per ring and relation, AT_END of the ring's vertices have their home in the last two slots of the call's vertex
    table; the positions are searched among (10 + k / 8192, 20) through the shim."""
    L = shim()
    slots = int(L.shim_vertex_slots(2 * relations * sum(sizes)))
    cand = np.stack([10.0 + np.arange(65536) / 8192.0, np.full(65536, 20.0)], axis=1)
    bits = np.ascontiguousarray(cand).view(np.uint64)
    free = np.ones(len(cand), bool)
    at_end = []
    for rel in range(relations):
        homes = np.zeros(len(cand), np.uint32)
        L.shim_vertex_homes(bits.ctypes.data, len(cand), rel, 32, slots - 1, homes.ctypes.data)
        at_end.append(homes >= slots - 2)
    nodes, ways, members = [], [], []
    for k, n in enumerate(sizes):
        assert n >= AT_END * relations
        picked = []
        for rel in range(relations):
            hits = np.flatnonzero(at_end[rel] & free)[:AT_END]
            assert len(hits) == AT_END, (slots, rel, len(hits))
            free[hits] = False
            picked += hits.tolist()
        rest = np.flatnonzero(free)[: n - len(picked)]
        free[rest] = False
        base = len(nodes)
        nodes += [tuple(cand[i]) for i in picked + rest.tolist()]
        ring = [base + i for i in range(n)] + [base]
        for a in range(0, n, way_len):
            members.append((len(ways), roles[k] if roles else 0))
            ways.append(ring[a:a + way_len + 1])
    return mp.World(nodes, ways, [members] * relations)


def homes_at_end(world):
    """per relation: how many distinct vertices of the world have their home in the last two slots of its vertex table"""
    L = shim()
    slots = int(L.shim_vertex_slots(2 * sum(world.segment_counts())))
    bits = world.nodes.view(np.uint64).reshape(-1, 2)
    out = []
    for rel, members in enumerate(world.relations):
        used = sorted({i for w, _ in members for i in world.ways[w]})
        out.append(sum(1 for i in used if L.shim_vertex_first_slot(int(bits[i, 0]), int(bits[i, 1]), rel, 32, slots - 1) >= slots - 2))
    return slots, out


# name: (builder, slots of the table, rings per relation)
RING_WORLDS = {
    "ring 6": (lambda: wrap_ring_world([6]), 64, 1),
    "ring 16": (lambda: wrap_ring_world([16]), 64, 1),
    "ring 17": (lambda: wrap_ring_world([17]), 128, 1),
    "ring 600": (lambda: wrap_ring_world([600]), 4096, 1),
    "ring 16 under two relations": (lambda: wrap_ring_world([16], relations=2), 128, 1),
    "rings 16 outer and 16 inner": (lambda: wrap_ring_world([16, 16], roles=[0, 1]), 128, 2),
}
RING_MIN_CROSSINGS = 4

# ---- wrapping probes, resolution ---------------------------------------------------------------------------------------------
PATH_NODES = 65536
PATH_LENGTHS = [8, 33, 34, 256, 1024]  # tables of 64, 64, 128, 512 (the cap at the default bound) and 2048 slots (the cap at bound 1024)
PATH_SLOTS = [64, 64, 128, 512, 2048]
PATH_BOUND = 1024  # the bound under which the longest path dedups in LDS
PATH_MIN_CHAIN = 3


def wrap_path(length, start):
    """`length` node indices: a path over length // 2 + 1 nodes there and back (tests/_resolve.py: walk).  Every pair of the way
    out has its home in the last slot but one of the way's table, so the pairs queue up through the last slot and on from slot
    0, and the way back finds each of them only past the wrap.  A greedy search over PATH_NODES indices through the shim."""
    L = shim()
    slots = int(L.shim_pair_slots(length))
    cand, homes = np.arange(PATH_NODES, dtype=np.uint32), np.zeros(PATH_NODES, np.uint32)
    free = np.ones(PATH_NODES, bool)
    free[start] = False
    path = [start]
    for _ in range(length // 2):
        L.shim_pair_homes(path[-1], cand.ctypes.data, PATH_NODES, slots - 1, homes.ctypes.data)
        hits = np.flatnonzero((homes == slots - 2) & free)
        assert len(hits), (length, len(path))
        path.append(int(hits[0]))
        free[hits[0]] = False
    return (path + path[-2::-1])[:length]


class PathWorld(rs.World):
    """one way per length of PATH_LENGTHS over PATH_NODES nodes with the ids 1000 + 7 i, a relation that names them all; every
    reference resolves, so `paths` are the ways' resolved references"""

    def __init__(self):
        self.paths = [wrap_path(n, 100 * k) for k, n in enumerate(PATH_LENGTHS)]
        ways = [(100 + k, [1000 + 7 * i for i in p]) for k, p in enumerate(self.paths)]
        super().__init__([1000 + 7 * i for i in range(PATH_NODES)], ways, [[(100 + k, k & 1) for k in range(len(ways))]])
        self.resolved_off = np.concatenate([[0], np.cumsum([len(p) for p in self.paths])]).astype(np.uint32)
        self.resolved_refs = np.array([i for p in self.paths for i in p], np.uint32)
        self.kept = [n // 2 + 1 for n in PATH_LENGTHS]


# ---- many ways -------------------------------------------------------------------------------------------------------------
N_NODES_MANY = 256 * rs.SORT_BLOCK + 1  # the node id table takes 257 sort blocks: the block-total scan's second chunk
NO_NODE, NO_WAY = 4, 7  # ids nothing has: nodes are 5 + 3 i, ways 10 + 2 i
MANY_WAYS_MIN_CROSSING = 100


class ManyWays:
    """n_ways ways over N_NODES_MANY nodes, built with numpy straight into a styled.RawOsm: raw lengths 0 .. 43, each reference
    one of a window of 5 nodes of its way (pairs repeat), every 13th reference of the file an id that is no node (so a way
    resolves 0 .. 40 references; the last way has 32 raw ones); node i has the id 5 + 3 p(i) for a permutation p.  Three
    relations name the ways at the indices 0, OWNERS - 1 and OWNERS, and an id that is no way.  resolved_off / resolved_refs:
    the ways' references as they resolve, before the dedup."""

    def __init__(self, n_ways, seed=1):
        rng = np.random.default_rng(seed)
        n_nodes, win = N_NODES_MANY, 5
        node_ids = (5 + 3 * rng.permutation(n_nodes)).astype(np.uint64)
        raw_len = rng.integers(0, 44, n_ways)
        raw_len[-1] = 32
        off = np.concatenate([[0], np.cumsum(raw_len)])
        n_refs = int(off[-1])
        owner = np.repeat(np.arange(n_ways), raw_len)
        idx = rng.integers(0, n_nodes - win, n_ways)[owner] + rng.integers(0, win, n_refs)
        miss = np.arange(n_refs) % 13 == 12
        way_id = lambda i: 10 + 2 * i
        named = [[way_id(0), NO_WAY], [way_id(OWNERS - 1), way_id(0)], [way_id(OWNERS), NO_WAY, way_id(OWNERS - 1)]]
        r = styled.RawOsm([], [], [])
        r.node_ids, r.way_ids = node_ids, way_id(np.arange(n_ways)).astype(np.uint64)
        r.way_ref_off, r.way_refs = off.astype(np.uint32), np.where(miss, np.uint64(NO_NODE), node_ids[idx])
        r.relation_ids = np.array([7000, 7003, 7006], np.uint64)
        r.relation_ref_off = np.concatenate([[0], np.cumsum([len(m) for m in named])]).astype(np.uint32)
        r.relation_refs = np.array([g for m in named for g in m], np.uint64)
        r.relation_ref_inner = (np.arange(len(r.relation_refs)) & 1).astype(np.uint8)
        self.r, self.n_ways = r, n_ways
        self.resolved_off = np.concatenate([[0], np.cumsum(np.bincount(owner[~miss], minlength=n_ways))]).astype(np.uint32)
        self.resolved_refs = idx[~miss].astype(np.uint32)
        self.members = sum(1 for m in named for g in m if g != NO_WAY and (g - 10) // 2 < n_ways)


# ---- many relations --------------------------------------------------------------------------------------------------------
BASE_RELATIONS = 2048
BASE_SEED = 33  # relations 0, BASE_RELATIONS - 2 and BASE_RELATIONS - 1 of this world are accepted with rings: they end the three worlds
_base = None


def base_world():
    global _base
    if _base is None:
        _base = mp.random_world(BASE_SEED, BASE_RELATIONS)
    return _base


class ManyRelations:
    """n_rels relations: the arrays of mp.random_world(BASE_SEED, BASE_RELATIONS) tiled with numpy, copy c with its latitudes
    shifted by c / 4 and its own nodes and ways; the relation arrays cut to the count"""

    def __init__(self, n_rels):
        b = base_world().r
        copies = -(-n_rels // BASE_RELATIONS)
        c = np.arange(copies)
        r = styled.Relations(np.zeros((0, 2)), [], [])
        r.nodes = np.ascontiguousarray((b.nodes[None, :, :] + np.stack([c / 4.0, 0.0 * c], axis=1)[:, None, :]).reshape(-1, 2))
        n_nodes, n_ways, n_wn, n_rw = len(b.nodes), len(b.way_node_off) - 1, len(b.way_nodes), len(b.relation_ways)
        tile_off = lambda off, step: np.concatenate([(off[:-1][None, :].astype(np.int64) + (c * step)[:, None]).reshape(-1), [copies * step]])
        r.way_node_off = tile_off(b.way_node_off, n_wn).astype(np.uint32)
        r.way_nodes = (b.way_nodes[None, :].astype(np.int64) + (c * n_nodes)[:, None]).reshape(-1).astype(np.uint32)
        rel_off = tile_off(b.relation_way_off, n_rw)[: n_rels + 1]
        r.relation_way_off = rel_off.astype(np.uint32)
        r.relation_ways = (b.relation_ways[None, :].astype(np.int64) + (c * n_ways)[:, None]).reshape(-1)[: rel_off[-1]].astype(np.uint32)
        r.relation_way_inner = np.ascontiguousarray(np.tile(b.relation_way_inner, copies)[: rel_off[-1]])
        r.relation_ids = (7000 + 3 * np.arange(n_rels)).astype(np.uint64)
        self.r, self.n_rels = r, n_rels


# ---- no segments -----------------------------------------------------------------------------------------------------------
def no_segments_world():
    """relations that name a way of no node and a way of one node, and one that names nothing: three relations, no segment"""
    return mp.World([(1.0, 2.0)], [[], [0]], [[(0, 0)], [], [(1, 1)]])


# ---- the large worlds and their twins, made once ---------------------------------------------------------------------------
_made = {}


def made(kind, n=None):
    """(world, the twin's arrays, seconds the twin took) of ManyWays / ManyRelations at a count, or of the PathWorld"""
    import time

    if (kind, n) not in _made:
        w = {"ways": ManyWays, "relations": ManyRelations}[kind](n) if n is not None else PathWorld()
        t = time.perf_counter()
        want = mp.twin(w) if kind == "relations" else rs.twin(w)
        _made[(kind, n)] = (w, want, time.perf_counter() - t)
    return _made[(kind, n)]
