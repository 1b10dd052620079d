"""Shared helpers of the id resolution tests (tests/test_resolve_cpu.py, tests/test_gpu_resolve.py): a Python restatement of the
three importer steps — OsmEntityStorage::translate_id (importer.rs:45-71), the drop of references that do not resolve
(importer.rs:365-400) and postprocess_node_refs (importer.rs:334-353) — with a dict and a set and no sorting tricks (the
model); the shim over osmt::resolve_refs_host (host/osmt_resolve.hpp), the host twin of osmt_resolve_refs; the table of the
small inputs whose results are known; and the worlds both files use."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT

SHIM = os.path.join(ROOT, "tests", "_build", "libresolve_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "resolve_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_resolve.hpp"), os.path.join(ROOT, "include", "osmtile.h")]
ARRAYS = ("way_node_off", "way_nodes", "relation_way_off", "relation_ways", "relation_way_inner")
DTYPES = {"relation_way_inner": np.uint8}
SORT_BLOCK = 1024  # OSMT_PYR_SORT_BLOCK (csrc/osmt_internal.h)
SHORT_WAY_MAX = 256  # OSMT_RES_SHORT_WAY_DEFAULT (csrc/osmt_internal.h): the W of the dedup's two paths
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "resolve_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", tmp, src])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz = C.c_void_p, C.c_size_t
        L.res_new.restype = vp
        L.res_new.argtypes = [C.POINTER(abi.RawOsmDesc)]
        L.res_free.argtypes = [vp]
        L.res_get.restype = sz
        L.res_get.argtypes = [vp, C.c_int, vp, sz]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt::resolve_refs_host, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "resolve_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


class World:
    """node_ids: [global id]; ways: [(global id, [node id])]; relations: [[(way id, inner)]] — relation i has the global id
    7000 + 3 i; nodes_seen / ways_seen: per way / relation, or None."""

    def __init__(self, node_ids, ways=(), relations=(), nodes_seen=None, ways_seen=None):
        self.node_ids = [int(g) for g in node_ids]
        self.ways = [(int(g), [int(x) for x in refs]) for g, refs in ways]
        self.relations = [[(int(g), int(i)) for g, i in r] for r in relations]
        self.nodes_seen = None if nodes_seen is None else [int(s) for s in nodes_seen]
        self.ways_seen = None if ways_seen is None else [int(s) for s in ways_seen]
        self.r = styled.RawOsm(self.node_ids, self.ways, [(7000 + 3 * i, r) for i, r in enumerate(self.relations)], self.nodes_seen, self.ways_seen)

    def write_text(self, path):
        """the form tests/resolve_host_main.cpp reads"""
        with_seen = self.nodes_seen is not None
        assert with_seen == (self.ways_seen is not None)
        lines = [f"{int(with_seen)} {len(self.node_ids)}"] + [str(g) for g in self.node_ids] + [str(len(self.ways))]
        for k, (g, refs) in enumerate(self.ways):
            lines.append(" ".join([str(g), str(self.nodes_seen[k] if with_seen else 0), str(len(refs))] + [str(x) for x in refs]))
        lines.append(str(len(self.relations)))
        for k, r in enumerate(self.relations):
            lines.append(" ".join([str(self.ways_seen[k] if with_seen else 0), str(len(r))] + [f"{g} {i}" for g, i in r]))
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- the model ------------------------------------------------------------------------------------------------------------
def storage(ids, seen):
    """OsmEntityStorage after `seen` calls of add(): insert overwrites"""
    global_id_to_local_id = {}
    for local, g in enumerate(ids[:seen]):
        global_id_to_local_id[g] = local
    return global_id_to_local_id


def postprocess_node_refs(refs):
    if not refs:
        return []
    seen_node_pairs = set()
    out = [refs[0]]
    for idx in range(1, len(refs)):
        cur, prev = refs[idx], refs[idx - 1]
        if (cur, prev) not in seen_node_pairs and (prev, cur) not in seen_node_pairs:
            seen_node_pairs.add((cur, prev))
            out.append(cur)
    return out


def model(world):
    """the arrays and counts osmt_resolve_refs gives, from the definition"""
    way_off, way_nodes, rel_off, rel_ways, rel_inner = [0], [], [0], [], []
    unresolved = removed = way_unresolved = 0
    table, table_seen = None, None
    for k, (_, refs) in enumerate(world.ways):
        seen = len(world.node_ids) if world.nodes_seen is None else world.nodes_seen[k]
        if seen != table_seen:
            table, table_seen = storage(world.node_ids, seen), seen
        local = [table[g] for g in refs if g in table]
        unresolved += len(refs) - len(local)
        kept = postprocess_node_refs(local)
        removed += len(local) - len(kept)
        way_nodes += kept
        way_off.append(len(way_nodes))
    way_ids = [g for g, _ in world.ways]
    table, table_seen = None, None
    for k, members in enumerate(world.relations):
        seen = len(way_ids) if world.ways_seen is None else world.ways_seen[k]
        if seen != table_seen:
            table, table_seen = storage(way_ids, seen), seen
        for g, inner in members:
            if g in table:
                rel_ways.append(table[g])
                rel_inner.append(inner)
            else:
                way_unresolved += 1
        rel_off.append(len(rel_ways))
    u32 = lambda v: np.array(v, dtype=np.uint32)
    return {"way_node_off": u32(way_off), "way_nodes": u32(way_nodes), "relation_way_off": u32(rel_off), "relation_ways": u32(rel_ways),
            "relation_way_inner": np.array(rel_inner, dtype=np.uint8), "counts": (len(way_nodes), len(rel_ways), unresolved, removed, way_unresolved)}


def twin(world):
    """osmt::resolve_refs_host as a dict of arrays and counts"""
    L, d = shim(), world.r.as_desc()
    h = L.res_new(C.byref(d))
    if not h:
        raise ValueError("osmt::resolve_refs_host threw")
    try:
        out = {}
        for k, name in enumerate(ARRAYS + ("counts",)):
            n = L.res_get(h, k, None, 0)
            a = np.zeros(n, np.uint64 if name == "counts" else DTYPES.get(name, np.uint32))
            L.res_get(h, k, a.ctypes.data, n)
            out[name] = a
        out["counts"] = tuple(int(c) for c in out["counts"])
        return out
    finally:
        L.res_free(h)


def same(got, want):
    for name in ARRAYS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (name, a[:40], b[:40])
    assert tuple(got["counts"]) == tuple(want["counts"]), (got["counts"], want["counts"])


def ways_of(arrays):
    off, nodes = arrays["way_node_off"], arrays["way_nodes"]
    return [nodes[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


# ---- the table of known results -----------------------------------------------------------------------------------------------
# node ids: a = 10, b = 20, c = 30 at the indices 0, 1, 2; X = 99 is no node.  (references, local result)
A, B, CC, X = 10, 20, 30, 99
TABLE = [
    ("empty", [], []),
    ("one", [A], [0]),
    ("two", [A, B], [0, 1]),
    ("there and back", [A, B, A], [0, 1]),
    ("one node three times", [A, A, A], [0, 0]),
    ("a loop and a step more", [A, B, CC, A, B], [0, 1, 2, 0]),
    ("to and fro", [A, B, A, B, A], [0, 1]),
    ("the original predecessor", [A, B, A, CC], [0, 1, 2]),
    ("the drop comes first", [A, X, B, A], [0, 1]),
]


def table_world(row):
    return World([A, B, CC], [(500, row[1])], [])


def table_arrays(row):
    u32 = lambda v: np.array(v, dtype=np.uint32)
    unresolved = sum(1 for g in row[1] if g == X)
    return {"way_node_off": u32([0, len(row[2])]), "way_nodes": u32(row[2]), "relation_way_off": u32([0]), "relation_ways": u32([]),
            "relation_way_inner": np.array([], dtype=np.uint8), "counts": (len(row[2]), 0, unresolved, len(row[1]) - unresolved - len(row[2]), 0)}


def table_world_all():
    """every row a way of one world, and a relation that names them all"""
    return World([A, B, CC], [(500 + i, r[1]) for i, r in enumerate(TABLE)], [[(500 + i, i & 1) for i in range(len(TABLE))]])


# ---- worlds both test files use ------------------------------------------------------------------------------------------------
def walk(n, back_and_forth):
    """n node indices: all distinct, or a walk over n // 2 + 1 nodes there and back, so that about half the positions repeat a pair"""
    if not back_and_forth:
        return list(range(n))
    k = n // 2 + 1
    return (list(range(k)) + list(range(k - 2, -1, -1)))[:n]


def way_length_world(lengths, back_and_forth, miss_every=0):
    """one way per length over nodes with the ids 1000 + 7 i; with miss_every, an id that is no node after every so many
    references (the way's resolved length stays what `lengths` says)"""
    n_nodes = max(lengths + [1])
    ways = []
    for k, n in enumerate(lengths):
        refs = []
        for j, i in enumerate(walk(n, back_and_forth)):
            refs.append(1000 + 7 * i)
            if miss_every and j % miss_every == miss_every - 1:
                refs.append(5)
        ways.append((100 + k, refs))
    return World([1000 + 7 * i for i in range(n_nodes)], ways, [[(100 + k, k & 1) for k in range(len(ways))]])


def counted_world(seed, n_nodes, n_ways, n_way_refs, n_rels, n_rel_refs, with_seen=False):
    """exact element counts and reference totals; ids from a range twice the node count, so that about half the references miss
    and ids repeat; a few ids above 2^36"""
    rng = np.random.default_rng(seed)
    span = max(2 * n_nodes, 4)

    def gid(v):
        v = int(v)
        return v if v % 11 else (1 << 40) + v

    def cut(total, owners):
        if owners == 0:
            assert total == 0
            return []
        marks = np.sort(rng.integers(0, total + 1, owners - 1)).tolist()
        return [b - a for a, b in zip([0] + marks, marks + [total])]

    node_ids = [gid(v) for v in rng.integers(0, span, n_nodes)]
    ways = [(gid(rng.integers(0, max(2 * n_ways, 4))), [gid(v) for v in rng.integers(0, span, n)]) for n in cut(n_way_refs, n_ways)]
    rels = [[(gid(v), int(rng.integers(0, 2))) for v in rng.integers(0, max(2 * n_ways, 4), n)] for n in cut(n_rel_refs, n_rels)]
    if not with_seen:
        return World(node_ids, ways, rels)
    return World(node_ids, ways, rels, np.sort(rng.integers(0, n_nodes + 1, n_ways)), np.sort(rng.integers(0, n_ways + 1, n_rels)))


def run_world(n_same, with_seen):
    """n_same nodes that share the global id 777 between nodes of lower and higher ids; ways that name it, seeing none, one, half
    and all of the run; the same for a run of ways under one id"""
    node_ids = [3, 776] + [777] * n_same + [778, 1 << 50]
    refs = [776, 777, 778, 777, 3, 1 << 50, 777]
    way_seen = [0, 1, 2, 3, 2 + n_same // 2, 2 + n_same, 3 + n_same, len(node_ids)]
    ways = [(42 if k % 2 else 40 + k, list(refs)) for k in range(len(way_seen))]
    rels = [[(42, 0), (40, 1), (41, 0), (42, 1)] for _ in range(len(ways) + 1)]
    if not with_seen:
        return World(node_ids, ways, rels)
    return World(node_ids, ways, rels, way_seen, list(range(len(ways) + 1)))


def key_byte_world(shifts):
    """ids that differ only in the byte(s) given by `shifts`"""
    base = 0x0102030405060708
    ids = [base ^ (v << s) for s in shifts for v in (0, 1, 2, 0x80, 0xFF)]
    ids = list(dict.fromkeys(ids))
    rng = np.random.default_rng(len(shifts))
    order = rng.permutation(len(ids)).tolist()
    node_ids = [ids[i] for i in order]
    ways = [(ids[k], [ids[j] for j in rng.integers(0, len(ids), 9)] + [base ^ (3 << shifts[0])]) for k in range(len(ids))]
    return World(node_ids, ways, [[(g, 1) for g in ids] + [(base ^ (5 << shifts[-1]), 0)]])


BIG_IDS = [(1 << 36) + 1, (1 << 40) + 7, (1 << 63) + 2, (1 << 64) - 1]


def random_world(seed):
    """a small file in a random element order: ids from a small range (collisions, repeats and misses are common) and a few
    above 2^36, one at 2^64 - 1; `seen` from the file order, absent, or arbitrary"""
    rng = np.random.default_rng(seed)
    pool = list(range(1, 10)) + BIG_IDS
    pick = lambda: pool[int(rng.integers(0, len(pool)))]
    kinds = rng.permutation(["n"] * int(rng.integers(0, 14)) + ["w"] * int(rng.integers(0, 8)) + ["r"] * int(rng.integers(0, 4))).tolist()
    node_ids, ways, rels, nodes_seen, ways_seen = [], [], [], [], []
    for kind in kinds:
        if kind == "n":
            node_ids.append(pick())
        elif kind == "w":
            few = [pick() for _ in range(int(rng.integers(1, 4)))]  # a way that walks over a few ids repeats pairs
            n = int(rng.integers(0, 12))
            ways.append((pick(), [few[int(rng.integers(0, len(few)))] if rng.random() < 0.7 else pick() for _ in range(n)]))
            nodes_seen.append(len(node_ids))
        else:
            rels.append([(pick(), int(rng.integers(0, 2))) for _ in range(int(rng.integers(0, 6)))])
            ways_seen.append(len(ways))
    how = seed % 3
    if how == 0:  # nodes, then ways, then relations
        return World(node_ids, ways, rels)
    if how == 2:  # any values the validation admits
        nodes_seen = rng.integers(0, len(node_ids) + 1, len(ways)).tolist()
        ways_seen = rng.integers(0, len(ways) + 1, len(rels)).tolist()
    return World(node_ids, ways, rels, nodes_seen, ways_seen)
