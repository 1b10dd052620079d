"""Shared helpers of the multipolygon assembly tests (tests/test_polygons_cpu.py, tests/test_gpu_polygons.py): a Python
restatement of find_polygons_in_multipolygon (find_polygons.rs) over RawRelation::to_segments (importer.rs:516-537) with dicts
and sets and no sorting tricks; the shim over osmt::assemble_multipolygons_host (host/osmt_polygons.hpp), the host twin of
osmt_assemble_multipolygons; the table of the small inputs whose results are known; and the random worlds both files use."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT

SHIM = os.path.join(ROOT, "tests", "_build", "libpolygons_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "polygons_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_polygons.hpp", "osmt_geodata.hpp")] + [os.path.join(ROOT, "include", "osmtile.h")]
ARRAYS = ("polygon_node_off", "polygon_nodes", "multipolygon_ids", "multipolygon_polygon_off", "multipolygon_polygons", "multipolygon_relation", "status")
DTYPES = {"multipolygon_ids": np.uint64, "status": styled.RELATION_STATUS_DTYPE}
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "polygons_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz = C.c_void_p, C.c_size_t
        L.mpa_new.restype = vp
        L.mpa_new.argtypes = [C.POINTER(abi.RelationsDesc)]
        L.mpa_free.argtypes = [vp]
        L.mpa_get.restype = sz
        L.mpa_get.argtypes = [vp, C.c_int, vp, sz]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt::assemble_multipolygons_host, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "polygons_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


class World:
    """nodes: [n, 2] (lat, lon), any bit pattern; ways: [[node]]; relations: [[(way, inner)]] — relation i has the global id
    7000 + 3 i."""

    def __init__(self, nodes, ways, relations):
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 2)
        self.ways = [list(w) for w in ways]
        self.relations = [[(int(w), int(i)) for w, i in r] for r in relations]
        self.r = styled.Relations(self.nodes, self.ways, [(7000 + 3 * i, r) for i, r in enumerate(self.relations)])

    def segment_counts(self):
        return [sum(max(len(self.ways[w]) - 1, 0) for w, _ in r) for r in self.relations]

    def write_text(self, path):
        """the form tests/polygons_host_main.cpp reads: positions as the hex bits of (lat, lon)"""
        bits = self.nodes.view(np.uint64).reshape(-1)
        lines = [str(len(self.nodes))] + [f"{int(b):x}" for b in bits]
        lines += [str(len(self.ways))] + [" ".join([str(len(w))] + [str(i) for i in w]) for w in self.ways]
        lines += [str(len(self.relations))] + [" ".join([str(7000 + 3 * i), str(len(r))] + [f"{w} {k}" for w, k in r]) for i, r in enumerate(self.relations)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def concat(worlds):
    """the worlds' relations one after another over one node and way table"""
    n0, ways, rels = 0, [], []
    for w in worlds:
        w0 = len(ways)
        ways += [[i + n0 for i in way] for way in w.ways]
        rels += [[(k + w0, inner) for k, inner in r] for r in w.relations]
        n0 += len(w.nodes)
    return World(np.concatenate([w.nodes for w in worlds]) if worlds else np.zeros((0, 2)), ways, rels)  # the bits as they are


# ---- the restatement ------------------------------------------------------------------------------------------------------
def find_polygons(segments):
    """segments: [((id1, pos1), (id2, pos2), inner)].  (polygons, None) or (None, (rings built, unmatched))."""
    connections = {}
    for idx, (n1, n2, inner) in enumerate(segments):
        connections.setdefault(n1[1], []).append((n2[1], idx, inner))
        connections.setdefault(n2[1], []).append((n1[1], idx, inner))
    available = [True] * len(segments)
    rings, unmatched = [], len(segments)
    for start in range(len(segments)):
        if not available[start]:
            continue
        available[start] = False
        n1, n2, inner = segments[start]
        used, used_vertices, first, at = [start], {n1[1], n2[1]}, n1[1], n2[1]
        ok = False
        while True:
            nxt = None
            for other, idx, seg_inner in connections.get(at, []):
                can_use = seg_inner == inner and available[idx]
                is_duplicate = other in used_vertices and other != first
                if can_use and not is_duplicate:
                    nxt = (other, idx)
                    break
            if nxt is None:
                break
            available[nxt[1]] = False
            used.append(nxt[1])
            used_vertices.add(nxt[0])
            if nxt[0] == first:
                ok = len(used) >= 3
                break
            at = nxt[0]
        if not ok:
            return None, (len(rings), unmatched)
        unmatched -= len(used)
        rings.append(used)
    polygons = []
    for ring in rings:
        poly = []
        for k, idx in enumerate(ring):
            n1, n2, _ = segments[idx]
            if k == 0:
                poly.append(n1[0])
            poly.append(n2[0] if poly[-1] == n1[0] else n1[0])
        polygons.append(poly)
    return polygons, None


def restate(world):
    """the arrays osmt_assemble_multipolygons gives, from the definition"""
    raw = world.nodes.view(np.uint64).reshape(-1, 2)
    pos = [(int(a), int(b)) for a, b in raw]
    poly_off, poly_nodes, ids, mp_off, mp_polys, mp_rel, status = [0], [], [], [0], [], [], []
    for r, members in enumerate(world.relations):
        segments = []
        for w, inner in members:
            nodes = world.ways[w]
            for k in range(1, len(nodes)):
                segments.append(((nodes[k - 1], pos[nodes[k - 1]]), (nodes[k], pos[nodes[k]]), bool(inner)))
        polygons, figures = find_polygons(segments)
        if polygons is None:
            status.append((0, figures[0], figures[1]))
            continue
        status.append((1, len(polygons), 0))
        for p in polygons:
            mp_polys.append(len(poly_off) - 1)
            poly_nodes += p
            poly_off.append(len(poly_nodes))
        ids.append(7000 + 3 * r)
        mp_rel.append(r)
        mp_off.append(len(mp_polys))
    u32 = lambda v: np.array(v, dtype=np.uint32)
    return {"polygon_node_off": u32(poly_off), "polygon_nodes": u32(poly_nodes), "multipolygon_ids": np.array(ids, dtype=np.uint64),
            "multipolygon_polygon_off": u32(mp_off), "multipolygon_polygons": u32(mp_polys), "multipolygon_relation": u32(mp_rel),
            "status": np.array(status, dtype=styled.RELATION_STATUS_DTYPE).reshape(-1)}


def twin(world):
    """osmt::assemble_multipolygons_host as a dict of arrays"""
    L, d = shim(), world.r.as_desc()
    h = L.mpa_new(C.byref(d))
    if not h:
        raise ValueError("osmt::assemble_multipolygons_host threw")
    try:
        out = {}
        for k, name in enumerate(ARRAYS):
            n = L.mpa_get(h, k, None, 0)
            a = np.zeros(n, DTYPES.get(name, np.uint32))
            L.mpa_get(h, k, a.ctypes.data, n)
            out[name] = a
        return out
    finally:
        L.mpa_free(h)


def same(got, want):
    for name in ARRAYS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (name, a[:40], b[:40])


def polygons_of(arrays):
    """[[polygon]] per multipolygon, as lists of node ids"""
    off, nodes = arrays["polygon_node_off"], arrays["polygon_nodes"]
    mo, mp = arrays["multipolygon_polygon_off"], arrays["multipolygon_polygons"]
    return [[nodes[off[p]:off[p + 1]].tolist() for p in mp[mo[m]:mo[m + 1]]] for m in range(len(mo) - 1)]


# ---- the table of known results -----------------------------------------------------------------------------------------------
# (name, outer segments, inner segments, {node: the node whose position it has}, polygons or (rings built, unmatched))
TABLE = [
    ("triangle", "0-1 1-2 2-0", "", {}, [[0, 1, 2, 0]]),
    ("a reversed way", "0-1 2-1 2-0", "", {}, [[0, 1, 2, 0]]),
    ("two segments there and back", "0-1 1-0", "", {}, (0, 2)),
    ("open", "0-1 1-2", "", {}, (0, 2)),
    ("a degenerate start", "0-0 0-1 1-2 2-0", "", {}, [[0, 0, 1, 2, 0]]),
    ("a degenerate segment inside", "0-1 1-1 1-2 2-0", "", {}, (1, 1)),
    ("figure eight", "0-1 1-2 2-0 0-3 3-4 4-0", "", {}, [[0, 1, 2, 0], [0, 3, 4, 0]]),
    ("figure eight started off-centre", "1-2 2-0 0-3 3-4 4-0 0-1", "", {}, (0, 6)),
    ("outer and inner", "0-1 1-2 2-0", "0-5 5-6 6-0", {}, [[0, 1, 2, 0], [0, 5, 6, 0]]),
    ("closed by position", "0-1 1-2 2-7", "", {7: 0}, [[0, 1, 2, 7]]),
    ("not closed by id", "0-1 7-2 2-0", "", {7: 1}, [[0, 1, 7, 2]]),
    ("a repeated segment", "0-1 1-2 2-0 0-1", "", {}, (1, 1)),
    ("a ring and a rest", "0-1 1-2 2-0 5-6 6-7", "", {}, (1, 2)),
    ("lollipop", "0-1 1-2 2-3 3-1 1-0", "", {}, (0, 5)),
    ("no segments", "", "", {}, []),
]


def table_world(row):
    """the row as a world of one relation: every segment a way of its own, node i at (i, 0) unless the row says otherwise"""
    _, outer, inner, same_pos, _ = row
    segs = [(s, 0) for s in outer.split()] + [(s, 1) for s in inner.split()]
    ways = [[int(x) for x in s.split("-")] for s, _ in segs]
    n = max([i for w in ways for i in w] + list(same_pos) + [0]) + 1
    nodes = [(float(same_pos.get(i, i)), 0.0) for i in range(n)]
    return World(nodes, ways, [[(k, role) for k, (_, role) in enumerate(segs)]])


def table_arrays(row):
    """what the row's world must give, from the expected column alone"""
    want = row[4]
    st = styled.RELATION_STATUS_DTYPE
    u32 = lambda v: np.array(v, dtype=np.uint32)
    if isinstance(want, tuple):
        return {"polygon_node_off": u32([0]), "polygon_nodes": u32([]), "multipolygon_ids": np.array([], dtype=np.uint64), "multipolygon_polygon_off": u32([0]),
                "multipolygon_polygons": u32([]), "multipolygon_relation": u32([]), "status": np.array([(0, want[0], want[1])], dtype=st)}
    return {"polygon_node_off": u32(np.concatenate([[0], np.cumsum([len(p) for p in want])])), "polygon_nodes": u32([i for p in want for i in p]),
            "multipolygon_ids": np.array([7000], dtype=np.uint64), "multipolygon_polygon_off": u32([0, len(want)]), "multipolygon_polygons": u32(list(range(len(want)))),
            "multipolygon_relation": u32([0]), "status": np.array([(1, len(want), 0)], dtype=st)}


# ---- worlds both test files use ------------------------------------------------------------------------------------------------
def ring_world(sizes, roles=None, way_len=3):
    """one relation of closed rings of the given sizes (segments), each cut into ways of way_len segments"""
    nodes, ways, members = [], [], []
    for k, n in enumerate(sizes):
        base = len(nodes)
        nodes += [(float(base + i), float(k)) for i in range(n)]
        ring = [base + i for i in range(n)] + [base]
        for a in range(0, n, way_len):
            members.append((len(ways), roles[k] if roles else 0))
            ways.append(ring[a:a + way_len + 1])
    return World(nodes, ways, [members])


def star_world(n_triangles, relations=1, dangling=False):
    """n thin triangles THROUGH node 0, each a way of its own (a, 0, b, a): a ring starts on a - 0 and must pick 0 - b out of node
    0's list, which has 2 n entries per relation (one more with `dangling`, a last way 0 - z that rejects the relation after n
    rings); the entry ring t takes is number 2 t + 1 of the list.  Every relation names all the ways, so the relations share
    every vertex."""
    nodes = [(0.0, 0.0)] + [(float(i + 1), 1.0) for i in range(2 * n_triangles + 1)]
    ways = [[1 + 2 * t, 0, 2 + 2 * t, 1 + 2 * t] for t in range(n_triangles)] + ([[0, 2 * n_triangles + 1]] if dangling else [])
    return World(nodes, ways, [[(t, 0) for t in range(len(ways))] for _ in range(relations)])


def counted_world(n_relations, n_segments):
    """n_relations relations with n_segments segments in all: triangles, the last relation one ring of what is left (at least 3)"""
    assert n_segments >= 3 * n_relations
    sizes = [3] * (n_relations - 1) + [n_segments - 3 * (n_relations - 1)]
    nodes, ways, rels = [], [], []
    for n in sizes:
        base = len(nodes)
        nodes += [(float(base + i), 2.0) for i in range(n)]
        rels.append([(len(ways), 0)])
        ways.append([base + i for i in range(n)] + [base])
    return World(nodes, ways, rels)


def random_world(seed, n_relations=300):
    """relations of 0 .. 40 segments from random closed rings cut into ways: ways reversed, roles mixed, nodes duplicated at equal
    positions, rings that share a vertex, and a share of the relations damaged (a segment dropped, a way repeated, a role flipped)"""
    rng = np.random.default_rng(seed)
    nodes, ways, rels = [], [], []

    def new_node(pos=None):
        nodes.append(pos if pos is not None else (float(rng.integers(-80_000, 80_000)) / 1000.0 + len(nodes) * 1e-7, float(rng.integers(-170_000, 170_000)) / 1000.0))
        return len(nodes) - 1

    for _ in range(n_relations):
        members, budget = [], 36  # a repeated way adds at most 4
        shared = None
        for _ring in range(int(rng.integers(0, 4))):
            n = int(rng.integers(3, 13))
            if n > budget:
                break
            budget -= n
            role = int(rng.integers(0, 2))
            ring = [new_node() for _ in range(n)]
            if shared is not None and rng.random() < 0.15:
                ring[0] = new_node(nodes[shared])  # a second ring through a vertex of the first
            shared = ring[0]
            ring.append(ring[0])
            at = 0
            while at < n:
                k = min(int(rng.integers(1, 5)), n - at)
                way = ring[at:at + k + 1]
                if at and rng.random() < 0.3:
                    way[0] = new_node(nodes[way[0]])  # another node at the same position
                if rng.random() < 0.4:
                    way.reverse()
                members.append((len(ways), role))
                ways.append(way)
                at += k
        if rng.random() < 0.5:
            members = [members[i] for i in rng.permutation(len(members))]
        if members and rng.random() < 0.25:
            k = int(rng.integers(0, len(members)))
            how = int(rng.integers(0, 3))
            if how == 0:
                w = list(ways[members[k][0]])
                members[k] = (len(ways), members[k][1])
                ways.append(w[:-1])  # a segment dropped
            elif how == 1:
                members.insert(int(rng.integers(0, len(members) + 1)), members[k])  # a way repeated
            else:
                members[k] = (members[k][0], 1 - members[k][1])  # a role flipped
        rels.append(members)
    ways.append([])  # a way nobody names, and one of one node
    ways.append([0] if nodes else [])
    return World(nodes if nodes else np.zeros((0, 2)), ways, rels)
