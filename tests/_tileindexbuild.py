"""Shared helpers of the tile index build tests (tests/test_tile_index_build_cpu.py, tests/test_gpu_tile_index_build.py): the
shim over osmt::tile_index_of (host/osmt_tilequery.hpp), the host twin of osmt_build_tile_index; the restatement of the same
index through tests/_geodata.get_tile_references (the Python saver.rs); and small worlds whose nodes are placed by their
Mercator factors — the factors are an input of the build, so a test states them exactly."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT, get_tile_references

SHIM = os.path.join(ROOT, "tests", "_build", "libtile_index_build_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "tile_index_build_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_tilequery.hpp", "osmt_geodata.hpp")] + [os.path.join(ROOT, "include", "osmtile.h")]
ARRAYS = ("tile_xy", "way_off", "ways", "mp_off", "mps", "node_off", "nodes")
WORLD = 1 << 18
HI = WORLD - 1
B = 1024  # OSMT_PYR_SORT_BLOCK
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "tile_index_build_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz = C.c_void_p, C.c_size_t
        L.tib_new.restype = vp
        L.tib_new.argtypes = [C.POINTER(abi.GeodataDesc), vp]
        L.tib_free.argtypes = [vp]
        L.tib_get.restype = sz
        L.tib_get.argtypes = [vp, C.c_int, vp, sz]
        L.tib_refused.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_int)]
        L.tib_node_tiles.argtypes = [vp, sz, vp]
        L.tib_node_tiles.restype = None
        L.tib_mercator_factors.argtypes = [vp, sz, vp]
        L.tib_mercator_factors.restype = None
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt::tile_index_of, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "tile_index_build_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


class Refused(Exception):
    """a factor of exactly 1.0: (node, 'x' or 'y')"""

    def __init__(self, node, axis):
        super().__init__(f"node {node}: {axis} factor is exactly 1.0")
        self.node, self.axis = node, axis


class World:
    """factors: [n, 2] Mercator factors of the nodes; ways: [[node]]; polygons: [[node]]; mps: [[polygon]].  The (lat, lon) of
    the geodata are zeros: the build reads the factors alone."""

    def __init__(self, factors, ways=(), polygons=(), mps=()):
        self.factors = np.ascontiguousarray(factors, dtype=np.float64).reshape(-1, 2)
        self.ways, self.polygons, self.mps = [list(w) for w in ways], [list(p) for p in polygons], [list(m) for m in mps]
        self.node_gids = np.arange(len(self.factors), dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
        self.g = styled.Geodata(np.zeros((len(self.factors), 2)), [(5000 + i, w) for i, w in enumerate(self.ways)], self.polygons,
                                [(9000 + i, m) for i, m in enumerate(self.mps)])

    @classmethod
    def at_tiles(cls, tiles, ways=(), polygons=(), mps=(), frac=0.5):
        """nodes in the middle (frac) of the z18 tiles `tiles`: (t + frac) / 2^18 is exact"""
        t = np.asarray(tiles, dtype=np.float64).reshape(-1, 2)
        return cls((t + frac) / WORLD, ways, polygons, mps)

    def node_tiles(self):
        """osmt::max_zoom_coordinate of every factor: [n, 2] uint32"""
        out = np.zeros((len(self.factors), 2), np.uint32)
        shim().tib_node_tiles(self.factors.ctypes.data, len(self.factors), out.ctypes.data)
        return out

    def write_text(self, path):
        """the form tests/tile_index_build_host_main.cpp reads"""
        def lists(v):
            return [str(len(v))] + [" ".join([str(len(x))] + [str(i) for i in x]) for x in v]

        lines = [str(len(self.factors))] + [float(f).hex() for f in self.factors.reshape(-1)] + lists(self.ways) + lists(self.polygons) + lists(self.mps)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def mercator_factors(latlon):
    """osmt::mercator_factors with this machine's libm"""
    ll = np.ascontiguousarray(latlon, np.float64).reshape(-1, 2)
    out = np.zeros_like(ll)
    shim().tib_mercator_factors(ll.ctypes.data, len(ll), out.ctypes.data)
    return out


def twin_of(g, factors):
    """osmt::tile_index_of over a styled.Geodata as a dict of uint32 arrays; raises Refused"""
    L, d = shim(), g.as_desc()
    f = np.ascontiguousarray(factors, dtype=np.float64).reshape(-1, 2)
    h = L.tib_new(C.byref(d), f.ctypes.data)
    if not h:
        raise ValueError("osmt::tile_index_of threw: a factor outside [0, 1]")
    try:
        node, axis = C.c_size_t(), C.c_int()
        if L.tib_refused(h, C.byref(node), C.byref(axis)):
            raise Refused(int(node.value), "xy"[axis.value])
        out = {}
        for k, name in enumerate(ARRAYS):
            n = L.tib_get(h, k, None, 0)
            a = np.zeros(n, np.uint32)
            L.tib_get(h, k, a.ctypes.data, n)
            out[name] = a.reshape(-1, 2) if name == "tile_xy" else a
        return out
    finally:
        L.tib_free(h)


def twin(world):
    return twin_of(world.g, world.factors)


def restate(world, node_tiles=None):
    """the same index through get_tile_references, the Python restatement of saver.rs:167-226, with max_zoom_tile answered from
    the nodes' tiles (default: the twin's formula over the world's factors)"""
    t = world.node_tiles() if node_tiles is None else node_tiles
    nodes = [(i, float(i), 0.0, {}) for i in range(len(t))]  # the "latitude" is the node's index
    refs = get_tile_references(nodes, [(0, w, {}) for w in world.ways], world.polygons, [(0, m, {}) for m in world.mps],
                               lambda lat, lon: (int(t[int(lat)][0]), int(t[int(lat)][1])))
    return arrays_of(refs)


def arrays_of(refs):
    """{(x, y): (nodes, ways, multipolygons)} as the dict of arrays osmt_read_tile_index gives"""
    keys = sorted(refs)
    out = {"tile_xy": np.array(keys, dtype=np.uint32).reshape(-1, 2)}
    for which, (off, pool) in zip((1, 2, 0), (("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes"))):
        lists = [sorted(refs[k][which]) for k in keys]
        out[off] = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.uint32)
        out[pool] = np.array([e for v in lists for e in v], dtype=np.uint32)
    return out


def same(got, want):
    for name in ARRAYS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


# ---- worlds both test files use -----------------------------------------------------------------------------------------
def random_world(seed, n_nodes=400, n_ways=120, n_polys=40, n_mps=25):
    """clusters of nodes, ways of 0 .. 9 nodes inside a cluster, polygons, multipolygons of 0 .. 3 polygons"""
    rng = np.random.default_rng(seed)
    centres = [(131072, 131072), (70000, 70011), (10, 262100), (262100, 10)]
    c = rng.integers(0, len(centres), n_nodes)
    t = np.array([centres[k] for k in c], dtype=np.float64) + rng.integers(-6, 7, (n_nodes, 2))
    f = (t + rng.random((n_nodes, 2))) / WORLD
    by = [np.nonzero(c == k)[0] for k in range(len(centres))]

    def some(most):
        k = int(rng.integers(0, len(centres)))
        n = int(rng.integers(0, most + 1))
        return rng.choice(by[k], n).tolist() if len(by[k]) else []  # inside one cluster: no rectangle of 60 000 x 60 000 tiles

    ways = [some(9) for _ in range(n_ways)]
    polys = [some(6) for _ in range(n_polys)]
    mps = []
    for _ in range(n_mps):
        k = int(rng.integers(0, 4))
        cand = rng.integers(0, n_polys, k).tolist()
        first = [p for p in cand if polys[p]]
        keep = [p for p in cand if not polys[p] or not first or int(c[polys[p][0]]) == int(c[polys[first[0]][0]])]
        mps.append(keep)
    return World(f, ways, polys, mps)


def shapes_world():
    """every shape of entity the definition names, around tile (1000, 2000)"""
    X, Y = 1000, 2000
    tiles = [(X, Y), (X + 3, Y + 2), (X + 3, Y), (X + 9, Y + 9), (X + 20, Y), (X + 20, Y + 1), (X + 30, Y + 5), (X + 31, Y + 7), (X + 50, Y)]
    ways = [[], [], [0], [0, 1], [], [], [2, 2], [1, 0, 2], [], []]  # empty first, two in a row in the middle, two last
    polys = [[0, 1, 2], [], [4, 5], [6, 7], [3], []]  # 1 and 5 empty; 4 is named by nobody
    mps = [[], [1], [1, 5], [0, 1, 2], [3], [3, 0], [5, 2, 1]]  # none; empty only; an empty one between two full; 3 shared by two
    return World.at_tiles(tiles, ways, polys, mps)


def rectangles_world():
    X, Y = 5000, 7000
    tiles = [(X, Y), (X, Y + 6), (X + 6, Y), (X + 39, Y + 39), (X + 100, Y + 100), (X + 103, Y + 104), (X + 200, Y), (X + 300, Y + 1), (X + 100, Y + 104)]
    ways = [[0], [0, 1], [0, 2], [0, 3], [4, 5], [5, 4], [0, 1, 2]]  # 1x1, 1xN, Nx1, 40x40, a diagonal and its twin, an L
    polys = [[4, 5], [7]]
    mps = [[0], [1]]  # shares the diagonal's tiles; a single tile
    return World.at_tiles(tiles, ways, polys, mps)  # node 6: a tile with a node and nothing else


def edges_world():
    """tile edges, stated as factors: k / 2^18 belongs to tile k, its predecessor to k - 1; 0.0; the largest double below 1.0"""
    k = 77777
    below_one = np.nextafter(1.0, 0.0)
    f = [(k / WORLD, k / WORLD), (np.nextafter(k / WORLD, 0.0), k / WORLD), (k / WORLD, np.nextafter(k / WORLD, 0.0)), (0.0, 0.0), (below_one, below_one),
         (0.0, below_one), (below_one, 0.0), (np.nextafter(0.0, 1.0), 0.5), (0.5, np.nextafter(0.5, 0.0)), (1.0 / WORLD, np.nextafter(1.0 / WORLD, 0.0))]
    return World(f, [[0, 1], [2], [3], [4]], [[5], [6]], [[0], [1]])


EDGE_WORLDS = {"shapes": shapes_world, "rectangles": rectangles_world, "edges": edges_world, "nothing": lambda: World(np.zeros((0, 2))),
               "one node": lambda: World.at_tiles([(HI, 0)]), "ways without nodes": lambda: World.at_tiles([(3, 4)], [[], []], [[]], [[0], []])}
