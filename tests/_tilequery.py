"""Shared helpers of the tile-query tests (tests/test_tile_query_cpu.py, tests/test_gpu_tile_query.py): the shim over
osm_renderer_amd/host/osmt_tilequery.hpp (osmt::TileIndexDesc, osmt::StyleBindings, the host mirror
osmt::styled_areas_of_tile), a Python restatement of the query written from its specification alone, and small worlds whose
tile index is placed freely."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT, Reader, write_geodata

LAT0, LON0 = 55.75, 37.61
WORLD = 1 << 18
SHIM = os.path.join(ROOT, "tests", "_build", "libtilequery_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "tilequery_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_tilequery.hpp", "osmt_geodata.hpp")] + [os.path.join(ROOT, "include", "osmtile.h")]
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "tilequery_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SHIM, src])
        L = C.CDLL(SHIM)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.tq_index_new.restype = vp
        L.tq_index_new.argtypes = [vp]
        L.tq_index_get.restype = C.POINTER(abi.TileIndexDesc)
        L.tq_index_get.argtypes = [vp]
        L.tq_index_free.argtypes = [vp]
        L.tq_bindings_new.restype = vp
        L.tq_bindings_new.argtypes = [C.c_uint32, C.c_uint8, C.c_uint8, sz, u32p, u32p, sz, u32p, u32p]
        L.tq_bindings_get.restype = C.POINTER(abi.StyleBindingsDesc)
        L.tq_bindings_get.argtypes = [vp]
        L.tq_bindings_free.argtypes = [vp]
        L.tq_areas.restype = sz
        L.tq_areas.argtypes = [vp, vp, C.c_uint8, C.c_uint32, C.c_uint32, vp, sz]
        L.tq_batch.restype = sz
        L.tq_batch.argtypes = [vp, vp, vp, sz, vp, vp, sz]
        L.tq_sizeof.restype = sz
        L.tq_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt_tilequery.hpp, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "tilequery_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


class Mirror:
    """osmt::StyleBindings + osmt::styled_areas_of_tile over a tests._geodata.Reader"""

    def __init__(self, r, way_styles, mp_styles, geodata_id=0, zoom_lo=0, zoom_hi=18):
        self.r = r
        self._b = styled.StyleBindings(geodata_id, zoom_lo, zoom_hi, way_styles, mp_styles)  # the CSR arrays
        u32 = C.POINTER(C.c_uint32)
        b = self._b
        self.h = shim().tq_bindings_new(geodata_id, zoom_lo, zoom_hi, len(way_styles), b.way_style_off.ctypes.data_as(u32), b.way_styles.ctypes.data_as(u32),
                                        len(mp_styles), b.multipolygon_style_off.ctypes.data_as(u32), b.multipolygon_styles.ctypes.data_as(u32))

    def desc(self):
        return shim().tq_bindings_get(self.h).contents

    def areas(self, zoom, x, y):
        cap = 1 << 12
        while True:
            out = np.zeros(cap, styled.STYLED_AREA_DTYPE)
            n = shim().tq_areas(self.r.h, self.h, zoom, x, y, out.ctypes.data, cap)
            if n <= cap:
                return out[:n].copy()
            cap = n

    def close(self):
        if self.h:
            shim().tq_bindings_free(self.h)
            self.h = None


def rect(zoom, x, y):
    """the z18 coordinates the 3 x 3 neighbourhood of (zoom, x, y) covers, clipped to the world: (x0, x1, y0, y1) inclusive"""
    f = 1 << (18 - zoom)
    return max(0, (x - 1) * f), min(WORLD - 1, (x + 2) * f - 1), max(0, (y - 1) * f), min(WORLD - 1, (y + 2) * f - 1)


def restate(tile_refs, n_polygons_of, way_styles, mp_styles, zoom, x, y):
    """The areas of a tile, from the specification alone: the clipped rectangle over the tile_refs dict, sorted(set()), the
    polygon-count filter, the binding expansion.  Returns (areas as [(entity, style)], references gathered before dedup,
    distinct entities among them)."""
    x0, x1, y0, y1 = rect(zoom, x, y)
    ways, mps = [], []
    for (tx, ty), (_, w, m) in tile_refs.items():
        if x0 <= tx <= x1 and y0 <= ty <= y1:
            ways += list(w)
            mps += list(m)
    out = []
    for w in sorted(set(ways)):
        out += [(w, s) for s in way_styles[w]]
    for m in sorted(set(mps)):
        if n_polygons_of[m] > 0:
            out += [(m | abi.STYLED_MULTIPOLYGON, s) for s in mp_styles[m]]
    return out, len(ways) + len(mps), len(set(ways)) + len(set(mps))


def pairs(a):
    return list(zip(a["entity"].tolist(), a["style"].tolist()))


def center_z18():
    """the z18 tile of (LAT0, LON0) by the textbook formula (the tests only need a tile near their geometry)"""
    lat = math.radians(LAT0)
    return int((LON0 + 180.0) / 360.0 * WORLD), int((1.0 - math.asinh(math.tan(lat)) / math.pi) / 2.0 * WORLD)


def max_zoom_tile(lat, lon):
    la = math.radians(lat)
    return int((lon + 180.0) / 360.0 * WORLD), int((1.0 - math.asinh(math.tan(la)) / math.pi) / 2.0 * WORLD)


def square(node, k, size=0.0004, row=7):
    """a closed way of five nodes, the k-th of a band across the centre tile"""
    lat, lon = LAT0 - 0.002 + 0.0003 * (k % row), LON0 - 0.004 + 0.0011 * (k % 9) + 0.00002 * (k // 9)
    ids = [node(lat, lon), node(lat + size, lon), node(lat + size, lon + 1.5 * size), node(lat, lon + 1.5 * size)]
    return ids + [ids[0]]


def make_world(path, n_ways, mp_polygons=(), tile_refs=None, shared_nodes=False):
    """n_ways closed ways (or, shared_nodes, ways of two nodes that all share one pair: only their ids matter) and one
    multipolygon per entry of mp_polygons with that many polygons.  Returns (Reader, tile_refs as written)."""
    nodes = []

    def node(lat, lon):
        nodes.append((1000 + len(nodes), lat, lon, {}))
        return len(nodes) - 1

    if shared_nodes:
        a, b = node(LAT0, LON0), node(LAT0 + 0.001, LON0 + 0.002)
        ways = [(5000 + k, [a, b], {}) for k in range(n_ways)]
    else:
        ways = [(5000 + k, square(node, k), {}) for k in range(n_ways)]
    polygons, multis = [], []
    for m, n in enumerate(mp_polygons):
        multis.append((9000 + m, list(range(len(polygons), len(polygons) + n)), {}))
        polygons += [square(node, 3 * m + j, size=0.0007) for j in range(n)]
    refs = write_geodata(path, nodes, ways, polygons, multis, tile_refs=tile_refs, max_zoom_tile=max_zoom_tile)
    return Reader(path), refs


def index_of(tile_refs, shuffle=None):
    """tile_refs as a styled.TileIndex; shuffle (a numpy Generator): every list in a random order — what the file holds sorted"""
    tiles = []
    for k in sorted(tile_refs):
        _, w, m = tile_refs[k]
        w, m = sorted(w), sorted(m)
        if shuffle is not None:
            w, m = list(shuffle.permutation(w)), list(shuffle.permutation(m))
        tiles.append((k, w, m))
    return styled.TileIndex(tiles)
