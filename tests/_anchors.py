"""Shared helpers of the tile-anchor tests (tests/test_label_positions_tiles_cpu.py, tests/test_gpu_label_positions_tiles.py):
the shim over osmt::mercator_factors / osmt::label_rings_of (tests/anchors_shim.cpp), the sanitized stand-alone host program,
the demo of osmt::TileLabelPositions, restatements of the projection in Python floats and in numpy, and a small synthetic
world whose shapes are stated in pixels of one z18 tile and converted to degrees."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, labels, styled
from tests._geodata import ROOT
from tests._tilequery import center_z18

SHIM = os.path.join(ROOT, "tests", "_build", "libanchors_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "anchors_host_main")
DEMO = os.path.join(ROOT, "tests", "_build", "anchors_fallback_demo")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_labelable.hpp", "osmt_geodata.hpp")] + [os.path.join(ROOT, "include", "osmtile.h")]
_lib = None
MP = abi.STYLED_MULTIPOLYGON


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "anchors_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
        L.an_mercator_factors.argtypes = [vp, sz, vp]
        L.an_mercator_factors.restype = None
        L.an_label_rings.argtypes = [C.POINTER(abi.GeodataDesc), vp, u32, C.c_uint8, u32, u32, u32, vp, sz, vp, sz, C.POINTER(sz)]
        L.an_position.argtypes = [C.POINTER(abi.GeodataDesc), vp, u32, C.c_uint8, u32, u32, u32, C.c_int, vp]
        L.an_sizeof.argtypes = [C.c_int]
        L.an_sizeof.restype = sz
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over the mirror, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "anchors_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def build_demo():
    """osmt::TileLabelPositions (device call + host fallback) linked to the C ABI"""
    src = os.path.join(ROOT, "tests", "anchors_fallback_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    so = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(so), "build libosmtile.so first (__graft_entry__.build())"
    if _stale(DEMO, [src, so] + _HDRS):
        os.makedirs(os.path.dirname(DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", DEMO, src, "-L" + libdir, "-losmtile", "-Wl,-rpath," + libdir,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
    return DEMO


# ---- the host mirror ----------------------------------------------------------------------------------------------------
def mercator_factors(latlon):
    """osmt::mercator_factors: [n, 2] (lat, lon) in degrees -> [n, 2] factors, with the host's libm"""
    ll = np.ascontiguousarray(latlon, np.float64).reshape(-1, 2)
    out = np.zeros_like(ll)
    shim().an_mercator_factors(ll.ctypes.data, len(ll), out.ctypes.data)
    return out


def label_rings(geodata, factors, entity, zoom, x, y, scale):
    """osmt::label_rings_of -> (points per ring [k] uint32, points [m, 2] float64); None for an id the geodata does not have"""
    d = geodata.as_desc()
    f = np.ascontiguousarray(factors, np.float64)
    counts = (C.c_size_t * 2)()
    rc = shim().an_label_rings(C.byref(d), f.ctypes.data, entity, zoom, x, y, scale, None, 0, None, 0, counts)
    if rc == 2:
        return None
    ring_n = np.zeros(counts[0], np.uint32)
    pts = np.zeros((counts[1], 2), np.float64)
    rc = shim().an_label_rings(C.byref(d), f.ctypes.data, entity, zoom, x, y, scale, ring_n.ctypes.data, len(ring_n), pts.ctypes.data, len(pts), counts)
    assert rc == 0
    return ring_n, pts


def mirror_position(geodata, factors, entity, zoom, x, y, scale, capped=False):
    d = geodata.as_desc()
    f = np.ascontiguousarray(factors, np.float64)
    out = np.zeros(1, labels.LABEL_POSITION_DTYPE)
    assert shim().an_position(C.byref(d), f.ctypes.data, entity, zoom, x, y, scale, int(capped), out.ctypes.data) == 0
    return out[0]


# ---- restatements -------------------------------------------------------------------------------------------------------
def py_factors(lat, lon):
    """the factors of one node in Python floats: tile.rs:88-95 up to the division by 2 PI"""
    lat_rad, lon_rad = lat * (math.pi / 180.0), lon * (math.pi / 180.0)
    x = lon_rad + math.pi
    y = math.pi - math.log(math.tan((math.pi / 4.0) + (lat_rad / 2.0)))
    return x / (2.0 * math.pi), y / (2.0 * math.pi)


def py_project(f, zoom, x, y, scale):
    """one point from its factors in Python floats: three roundings"""
    dim = float(256 * (1 << zoom))
    px, py = f[0] * dim, f[1] * dim
    px, py = px - float((x * 256) & 0xFFFFFFFF), py - float((y * 256) & 0xFFFFFFFF)
    return px * float(scale), py * float(scale)


def np_project(f, zoom, x, y, scale):
    """[n, 2] factors -> [n, 2] points: the three operations as three numpy statements (each elementwise, each rounds once)"""
    f = np.asarray(f, np.float64).reshape(-1, 2)
    dim = np.float64(256 * (1 << zoom))
    off = np.array([float((x * 256) & 0xFFFFFFFF), float((y * 256) & 0xFFFFFFFF)], np.float64)
    p = f * dim
    p = p - off
    p = p * np.float64(scale)
    return p


def round_half_away(v):
    """f64::round"""
    v = np.asarray(v, np.float64)
    t = np.trunc(v)
    return (t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)).astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- a synthetic world --------------------------------------------------------------------------------------------------
T18 = center_z18()  # the z18 tile the shapes are stated in


def latlon_of_px(px, py, tile=None):
    """pixel (px, py) of the z18 tile `tile` (scale 1) -> (lat, lon) in degrees"""
    tx, ty = tile or T18
    dim = 256.0 * (1 << 18)
    wx, wy = tx * 256.0 + px, ty * 256.0 + py
    return math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * wy / dim)))), wx / dim * 360.0 - 180.0


class World:
    """Nodes are added by pixel shape; ways / polygons / multipolygons name them.  geodata(): a styled.Geodata."""

    def __init__(self):
        self.nodes, self.ways, self.polygons, self.mps = [], [], [], []

    def shape(self, pts_px):
        ids = []
        for px, py in np.asarray(pts_px, np.float64).reshape(-1, 2):
            self.nodes.append(latlon_of_px(float(px), float(py)))
            ids.append(len(self.nodes) - 1)
        return ids

    def way(self, node_ids):
        self.ways.append((5000 + len(self.ways), list(node_ids)))
        return len(self.ways) - 1

    def polygon(self, node_ids):
        self.polygons.append(list(node_ids))
        return len(self.polygons) - 1

    def mp(self, polygon_ids):
        self.mps.append((9000 + len(self.mps), list(polygon_ids)))
        return (len(self.mps) - 1) | MP

    def geodata(self):
        return styled.Geodata(np.array(self.nodes, np.float64).reshape(-1, 2), self.ways, self.polygons, self.mps)


def entity_rings(g, entity):
    """the node lists get_label_position is given for an entity of a styled.Geodata: a way's one ring, ALL polygons of a multipolygon"""
    i = entity & ~MP
    if entity & MP:
        polys = g.multipolygon_polygons[g.multipolygon_polygon_off[i]:g.multipolygon_polygon_off[i + 1]]
        return [g.polygon_nodes[g.polygon_node_off[p]:g.polygon_node_off[p + 1]] for p in polys]
    return [g.way_nodes[g.way_node_off[i]:g.way_node_off[i + 1]]]


def expected_expansion(g, factors, tiles, requests, scale):
    """(rings [n, 2] uint32, points [m, 2] float64) of a batch from the numpy restatement; tiles: [(zoom, x, y)], requests: [(entity, tile)]"""
    rings, pts, at = [], [], 0
    for entity, t in requests:
        zoom, x, y = tiles[t]
        for nodes in entity_rings(g, entity):
            rings.append((at, len(nodes)))
            at += len(nodes)
            if len(nodes):
                pts.append(np_project(factors[nodes], zoom, x, y, scale))
    return np.array(rings, np.uint32).reshape(-1, 2), (np.concatenate(pts) if pts else np.zeros((0, 2)))


def as_label_requests(g, requests, scale):
    """the osmt_label_request records of the same batch (for osmt_label_positions / the mirror over expected_expansion's arrays)"""
    rq = np.zeros(len(requests), labels.LABEL_REQUEST_DTYPE)
    at = 0
    for i, (entity, _) in enumerate(requests):
        n = len(entity_rings(g, entity))
        rq[i] = (at, n, float(scale))
        at += n
    return rq
