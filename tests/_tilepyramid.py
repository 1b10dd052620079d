"""Shared helpers of the tile pyramid tests (tests/test_tile_pyramid_cpu.py, tests/test_gpu_tile_pyramid.py): the shim over
osm_renderer_amd/host/osmt_tilequery.hpp (osmt::tile_pyramid_level, the host twin of the device-built levels, and the mirror
queries with a pyramid) and a Python restatement of a level written from its definition alone: a dict of sets."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT

SHIM = os.path.join(ROOT, "tests", "_build", "libtile_pyramid_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "tile_pyramid_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_tilequery.hpp", "osmt_geodata.hpp")] + [os.path.join(ROOT, "include", "osmtile.h")]
ARRAYS = ("tile_xy", "way_off", "ways", "mp_off", "mps", "node_off", "nodes")
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "tile_pyramid_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SHIM, src])
        L = C.CDLL(SHIM)
        vp, sz, u32p, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.tp_level_new.restype = vp
        L.tp_level_new.argtypes = [C.POINTER(abi.TileIndexDesc), C.c_uint32, u32p, u32p]
        L.tp_level_free.argtypes = [vp]
        L.tp_level_get.restype = sz
        L.tp_level_get.argtypes = [vp, C.c_int, vp, sz]
        L.tp_pyramid_new.restype = vp
        L.tp_pyramid_add.argtypes = [vp, C.POINTER(abi.TileIndexDesc), C.c_uint32, u32p, u32p]
        L.tp_pyramid_free.argtypes = [vp]
        L.tp_pyramid_level_for.argtypes = [vp, C.c_uint32]
        L.tp_entities.restype = sz
        L.tp_entities.argtypes = [vp, vp, C.c_uint8, C.c_uint32, C.c_uint32, u64p, sz, C.c_int, C.c_int, vp, sz]
        L.tp_areas.restype = sz
        L.tp_areas.argtypes = [vp, vp, vp, C.c_uint8, C.c_uint32, C.c_uint32, u64p, sz, C.c_int, vp, sz]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt::tile_pyramid_level, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "tile_pyramid_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _node_arrays(node_lists):
    if node_lists is None:
        return None, None
    off = np.concatenate([[0], np.cumsum([len(v) for v in node_lists])]).astype(np.uint32)
    flat = np.array([n for v in node_lists for n in v] + [0], dtype=np.uint32)  # never empty: a pointer to pass
    return off, flat


def twin_level(index, level, node_lists=None):
    """osmt::tile_pyramid_level over a styled.TileIndex (node_lists: one list per index tile, or None) as a dict of uint32 arrays"""
    d = index.as_desc()
    off, flat = _node_arrays(node_lists)
    h = shim().tp_level_new(C.byref(d), level, _u32p(off) if off is not None else None, _u32p(flat) if off is not None else None)
    out = {}
    for k, name in enumerate(ARRAYS):
        n = shim().tp_level_get(h, k, None, 0)
        a = np.zeros(n, np.uint32)
        shim().tp_level_get(h, k, a.ctypes.data, n)
        out[name] = a.reshape(-1, 2) if name == "tile_xy" else a
    shim().tp_level_free(h)
    return out


def restate_level(tiles, level, with_nodes):
    """Level `level` from its definition.  tiles: [((x, y), ways, mps, nodes)] of the z18 index, lists in any order with repeats.
    A dict of sets over (x >> s, y >> s); every tile of the index gives its parent a tile, lists or not."""
    s = 18 - level
    parents = {}
    for (x, y), w, m, n in tiles:
        p = parents.setdefault((x >> s, y >> s), (set(), set(), set()))
        p[0].update(w), p[1].update(m), p[2].update(n if with_nodes else ())
    keys = sorted(parents)
    out = {"tile_xy": np.array(keys, dtype=np.uint32).reshape(-1, 2)}
    for k, (off, pool) in enumerate((("way_off", "ways"), ("mp_off", "mps"), ("node_off", "nodes"))):
        lists = [sorted(parents[key][k]) for key in keys]
        out[off] = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.uint32)
        out[pool] = np.array([e for v in lists for e in v], dtype=np.uint32)
    return out


def same_level(got, want):
    for name in ARRAYS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


def index_of(tiles):
    """[((x, y), ways, mps, nodes)] in ascending (x, y) as (styled.TileIndex, node lists)"""
    tiles = sorted(tiles, key=lambda t: t[0])
    return styled.TileIndex([(k, w, m) for k, w, m, _ in tiles]), [list(n) for _, _, _, n in tiles]


class Pyramid:
    """osmt::TilePyramid over a styled.TileIndex: the levels of `levels`, with node lists iff node_lists is given"""

    def __init__(self, index, levels, node_lists=None):
        self.h = shim().tp_pyramid_new()
        d = index.as_desc()
        off, flat = _node_arrays(node_lists)
        for lv in levels:
            shim().tp_pyramid_add(self.h, C.byref(d), lv, _u32p(off) if off is not None else None, _u32p(flat) if off is not None else None)

    def level_for(self, zoom):
        return shim().tp_pyramid_level_for(self.h, zoom)

    def close(self):
        if self.h:
            shim().tp_pyramid_free(self.h)
            self.h = None


def _ids(ids):
    if ids is None:
        return None, 0, 0
    a = np.ascontiguousarray(ids, dtype=np.uint64)
    keep = a if len(a) else np.zeros(1, np.uint64)
    return keep, len(a), 1


def entities(r, pyramid, zoom, x, y, ids=None):
    """osmt::entities_of_tile over a tests._geodata.Reader: (nodes, ways, multipolygons) as lists; pyramid: a Pyramid or None"""
    a, n, has = _ids(ids)
    out = []
    for kind in range(3):
        cap = 1 << 12
        while True:
            buf = np.zeros(cap, np.uint32)
            k = shim().tp_entities(r.h, pyramid.h if pyramid else None, zoom, x, y, a.ctypes.data_as(C.POINTER(C.c_uint64)) if has else None, n, has, kind,
                                   buf.ctypes.data, cap)
            if k <= cap:
                out.append(buf[:k].tolist())
                break
            cap = k
    return tuple(out)


def areas(tq_mirror, pyramid, zoom, x, y, ids=None):
    """osmt::styled_areas_of_tile(.., osm_ids, pyramid) over a tests._tilequery.Mirror"""
    a, n, has = _ids(ids)
    cap = 1 << 12
    while True:
        out = np.zeros(cap, styled.STYLED_AREA_DTYPE)
        k = shim().tp_areas(tq_mirror.r.h, tq_mirror.h, pyramid.h if pyramid else None, zoom, x, y, a.ctypes.data_as(C.POINTER(C.c_uint64)) if has else None, n, has,
                            out.ctypes.data, cap)
        if k <= cap:
            return out[:k].copy()
        cap = k
