"""Shared helpers of the styled-feed tests (tests/test_styled_feed_cpu.py, tests/test_gpu_styled_feed.py, tests/test_gpu_styled_feed_scale.py): the shim over
osmt::style_rec_of / osmt::GeodataDesc, the conversion of test_styled_builder's style table to osmt_style_rec, a geodata
file as styled.Geodata, and a Reader look-alike that remembers what it was asked (the twin asks the same things often)."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT, Reader, write_geodata

LAT0, LON0 = 55.75, 37.61

# the integrator's Style record as tests/styled_shim.cpp reads it (osmt_style_rec without the background colour)
STYLE_DTYPE = np.dtype(
    [
        ("layer", "<i8"), ("z_index", "<f8"), ("opacity", "<f8"), ("fill_opacity", "<f8"), ("width", "<f8"), ("casing_width", "<f8"),
        ("fill_image", "<u4"), ("dashes_off", "<u4"), ("n_dashes", "<u4"), ("casing_dashes_off", "<u4"), ("n_casing_dashes", "<u4"),
        ("has_layer", "u1"), ("is_foreground_fill", "u1"),
        ("has_color", "u1"), ("color", "u1", (3,)),
        ("has_fill_color", "u1"), ("fill_color", "u1", (3,)),
        ("has_opacity", "u1"), ("has_fill_opacity", "u1"), ("has_width", "u1"), ("has_dashes", "u1"), ("line_cap", "u1"),
        ("has_casing_color", "u1"), ("casing_color", "u1", (3,)),
        ("has_casing_width", "u1"), ("has_casing_dashes", "u1"), ("casing_line_cap", "u1"), ("has_fill_image", "u1"),
    ]
)

SHIM = os.path.join(ROOT, "tests", "_build", "libstyled_feed_shim.so")
_lib = None


def shim():
    global _lib
    if _lib is None:
        srcs = [os.path.join(ROOT, "tests", f) for f in ("styled_feed_shim.cpp", "styled_shim.cpp")]
        hdrs = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_styled.hpp", "osmt_geodata.hpp", "osmt_draw.hpp")]
        hdrs.append(os.path.join(ROOT, "include", "osmtile.h"))
        if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(p) for p in srcs + hdrs):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SHIM, srcs[0]])
        L = C.CDLL(SHIM)
        vp, sz = C.c_void_p, C.c_size_t
        L.sf_style_recs.restype = sz
        L.sf_style_recs.argtypes = [vp, sz, vp, vp, vp, sz]
        L.sf_desc_new.restype = vp
        L.sf_desc_new.argtypes = [vp]
        L.sf_desc_get.restype = C.POINTER(abi.GeodataDesc)
        L.sf_desc_get.argtypes = [vp]
        L.sf_desc_free.argtypes = [vp]
        L.sf_sizeof.restype = sz
        L.sf_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def recs_of(st):
    """STYLE_DTYPE records -> styled.STYLE_REC_DTYPE, field by field (same names, same dash pool)"""
    out = np.zeros(len(st), styled.STYLE_REC_DTYPE)
    for name in st.dtype.names:
        out[name] = st[name]
    return out


def geodata_of(r):
    """a tests._geodata.Reader as styled.Geodata"""
    return styled.Geodata(
        r.node_table(),
        [(r.global_id(1, i), r.way_nodes(i)) for i in range(r.n_ways)],
        [r.polygon_nodes(i) for i in range(r.n_polygons)],
        [(r.global_id(2, i), r.multipolygon_polygons(i)) for i in range(r.n_multipolygons)],
    )


class CachedReader:
    """what _twin_areas / _twin_ops ask of a Reader, answered once per question"""

    def __init__(self, r):
        self.r, self.memo = r, {}

    def _ask(self, name, *args):
        key = (name,) + args
        if key not in self.memo:
            self.memo[key] = getattr(self.r, name)(*args)
        return self.memo[key]

    def global_id(self, kind, i):
        return self._ask("global_id", kind, i)

    def way_nodes(self, i):
        return self._ask("way_nodes", i)

    def polygon_nodes(self, i):
        return self._ask("polygon_nodes", i)

    def multipolygon_polygons(self, i):
        return self._ask("multipolygon_polygons", i)


def _file(tmp_path, oracle, nodes, ways, polygons, multis, name="w.bin"):
    p = str(tmp_path / name)
    write_geodata(p, nodes, ways, polygons, multis, max_zoom_tile=lambda a, b: oracle.coords_to_max_zoom_tile(a, b))
    return Reader(p)


def _center_tile(oracle, zoom=15, dx=0):
    cx, cy = oracle.coords_to_max_zoom_tile(LAT0, LON0)
    f = 1 << (18 - zoom)
    return cx // f + dx, cy // f


def _square(node, k, size=0.0004):
    """a closed way of five nodes, the k-th of a row across the centre tile"""
    lat, lon = LAT0 - 0.002 + 0.0003 * (k % 7), LON0 - 0.004 + 0.0011 * k
    ids = [node(lat, lon), node(lat + size, lon), node(lat + size, lon + 1.5 * size), node(lat, lon + 1.5 * size)]
    return ids + [ids[0]]


# global ids at the edges of the sort key's two words (rank:32 | gid:64 split 32 / 32) and of a signed comparison
EXTREME_WAY_GIDS = [0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 1, 5, 2**32 + 5, 2**33 + 5, 777, 2**63 + 1, 2**64 - 2, 2**31, 2**31 - 1, 2**62, 3,
                    2**63 - 2, 100, 101]
EXTREME_MP_GIDS = [2**63, 2**64 - 1, 0, 2**32, 777, 2**63 - 1]  # every one of them is a way's id too


def extreme_id_world(tmp_path, oracle, name="x.bin"):
    """20 ways and 6 relations with the ids above; every entity owns its nodes and has a usable ring, so the first node
    reference of an op names its entity (tests/_styled_order_model.py)"""
    nodes = []

    def node(lat, lon):
        nodes.append((1000 + len(nodes), lat, lon, {}))
        return len(nodes) - 1

    ways = [(g, _square(node, k) if k % 3 else _square(node, k)[:3], {}) for k, g in enumerate(EXTREME_WAY_GIDS)]
    polygons = [_square(node, 20 + k, size=0.0008) for k in range(8)]
    multis = [(g, p, {}) for g, p in zip(EXTREME_MP_GIDS, ([0], [1, 2], [3], [4], [5, 6], [7]))]
    return _file(tmp_path, oracle, nodes, ways, polygons, multis, name)


FILL_Z = [0.0, -0.0, 1.0, 2.5, -1.0, 1e300, 5e-324]


def fill_only_styles(rng, n=200):
    """n styles that fill and do nothing else, each with a colour of its own; many equal keys, layers on half of them"""
    assert n <= 256
    st = np.zeros(n, STYLE_DTYPE)
    st["has_fill_color"] = 1
    st["is_foreground_fill"] = rng.random(n) < 0.7
    st["z_index"] = rng.choice(FILL_Z, n)
    st["layer"] = rng.integers(-2, 3, n)
    st["has_layer"] = np.arange(n) % 2
    for k in range(n):
        st[k]["fill_color"] = (k, (7 * k + 3) & 255, 255 - k)
    return st, np.zeros(1)


def random_pairs(rng, n, n_entities, n_styles):
    return list(zip(rng.integers(0, n_entities, n).tolist(), rng.integers(0, n_styles, n).tolist()))
