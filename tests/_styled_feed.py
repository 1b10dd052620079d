"""Shared helpers of the styled-feed tests (tests/test_styled_feed_cpu.py, tests/test_gpu_styled_feed.py): the shim over
osmt::style_rec_of / osmt::GeodataDesc, the conversion of test_styled_builder's style table to osmt_style_rec, a geodata
file as styled.Geodata, and a Reader look-alike that remembers what it was asked (the twin asks the same things often)."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from tests._geodata import ROOT

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
    """test_styled_builder.STYLE_DTYPE records -> styled.STYLE_REC_DTYPE, field by field (same names, same dash pool)"""
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
