"""Builds and loads tests/polylabel_shim.cpp (host build of osm_renderer_amd/host/osmt_labelable.hpp) and builds
tests/polylabel_fallback_demo.cpp (osmt::LabelPositions against libosmtile.so)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "_build", "libpolylabelshim.so")
_HPP = os.path.join(_ROOT, "osm_renderer_amd", "host", "osmt_labelable.hpp")
_ABI = os.path.join(_ROOT, "include", "osmtile.h")
DEMO = os.path.join(_HERE, "_build", "polylabel_fallback_demo")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "polylabel_shim.cpp")
        deps = [src, _HPP, _ABI]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            tmp = f"{_SO}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-o", tmp, src, "-lm"])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.shim_polylabel_batch.argtypes = [vp, C.c_size_t, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.shim_polylabel_batch.restype = C.c_uint64
        L.shim_polylabel_sizeof.argtypes = [C.c_int]
        L.shim_polylabel_sizeof.restype = C.c_size_t
        _lib = L
    return _lib


def mirror(rings, points, requests, capped=True, threads=1):
    """The host mirror over an ABI batch -> (positions, queue peaks, pop counts); asserts that no NaN reached a minimum or a key."""
    from osm_renderer_amd import labels

    rings = np.ascontiguousarray(rings, np.uint32).reshape(-1, 2)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
    requests = np.ascontiguousarray(requests, labels.LABEL_REQUEST_DTYPE)
    out = np.zeros(len(requests), labels.LABEL_POSITION_DTYPE)
    peak = np.zeros(len(requests), np.uint64)
    pops = np.zeros(len(requests), np.uint64)
    nans = lib().shim_polylabel_batch(requests.ctypes.data, len(requests), rings.ctypes.data, points.ctypes.data, int(capped), threads,
                                      out.ctypes.data, peak.ctypes.data, pops.ctypes.data)
    assert nans == 0, f"{nans} NaNs reached a distance minimum or a queue key"
    return out, peak, pops


def build_demo():
    src = os.path.join(_HERE, "polylabel_fallback_demo.cpp")
    libdir = os.path.join(_ROOT, "osm_renderer_amd")
    so = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(so), "build libosmtile.so first (__graft_entry__.build())"
    if not os.path.exists(DEMO) or os.path.getmtime(DEMO) < max(os.path.getmtime(p) for p in (src, _HPP, _ABI, so)):
        os.makedirs(os.path.dirname(DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", DEMO, src, "-L" + libdir, "-losmtile",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    return DEMO
