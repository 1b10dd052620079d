"""Builds and loads tests/glyph_shim.cpp (host build of the glyph walk of osm_renderer_amd/csrc/osmt_glyph.h)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libglyphshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "glyph_shim.cpp")
        deps = [src, os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_glyph.h"),
                os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_geom.h"), os.path.join(_HERE, "..", "include", "osmtile.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            tmp = f"{_SO}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        dp, vp = C.POINTER(C.c_double), C.c_void_p
        L.shim_hypot.argtypes = [dp, C.c_size_t, dp]
        L.shim_hypot.restype = None
        L.shim_hypot_mismatches.argtypes = [dp, C.c_size_t]
        L.shim_hypot_mismatches.restype = C.c_size_t
        L.shim_glyph_expand.argtypes = [vp, vp, vp, C.c_size_t, dp, C.c_size_t]
        L.shim_glyph_expand.restype = C.c_int64
        L.shim_label_extent.argtypes = [dp, C.c_size_t, C.c_int32, C.POINTER(C.c_int32)]
        L.shim_label_extent.restype = None
        L.shim_glyph_sizeof.argtypes = [C.c_int]
        L.shim_glyph_sizeof.restype = C.c_size_t
        _lib = L
    return _lib
