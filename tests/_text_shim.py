"""Builds and loads tests/text_shim.cpp (host build of osm_renderer_amd/host/osmt_textplacer.hpp)."""
import ctypes as C
import os
import subprocess

from osm_renderer_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libtextshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "text_shim.cpp")
        deps = [src, os.path.join(_HERE, "..", "osm_renderer_amd", "host", "osmt_textplacer.hpp"), os.path.join(_HERE, "..", "include", "osmtile.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            tmp = f"{_SO}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.shim_text_place.argtypes = [C.POINTER(abi.TextLabelBatch), C.POINTER(abi.GlyphInstance)]
        L.shim_text_place.restype = None
        L.shim_text_validate.argtypes = [C.POINTER(abi.TextLabelBatch), C.c_size_t, C.c_char_p, C.c_size_t]
        L.shim_text_validate.restype = C.c_int
        L.shim_text_abi_sizeof.argtypes = [C.c_int]
        L.shim_text_abi_sizeof.restype = C.c_size_t
        _lib = L
    return _lib


def place(tl):
    """The host mirror on a labels.TextLabelList: GLYPH_INSTANCE_DTYPE [n_glyphs] in slot order."""
    import numpy as np

    from osm_renderer_amd import labels

    out = np.zeros(len(tl.glyphs), labels.GLYPH_INSTANCE_DTYPE)
    b = tl.as_batch()
    lib().shim_text_place(C.byref(b), out.ctypes.data_as(C.POINTER(abi.GlyphInstance)))
    return out


def validate(tl, n_jobs=None):
    """(status, reason) of osmt::validate_text_labels."""
    why = C.create_string_buffer(256)
    b = tl.as_batch()
    rc = lib().shim_text_validate(C.byref(b), tl.n_jobs if n_jobs is None else n_jobs, why, 256)
    return rc, why.value.decode()
