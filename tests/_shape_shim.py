"""Builds and loads tests/shape_shim.cpp (host build of osm_renderer_amd/host/osmt_textshaper.hpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, labels

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libshapeshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "shape_shim.cpp")
        host = os.path.join(_HERE, "..", "osm_renderer_amd", "host")
        deps = [src, os.path.join(host, "osmt_textshaper.hpp"), os.path.join(host, "osmt_textplacer.hpp"), os.path.join(_HERE, "..", "include", "osmtile.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            tmp = f"{_SO}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", tmp, src, "-lm"])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        fpp = C.POINTER(C.POINTER(abi.FontDesc))
        L.shim_shape_text.argtypes = [C.POINTER(abi.FontDesc), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(abi.TextGlyph)]
        L.shim_shape_text.restype = None
        L.shim_shape_labels.argtypes = [C.POINTER(abi.StringLabelBatch), fpp, C.POINTER(abi.TextGlyph)]
        L.shim_shape_labels.restype = None
        L.shim_string_scale.argtypes = [C.POINTER(abi.FontDesc), C.c_double]
        L.shim_string_scale.restype = C.c_double
        L.shim_font_validate.argtypes = [C.POINTER(abi.FontDesc), C.c_size_t, C.c_char_p, C.c_size_t]
        L.shim_font_validate.restype = C.c_int
        L.shim_string_validate.argtypes = [C.POINTER(abi.StringLabelBatch), C.c_size_t, fpp, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(abi.TextRun)]
        L.shim_string_validate.restype = C.c_int
        L.shim_shape_abi_sizeof.argtypes = [C.c_int]
        L.shim_shape_abi_sizeof.restype = C.c_size_t
        _lib = L
    return _lib


def _font_array(fonts):
    descs = [f.as_desc() for f in fonts]
    arr = (C.POINTER(abi.FontDesc) * max(len(descs), 1))(*[C.pointer(d) for d, _ in descs])
    return arr, descs


def shape_text(font, chars):
    """The host mirror on one text: TEXT_GLYPH_DTYPE [len(chars)]."""
    chars = np.ascontiguousarray(chars, dtype=np.uint32)
    out = np.zeros(len(chars), labels.TEXT_GLYPH_DTYPE)
    d, _keep = font.as_desc()
    lib().shim_shape_text(C.byref(d), chars.ctypes.data_as(C.POINTER(C.c_uint32)), len(chars), out.ctypes.data_as(C.POINTER(abi.TextGlyph)))
    return out


def shape_labels(sl, fonts):
    """The host mirror on a labels.StringLabelList (fonts indexed by font id): TEXT_GLYPH_DTYPE [n_chars] in slot order."""
    out = np.zeros(len(sl.chars), labels.TEXT_GLYPH_DTYPE)
    arr, _keep = _font_array(fonts)
    b = sl.as_batch()
    lib().shim_shape_labels(C.byref(b), arr, out.ctypes.data_as(C.POINTER(abi.TextGlyph)))
    return out


def string_scale(font, font_size):
    d, _keep = font.as_desc()
    return lib().shim_string_scale(C.byref(d), float(font_size))


def validate_font(font, n_outlines):
    """(status, reason) of osmt::validate_font; `font` a labels.FontTable or an abi.FontDesc."""
    why = C.create_string_buffer(256)
    d, _keep = font.as_desc() if hasattr(font, "as_desc") else (font, None)
    rc = lib().shim_font_validate(C.byref(d), n_outlines, why, 256)
    return rc, why.value.decode()


def validate(sl, fonts, n_jobs=None, want_runs=False):
    """(status, reason[, TEXT_RUN_DTYPE runs]) of osmt::validate_string_labels."""
    why = C.create_string_buffer(256)
    arr, _keep = _font_array(fonts)
    runs = np.zeros(len(sl.labels), labels.TEXT_RUN_DTYPE)
    b = sl.as_batch()
    rc = lib().shim_string_validate(C.byref(b), sl.n_jobs if n_jobs is None else n_jobs, arr, len(fonts), why, 256,
                                    runs.ctypes.data_as(C.POINTER(abi.TextRun)))
    return (rc, why.value.decode(), runs) if want_runs else (rc, why.value.decode())
