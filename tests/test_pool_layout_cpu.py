"""The layout of one device allocation (osm_renderer_amd/csrc/osmt_pool_layout.h), host build.  Every registered table and every
work buffer of a per-call pipeline is laid out by it: arrays start on 256-byte boundaries, an empty array still has an offset
of its own, and the table of osmt_register_label_bindings lies where the hand-written formula it replaces put it.

What this does not cover: the order in which register_label_bindings_body adds its arrays.  The shim restates the four add()
calls (the function itself needs a device), so the last test holds pool_layout's rule against the old formula on that table's
sizes, nothing more; the table's content is read back and compared on the GPU by tests/test_gpu_tile_labels.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libpoollayoutshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "pool_layout_shim.cpp")
        hdr = os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_pool_layout.h")
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", _SO, src])
        L = C.CDLL(_SO)
        for f in (L.shim_pool_align, L.shim_pool_min_bytes, L.shim_sizeof_label_binding):
            f.restype = C.c_uint64
        L.shim_pool_layout.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64)]
        L.shim_pool_layout.restype = C.c_uint64
        L.shim_label_bindings_layout.argtypes = [C.c_uint64] * 4 + [C.POINTER(C.c_uint64)]
        L.shim_label_bindings_layout.restype = C.c_uint64
        _lib = L
    return _lib


def layout(sizes):
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offs = np.zeros(len(sizes), dtype=np.uint64)
    total = lib().shim_pool_layout(sizes.ctypes.data_as(C.POINTER(C.c_uint64)), len(sizes), offs.ctypes.data_as(C.POINTER(C.c_uint64)))
    return [int(o) for o in offs], int(total)


def _cases():
    rng = np.random.default_rng(7)
    cases = [[0], [1], [4], [255], [256], [257], [0, 0, 0], [0, 5, 0, 0, 1000, 0], [256, 256], [255, 1, 257, 0, 512, 3]]
    for _ in range(40):
        n = int(rng.integers(1, 12))
        kind = rng.integers(0, 4, size=n)  # empty, tiny, around a boundary, large
        sizes = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 8, size=n),
                                               np.where(kind == 2, 256 * rng.integers(1, 5, size=n) + rng.integers(-2, 3, size=n),
                                                        rng.integers(1, 1 << 33, size=n))))
        cases.append([int(s) for s in sizes])
    return cases


def test_constants():
    assert lib().shim_pool_align() == 256 and lib().shim_pool_min_bytes() == 4


@pytest.mark.parametrize("sizes", _cases(), ids=lambda s: "-".join(str(x) for x in s)[:40])
def test_offsets_aligned_distinct_and_inside(sizes):
    offs, total = layout(sizes)
    assert offs[0] == 0
    assert all(o % 256 == 0 for o in offs)
    assert all(b > a for a, b in zip(offs, offs[1:]))  # strictly increasing: an empty array shares its offset with nobody
    for i, (o, b) in enumerate(zip(offs, sizes)):
        end = offs[i + 1] if i + 1 < len(offs) else total
        assert o + max(b, 4) <= end  # every array, the last included, lies inside what precedes the next one
    assert total >= offs[-1] + max(sizes[-1], 4) and total % 256 == 0


def test_empty_layout_is_empty():
    assert layout([])[1] == 0


def _label_bindings_before(n_nodes, n_bindings, n_texts, n_chars, sizeof_binding):
    """register_label_bindings_body as it was before pool_layout: off = align_up(off + max(bytes, 4), 256) per array"""
    off = 0
    offs = []
    for b in ((n_nodes + 1) * 4, n_bindings * sizeof_binding, (n_texts + 1) * 4, n_chars * 4):
        offs.append(off)
        off = (off + max(b, 4) + 255) // 256 * 256
    return offs, off


@pytest.mark.parametrize("counts", [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (63, 0, 0, 0), (64, 0, 0, 0), (0, 300, 0, 0),
                                    (0, 0, 1000, 0), (0, 0, 0, 65), (1000, 777, 41, 12345)])
def test_label_bindings_table_lies_where_it_lay(counts):
    sb = int(lib().shim_sizeof_label_binding())
    offs = (C.c_uint64 * 4)()
    total = lib().shim_label_bindings_layout(*counts, offs)
    want, want_total = _label_bindings_before(*counts, sb)
    assert [int(o) for o in offs] == want and int(total) == want_total
