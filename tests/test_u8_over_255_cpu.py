"""f64::from(c) / 255.0 (tile_pixels.rs:226-228) the two ways k_raster gets it (osm_renderer_amd/csrc/osmt_u8_over_255.h),
host build: the table and the computed quotient agree on all 256 bytes, bit for bit, with each other, with a division done
at run time and with numpy's."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libu8over255shim.so")


def _values():
    src = os.path.join(_HERE, "u8_over_255_shim.cpp")
    hdrs = [os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", h) for h in ("osmt_u8_over_255.h", "osmt_geom.h")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(f) for f in [src] + hdrs):
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _SO, src])
    lib = C.CDLL(_SO)
    out = np.zeros((256, 3), dtype=np.uint64)
    lib.shim_u8_over_255.argtypes = [C.POINTER(C.c_uint64)]
    lib.shim_u8_over_255.restype = None
    lib.shim_u8_over_255(out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out


def test_all_256_values_agree_bit_for_bit():
    v = _values()
    want = (np.arange(256, dtype=np.float64) / 255.0).view(np.uint64)
    for k, name in enumerate(("the table", "osmt_u8_over_255", "a run-time division")):
        bad = np.nonzero(v[:, k] != want)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} values differ from c / 255.0, first c = {int(bad[0])}: {int(v[bad[0], k]):#018x} != {int(want[bad[0]]):#018x}"


def test_the_ends_are_exact():
    v = _values()
    assert int(v[0, 1]) == 0, "0 / 255 is +0.0: a tile without a canvas is opaque black through the same quotient"
    assert v[255, 1:2].view(np.float64)[0] == 1.0
