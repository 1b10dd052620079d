"""k_prebin's block-to-role mapping (osm_renderer_amd/csrc/osmt_prebin_roles.h), host build: every block of the grid is
one stroke block or one fill group, every one of either is mapped exactly once, and the stroke blocks are spread evenly
(any prefix of the grid holds its proportional share of them, give or take one)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libprebinshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "prebin_shim.cpp")
        hdr = os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_prebin_roles.h")
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _SO, src])
        L = C.CDLL(_SO)
        u32 = C.c_uint32
        L.shim_prebin_role.argtypes = [u32, u32, u32, C.POINTER(u32)]
        L.shim_prebin_role.restype = u32
        L.shim_prebin_check_all.argtypes = [u32, u32]
        L.shim_prebin_check_all.restype = C.c_uint64
        L.shim_prebin_check_at.argtypes = [u32, u32, u32]
        L.shim_prebin_check_at.restype = u32
        L.shim_prebin_n_vblk.argtypes = [u32, u32]
        L.shim_prebin_n_vblk.restype = u32
        L.shim_prebin_bin_segs_default.restype = u32
        _lib = L
    return _lib


def _role(nv, nf, b):
    idx = C.c_uint32(0xFFFFFFFF)
    r = lib().shim_prebin_role(nv, nf, b, C.byref(idx))
    return int(r), int(idx.value)


def test_small_grids_exhaustively():
    L = lib()
    for nv in range(71):
        for nf in range(71):
            assert L.shim_prebin_check_all(nv, nf) == 0, (nv, nf)


def test_small_grids_in_python():
    """The same three properties spelled out here on a few grids, so that the checker in the shim is itself checked."""
    for nv, nf in [(0, 0), (0, 5), (5, 0), (1, 1), (1, 9), (9, 1), (3, 7), (7, 3), (37, 46), (64, 64), (70, 69)]:
        T = nv + nf
        seen = {0: [], 1: []}
        strokes = 0
        for b in range(T):
            assert abs(strokes * T - b * nv) <= T, (nv, nf, b)
            role, idx = _role(nv, nf, b)
            assert role in (0, 1) and 0 <= idx < (nv if role else nf), (nv, nf, b, role, idx)
            seen[role].append(idx)
            strokes += role
        assert sorted(seen[1]) == list(range(nv)) and sorted(seen[0]) == list(range(nf)), (nv, nf)
        # any run of consecutive blocks, not only prefixes
        pre = np.concatenate([[0], np.cumsum([_role(nv, nf, b)[0] for b in range(T)])]) if T else np.zeros(1, dtype=np.int64)
        for a in range(T + 1):
            for b in range(a, T + 1):
                assert abs(int(pre[b] - pre[a]) * T - (b - a) * nv) <= T, (nv, nf, a, b)


REAL_SHAPES = [(3707, 46080), (96000, 1152000), (4 * 3707, 46080), (4 * 96000, 1152000)]


def _random_pairs():
    rnd = np.random.default_rng(20250)
    top = 2**31 - 1
    pairs = list(REAL_SHAPES) + [(1, top - 1), (top - 1, 1), (top, 0), (0, top), (top // 2, top - top // 2), (top // 2 + 1, top // 2),
                                 (2**30, 2**30 - 1), (2**16, 2**31 - 1 - 2**16), (3, top - 3), (top - 3, 3)]
    while len(pairs) < 1000:
        total = int(min(top, 2.0 ** rnd.uniform(1.0, 31.0)))
        kind = int(rnd.integers(0, 4))
        if kind == 0:
            nv = int(rnd.integers(0, total + 1))
        elif kind == 1:  # few stroke blocks
            nv = int(min(total, 2.0 ** rnd.uniform(0.0, 12.0)))
        elif kind == 2:  # few fill groups
            nv = total - int(min(total, 2.0 ** rnd.uniform(0.0, 12.0)))
        else:  # close to config 2's ratio
            nv = int(total * rnd.uniform(0.05, 0.12))
        pairs.append((nv, total - nv))
    return pairs, rnd


def test_random_grids_up_to_the_largest():
    L = lib()
    pairs, rnd = _random_pairs()
    assert all(0 < nv + nf <= 2**31 - 1 for nv, nf in pairs)
    for nv, nf in pairs:
        T = nv + nf
        if T <= 200_000:
            assert L.shim_prebin_check_all(nv, nf) == 0, (nv, nf)
            continue
        bs = set(int(v) for v in rnd.integers(0, T, size=192))
        bs |= {0, 1, 2, T - 3, T - 2, T - 1, T // 2, T // 2 + 1}
        if nv:  # around the places where a stroke block is due
            for i in (0, 1, nv // 3, nv - 1):
                c = (i * T) // nv
                bs |= {min(T - 1, max(0, c + d)) for d in (-2, -1, 0, 1, 2)}
        for b in bs:
            assert L.shim_prebin_check_at(nv, nf, b) == 0, (nv, nf, b, L.shim_prebin_check_at(nv, nf, b))


@pytest.mark.parametrize("shape", REAL_SHAPES[:2])
def test_real_shapes_exhaustively(shape):
    assert lib().shim_prebin_check_all(*shape) == 0


@pytest.mark.parametrize("bin_segs", [64, 32, 16])
def test_stroke_block_count(bin_segs):
    L = lib()
    assert L.shim_prebin_bin_segs_default() in (64, 32, 16)
    for n, want in [(0, 0), (1, 1), (bin_segs - 1, 1), (bin_segs, 1), (bin_segs + 1, 2), (237_000, -(-237_000 // bin_segs)),
                    (2**32 - 1, -(-(2**32 - 1) // bin_segs))]:
        assert L.shim_prebin_n_vblk(n, bin_segs) == want, (bin_segs, n)
