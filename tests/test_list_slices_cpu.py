"""The list arena's slices (osm_renderer_amd/csrc/osmt_list_slices.h), host build.  Random batches — tile counts on both
sides of the threshold, counts that are even, skewed, mostly zero or all in one tile, reservation orders of every kind —
are played through the functions k_sublist uses: a batch whose lists have at most ent_cap entries in all (what fits the
arena of one cursor) is never refused, every tile's entries lie inside the arena, and no two tiles' entries overlap.
An arena that is too small refuses tiles and still places the others inside it."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liblistslicesshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "list_slices_shim.cpp")
        hdr = os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_list_slices.h")
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _SO, src])
        L = C.CDLL(_SO)
        L.shim_list_slices.restype = C.c_uint32
        L.shim_list_min_jobs.restype = C.c_uint32
        L.shim_list_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.shim_list_layout.restype = None
        L.shim_list_play.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint8)]
        L.shim_list_play.restype = C.c_uint32
        _lib = L
    return _lib


def layout(n_jobs, ent_cap):
    out = (C.c_uint64 * 3)()
    lib().shim_list_layout(n_jobs, ent_cap, out)
    return int(out[0]), int(out[1]), int(out[2])


def play(counts, order, ent_cap):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    n = len(counts)
    base = np.zeros(n, dtype=np.uint64)
    where = np.zeros(n, dtype=np.uint8)
    refused = lib().shim_list_play(n, ent_cap, counts.ctypes.data_as(C.POINTER(C.c_uint32)), order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   base.ctypes.data_as(C.POINTER(C.c_uint64)), where.ctypes.data_as(C.POINTER(C.c_uint8)))
    return int(refused), base, where


def check_placed(counts, base, where, total):
    """the tiles that were placed lie inside the arena and do not overlap"""
    placed = np.nonzero(where < 2)[0]
    lo = base[placed].astype(np.int64)
    hi = lo + counts[placed].astype(np.int64)
    assert (hi <= total).all()
    o = np.argsort(lo, kind="stable")
    assert (hi[o][:-1] <= lo[o][1:]).all()


def _counts(rnd, n, kind):
    if kind == 0:  # even
        return rnd.integers(0, 200, size=n)
    if kind == 1:  # skewed
        return (rnd.pareto(0.7, size=n) * 20).clip(0, 5_000_000).astype(np.int64)
    if kind == 2:  # mostly empty tiles
        return np.where(rnd.random(n) < 0.9, 0, rnd.integers(1, 100_000, size=n))
    if kind == 3:  # everything in one tile
        c = np.zeros(n, dtype=np.int64)
        c[int(rnd.integers(0, n))] = int(rnd.integers(1, 3_000_000))
        return c
    c = rnd.integers(0, 50, size=n)  # every tile of one slice is long
    c[int(rnd.integers(0, 16))::16] = rnd.integers(1000, 100_000)
    return c


def _order(rnd, n, kind):
    if kind == 0:
        return np.arange(n)
    if kind == 1:
        return np.arange(n)[::-1]
    if kind == 2:
        return rnd.permutation(n)
    return np.concatenate([np.arange(s, n, 16) for s in rnd.permutation(16)])[:n]  # slice after slice


def test_layout():
    S, M = lib().shim_list_slices(), lib().shim_list_min_jobs()
    assert S == 16 and M == 128
    for n in (0, 1, 64, 65, M - 1):
        assert layout(n, 12345) == (1, 12345, 12345)  # small batches: one cursor, the arena as it was
    for cap in (1, 15, 16, 17, 12345, 2_000_000_000):
        n_slices, slice_cap, total = layout(M, cap)
        assert n_slices == S and slice_cap == -(-cap // S) and total == S * slice_cap + cap
    # a partitioned arena that the headers' 32-bit positions could not address falls back to one cursor: what fitted still fits
    for cap in (2_200_000_000, 0xFFFFFFFE):
        assert layout(1024, cap) == (1, cap, cap)
    assert layout(1024, 2_100_000_000)[0] == S


def test_nothing_that_fits_one_cursor_is_refused():
    rnd = np.random.default_rng(31)
    tile_counts = [1, 2, 17, 64, 65, 127, 128, 129, 300, 1024, 4097, 10_000]
    trials = 0
    for n in tile_counts:
        for kind in range(5):
            for okind in range(4):
                counts = np.asarray(_counts(rnd, n, kind), dtype=np.uint32)
                entries = int(counts.astype(np.int64).sum())
                for slack in (0, 1, int(rnd.integers(0, 1000))):  # ent_cap is the batch's entries or a little more
                    ent_cap = entries + slack
                    if ent_cap == 0:
                        continue
                    refused, base, where = play(counts, _order(rnd, n, okind), ent_cap)
                    assert refused == 0, (n, kind, okind, slack)
                    check_placed(counts, base, where, layout(n, ent_cap)[2])
                    assert (where[counts == 0] == 3).all() and (where[counts > 0] < 2).all()
                    trials += 1
    assert trials > 500


def test_the_overflow_slice_is_used_and_an_arena_too_small_refuses():
    rnd = np.random.default_rng(32)
    counts = np.asarray(_counts(rnd, 300, 0), dtype=np.uint32)
    counts[5] = 50_000  # far more than a slice holds
    counts[37] = 100
    entries = int(counts.astype(np.int64).sum())
    refused, base, where = play(counts, np.arange(300), entries)
    n_slices, slice_cap, total = layout(300, entries)
    assert refused == 0 and where[5] == 1 and where[37] == 1 and where[21] == 1  # tile 5 ran its slice's cursor past the end
    assert base[5] >= n_slices * slice_cap
    check_placed(counts, base, where, total)
    for n in (300, 64):  # sixteen cursors, one cursor
        c = counts[:n]
        cap = int(c.astype(np.int64).sum()) // 3
        refused, base, where = play(c, rnd.permutation(n), cap)
        assert refused > 0 and (where == 2).sum() == refused
        check_placed(c, base, where, layout(n, cap)[2])
