"""The fill slots of k_prebin (osm_renderer_amd/csrc/osmt_fill_slots.h), host build.  k_opinfo's placement of the slot
descriptors is played with the header's own functions over random vectors of slot counts per op (nsr), workgroups
reserving in random order: every slot below the cursor is stored exactly once, an op's slots are consecutive and in op
order inside its workgroup, a workgroup's reservation is a whole number of passes with at most three empty slots, no
pass holds ops of two workgroups, and the capacity bound the host allocates by is never exceeded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libfillslotsshim.so")
_lib = None
PAD = 0xFFFFFFFE


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "fill_slots_shim.cpp")
        hdr = os.path.join(_HERE, "..", "osm_renderer_amd", "csrc", "osmt_fill_slots.h")
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _SO, src])
        L = C.CDLL(_SO)
        u32, u64, p32 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)
        L.shim_fill_wg_ops.restype = u32
        L.shim_fill_pass_slots.restype = u32
        L.shim_fill_slots_round.argtypes = [u32]
        L.shim_fill_slots_round.restype = u32
        L.shim_fill_slot_wgs.argtypes = [u32]
        L.shim_fill_slot_wgs.restype = u32
        L.shim_fill_slot_capacity.argtypes = [u64, u64, u32, u32]
        L.shim_fill_slot_capacity.restype = u64
        L.shim_fill_pass_count.argtypes = [u64, u64]
        L.shim_fill_pass_count.restype = u32
        L.shim_fill_slot_pack.argtypes = [u32] * 9 + [p32]
        L.shim_fill_slot_pack.restype = None
        L.shim_fill_slots_play.argtypes = [u32, p32, p32, u32, p32, p32, u64]
        L.shim_fill_slots_play.restype = u64
        _lib = L
    return _lib


def play(nsr, order=None, cap=None, ncols=None, sub_rows=64):
    """-> cursor, dropped, owner, hits, capacity.  ncols (per op, >= 1 where nsr > 0) gives the scene's fill groups."""
    L = lib()
    nsr = np.ascontiguousarray(nsr, dtype=np.uint32)
    n_ops = len(nsr)
    n_wg = int(L.shim_fill_slot_wgs(n_ops))
    if order is None:
        order = np.arange(n_wg)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    if ncols is None:
        ncols = np.ones(n_ops, dtype=np.uint64)
    groups = int((nsr.astype(np.uint64) * np.asarray(ncols, dtype=np.uint64)).sum())
    n_fills = int(np.count_nonzero(nsr))
    capacity = int(L.shim_fill_slot_capacity(groups, n_fills, sub_rows, n_ops))
    if cap is None:
        cap = capacity
    owner = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    hits = np.zeros(max(cap, 1), dtype=np.uint32)
    p32 = C.POINTER(C.c_uint32)
    r = int(L.shim_fill_slots_play(n_ops, nsr.ctypes.data_as(p32), order.ctypes.data_as(p32), n_wg, owner.ctypes.data_as(p32),
                                   hits.ctypes.data_as(p32), cap))
    return r & 0xFFFFFFFF, r >> 32, owner, hits, capacity


def check(nsr, order=None, ncols=None, sub_rows=64):
    L = lib()
    wg_ops, ps = int(L.shim_fill_wg_ops()), int(L.shim_fill_pass_slots())
    nsr = np.asarray(nsr, dtype=np.int64)
    cursor, dropped, owner, hits, capacity = play(nsr, order, None, ncols, sub_rows)
    n_wg = -(-len(nsr) // wg_ops) if len(nsr) else 0
    wg_tot = [int(nsr[w * wg_ops:(w + 1) * wg_ops].sum()) for w in range(n_wg)]
    # the rounding: whole passes, at most three empty slots per workgroup, nothing for a workgroup without slots
    assert cursor == sum(-(-t // ps) * ps for t in wg_tot)
    assert cursor % ps == 0 and cursor - int(nsr.sum()) <= (ps - 1) * sum(1 for t in wg_tot if t)
    # the capacity bound holds, nothing is dropped, and the pass count is the cursor's
    assert dropped == 0 and cursor <= capacity and capacity % ps == 0
    assert int(L.shim_fill_pass_count(cursor, capacity)) == cursor // ps
    # every slot below the cursor stored exactly once, none above it
    assert (hits[:cursor] == 1).all() and (hits[cursor:] == 0).all()
    own = owner[:cursor].astype(np.int64)
    real = own[own != PAD]
    # every op owns exactly its nsr slots, consecutive, in row order = store order; ops of a workgroup in op order
    assert np.array_equal(np.bincount(real, minlength=len(nsr))[:len(nsr)], nsr)
    for p in range(0, cursor, ps):  # no pass holds ops of two workgroups
        ops = own[p:p + ps]
        ops = ops[ops != PAD]
        assert len(set((ops // wg_ops).tolist())) <= 1
    i = 0
    while i < cursor:  # a workgroup's reservation: its ops ascending, each one's slots together, then the padding
        if own[i] == PAD:
            i += 1
            continue
        w = own[i] // wg_ops
        n = -(-wg_tot[w] // ps) * ps
        assert i % ps == 0
        seg = own[i:i + n]
        body = seg[:wg_tot[w]]
        assert (seg[wg_tot[w]:] == PAD).all() and (body != PAD).all()
        assert (np.diff(body) >= 0).all() and (body // wg_ops == w).all()
        i += n
    return cursor, capacity


def test_constants_and_rounding():
    L = lib()
    assert L.shim_fill_pass_slots() == 4 and L.shim_fill_wg_ops() == 512
    for t, want in [(0, 0), (1, 4), (3, 4), (4, 4), (5, 8), (2**31, 2**31), (2**31 - 3, 2**31)]:
        assert L.shim_fill_slots_round(t) == want
    for n, want in [(0, 0), (1, 1), (512, 1), (513, 2), (1024, 2), (2**32 - 1, 2**23)]:
        assert L.shim_fill_slot_wgs(n) == want
    assert L.shim_fill_pass_count(40, 400) == 10 and L.shim_fill_pass_count(400, 40) == 10 and L.shim_fill_pass_count(0, 40) == 0


def test_named_vectors():
    assert check(np.zeros(0, dtype=np.int64))[0] == 0
    assert check(np.zeros(1500, dtype=np.int64))[0] == 0  # all-zero: no slots, no padding
    assert check([64])[0] == 64  # a single op of 64 rows
    assert check([1])[0] == 4  # one slot and three empty ones
    assert check(np.ones(512, dtype=np.int64))[0] == 512  # 512 ops of one row: exactly one workgroup, no padding
    assert check(np.ones(513, dtype=np.int64))[0] == 516
    assert check(np.ones(600, dtype=np.int64), order=[1, 0])[0] == 512 + 88
    assert check(np.full(1024, 256, dtype=np.int64), sub_rows=256, ncols=np.full(1024, 128))[0] == 1024 * 256  # scale 4, whole tiles


def test_random_vectors_and_orders():
    rnd = np.random.default_rng(20260)
    for it in range(300):
        n_ops = int(rnd.choice([1, 2, 63, 64, 65, 511, 512, 513, 1023, 1025, int(rnd.integers(1, 6000))]))
        kind = it % 5
        if kind == 0:
            nsr = rnd.integers(0, 5, size=n_ops)
        elif kind == 1:  # mostly strokes
            nsr = np.where(rnd.random(n_ops) < 0.1, rnd.integers(1, 17, size=n_ops), 0)
        elif kind == 2:  # tall polygons
            nsr = rnd.integers(0, 65, size=n_ops)
        elif kind == 3:  # one op per workgroup
            nsr = np.zeros(n_ops, dtype=np.int64)
            nsr[::512] = rnd.integers(1, 65, size=len(nsr[::512]))
        else:
            nsr = rnd.integers(1, 3, size=n_ops)
        ncols = rnd.integers(1, 9, size=n_ops)
        n_wg = -(-n_ops // 512)
        check(nsr, order=rnd.permutation(n_wg), ncols=ncols)


def test_capacity_is_reached_and_a_short_array_drops_only_what_lies_past_it():
    # every workgroup holds one one-row polygon of one column: groups + 3 per workgroup, to the slot
    nsr = np.zeros(512 * 7, dtype=np.int64)
    nsr[::512] = 1
    cursor, capacity = check(nsr)
    assert cursor == capacity == 28
    # an array that is too short (guessed arenas): slots below it are still stored exactly once, the rest is dropped
    nsr = np.random.default_rng(5).integers(0, 9, size=2000)
    full, _, owner_full, _, _ = play(nsr)
    cap = (full // 2) & ~3
    cursor, dropped, owner, hits, _ = play(nsr, cap=cap)
    assert cursor == full and dropped == full - cap
    assert (hits == 1).all() and np.array_equal(owner, owner_full[:cap])
    assert lib().shim_fill_pass_count(cursor, cap) == cap // 4


def test_descriptor_round_trip():
    L = lib()
    out = (C.c_uint32 * 8)()
    rnd = np.random.default_rng(7)
    for _ in range(2000):
        op, arena, first_pt = (int(v) for v in rnd.integers(0, 2**24, size=3))
        sr0, r = int(rnd.integers(0, 200)), int(rnd.integers(0, 56))
        c0 = int(rnd.integers(0, 128))
        ncols = int(rnd.integers(1, 129 - c0))
        n_rings, n_edges = int(rnd.integers(1, 4)), int(rnd.integers(0, 40))
        L.shim_fill_slot_pack(op, arena, r, sr0, c0, ncols, n_rings, n_edges, first_pt, out)
        simple = n_rings == 1 and n_edges <= 16
        want = [op, (arena + r * ncols) * 16, sr0 + r, c0, ncols, int(simple)]
        assert list(out)[:6] == want and out[7] == first_pt
        if simple:
            assert out[6] == n_edges
    # the largest window of scale 4 and the last group below 2^28
    L.shim_fill_slot_pack(2**32 - 2, 2**28 - 129, 1, 254, 0, 128, 1, 16, 5, out)
    assert list(out) == [2**32 - 2, (2**28 - 1) * 16, 255, 0, 128, 1, 16, 5]
