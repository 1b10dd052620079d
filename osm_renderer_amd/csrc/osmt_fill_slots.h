/*
 * osmt_fill_slots.h — the slot descriptors that deal fill rows to the waves of k_prebin.
 *
 * A SLOT is one sub-tile row (16 pixel rows) of one FILL op's clipped window; a PASS of k_prebin's fill role is four
 * consecutive slots = the 64 rows of one wave, whichever ops they belong to.  k_opinfo, which knows every fill op's
 * window, writes one 16-byte descriptor per slot:
 *
 *   a workgroup of k_opinfo (OSMT_FILL_SLOT_WG_OPS ops) scans the slot counts (nsr) of its ops, rounds its total up to
 *   a whole number of passes and reserves that many slots with ONE atomicAdd on the slot cursor.  Op i stores its nsr
 *   descriptors at [base + before(i), base + before(i) + nsr_i), the workgroup stores the <= 3 slots of the rounding
 *   as EMPTY ones.  A reservation therefore always starts and ends on a pass boundary: no pass straddles two
 *   workgroups, and the cursor's final value is four times the pass count whatever order the workgroups arrive in.
 *
 * An op whose arena reservation is refused (guessed arenas, see scene_size_arenas) still owns its slots and stores
 * them empty.  Capacity: an op has at least one coverage group per slot and at most sub_rows slots, so a scene of
 * G fill groups and F fill ops has at most min(G, F * sub_rows) real slots, plus three of rounding per workgroup.
 * (With GUESSED arenas G is the guess: a descriptor past the capacity is not stored and the passes past it are not
 * run — the fill arena has then overflowed as well and the scene is rendered again with exact sizes.)
 *
 * Shared with a host test (tests/fill_slots_shim.cpp).
 */
#ifndef OSMT_FILL_SLOTS_H
#define OSMT_FILL_SLOTS_H

#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

#define OSMT_FILL_PASS_SLOTS 4u /* slots of a pass: 64 lanes / 16 rows */
/* ops of one k_opinfo workgroup: ops per wave x waves (the kernel's own constants come from these two) */
#ifndef OSMT_V_OPINFO_THREADS
#define OSMT_V_OPINFO_THREADS 64
#endif
#ifndef OSMT_V_OPINFO_WAVES
#define OSMT_V_OPINFO_WAVES 8
#endif
#define OSMT_FILL_SLOT_WG_OPS ((uint32_t)(OSMT_V_OPINFO_THREADS * OSMT_V_OPINFO_WAVES))

/* One slot.  geom == 0 (ncols == 0): an empty slot, nothing is read through it. */
struct alignas(16) osmt_fill_slot {
    uint32_t op;       /* op index; 0xFFFFFFFF for an empty slot */
    uint32_t word0;    /* 32-bit word index of the row's first coverage group: (arena_off + r * ncols) * 16 */
    uint32_t geom;     /* sr | c0 << 8 | ncols << 16 | n_edges << 24 (SIMPLE ops only, <= 16) | OSMT_FILL_SLOT_SIMPLE */
    uint32_t first_pt; /* first point of the op's first ring */
};
#define OSMT_FILL_SLOT_SIMPLE 0x80000000u /* one ring of at most 16 edges: everything step 1 needs is in the descriptor */
#define OSMT_FILL_SLOT_MAX_SIMPLE_EDGES 16u

OSMT_HD osmt_fill_slot osmt_fill_slot_empty(void) {
    osmt_fill_slot s;
    s.op = 0xFFFFFFFFu;
    s.word0 = 0u;
    s.geom = 0u;
    s.first_pt = 0u;
    return s;
}

/* sr, c0 < 256 and 1 <= ncols <= 128 (scale <= 4: 256 sub-tile rows, 128 columns) */
OSMT_HD osmt_fill_slot osmt_fill_slot_make(uint32_t op, uint32_t arena_off, uint32_t r, uint32_t sr0, uint32_t c0, uint32_t ncols,
                                           uint32_t n_rings, uint32_t n_edges, uint32_t first_pt) {
    osmt_fill_slot s;
    s.op = op;
    s.word0 = (arena_off + r * ncols) * 16u;
    s.geom = (sr0 + r) | (c0 << 8) | (ncols << 16);
    if (n_rings == 1u && n_edges <= OSMT_FILL_SLOT_MAX_SIMPLE_EDGES) s.geom |= (n_edges << 24) | OSMT_FILL_SLOT_SIMPLE;
    s.first_pt = first_pt;
    return s;
}
OSMT_HD uint32_t osmt_fill_slot_sr(uint32_t geom) { return geom & 255u; }
OSMT_HD uint32_t osmt_fill_slot_c0(uint32_t geom) { return (geom >> 8) & 255u; }
OSMT_HD uint32_t osmt_fill_slot_ncols(uint32_t geom) { return (geom >> 16) & 255u; }
OSMT_HD uint32_t osmt_fill_slot_simple(uint32_t geom) { return geom >> 31; }
OSMT_HD uint32_t osmt_fill_slot_edges(uint32_t geom) { return (geom >> 24) & 31u; } /* simple slots only */

/* slots a workgroup reserves for `total` real ones: whole passes */
OSMT_HD uint32_t osmt_fill_slots_round(uint32_t total) { return (total + OSMT_FILL_PASS_SLOTS - 1u) & ~(OSMT_FILL_PASS_SLOTS - 1u); }

/* first slot of an op inside its workgroup's reservation: the slots of the workgroup's ops in front of it
 * (`incl_in_wave`: inclusive scan of nsr over the op's wave, `before_wave`: total of the waves in front) */
OSMT_HD uint32_t osmt_fill_slot_first(uint32_t before_wave, uint32_t incl_in_wave, uint32_t nsr) { return before_wave + (incl_in_wave - nsr); }

/* workgroups of k_opinfo over n_ops ops */
OSMT_HD uint32_t osmt_fill_slot_wgs(uint32_t n_ops) { return n_ops / OSMT_FILL_SLOT_WG_OPS + (n_ops % OSMT_FILL_SLOT_WG_OPS ? 1u : 0u); }

/* Descriptors the array must hold (a multiple of four), for a scene whose fill arena holds `groups` groups (exact,
 * guessed or worst case) and that has n_fills fill ops among n_ops ops. */
OSMT_HD uint64_t osmt_fill_slot_capacity(uint64_t groups, uint64_t n_fills, uint32_t sub_rows, uint32_t n_ops) {
    const uint64_t by_ops = n_fills * sub_rows;
    const uint64_t real = groups < by_ops ? groups : by_ops;
    const uint64_t cap = real + (uint64_t)(OSMT_FILL_PASS_SLOTS - 1u) * osmt_fill_slot_wgs(n_ops);
    return (cap + OSMT_FILL_PASS_SLOTS - 1u) & ~(uint64_t)(OSMT_FILL_PASS_SLOTS - 1u);
}

/* passes k_prebin runs: the cursor's whole passes that lie inside the array */
OSMT_HD uint32_t osmt_fill_pass_count(uint64_t cursor, uint64_t capacity) {
    const uint64_t n = cursor < capacity ? cursor : capacity;
    return (uint32_t)(n / OSMT_FILL_PASS_SLOTS);
}

#endif
