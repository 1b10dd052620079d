/*
 * osmt_list_slices.h — where k_sublist's workgroups (one per tile) reserve the entries of their tile's lists.
 *
 * One cursor for all tiles is one address for all reservations, and same-address atomics are served one after the
 * other.  A batch of at least OSMT_LIST_SLICE_MIN_JOBS tiles therefore has OSMT_LIST_SLICES cursors, each on a cache
 * line of its own, and tile t reserves with cursor t % OSMT_LIST_SLICES: workgroups that run at the same time have
 * neighbouring indices and so different cursors.  Cursor c hands out places in its own slice of the entry arena,
 * [c * slice_cap, (c + 1) * slice_cap).  A reservation that does not fit its slice is made again with the overflow
 * cursor, whose slice lies behind the others and holds ent_cap entries.
 *
 * Sizing.  ent_cap keeps its meaning: the number of entries that the binning can produce for this scene.  The slices
 * together hold ent_cap (rounded up to a multiple of their number) and the overflow slice holds ent_cap again, so the
 * arena has  n_slices * slice_cap + ent_cap  entries.  Whatever the order in which the tiles reserve, a batch whose
 * lists have at most ent_cap entries in all is never refused: the tiles that end up in the overflow slice are a subset
 * of all tiles, and their entries together are at most ent_cap.  (A slice's cursor that has run past its end stays
 * there, so the later tiles of that slice overflow too; the bound holds all the same.)  Smaller batches, and arenas
 * whose partitioned size would not fit the 32-bit positions of the list headers, keep ONE cursor and an arena of
 * ent_cap entries — exactly what every batch had before.
 *
 * Shared with a host test (tests/list_slices_shim.cpp) that plays random batches through these functions.
 */
#ifndef OSMT_LIST_SLICES_H
#define OSMT_LIST_SLICES_H

#include <stddef.h>
#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

#ifndef OSMT_V_LIST_SLICES
#define OSMT_V_LIST_SLICES 16
#endif
#define OSMT_LIST_SLICES ((uint32_t)OSMT_V_LIST_SLICES)
#define OSMT_LIST_SLICE_MIN_JOBS 128u  /* fewer tiles than this: one cursor, as before */
#define OSMT_LIST_CURSOR_STRIDE 16u    /* 64-bit words between two cursors: 128 bytes, a cache line each */
/* 32-bit words of the cursor block behind the list counts: the slices' cursors and the overflow cursor */
#define OSMT_LIST_CURSOR_WORDS ((OSMT_LIST_SLICES + 1u) * OSMT_LIST_CURSOR_STRIDE * 2u)

struct osmt_list_layout {
    uint32_t n_slices;            /* 1: the single cursor, no overflow slice */
    unsigned long long slice_cap; /* entries per slice */
    unsigned long long total;     /* entries of the whole arena */
};

OSMT_HD osmt_list_layout osmt_list_layout_make(uint32_t n_jobs, unsigned long long ent_cap) {
    osmt_list_layout l;
    l.n_slices = 1u;
    l.slice_cap = ent_cap;
    l.total = ent_cap;
    if (n_jobs >= OSMT_LIST_SLICE_MIN_JOBS && OSMT_LIST_SLICES > 1u) {
        const unsigned long long cap = (ent_cap + OSMT_LIST_SLICES - 1u) / OSMT_LIST_SLICES;
        const unsigned long long total = cap * OSMT_LIST_SLICES + ent_cap;
        if (total < 0xFFFFFFFFull) { /* list headers hold 32-bit positions */
            l.n_slices = OSMT_LIST_SLICES;
            l.slice_cap = cap;
            l.total = total;
        }
    }
    return l;
}

/* first 32-bit word of the slices' cursors, counted from the pre-pass cursors: behind the 8 words of those and the
 * n_cnt list counts, on a 128-byte boundary of that word count */
OSMT_HD size_t osmt_list_cursor_word0(size_t n_cnt) { return 8u + ((n_cnt + 31u) & ~(size_t)31u); }

OSMT_HD uint32_t osmt_list_slice_of(const osmt_list_layout l, uint32_t tile) { return l.n_slices > 1u ? tile % l.n_slices : 0u; }

/* A tile of `n` entries whose atomicAdd on its slice's cursor returned `first`: 1 and the arena position if it fits the slice */
OSMT_HD uint32_t osmt_list_place(const osmt_list_layout l, uint32_t slice, unsigned long long first, unsigned long long n,
                                 unsigned long long* base) {
    if (first + n > l.slice_cap) return 0u;
    *base = (unsigned long long)slice * l.slice_cap + first;
    return 1u;
}

/* The same tile after an atomicAdd on the overflow cursor returned `first` (n_slices > 1 only) */
OSMT_HD uint32_t osmt_list_place_overflow(const osmt_list_layout l, unsigned long long ent_cap, unsigned long long first, unsigned long long n,
                                          unsigned long long* base) {
    if (first + n > ent_cap) return 0u;
    *base = (unsigned long long)l.n_slices * l.slice_cap + first;
    return 1u;
}

#endif
