/*
 * osmt_prebin_roles.h — which block of k_prebin does what.
 *
 * The launch has n_vblk stroke blocks (OSMT_BIN_SEGS virtual segments each, latency-bound) and n_fblk fill blocks
 * (passes of four fill slots, issue-bound).  The dispatcher places workgroups in index order, so stroke blocks that own the lowest indices all start
 * first and the two halves run one after the other.  Here the stroke blocks are spread evenly through the grid instead:
 * with T = n_vblk + n_fblk and S(b) = floor(b * n_vblk / T) stroke blocks among the indices [0, b), block b is stroke
 * block S(b) when S(b + 1) > S(b) and fill block b - S(b) otherwise.  S(0) = 0, S(T) = n_vblk and S grows by at most
 * one per index, so every block of either role is mapped exactly once, and any run [a, b) of indices holds
 * S(b) - S(a) stroke blocks, less than one away from its share (b - a) * n_vblk / T.
 *
 * The kernel divides by multiplying: floor(x / T) is the high word of x * magic or one more (magic = floor((2^64-1) / T);
 * the estimate is short by x * e / (T * 2^64) < 1 with e <= T), and the remainder says which.  Shared with a host test
 * (tests/prebin_shim.cpp) that checks the three properties exhaustively.
 */
#ifndef OSMT_PREBIN_ROLES_H
#define OSMT_PREBIN_ROLES_H

#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

/* virtual segments per stroke block: 64, 32 or 16 (measured: DESIGN.md 3.3) */
#ifndef OSMT_V_BIN_SEGS
#define OSMT_V_BIN_SEGS 32
#endif
#if OSMT_V_BIN_SEGS != 64 && OSMT_V_BIN_SEGS != 32 && OSMT_V_BIN_SEGS != 16
#error "OSMT_V_BIN_SEGS is 64, 32 or 16"
#endif
#define OSMT_BIN_SEGS ((uint32_t)OSMT_V_BIN_SEGS)

/* 1: stroke blocks spread through the grid; 0: stroke blocks first (the layout before) */
#ifndef OSMT_V_PREBIN_INTERLEAVE
#define OSMT_V_PREBIN_INTERLEAVE 1
#endif

struct osmt_prebin_map {
    uint32_t n_vblk, n_fblk; /* n_vblk + n_fblk <= 2^31 - 1 (a grid's x dimension) */
    uint64_t magic;          /* floor((2^64 - 1) / (n_vblk + n_fblk)); unused when there are no blocks */
};

OSMT_HD uint32_t osmt_prebin_n_vblk(uint32_t n_vsegs, uint32_t bin_segs) {
    return n_vsegs / bin_segs + (n_vsegs % bin_segs ? 1u : 0u);
}

OSMT_HD osmt_prebin_map osmt_prebin_map_make(uint32_t n_vblk, uint32_t n_fblk) {
    osmt_prebin_map m;
    m.n_vblk = n_vblk;
    m.n_fblk = n_fblk;
    const uint64_t T = (uint64_t)n_vblk + n_fblk;
    m.magic = T ? ~(uint64_t)0 / T : 0u; /* host only: the kernel gets the struct as an argument */
    return m;
}

OSMT_HD uint64_t osmt_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

/* Role of block b < n_vblk + n_fblk: returns 1 and the stroke block's index, or 0 and the fill block's index. */
OSMT_HD uint32_t osmt_prebin_role(const osmt_prebin_map m, uint32_t b, uint32_t* idx) {
#if OSMT_V_PREBIN_INTERLEAVE
    const uint64_t T = (uint64_t)m.n_vblk + m.n_fblk;
    const uint64_t x = (uint64_t)b * m.n_vblk; /* < 2^62 */
    uint64_t s = osmt_mulhi64(x, m.magic);     /* floor(x / T) or one less */
    uint64_t r = x - s * T;
    if (r >= T) {
        r -= T;
        ++s;
    }
    if (r + m.n_vblk >= T) { /* S(b + 1) > S(b) */
        *idx = (uint32_t)s;
        return 1u;
    }
    *idx = b - (uint32_t)s;
    return 0u;
#else
    if (b < m.n_vblk) {
        *idx = b;
        return 1u;
    }
    *idx = b - m.n_vblk;
    return 0u;
#endif
}

#endif
