/*
 * osmt_tilepyramid.hip — the levels of a tile index pyramid (osmt_register_tile_pyramid), built on the device from a
 * registered z18 tile index or from the next finer level.  Level L holds, per tile (x >> s, y >> s) with s = 18 - L, the
 * union of the reference lists of its z18 children, ascending and without repeats; the tile query (osmt_tilequery.hip) reads
 * the smallest registered level >= the zoom of a tile instead of 9 * 4^(18 - zoom) z18 tiles.  The host twin, and the
 * yardstick of the tests, is osmt::tile_pyramid_level (host/osmt_tilequery.hpp).  gfx950 only.
 *
 * One level is four jobs of the same shape, the tiles and one per kind (ways, multipolygons, nodes):
 *
 *   k_pyr_pairs     one lane per reference of the source: its source tile by bisection over the offsets, the tile's x by
 *                   bisection over the column directory, and the pair (parent key, id) with key = (x >> s) << 18 | (y >> s).
 *   k_pyr_tilekeys  one lane per source tile: (parent key, 0) — a tile with empty lists still gives its parent a tile.
 *   k_pyr_digits    the histograms of all nine 8-bit digits of the pairs (four of the id, five of the 36-bit key) in one
 *                   read: the host skips every digit whose histogram has one non-empty bin (the ids' high bytes, the key's
 *                   high bits), so a sort runs as many passes as its pairs have digits that differ.
 *   k_pyr_keydigits the same for a caller whose key is any 64 bits and whose ids need no passes (osmt_resolve.hip): the
 *                   histograms of the key's eight bytes.  A pass takes any of the twelve digits; the callers above never ask
 *                   for the last three, so their passes and results are what they were.
 *   k_pyr_hist      one pass of the LSD radix sort, per workgroup of OSMT_PYR_SORT_BLOCK pairs: an LDS histogram of the
 *                   digit, stored as counts[digit][workgroup]; the tile query's scan turns the counts into bases.
 *   k_pyr_scatter   the same workgroups again: four rounds of 256 pairs; in a round a lane finds the lanes of its wave with
 *                   its digit by eight wave64 ballots, its rank among them by a population count, the waves in front by
 *                   per-wave counts in LDS — ranks follow the pairs' order, so every pass is stable.
 *   k_pyr_mark      one lane per sorted pair: 1 for the first of its pair (and, for the tiles, 1 for the first of its x);
 *                   scans number the distinct pairs and the columns.
 *   k_pyr_emit_tiles / k_pyr_emit_lists
 *                   the level's arrays: tile_x, tile_y and the column directory; per kind the pool and, one lane per tile,
 *                   the offsets by bisection of the tile's key over the sorted pairs.
 *
 * A (key, id) pair takes 36 + 32 bits and does not fit one word: keys and ids travel as two arrays and a pass takes its digit
 * from either.  Every store lands below a count the arrays were sized with (the source's reference total, read back by the
 * host before anything is launched; the distinct totals, read back before the level is allocated); every word is written
 * before it is read.  No kernel here uses scratch (profiles/tile_pyramid_kernel_resources.txt).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t ROUNDS = OSMT_PYR_SORT_BLOCK / WG;
constexpr uint32_t BINS = 256u;
constexpr uint32_t KEY_Y_BITS = OSMT_MAX_ZOOM; /* key = x << 18 | y */
static_assert(OSMT_PYR_SORT_BLOCK % WG == 0u, "a workgroup takes whole rounds");
static_assert(BINS == WG, "one lane per bin");

typedef unsigned long long u64;

/* d < OSMT_PYR_PASS_DIGITS: 0..3 the bytes of the id, 4..11 the bytes of the key */
__device__ __forceinline__ uint32_t digit_of(u64 key, uint32_t id, uint32_t d) {
    return d < 4u ? (id >> (8u * d)) & 255u : (uint32_t)(key >> (8u * (d - 4u))) & 255u;
}

/* the source tile of reference r: the smallest i with off[i + 1] > r (tiles without references own none); r < off[n] */
__device__ __forceinline__ uint32_t tile_of_ref(const uint32_t* __restrict__ off, uint32_t n, uint32_t r) {
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid + 1u] > r)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

/* the parent key of source tile i: its column is the last one that starts at or before i (col_first[0] = 0) */
__device__ __forceinline__ u64 parent_key(const osmt_pyr_src& S, uint32_t i) {
    uint32_t lo = 0u, hi = S.n_cols - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (S.col_first[mid] <= i)
            lo = mid;
        else
            hi = mid - 1u;
    }
    return ((u64)(S.col_x[lo] >> S.shift) << KEY_Y_BITS) | (u64)(S.tile_y[i] >> S.shift);
}

__global__ __launch_bounds__(256) void k_pyr_pairs(osmt_pyr_src S, u64* __restrict__ key, uint32_t* __restrict__ id) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= S.n_refs) return;
    key[r] = parent_key(S, tile_of_ref(S.off, S.n_tiles, r));
    id[r] = S.pool[r];
}

__global__ __launch_bounds__(256) void k_pyr_tilekeys(osmt_pyr_src S, u64* __restrict__ key, uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= S.n_tiles) return;
    key[i] = parent_key(S, i);
    id[i] = 0u;
}

/* ---- the sort ---------------------------------------------------------------------------------------------------- */
/* hist: [OSMT_PYR_DIGITS][256], zeroed before the launch */
__global__ __launch_bounds__(256) void k_pyr_digits(const u64* __restrict__ key, const uint32_t* __restrict__ id, uint32_t n, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[OSMT_PYR_DIGITS * BINS];
    for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) h[d * BINS + threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t j = 0; j < ROUNDS; ++j) {
        const uint32_t e = blockIdx.x * OSMT_PYR_SORT_BLOCK + j * WG + threadIdx.x;
        if (e >= n) break;
        const u64 k = key[e];
        const uint32_t v = id[e];
        for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) atomicAdd(&h[d * BINS + digit_of(k, v, d)], 1u);
    }
    __syncthreads();
    for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) {
        const uint32_t c = h[d * BINS + threadIdx.x];
        if (c) atomicAdd(&hist[d * BINS + threadIdx.x], c);
    }
}

/* hist: [OSMT_PYR_KEY_DIGITS][256], zeroed before the launch: the eight bytes of the key, nothing of the id */
__global__ __launch_bounds__(256) void k_pyr_keydigits(const u64* __restrict__ key, uint32_t n, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[OSMT_PYR_KEY_DIGITS * BINS];
    for (uint32_t d = 0; d < OSMT_PYR_KEY_DIGITS; ++d) h[d * BINS + threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t j = 0; j < ROUNDS; ++j) {
        const uint32_t e = blockIdx.x * OSMT_PYR_SORT_BLOCK + j * WG + threadIdx.x;
        if (e >= n) break;
        const u64 k = key[e];
        for (uint32_t d = 0; d < OSMT_PYR_KEY_DIGITS; ++d) atomicAdd(&h[d * BINS + digit_of(k, 0u, 4u + d)], 1u);
    }
    __syncthreads();
    for (uint32_t d = 0; d < OSMT_PYR_KEY_DIGITS; ++d) {
        const uint32_t c = h[d * BINS + threadIdx.x];
        if (c) atomicAdd(&hist[d * BINS + threadIdx.x], c);
    }
}

/* counts: [256][n_wg], n_wg = the grid; every word is written */
__global__ __launch_bounds__(256) void k_pyr_hist(const u64* __restrict__ key, const uint32_t* __restrict__ id, uint32_t n, uint32_t d,
                                                  uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t j = 0; j < ROUNDS; ++j) {
        const uint32_t e = blockIdx.x * OSMT_PYR_SORT_BLOCK + j * WG + threadIdx.x;
        if (e >= n) break;
        atomicAdd(&h[digit_of(key[e], id[e], d)], 1u);
    }
    __syncthreads();
    counts[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

/* counts: the exclusive scan of k_pyr_hist's, so counts[digit][workgroup] is where the workgroup's first pair of the digit goes */
__global__ __launch_bounds__(256) void k_pyr_scatter(const u64* __restrict__ key, const uint32_t* __restrict__ id, uint32_t n, uint32_t d,
                                                     const uint32_t* __restrict__ counts, u64* __restrict__ out_key, uint32_t* __restrict__ out_id) {
    __shared__ uint32_t base[BINS];           /* where the next pair of the bin goes */
    __shared__ uint32_t wcnt[WG / 64u][BINS]; /* pairs of the bin in each wave, this round */
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    base[threadIdx.x] = counts[threadIdx.x * gridDim.x + blockIdx.x];
    for (uint32_t j = 0; j < ROUNDS; ++j) {
        for (uint32_t x = 0; x < WG / 64u; ++x) wcnt[x][threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t e = blockIdx.x * OSMT_PYR_SORT_BLOCK + j * WG + threadIdx.x;
        const bool valid = e < n;
        const u64 k = valid ? key[e] : 0ull;
        const uint32_t v = valid ? id[e] : 0u;
        const uint32_t dg = digit_of(k, v, d);
        u64 peers = __ballot(valid); /* the valid lanes of the wave with this lane's digit */
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = (dg >> b) & 1u;
            const u64 m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wcnt[w][dg] = __popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t dst = base[dg] + rank;
            for (uint32_t x = 0; x < w; ++x) dst += wcnt[x][dg];
            out_key[dst] = k;
            out_id[dst] = v;
        }
        __syncthreads();
        uint32_t t = 0u;
        for (uint32_t x = 0; x < WG / 64u; ++x) t += wcnt[x][threadIdx.x];
        base[threadIdx.x] += t; /* the lane that owns the bin: it alone zeroes the bin's counts in the next round */
    }
}

/* ---- mark, emit -------------------------------------------------------------------------------------------------- */
/* pos[i] = 1 for the first of its pair; cpos (the tiles' job, else NULL): 1 for the first of its x */
__global__ __launch_bounds__(256) void k_pyr_mark(const u64* __restrict__ key, const uint32_t* __restrict__ id, uint32_t n, uint32_t* __restrict__ pos,
                                                  uint32_t* __restrict__ cpos) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i], p = i ? key[i - 1u] : 0ull;
    pos[i] = (i == 0u || k != p || id[i] != id[i - 1u]) ? 1u : 0u;
    if (cpos) cpos[i] = (i == 0u || (k >> KEY_Y_BITS) != (p >> KEY_Y_BITS)) ? 1u : 0u;
}

/* pos, cpos: scanned, [n + 1]; the level has pos[n] = n_tiles tiles in cpos[n] = n_cols columns */
__global__ __launch_bounds__(256) void k_pyr_emit_tiles(const u64* __restrict__ key, uint32_t n, const uint32_t* __restrict__ pos,
                                                        const uint32_t* __restrict__ cpos, uint32_t n_tiles, uint32_t n_cols, uint32_t* __restrict__ tile_x,
                                                        uint32_t* __restrict__ tile_y, uint32_t* __restrict__ col_x, uint32_t* __restrict__ col_first) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i == 0u) col_first[n_cols] = n_tiles;
    if (i >= n) return;
    const uint32_t t = pos[i];
    if (pos[i + 1u] == t) return; /* a repeat */
    const u64 k = key[i];
    const uint32_t x = (uint32_t)(k >> KEY_Y_BITS);
    tile_x[t] = x;
    tile_y[t] = (uint32_t)k & ((1u << KEY_Y_BITS) - 1u);
    const uint32_t c = cpos[i];
    if (cpos[i + 1u] != c) col_x[c] = x, col_first[c] = t;
}

/* lanes [0, n): the pool; lanes [0, n_tiles]: the offsets.  grid: over max(n, n_tiles + 1) */
__global__ __launch_bounds__(256) void k_pyr_emit_lists(const u64* __restrict__ key, const uint32_t* __restrict__ id, uint32_t n,
                                                        const uint32_t* __restrict__ pos, const uint32_t* __restrict__ tile_x,
                                                        const uint32_t* __restrict__ tile_y, uint32_t n_tiles, uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ pool) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) {
        const uint32_t p = pos[i];
        if (pos[i + 1u] != p) pool[p] = id[i];
    }
    if (i > n_tiles) return;
    uint32_t lo = n;
    if (i < n_tiles) { /* the first sorted pair whose key is not below the tile's */
        const u64 k = ((u64)tile_x[i] << KEY_Y_BITS) | (u64)tile_y[i];
        uint32_t hi = n;
        lo = 0u;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (key[mid] < k)
                lo = mid + 1u;
            else
                hi = mid;
        }
    }
    off[i] = pos[lo];
}

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }
inline uint32_t sort_blocks(uint32_t n) { return (n + OSMT_PYR_SORT_BLOCK - 1u) / OSMT_PYR_SORT_BLOCK; }

}  // namespace

hipError_t osmt_launch_pyr_pairs(const osmt_pyr_src& s, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (s.n_refs) hipLaunchKernelGGL(k_pyr_pairs, grid_of(s.n_refs), dim3(WG), 0, st, s, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_tilekeys(const osmt_pyr_src& s, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (s.n_tiles) hipLaunchKernelGGL(k_pyr_tilekeys, grid_of(s.n_tiles), dim3(WG), 0, st, s, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_digits(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t* hist, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(hist, 0, OSMT_PYR_DIGITS * BINS * 4u, st);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_pyr_digits, dim3(sort_blocks(n)), dim3(WG), 0, st, key, id, n, hist);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_keydigits(const unsigned long long* key, uint32_t n, uint32_t* hist, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(hist, 0, OSMT_PYR_KEY_DIGITS * BINS * 4u, st);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_pyr_keydigits, dim3(sort_blocks(n)), dim3(WG), 0, st, key, n, hist);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_pass(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t digit, uint32_t* counts, unsigned long long* blk,
                                unsigned long long* tot, unsigned long long* out_key, uint32_t* out_id, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t n_wg = sort_blocks(n);
    hipLaunchKernelGGL(k_pyr_hist, dim3(n_wg), dim3(WG), 0, st, key, id, n, digit, counts);
    const hipError_t e = osmt_tq_scan(counts, BINS * n_wg, blk, tot, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pyr_scatter, dim3(n_wg), dim3(WG), 0, st, key, id, n, digit, counts, out_key, out_id);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_mark(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t* pos, uint32_t* cpos, unsigned long long* blk,
                                unsigned long long* tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_pyr_mark, grid_of(n), dim3(WG), 0, st, key, id, n, pos, cpos);
    hipError_t e = osmt_tq_scan(pos, n, blk, tot, st);
    if (e == hipSuccess && cpos) e = osmt_tq_scan(cpos, n, blk, tot + 1, st);
    return e;
}

hipError_t osmt_launch_pyr_emit_tiles(const unsigned long long* key, uint32_t n, const uint32_t* pos, const uint32_t* cpos, uint32_t n_tiles, uint32_t n_cols,
                                      uint32_t* tile_x, uint32_t* tile_y, uint32_t* col_x, uint32_t* col_first, hipStream_t st) {
    hipLaunchKernelGGL(k_pyr_emit_tiles, grid_of(n ? n : 1u), dim3(WG), 0, st, key, n, pos, cpos, n_tiles, n_cols, tile_x, tile_y, col_x, col_first);
    return hipGetLastError();
}

hipError_t osmt_launch_pyr_emit_lists(const unsigned long long* key, const uint32_t* id, uint32_t n, const uint32_t* pos, const uint32_t* tile_x,
                                      const uint32_t* tile_y, uint32_t n_tiles, uint32_t* off, uint32_t* pool, hipStream_t st) {
    const uint32_t lanes = n > n_tiles + 1u ? n : n_tiles + 1u;
    hipLaunchKernelGGL(k_pyr_emit_lists, grid_of(lanes), dim3(WG), 0, st, key, id, n, pos, tile_x, tile_y, n_tiles, off, pool);
    return hipGetLastError();
}
