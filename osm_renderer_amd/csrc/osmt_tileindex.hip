/*
 * osmt_tileindex.hip — the z18 tile index of a geodata file built on the device (osmt_build_tile_index) from the registered
 * nodes' Mercator factors and the file's topology: get_tile_references (saver.rs:167-226) with max_zoom_tile of tile.rs:30-38.
 * A node is listed in its own tile; a way in every tile of the inclusive rectangle over its nodes' tiles; a multipolygon
 * likewise over all nodes of all its polygons.  The host twin, and the yardstick of the tests, is osmt::tile_index_of
 * (host/osmt_tilequery.hpp).  gfx950 only.
 *
 *   k_tix_init        the boxes {min_x, max_x, min_y, max_y} = {~0, 0, ~0, 0} (the neutral element of the reduction) and the
 *                     words the host reads back.
 *   k_tix_node_tiles  one lane per node: x = (u32)(fx * 2^26) >> 8, y likewise — the product with a power of two is exact, the
 *                     conversion truncates, the shift is the / 256; no libm.  A factor of exactly 1.0 (coordinate 2^18) goes by
 *                     atomicMin of 2 * node + axis into the offender word: the host refuses the build.
 *   k_tix_bbox        one lane per node reference (the ways', then once more the polygons'): the entity by bisection over the
 *                     offsets, then a segmented min / max inside the wave over each run of lanes with the same entity; the run's
 *                     first lane issues the four atomics.  An entity of 100 000 references costs 4 atomics per wave, not per lane.
 *   k_tix_mp_bbox     one lane per (multipolygon, polygon) reference: the same reduction over the polygons' boxes; the box of a
 *                     polygon without nodes is the neutral element and changes nothing.
 *   k_tix_count       one lane per entity: W * H tiles, 0 for an empty box.  The exact 64-bit total is summed per wave and added
 *                     once; the per-entity count goes into the 32-bit scan SATURATED at 2^32 - 1, so the scanned offsets are
 *                     exact whenever the total fits 32 bits, and the host launches nothing more when it does not.
 *   k_tix_pairs       one lane per (tile, entity) reference: the entity by bisection over the scanned offsets, rank r inside it,
 *                     x = min_x + r / H, y = min_y + r % H, key = x << 18 | y, id = entity.
 *   k_tix_node_pairs  (key of the node's tile, node).
 *   k_tix_keymark / k_tix_keycompact
 *                     over one kind's SORTED pairs: 1 for the first of its key, scanned; the distinct keys compacted into the
 *                     tiles' job, which therefore sorts the kinds' distinct tiles, not every pair.
 *
 * The pairs are sorted, marked and emitted by the pyramid's kernels (osmt_tilepyramid.hip).  Integer min and max do not depend
 * on arrival order, so every array is deterministic.  Every store lands below a count its array was sized with; every word is
 * written before it is read.  No kernel here uses scratch (profiles/tile_index_build_kernel_resources.txt).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t KEY_Y_BITS = OSMT_MAX_ZOOM; /* key = x << 18 | y */
constexpr uint32_t NO_ENTITY = 0xFFFFFFFFu;

typedef unsigned long long u64;

/* the entity of reference r: the smallest i with off[i + 1] > r (entities without references own none); off[0] <= r < off[n] */
__device__ __forceinline__ uint32_t owner_of(const uint32_t* __restrict__ off, uint32_t n, uint32_t r) {
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

__global__ __launch_bounds__(256) void k_tix_init(uint4* __restrict__ box, uint32_t n, u64* __restrict__ words) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) box[i] = make_uint4(~0u, 0u, ~0u, 0u);
    if (words && i < OSMT_TIX_WORDS) words[i] = i == OSMT_TIX_OFFENDER ? ~0ull : 0ull;
}

__global__ __launch_bounds__(256) void k_tix_node_tiles(const double2* __restrict__ factors, uint32_t n, uint32_t* __restrict__ tx, uint32_t* __restrict__ ty,
                                                        u64* __restrict__ words) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const double2 f = factors[i];
    const uint32_t x = (uint32_t)(f.x * 67108864.0) >> 8, y = (uint32_t)(f.y * 67108864.0) >> 8; /* factors in [0, 1]: at most 2^26 */
    tx[i] = x;
    ty[i] = y;
    const uint32_t world = 1u << OSMT_MAX_ZOOM;
    if (x >= world || y >= world) atomicMin(&words[OSMT_TIX_OFFENDER], 2ull * i + (x >= world ? 0ull : 1ull));
}

/* The min / max of v over each run of lanes of the wave with the same `ent` (runs are contiguous: ent does not decrease with
 * the lane), committed to box[ent] by the run's first lane.  Every lane of the wave calls this; ent == NO_ENTITY: no entity. */
__device__ __forceinline__ void commit_runs(uint32_t ent, uint4 v, uint4* __restrict__ box) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t e = __shfl_down(ent, d);
        const uint32_t a = __shfl_down(v.x, d), b = __shfl_down(v.y, d), c = __shfl_down(v.z, d), g = __shfl_down(v.w, d);
        if (lane + d < 64u && e == ent) v.x = min(v.x, a), v.y = max(v.y, b), v.z = min(v.z, c), v.w = max(v.w, g);
    }
    const uint32_t before = __shfl_up(ent, 1u);
    const bool first = lane == 0u || before != ent;
    if (!first || ent == NO_ENTITY || v.x > v.y) return; /* v.x > v.y: the neutral element, nothing to add */
    uint32_t* w = (uint32_t*)&box[ent];
    atomicMin(w + 0, v.x);
    atomicMax(w + 1, v.y);
    atomicMin(w + 2, v.z);
    atomicMax(w + 3, v.w);
}

/* off: [n_ent + 1] into idx, off[0] = base; lanes over the n_refs = off[n_ent] - base references */
__global__ __launch_bounds__(256) void k_tix_bbox(const uint32_t* __restrict__ off, uint32_t n_ent, const uint32_t* __restrict__ idx, uint32_t base,
                                                  uint32_t n_refs, const uint32_t* __restrict__ tx, const uint32_t* __restrict__ ty, uint4* __restrict__ box) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    uint32_t ent = NO_ENTITY;
    uint4 v = make_uint4(~0u, 0u, ~0u, 0u);
    if (r < n_refs) {
        ent = owner_of(off, n_ent, base + r);
        const uint32_t node = idx[base + r];
        const uint32_t x = tx[node], y = ty[node];
        v = make_uint4(x, x, y, y);
    }
    commit_runs(ent, v, box);
}

__global__ __launch_bounds__(256) void k_tix_mp_bbox(const uint32_t* __restrict__ mp_off, uint32_t n_mps, const uint32_t* __restrict__ mp_polys, uint32_t n_refs,
                                                     const uint4* __restrict__ poly_box, uint4* __restrict__ box) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    uint32_t ent = NO_ENTITY;
    uint4 v = make_uint4(~0u, 0u, ~0u, 0u);
    if (r < n_refs) {
        ent = owner_of(mp_off, n_mps, r);
        v = poly_box[mp_polys[r]];
    }
    commit_runs(ent, v, box);
}

/* cnt[i] = min(W * H, 2^32 - 1); *total += the exact sum */
__global__ __launch_bounds__(256) void k_tix_count(const uint4* __restrict__ box, uint32_t n, uint32_t* __restrict__ cnt, u64* __restrict__ total) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    u64 c = 0ull;
    if (i < n) {
        const uint4 b = box[i];
        if (b.x <= b.y) c = (u64)(b.y - b.x + 1u) * (u64)(b.w - b.z + 1u);
        cnt[i] = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
    }
    for (uint32_t d = 32u; d; d >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)c, d), hi = __shfl_down((uint32_t)(c >> 32), d);
        c += ((u64)hi << 32) | lo; /* lanes beyond the wave give their own value: only lane 0's sum is used */
    }
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(total, c);
}

/* off: the scan of k_tix_count's counts, [n_ent + 1], off[n_ent] = n_refs */
__global__ __launch_bounds__(256) void k_tix_pairs(const uint32_t* __restrict__ off, uint32_t n_ent, const uint4* __restrict__ box, uint32_t n_refs,
                                                   u64* __restrict__ key, uint32_t* __restrict__ id) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= n_refs) return;
    const uint32_t e = owner_of(off, n_ent, r);
    const uint4 b = box[e];
    const uint32_t rank = r - off[e], h = b.w - b.z + 1u;
    const uint32_t x = b.x + rank / h, y = b.z + rank % h;
    key[r] = ((u64)x << KEY_Y_BITS) | (u64)y;
    id[r] = e;
}

__global__ __launch_bounds__(256) void k_tix_node_pairs(const uint32_t* __restrict__ tx, const uint32_t* __restrict__ ty, uint32_t n, u64* __restrict__ key,
                                                        uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    key[i] = ((u64)tx[i] << KEY_Y_BITS) | (u64)ty[i];
    id[i] = i;
}

__global__ __launch_bounds__(256) void k_tix_keymark(const u64* __restrict__ key, uint32_t n, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0u || key[i] != key[i - 1u]) ? 1u : 0u;
}

/* head: scanned, [n + 1]; out: room for head[n] keys */
__global__ __launch_bounds__(256) void k_tix_keycompact(const u64* __restrict__ key, uint32_t n, const uint32_t* __restrict__ head, u64* __restrict__ out_key,
                                                        uint32_t* __restrict__ out_id) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = head[i];
    if (head[i + 1u] == p) return;
    out_key[p] = key[i];
    out_id[p] = 0u;
}

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

}  // namespace

hipError_t osmt_launch_tix_boxes(const osmt_tix_pass& a, hipStream_t st) {
    const osmt_geo_dev& g = a.geo;
    hipLaunchKernelGGL(k_tix_init, grid_of(a.n_ways > OSMT_TIX_WORDS ? a.n_ways : OSMT_TIX_WORDS), dim3(WG), 0, st, a.way_box, a.n_ways, a.words);
    if (a.n_polys) hipLaunchKernelGGL(k_tix_init, grid_of(a.n_polys), dim3(WG), 0, st, a.poly_box, a.n_polys, (u64*)nullptr);
    if (a.n_mps) hipLaunchKernelGGL(k_tix_init, grid_of(a.n_mps), dim3(WG), 0, st, a.mp_box, a.n_mps, (u64*)nullptr);
    if (a.n_nodes) hipLaunchKernelGGL(k_tix_node_tiles, grid_of(a.n_nodes), dim3(WG), 0, st, a.factors, a.n_nodes, a.tx, a.ty, a.words);
    if (a.n_way_nodes) hipLaunchKernelGGL(k_tix_bbox, grid_of(a.n_way_nodes), dim3(WG), 0, st, g.way_off, a.n_ways, g.idx, 0u, a.n_way_nodes, a.tx, a.ty, a.way_box);
    if (a.n_poly_nodes)
        hipLaunchKernelGGL(k_tix_bbox, grid_of(a.n_poly_nodes), dim3(WG), 0, st, g.poly_off, a.n_polys, g.idx, a.n_way_nodes, a.n_poly_nodes, a.tx, a.ty, a.poly_box);
    if (a.n_mp_polys) hipLaunchKernelGGL(k_tix_mp_bbox, grid_of(a.n_mp_polys), dim3(WG), 0, st, g.mp_off, a.n_mps, g.mp_polys, a.n_mp_polys, a.poly_box, a.mp_box);
    if (a.n_ways) hipLaunchKernelGGL(k_tix_count, grid_of(a.n_ways), dim3(WG), 0, st, a.way_box, a.n_ways, a.way_cnt, a.words + OSMT_TIX_WAY_REFS);
    hipError_t e = osmt_tq_scan(a.way_cnt, a.n_ways, a.blk, a.words + OSMT_TIX_SCAN, st);
    if (e != hipSuccess) return e;
    if (a.n_mps) hipLaunchKernelGGL(k_tix_count, grid_of(a.n_mps), dim3(WG), 0, st, a.mp_box, a.n_mps, a.mp_cnt, a.words + OSMT_TIX_MP_REFS);
    return osmt_tq_scan(a.mp_cnt, a.n_mps, a.blk, a.words + OSMT_TIX_SCAN, st);
}

hipError_t osmt_launch_tix_pairs(const uint32_t* off, uint32_t n_ent, const uint4* box, uint32_t n_refs, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (n_refs) hipLaunchKernelGGL(k_tix_pairs, grid_of(n_refs), dim3(WG), 0, st, off, n_ent, box, n_refs, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_tix_node_pairs(const uint32_t* tx, const uint32_t* ty, uint32_t n, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_tix_node_pairs, grid_of(n), dim3(WG), 0, st, tx, ty, n, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_tix_keymark(const unsigned long long* key, uint32_t n, uint32_t* head, unsigned long long* blk, unsigned long long* tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_tix_keymark, grid_of(n), dim3(WG), 0, st, key, n, head);
    return osmt_tq_scan(head, n, blk, tot, st);
}

hipError_t osmt_launch_tix_keycompact(const unsigned long long* key, uint32_t n, const uint32_t* head, unsigned long long* out_key, uint32_t* out_id,
                                      hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_tix_keycompact, grid_of(n), dim3(WG), 0, st, key, n, head, out_key, out_id);
    return hipGetLastError();
}
