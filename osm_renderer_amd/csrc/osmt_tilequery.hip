/*
 * osmt_tilequery.hip — scenes built from tile coordinates (osmt_scene_build_tiles): what
 * GeodataReader::get_entities_in_tile_with_neighbors (geodata/reader.rs:60-177) and the per-entity style lookup of
 * Styler::style_entities (mapcss/styler.rs:128-160, memoised there per (entity, zoom)) do per tile on the reference's worker
 * thread, for a whole batch.  The result is the styled batch osmt_styled.hip starts from.  The host twin, and the yardstick of
 * the tests, is osmt::styled_areas_of_tile (host/osmt_tilequery.hpp).  gfx950 only.
 *
 * A tile reads the registered z18 index, or — where the geodata id has a pyramid (osmt_tilepyramid.hip) — the smallest level L >=
 * its zoom: osmt_tq_pass::ixz names the index of every zoom, and below "z18", "18" and "2^18" read "level L", "L" and "2^L".
 *
 *   k_tq_span      one lane per requested tile: the rectangle of z18 tiles its 3 x 3 neighbourhood covers,
 *                  (x - 1) f <= tx <= (x + 2) f - 1 with f = 2^(18 - zoom), clipped to [0, 2^18) (every index coordinate is
 *                  below 2^18, so the reference's u32 wrap at the world's edge is this clip), and by two bisections in the
 *                  column directory the range of columns that exist.  A scan numbers the (tile, column) items.
 *   k_tq_columns   one lane per item: two bisections over y inside the column give the index tiles [i0, i1) of the item.
 *                  The index is sorted by (x, y), so their reference lists are ONE slice of each pool:
 *                  ways[way_off[i0] .. way_off[i1]), and the multipolygons' likewise.  Two scans give every slice its
 *                  place among the candidates.
 *   k_tq_tilecand  one lane per tile: its candidate counts and bases, the largest count, the first tile over the limit.
 *   k_tq_gather    one lane per candidate: its item by bisection over the items' bases, the id copied — consecutive lanes walk
 *                  along a slice, so loads and stores coalesce.  A tile's ways land in front of its multipolygons.
 *   k_tq_sort      one workgroup per (tile, kind): the one-direction bitonic network of k_styled_sort on 32-bit keys, in LDS up
 *                  to OSMT_QUERY_LDS_CANDIDATES ids and in place in device memory beyond.
 *   k_tq_mark      one lane per sorted candidate: 0 for a repeat of its predecessor, for a multipolygon without
 *                  polygons (reader.rs:86-93) and for an entity an id filter does not list (reader.rs:95-99), else the
 *                  number of styles bound to the entity under the tile's zoom.  A scan
 *                  turns the counts into area positions.
 *   k_tq_tiles     one lane per tile: its osmt_styled_tile, tile_base, the most areas of a tile, the first tile over the limit.
 *   k_tq_emit      one lane per candidate again: its osmt_styled_area records, in binding order.
 *
 * The scans are 32-bit with wrap-around and carry 64-bit block totals (osmt_styled.hip, k_styled_scan_apply): the host
 * reads the 64-bit totals back and launches nothing that uses an offset before it has seen them fit.  Every index read here
 * was checked on the host when the index and the bindings were registered and by osmt_validate_tile_batch; every store lands
 * below a total the arrays were sized with; every buffer is written before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_bitonic.h"
#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t SORT_WG = 1024u;

/* the first index in [lo, hi) whose value is >= v (hi if none) */
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}
/* the first index in [lo, hi) whose value is > v (hi if none) */
__device__ __forceinline__ uint32_t upper_bound(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}
/* the owner of slot v under the bases base[0 .. n]: the smallest k with base[k + 1] > v (owners without slots own none); v < base[n] */
__device__ __forceinline__ uint32_t owner_of(const uint32_t* __restrict__ base, uint32_t n, uint32_t v) {
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (base[mid + 1u] > v)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}
/* the same over the tiles' candidate slots, whose bases are t_wbase + t_mbase */
__device__ __forceinline__ uint32_t tile_of_slot(const osmt_tq_pass& P, uint32_t v) {
    uint32_t lo = 0u, hi = P.n_tiles - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.t_wbase[mid + 1u] + P.t_mbase[mid + 1u] > v)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

/* the index a tile of `zoom` reads: its pyramid level, or the registered z18 index */
__device__ __forceinline__ osmt_tq_index_dev index_of(const osmt_tq_pass& P, uint32_t zoom) { return P.ixz ? P.ixz[zoom] : P.ix; }

/* the clipped range of level-`level` coordinates the neighbourhood of coordinate c covers at `zoom` <= level (c < 2^zoom: at
 * most 2^19 before the clip).  The rectangle's z18 bounds are multiples of 2^(18 - level), so the level's tiles it covers are
 * exactly the parents of the z18 tiles it covers */
__device__ __forceinline__ void clip_range(uint32_t c, uint32_t zoom, uint32_t level, uint32_t& lo, uint32_t& hi) {
    const uint32_t sh = level - zoom, world = 1u << level;
    lo = c ? (c - 1u) << sh : 0u;
    hi = ((c + 2u) << sh) - 1u;
    if (hi > world - 1u) hi = world - 1u;
}

/* ---- scan: a[0 .. n) -> its exclusive scan, a[n] = the total (mod 2^32), *tot = the total ------------------------------ */
__global__ __launch_bounds__(256) void k_tq_scan_local(uint32_t* __restrict__ a, uint32_t n, unsigned long long* __restrict__ blk) {
    __shared__ unsigned long long wsum[WG / 64u];
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long v = e < n ? a[e] : 0ull;
    unsigned long long inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)inc, d), hi = __shfl_up((uint32_t)(inc >> 32), d);
        if (lane >= (uint32_t)d) inc += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    unsigned long long off = 0ull, tot = 0ull;
    for (uint32_t x = 0; x < WG / 64u; ++x) {
        if (x < w) off += wsum[x];
        tot += wsum[x];
    }
    if (e < n) a[e] = (uint32_t)(off + inc - v);
    if (threadIdx.x == 0u) blk[blockIdx.x] = tot;
}

/* one workgroup; n_blk = the grid of k_tq_scan_local (0: nothing to scan) */
__global__ __launch_bounds__(256) void k_tq_scan_blocks(unsigned long long* __restrict__ b, uint32_t n_blk, unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long wsum[WG / 64u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long carry = 0ull;
    for (uint32_t c0 = 0; c0 < n_blk; c0 += WG) {
        const uint32_t i = c0 + threadIdx.x;
        const unsigned long long v = i < n_blk ? b[i] : 0ull;
        unsigned long long inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)inc, d), hi = __shfl_up((uint32_t)(inc >> 32), d);
            if (lane >= (uint32_t)d) inc += ((unsigned long long)hi << 32) | lo;
        }
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        unsigned long long off = 0ull, t = 0ull;
        for (uint32_t x = 0; x < WG / 64u; ++x) {
            if (x < w) off += wsum[x];
            t += wsum[x];
        }
        if (i < n_blk) b[i] = carry + off + inc - v;
        carry += t;
        __syncthreads();
    }
    if (threadIdx.x == 0u) *tot = carry;
}

/* grid: the blocks of k_tq_scan_local, at least one */
__global__ __launch_bounds__(256) void k_tq_scan_apply(uint32_t* __restrict__ a, uint32_t n, const unsigned long long* __restrict__ blk, uint32_t n_blk,
                                                       const unsigned long long* __restrict__ tot) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e < n) a[e] += (uint32_t)blk[blockIdx.x];
    if (e == 0u) a[n] = (uint32_t)*tot;
}

hipError_t scan(uint32_t* a, uint32_t n, unsigned long long* blk, unsigned long long* tot, hipStream_t st) {
    const uint32_t n_blk = (n + WG - 1u) / WG;
    if (n_blk) hipLaunchKernelGGL(k_tq_scan_local, dim3(n_blk), dim3(WG), 0, st, a, n, blk);
    hipLaunchKernelGGL(k_tq_scan_blocks, dim3(1), dim3(WG), 0, st, blk, n_blk, tot);
    hipLaunchKernelGGL(k_tq_scan_apply, dim3(n_blk ? n_blk : 1u), dim3(WG), 0, st, a, n, blk, n_blk, tot);
    return hipGetLastError();
}

/* ---- span, columns ---------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void k_tq_span(osmt_tq_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t == 0u) {
        P.tot[OSMT_TQ_MAX_CAND] = 0ull;
        P.tot[OSMT_TQ_OVER_CAND] = ~0ull;
        P.tot[OSMT_TQ_MAX_AREAS] = 0ull;
        P.tot[OSMT_TQ_OVER_AREAS] = ~0ull;
    }
    if (t >= P.n_tiles) return;
    const osmt_query_tile q = P.q[t];
    const osmt_tq_index_dev ix = index_of(P, q.zoom);
    uint32_t xlo, xhi;
    clip_range(q.x, q.zoom, ix.level, xlo, xhi);
    const uint32_t c0 = lower_bound(ix.col_x, 0u, ix.n_cols, xlo);
    const uint32_t c1 = upper_bound(ix.col_x, c0, ix.n_cols, xhi);
    P.span_c0[t] = c0;
    P.item_base[t] = c1 - c0;
}

__global__ __launch_bounds__(256) void k_tq_columns(osmt_tq_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_items) return;
    const uint32_t t = owner_of(P.item_base, P.n_tiles, i);
    const uint32_t col = P.span_c0[t] + (i - P.item_base[t]);
    const osmt_query_tile q = P.q[t];
    const osmt_tq_index_dev ix = index_of(P, q.zoom);
    uint32_t ylo, yhi;
    clip_range(q.y, q.zoom, ix.level, ylo, yhi);
    const uint32_t a = ix.col_first[col], b = ix.col_first[col + 1u];
    const uint32_t i0 = lower_bound(ix.tile_y, a, b, ylo);
    const uint32_t i1 = upper_bound(ix.tile_y, i0, b, yhi);
    const uint32_t w0 = ix.way_off[i0], m0 = ix.mp_off[i0];
    P.item_tile[i] = t;
    P.item_wsrc[i] = w0;
    P.item_msrc[i] = m0;
    P.wbase[i] = ix.way_off[i1] - w0;
    P.mbase[i] = ix.mp_off[i1] - m0;
}

/* a tile's slices are disjoint parts of a pool of fewer than 2^32 references: its counts are exact even where the bases wrapped */
__global__ __launch_bounds__(256) void k_tq_tilecand(osmt_tq_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tiles) return;
    const uint32_t i0 = P.item_base[t], i1 = P.item_base[t + 1u];
    const uint32_t w0 = P.wbase[i0], w1 = P.wbase[i1], m0 = P.mbase[i0], m1 = P.mbase[i1];
    P.t_wbase[t] = w0;
    P.t_mbase[t] = m0;
    if (t == P.n_tiles - 1u) {
        P.t_wbase[P.n_tiles] = w1;
        P.t_mbase[P.n_tiles] = m1;
    }
    const uint32_t nw = w1 - w0, nm = m1 - m0, n = nw > nm ? nw : nm;
    if (n) atomicMax(P.tot + OSMT_TQ_MAX_CAND, (unsigned long long)n);
    if (n > OSMT_QUERY_MAX_TILE_CANDIDATES) atomicMin(P.tot + OSMT_TQ_OVER_CAND, (unsigned long long)t);
}

/* ---- gather ------------------------------------------------------------------------------------------------------ */
template <bool MP>
__global__ __launch_bounds__(256) void k_tq_gather(osmt_tq_pass P) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= (MP ? P.n_mps : P.n_ways)) return;
    const uint32_t* base = MP ? P.mbase : P.wbase;
    const uint32_t i = owner_of(base, P.n_items, c);
    const uint32_t t = P.item_tile[i];
    const uint32_t tw = P.t_wbase[t], tm = P.t_mbase[t];
    const uint32_t src = (MP ? P.item_msrc : P.item_wsrc)[i] + (c - base[i]);
    const uint32_t dst = MP ? tw + tm + (P.t_wbase[t + 1u] - tw) + (c - tm) : tw + tm + (c - tw);
    const uint32_t* pool = MP ? P.ix.mps : P.ix.ways; /* the pools the item slices: those of its tile's zoom */
    if (P.ixz) pool = MP ? P.ixz[P.q[t].zoom].mps : P.ixz[P.q[t].zoom].ways;
    P.cand[dst] = pool[src];
}

/* ---- sort -------------------------------------------------------------------------------------------------------- */
struct id_lt {
    __device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const { return a < b; }
};

/* grid (tiles, 2): y = 0 the tile's ways, 1 its multipolygons */
__global__ __launch_bounds__(1024) void k_tq_sort(osmt_tq_pass P) {
    __shared__ uint32_t lds_keys[OSMT_QUERY_LDS_CANDIDATES];
    const uint32_t t = blockIdx.x;
    const uint32_t tw = P.t_wbase[t], tm = P.t_mbase[t];
    const uint32_t nw = P.t_wbase[t + 1u] - tw, nm = P.t_mbase[t + 1u] - tm;
    const uint32_t n = blockIdx.y ? nm : nw;
    if (n < 2u) return; /* uniform over the workgroup */
    uint32_t* gk = P.cand + (tw + tm + (blockIdx.y ? nw : 0u));
    uint32_t N = 1u;
    while (N < n) N <<= 1;
    if (n <= OSMT_QUERY_LDS_CANDIDATES) {
        for (uint32_t i = threadIdx.x; i < n; i += SORT_WG) lds_keys[i] = gk[i];
        __syncthreads();
        osmt_bitonic<SORT_WG>(lds_keys, n, N, id_lt{});
        for (uint32_t i = threadIdx.x; i < n; i += SORT_WG) gk[i] = lds_keys[i];
    } else {
        osmt_bitonic<SORT_WG>(gk, n, N, id_lt{}); /* a workgroup sees its own global stores behind a barrier */
    }
}

/* ---- mark, tiles, emit ------------------------------------------------------------------------------------------- */
struct slot {
    uint32_t tile, id, n_styles, styles_off;
    bool mp, counts;
    const uint32_t* styles;
};

/* candidate slot p: whose it is, and the styles it expands to if it is the first of its id in its tile */
__device__ __forceinline__ void eval(const osmt_tq_pass& P, uint32_t p, slot& o) {
    const uint32_t t = tile_of_slot(P, p);
    const uint32_t tw = P.t_wbase[t], k = p - (tw + P.t_mbase[t]), nw = P.t_wbase[t + 1u] - tw;
    const uint32_t id = P.cand[p];
    const osmt_tq_bind_dev B = P.bind[P.q[t].zoom];
    o.tile = t;
    o.id = id;
    o.mp = k >= nw;
    o.counts = k == 0u || k == nw || P.cand[p - 1u] != id;
    const uint32_t* keep = o.mp ? P.keep_mp : P.keep_way; /* both NULL or neither: kernel arguments, the test is uniform */
    if (keep && !((keep[id >> 5] >> (id & 31u)) & 1u)) o.counts = false; /* filter_entities_by_ids (reader.rs:254-262) */
    if (o.mp) {
        if (P.geo_mp_off[id + 1u] == P.geo_mp_off[id]) o.counts = false;
        o.styles_off = B.mp_off[id];
        o.n_styles = B.mp_off[id + 1u] - o.styles_off;
        o.styles = B.mp_styles;
    } else {
        o.styles_off = B.way_off[id];
        o.n_styles = B.way_off[id + 1u] - o.styles_off;
        o.styles = B.way_styles;
    }
}

__global__ __launch_bounds__(256) void k_tq_mark(osmt_tq_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_ways + P.n_mps) return;
    slot o;
    eval(P, p, o);
    P.apos[p] = o.counts ? o.n_styles : 0u;
}

__global__ __launch_bounds__(256) void k_tq_tiles(osmt_tq_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tiles) return;
    const uint32_t a0 = P.apos[P.t_wbase[t] + P.t_mbase[t]], a1 = P.apos[P.t_wbase[t + 1u] + P.t_mbase[t + 1u]];
    const uint32_t n = a1 - a0;
    const osmt_query_tile q = P.q[t];
    osmt_styled_tile tl;
    tl.x = q.x, tl.y = q.y, tl.zoom = q.zoom, tl.has_canvas = q.has_canvas;
    tl.canvas_rgb[0] = q.canvas_rgb[0], tl.canvas_rgb[1] = q.canvas_rgb[1], tl.canvas_rgb[2] = q.canvas_rgb[2];
    tl._pad[0] = tl._pad[1] = tl._pad[2] = 0;
    tl.area_off = a0, tl.n_areas = n;
    P.tiles[t] = tl;
    P.tile_base[t] = a0;
    if (t == P.n_tiles - 1u) P.tile_base[P.n_tiles] = a1;
    if (n) atomicMax(P.tot + OSMT_TQ_MAX_AREAS, (unsigned long long)n);
    if (n > OSMT_STYLED_MAX_TILE_AREAS) atomicMin(P.tot + OSMT_TQ_OVER_AREAS, (unsigned long long)t);
}

__global__ __launch_bounds__(256) void k_tq_emit(osmt_tq_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_ways + P.n_mps) return;
    const uint32_t a0 = P.apos[p], n = P.apos[p + 1u] - a0;
    if (n == 0u) return;
    slot o;
    eval(P, p, o);
    const uint32_t entity = o.id | (o.mp ? OSMT_STYLED_MULTIPOLYGON : 0u);
    for (uint32_t j = 0; j < n; ++j) P.areas[a0 + j] = osmt_styled_area{entity, o.styles[o.styles_off + j]};
}

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

}  // namespace

hipError_t osmt_tq_scan(uint32_t* a, uint32_t n, unsigned long long* blk, unsigned long long* tot, hipStream_t st) { return scan(a, n, blk, tot, st); }

hipError_t osmt_launch_tq_span(const osmt_tq_pass& a, hipStream_t st) {
    hipLaunchKernelGGL(k_tq_span, grid_of(a.n_tiles), dim3(WG), 0, st, a);
    return scan(a.item_base, a.n_tiles, a.blk, a.tot + OSMT_TQ_ITEMS, st);
}

hipError_t osmt_launch_tq_columns(const osmt_tq_pass& a, hipStream_t st) {
    if (a.n_items) hipLaunchKernelGGL(k_tq_columns, grid_of(a.n_items), dim3(WG), 0, st, a);
    hipError_t e = scan(a.wbase, a.n_items, a.blk, a.tot + OSMT_TQ_WAYS, st);
    if (e == hipSuccess) e = scan(a.mbase, a.n_items, a.blk, a.tot + OSMT_TQ_MPS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tq_tilecand, grid_of(a.n_tiles), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tq_gather(const osmt_tq_pass& a, hipStream_t st) {
    if (a.n_ways) hipLaunchKernelGGL(k_tq_gather<false>, grid_of(a.n_ways), dim3(WG), 0, st, a);
    if (a.n_mps) hipLaunchKernelGGL(k_tq_gather<true>, grid_of(a.n_mps), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tq_sort(const osmt_tq_pass& a, hipStream_t st) {
    if (a.n_ways + a.n_mps) hipLaunchKernelGGL(k_tq_sort, dim3(a.n_tiles, 2), dim3(SORT_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tq_mark(const osmt_tq_pass& a, hipStream_t st) {
    const uint32_t n = a.n_ways + a.n_mps;
    if (n) hipLaunchKernelGGL(k_tq_mark, grid_of(n), dim3(WG), 0, st, a);
    const hipError_t e = scan(a.apos, n, a.blk, a.tot + OSMT_TQ_AREAS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tq_tiles, grid_of(a.n_tiles), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tq_emit(const osmt_tq_pass& a, hipStream_t st) {
    const uint32_t n = a.n_ways + a.n_mps;
    if (n) hipLaunchKernelGGL(k_tq_emit, grid_of(n), dim3(WG), 0, st, a);
    return hipGetLastError();
}
