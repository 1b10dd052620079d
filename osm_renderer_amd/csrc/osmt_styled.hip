/*
 * osmt_styled.hip — display lists built on the GPU (osmt_scene_build_styled): what Styler::style_areas
 * (mapcss/styler.rs:168-203,246-272) and the Fill / Casing / Stroke passes of Drawer::draw_to_pixels
 * (draw/drawer.rs:60-99,133-219) do per tile on the reference's worker thread, for a whole batch.  The host twin, and
 * the yardstick of the tests, is osmt::SceneBuilder (host/osmt_styled.hpp).  gfx950 only.
 *
 *   k_styled_sort         one workgroup per tile.  style_areas is two stable sorts and a merge that prefers the relation on
 *                         Equal: one sort under the TOTAL order (layer or 0, is_foreground_fill, z_index, global id,
 *                         multipolygon before way, input position).  The first three depend on the style alone and arrive
 *                         as its dense rank (computed when the styles were registered), so a key is 16 bytes:
 *                         rank:32 | gid:64 | way:1 | position:16.  A total order needs no stable algorithm: a bitonic
 *                         network in its one-direction form (first step of a merge mirrors, the others shift), where
 *                         the virtual +inf padding above n never moves and is never stored.  Tiles of up to
 *                         OSMT_STYLED_LDS_AREAS areas keep their keys in LDS, larger ones in device memory — the same
 *                         code, the same launch; a workgroup sees its own global stores behind a barrier.
 *   k_styled_count        one lane per (tile, pass, sorted area): exactly what SceneBuilder::draw_one_area would append —
 *                         an op or none, rings of >= 2 nodes, node references, dash entries (appended BEFORE the rings are
 *                         looked at: a dashed stroke of a ringless way leaves its dashes and no op) — and what
 *                         the scene's index tables count: stroke slots, 64-edge blocks, virtual segments.  Block totals in
 *                         64 bits.
 *   k_styled_scan_blocks  one workgroup: exclusive scan of the block totals, the seven grand totals.
 *   k_styled_scan_apply   counts -> exclusive scans in (tile, pass, position) order = op order.  32-bit with wrap-around:
 *                         a scan of non-negative terms whose true total is below 2^32 wrapped nowhere, so every offset
 *                         is exact once the host has seen the 64-bit totals (k_styled_count's block sums, their scan
 *                         and its carry: unsigned long long throughout) fit; nothing is emitted before.
 *   k_styled_tilemax      the most ops of any tile (the renderer chooses its list kernel by it).
 *   k_styled_emit         one lane per element again: the op header as four 16-byte stores, its rings, its scaled dashes,
 *                         op -> job / stroke slot / first block / first virtual segment.
 *   k_styled_jobs         one lane per tile: osmt_tile_job, also for tiles without ops.
 *   k_styled_refs         the byte-heavy part, one lane per node reference: consecutive lanes walk along a ring (its
 *                         source found by bisection over the rings' first points), so loads and stores coalesce.
 *
 * Every index read here was checked on the host: the geodata tables when they were registered, the batch's ids by
 * osmt_validate_styled_batch.  Every store lands below a total the arrays were sized with.  No LDS beyond the sort keys and
 * the scans' wave sums, no scratch, no device-side library.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_bitonic.h"
#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;

struct elem {
    uint32_t tile, pass;
    uint32_t id;       /* local entity id */
    uint32_t n_rings;  /* rings of >= 2 nodes */
    uint32_t n_refs;   /* their nodes */
    uint32_t n_dashes; /* dash entries the pass appends (whether or not an op follows) */
    uint32_t dash_src; /* first of them in the styles' pool */
    uint32_t cap;
    bool is_mp, draws, emits;
    const osmt_style_rec* s;
};

/* the tile of area slot v = element / 3: the smallest t with tile_base[t + 1] > v (empty tiles own no slot) */
__device__ __forceinline__ uint32_t find_tile(const uint32_t* __restrict__ base, uint32_t n_tiles, uint32_t v) {
    uint32_t lo = 0u, hi = n_tiles - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (base[mid + 1u] > v)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

/* SceneBuilder::draw_one_area's decisions for element e (drawer.rs:156-219) */
__device__ __forceinline__ void eval(const osmt_styled_pass& P, uint32_t e, elem& o) {
    const uint32_t t = find_tile(P.tile_base, P.n_tiles, e / 3u);
    const uint32_t base = P.tile_base[t], n = P.tile_base[t + 1u] - base;
    const uint32_t r = e - 3u * base;
    const uint32_t pass = r / n, k = r - pass * n;
    const osmt_styled_area a = P.areas[P.sorted[base + k]];
    const osmt_style_rec* s = P.styles + a.style;
    o.tile = t;
    o.pass = pass;
    o.is_mp = (a.entity & OSMT_STYLED_MULTIPOLYGON) != 0u;
    o.id = a.entity & ~OSMT_STYLED_MULTIPOLYGON;
    o.s = s;
    o.n_rings = o.n_refs = o.n_dashes = o.dash_src = o.cap = 0u;
    o.draws = o.emits = false;
    if (o.is_mp && pass != 0u) return; /* multipolygons draw in the Fill pass only (drawer.rs:77-99) */
    if (pass == 0u) {
        o.draws = s->has_fill_color != 0 || s->has_fill_image != 0;
    } else if (pass == 1u) {
        o.draws = s->has_casing_color != 0 && s->has_casing_width != 0;
        if (o.draws && s->has_casing_dashes != 0) o.n_dashes = s->n_casing_dashes, o.dash_src = s->casing_dashes_off;
        o.cap = s->casing_line_cap;
    } else {
        o.draws = s->has_color != 0;
        if (o.draws && s->has_dashes != 0) o.n_dashes = s->n_dashes, o.dash_src = s->dashes_off;
        o.cap = s->line_cap;
    }
    if (!o.draws) return;
    if (o.is_mp) {
        const uint2 sum = P.geo.mp_sum[o.id];
        o.n_rings = sum.x;
        o.n_refs = sum.y;
    } else {
        const uint32_t nn = P.geo.way_off[o.id + 1u] - P.geo.way_off[o.id];
        o.n_rings = nn >= 2u ? 1u : 0u;
        o.n_refs = nn >= 2u ? nn : 0u;
    }
    o.emits = o.n_rings != 0u;
}

__device__ __forceinline__ void counts_of(const elem& o, uint32_t c[OSMT_SQ_N]) {
    const uint32_t edges = o.n_refs - o.n_rings;
    const bool stroke = o.emits && o.pass != 0u;
    c[OSMT_SQ_OPS] = o.emits ? 1u : 0u;
    c[OSMT_SQ_RINGS] = o.emits ? o.n_rings : 0u;
    c[OSMT_SQ_REFS] = o.emits ? o.n_refs : 0u;
    c[OSMT_SQ_DASHES] = o.n_dashes;
    c[OSMT_SQ_STROKES] = stroke ? 1u : 0u;
    c[OSMT_SQ_BLOCKS] = (o.emits && edges > 64u) ? (edges + 63u) / 64u : 0u;
    c[OSMT_SQ_VSEGS] = stroke ? edges + ((o.cap == OSMT_CAP_ROUND || o.cap == OSMT_CAP_SQUARE) ? 2u : 0u) : 0u;
}

/* ---- sort ---------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ bool key_less(const ulonglong2& a, const ulonglong2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

struct key_lt {
    __device__ __forceinline__ bool operator()(const ulonglong2& a, const ulonglong2& b) const { return key_less(a, b); }
};

__global__ __launch_bounds__(256) void k_styled_sort(osmt_styled_pass P) {
    __shared__ ulonglong2 lds_keys[OSMT_STYLED_LDS_AREAS];
    const uint32_t t = blockIdx.x;
    const uint32_t base = P.tile_base[t], n = P.tile_base[t + 1u] - base;
    if (n == 0u) return; /* uniform over the workgroup */
    const uint32_t aoff = P.tiles[t].area_off;
    const bool in_lds = n <= OSMT_STYLED_LDS_AREAS;
    ulonglong2* gk = P.keys + base;
    for (uint32_t i = threadIdx.x; i < n; i += WG) {
        const osmt_styled_area a = P.areas[aoff + i];
        const bool mp = (a.entity & OSMT_STYLED_MULTIPOLYGON) != 0u;
        const uint32_t id = a.entity & ~OSMT_STYLED_MULTIPOLYGON;
        const unsigned long long gid = mp ? P.geo.mp_gid[id] : P.geo.way_gid[id];
        ulonglong2 key;
        key.x = ((unsigned long long)P.style_rank[a.style] << 32) | (gid >> 32);
        key.y = ((gid & 0xFFFFFFFFull) << 32) | (mp ? 0ull : 0x80000000ull) | (unsigned long long)i; /* i < 65536 */
        if (in_lds)
            lds_keys[i] = key;
        else
            gk[i] = key;
    }
    __syncthreads();
    uint32_t N = 1u;
    while (N < n) N <<= 1;
    if (in_lds) {
        osmt_bitonic<WG>(lds_keys, n, N, key_lt{});
        for (uint32_t i = threadIdx.x; i < n; i += WG) P.sorted[base + i] = aoff + (uint32_t)(lds_keys[i].y & 0xFFFFull);
    } else {
        osmt_bitonic<WG>(gk, n, N, key_lt{});
        for (uint32_t i = threadIdx.x; i < n; i += WG) P.sorted[base + i] = aoff + (uint32_t)(gk[i].y & 0xFFFFull);
    }
}

/* ---- count, scan ------------------------------------------------------------------------------------------------ */
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)v, d), hi = __shfl_down((uint32_t)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v; /* lane 0 */
}

__global__ __launch_bounds__(256) void k_styled_count(osmt_styled_pass P) {
    __shared__ unsigned long long wsum[OSMT_SQ_N][WG / 64u];
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    uint32_t c[OSMT_SQ_N];
#pragma unroll
    for (int q = 0; q < OSMT_SQ_N; ++q) c[q] = 0u;
    if (e < P.n_elems) {
        elem o;
        eval(P, e, o);
        counts_of(o, c);
#pragma unroll
        for (int q = 0; q < OSMT_SQ_N; ++q) P.pre[(size_t)q * (P.n_elems + 1u) + e] = c[q];
    }
#pragma unroll
    for (int q = 0; q < OSMT_SQ_N; ++q) {
        const unsigned long long s = wave_sum64(c[q]);
        if ((threadIdx.x & 63u) == 0u) wsum[q][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < OSMT_SQ_N) {
        unsigned long long s = 0ull;
        for (uint32_t w = 0; w < WG / 64u; ++w) s += wsum[threadIdx.x][w];
        P.blk[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

/* one workgroup; n_blk = the grid of k_styled_count (0: no element at all) */
__global__ __launch_bounds__(256) void k_styled_scan_blocks(osmt_styled_pass P, uint32_t n_blk) {
    __shared__ unsigned long long wsum[WG / 64u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t q = 0; q < OSMT_SQ_N; ++q) {
        unsigned long long* b = P.blk + (size_t)q * n_blk;
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
            unsigned long long off = 0ull, tot = 0ull;
            for (uint32_t x = 0; x < WG / 64u; ++x) {
                if (x < w) off += wsum[x];
                tot += wsum[x];
            }
            if (i < n_blk) b[i] = carry + off + inc - v;
            carry += tot;
            __syncthreads();
        }
        if (threadIdx.x == 0u) P.totals[q] = carry;
    }
    if (threadIdx.x == 0u) P.totals[OSMT_SQ_N] = 0ull; /* k_styled_tilemax */
}

/* grid: the blocks of k_styled_count, at least one (entry n_elems of every scan is its total) */
__global__ __launch_bounds__(256) void k_styled_scan_apply(osmt_styled_pass P, uint32_t n_blk) {
    __shared__ uint32_t wsum[WG / 64u];
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t q = 0; q < OSMT_SQ_N; ++q) {
        uint32_t* pre = P.pre + (size_t)q * (P.n_elems + 1u);
        const uint32_t v = e < P.n_elems ? pre[e] : 0u;
        uint32_t inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc += u;
        }
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        uint32_t off = 0u;
        for (uint32_t x = 0; x < w; ++x) off += wsum[x];
        const uint32_t bbase = blockIdx.x < n_blk ? (uint32_t)P.blk[(size_t)q * n_blk + blockIdx.x] : 0u;
        if (e < P.n_elems) pre[e] = bbase + off + inc - v;
        if (e == 0u) pre[P.n_elems] = (uint32_t)P.totals[q];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_styled_tilemax(osmt_styled_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tiles) return;
    const uint32_t* pre = P.pre + (size_t)OSMT_SQ_OPS * (P.n_elems + 1u);
    const uint32_t n = pre[3u * P.tile_base[t + 1u]] - pre[3u * P.tile_base[t]];
    if (n) atomicMax(P.totals + OSMT_SQ_N, (unsigned long long)n);
}

/* ---- emit ------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void k_styled_emit(osmt_styled_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_elems) return;
    elem o;
    eval(P, e, o);
    if (!o.draws) return;
    uint32_t at[OSMT_SQ_N];
#pragma unroll
    for (int q = 0; q < OSMT_SQ_N; ++q) at[q] = P.pre[(size_t)q * (P.n_elems + 1u) + e];
    const double scale = (double)P.scale;
    /* scale_dashes (drawer.rs:170-171), before the rings are looked at */
    for (uint32_t i = 0; i < o.n_dashes; ++i) P.dashes[at[OSMT_SQ_DASHES] + i] = P.style_dashes[o.dash_src + i] * scale;
    if (!o.emits) return;
    const osmt_style_rec* s = o.s;
    const uint32_t op = at[OSMT_SQ_OPS];
    uint32_t kind, c0 = 0u, c1 = 0u, c2 = 0u, image = 0u, has_d = 0u, caps = 0u, cap = 0u;
    double opacity, width = 0.0;
    if (o.pass == 0u) {
        opacity = s->has_fill_opacity ? s->fill_opacity : 1.0;
        if (s->has_fill_color) {
            kind = OSMT_OP_FILL_COLOR;
            c0 = s->fill_color[0], c1 = s->fill_color[1], c2 = s->fill_color[2];
        } else {
            kind = OSMT_OP_FILL_IMAGE;
            image = s->fill_image;
        }
    } else {
        kind = OSMT_OP_STROKE;
        cap = o.cap;
        caps = P.use_caps ? 1u : 0u;
        if (o.pass == 1u) {
            c0 = s->casing_color[0], c1 = s->casing_color[1], c2 = s->casing_color[2];
            opacity = 1.0;
            width = s->casing_width * scale;
            has_d = s->has_casing_dashes ? 1u : 0u;
        } else {
            c0 = s->color[0], c1 = s->color[1], c2 = s->color[2];
            opacity = s->has_opacity ? s->opacity : 1.0;
            width = scale * (s->has_width ? s->width : 1.0);
            has_d = s->has_dashes ? 1u : 0u;
        }
    }
    const unsigned long long ob = (unsigned long long)__double_as_longlong(opacity), wb = (unsigned long long)__double_as_longlong(width);
    uint4* dst = reinterpret_cast<uint4*>(P.ops + op);
    dst[0] = make_uint4(kind | cap << 8 | caps << 16 | has_d << 24, c0 | c1 << 8 | c2 << 16, (uint32_t)ob, (uint32_t)(ob >> 32));
    dst[1] = make_uint4((uint32_t)wb, (uint32_t)(wb >> 32), has_d ? o.n_dashes : 0u, has_d ? at[OSMT_SQ_DASHES] : 0u);
    dst[2] = make_uint4(o.n_rings, at[OSMT_SQ_RINGS], image, 0u);
    dst[3] = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t edges = o.n_refs - o.n_rings;
    P.op_job[op] = o.tile;
    P.op_aux[op] = o.pass != 0u ? at[OSMT_SQ_STROKES] : 0u;
    P.op_blk[op] = edges > 64u ? at[OSMT_SQ_BLOCKS] : 0xFFFFFFFFu;
    P.op_vseg[op] = o.pass != 0u ? at[OSMT_SQ_VSEGS] : 0u;
    /* to_point_pairs (point_pairs.rs:11-41) as rings of node indices; a ring of fewer than two nodes has no pair */
    uint32_t ring = at[OSMT_SQ_RINGS], pt = at[OSMT_SQ_REFS];
    if (!o.is_mp) {
        P.rings[ring] = osmt_ring{pt, o.n_refs};
        P.ring_src[ring] = P.geo.way_off[o.id];
    } else {
        for (uint32_t m = P.geo.mp_off[o.id], m1 = P.geo.mp_off[o.id + 1u]; m < m1; ++m) {
            const uint32_t poly = P.geo.mp_polys[m];
            const uint32_t a = P.geo.poly_off[poly], nn = P.geo.poly_off[poly + 1u] - a;
            if (nn < 2u) continue;
            P.rings[ring] = osmt_ring{pt, nn};
            P.ring_src[ring] = a;
            ++ring;
            pt += nn;
        }
    }
}

__global__ __launch_bounds__(256) void k_styled_jobs(osmt_styled_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tiles) return;
    const osmt_styled_tile tl = P.tiles[t];
    const size_t stride = (size_t)P.n_elems + 1u;
    const uint32_t e0 = 3u * P.tile_base[t], e1 = 3u * P.tile_base[t + 1u];
    const uint32_t* pre_op = P.pre + OSMT_SQ_OPS * stride;
    const uint32_t* pre_pt = P.pre + OSMT_SQ_REFS * stride;
    const bool cv = tl.has_canvas != 0;
    uint4* dst = reinterpret_cast<uint4*>(P.jobs + t);
    dst[0] = make_uint4(tl.x, tl.y,
                        (uint32_t)tl.zoom | (cv ? 1u : 0u) << 8 | (cv ? (uint32_t)tl.canvas_rgb[0] : 0u) << 16 | (cv ? (uint32_t)tl.canvas_rgb[1] : 0u) << 24,
                        cv ? (uint32_t)tl.canvas_rgb[2] : 0u);
    dst[1] = make_uint4(pre_op[e1] - pre_op[e0], pre_op[e0], pre_pt[e1] - pre_pt[e0], pre_pt[e0]);
}

__global__ __launch_bounds__(256) void k_styled_refs(osmt_styled_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_refs) return;
    /* the last ring with first_pt <= i: rings are in emission order, their point ranges back to back from 0 */
    uint32_t lo = 0u, hi = P.n_rings - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (P.rings[mid].first_pt <= i)
            lo = mid;
        else
            hi = mid - 1u;
    }
    P.refs[i] = P.geo.idx[P.ring_src[lo] + (i - P.rings[lo].first_pt)];
}

}  // namespace

hipError_t osmt_launch_styled_count(const osmt_styled_pass& a, hipStream_t st) {
    const uint32_t n_blk = (a.n_elems + WG - 1u) / WG;
    if (a.n_elems) {
        hipLaunchKernelGGL(k_styled_sort, dim3(a.n_tiles), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_styled_count, dim3(n_blk), dim3(WG), 0, st, a);
    }
    hipLaunchKernelGGL(k_styled_scan_blocks, dim3(1), dim3(WG), 0, st, a, n_blk);
    hipLaunchKernelGGL(k_styled_scan_apply, dim3(n_blk ? n_blk : 1u), dim3(WG), 0, st, a, n_blk);
    if (a.n_tiles) hipLaunchKernelGGL(k_styled_tilemax, dim3((a.n_tiles + WG - 1u) / WG), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_styled_emit(const osmt_styled_pass& a, hipStream_t st) {
    if (a.n_elems) hipLaunchKernelGGL(k_styled_emit, dim3((a.n_elems + WG - 1u) / WG), dim3(WG), 0, st, a);
    if (a.n_tiles) hipLaunchKernelGGL(k_styled_jobs, dim3((a.n_tiles + WG - 1u) / WG), dim3(WG), 0, st, a);
    if (a.n_refs) hipLaunchKernelGGL(k_styled_refs, dim3((a.n_refs + WG - 1u) / WG), dim3(WG), 0, st, a);
    return hipGetLastError();
}
