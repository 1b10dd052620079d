/*
 * osmt_glyphs.hip — label text given as glyph runs (osmt_scene_set_glyph_labels): the glyph walk of the reference
 * (Glyph::rasterize, font/text_placer.rs:232-259, and Rasterizer::draw_quad, font/rasterizer.rs:90-113) on the GPU,
 * writing exactly the draw_line calls the host walk would make, in its order, into the label pass's segment arena.
 * gfx950 only; -ffp-contract=off (every f64 operation is the reference's, osmt_glyph.h).
 *
 *   k_glyph_init    per label: the window summary's neutral values (osmt_label_extent), the error word
 *   k_glyph_count   one wave per (label, glyph instance) pair, lane = outline vertex (64 at a time): the vertex's
 *                   draw_line calls counted and reduced per label (n_segs, ry0 / ry1 / cx0 / cx1: integer min / max,
 *                   order-free) with one atomic per wave and quantity; the pair's call count for the scan
 *   k_glyph_scan_blocks / k_glyph_scan_top
 *                   exclusive scan of the pair counts (pairs are in label order, so a label's first call lands at
 *                   the running sum of the n_segs before it — what the host assigns as its seg_off)
 *   k_glyph_emit    the same walk again, each lane's calls written at pair base + wave-exclusive rank
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_glyph.h"
#include "osmt_internal.h"

namespace {

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}
__device__ __forceinline__ int32_t wave_min(int32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = min(x, __shfl_xor(x, m, 64));
    return x;
}
__device__ __forceinline__ int32_t wave_max(int32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = max(x, __shfl_xor(x, m, 64));
    return x;
}

/* per-lane sinks of the walk */
struct count_sink {
    osmt_label_extent e;
    uint32_t err;
    int32_t W;
    __device__ void operator()(double x0, double y0, double x1, double y1) {
        if (!osmt_label_seg_in_range(x0, y0, x1, y1)) err |= OSMT_GLYPH_ERR_COORD;
        osmt_label_extent_add(&e, x0, y0, x1, y1, W);
    }
};
struct tally_sink {
    uint32_t n;
    __device__ void operator()(double, double, double, double) { ++n; }
};
struct write_sink {
    double* segs;
    uint32_t at, end;
    uint32_t err;
    __device__ void operator()(double x0, double y0, double x1, double y1) {
        if (at < end) {
            double2* q = reinterpret_cast<double2*>(segs + 4 * (size_t)at);
            q[0] = make_double2(x0, y0);
            q[1] = make_double2(x1, y1);
        } else {
            err |= OSMT_GLYPH_ERR_ARENA;
        }
        ++at;
    }
};

constexpr uint32_t GLYPH_WAVES = 4; /* waves (pairs) per workgroup */

__global__ __launch_bounds__(256) void k_glyph_init(osmt_label_extent* __restrict__ sum, uint32_t n_labels, uint32_t* __restrict__ err) {
    const uint32_t l = blockIdx.x * 256 + threadIdx.x;
    if (l < n_labels) {
        osmt_label_extent e;
        osmt_label_extent_init(&e);
        sum[l] = e;
    }
    if (l == 0) *err = 0u;
}

__global__ __launch_bounds__(256) void k_glyph_count(osmt_glyph_pass a) {
    const uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * GLYPH_WAVES + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= a.n_pairs) return; /* whole wave */
    const osmt_glyph_instance& in = a.inst[a.pair_inst[p]];
    const uint32_t label = a.pair_label[p];
    const uint32_t form = in.form;
    /* OSMT_GLYPH_NONE (a text k_text_place skipped): no call */
    const uint32_t v0 = a.voff[in.glyph_id], nv = form == OSMT_GLYPH_NONE ? 0u : a.voff[in.glyph_id + 1] - v0;
    const double scale = in.scale;
    double prm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) prm[k] = in.p[k];
    count_sink s;
    osmt_label_extent_init(&s.e);
    s.err = 0u;
    s.W = a.W;
    for (uint32_t i = lane; i < nv; i += 64u) s.err |= osmt_glyph_vertex_walk(a.verts + v0, i, scale, form, prm, s);
    const uint32_t n = wave_sum(s.e.n_segs);
    const int32_t ry0 = wave_min(s.e.ry0), ry1 = wave_max(s.e.ry1), cx0 = wave_min(s.e.cx0), cx1 = wave_max(s.e.cx1);
    uint32_t err = s.err;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) err |= __shfl_xor(err, m, 64);
    if (lane == 0) {
        a.pair_cnt[p] = n;
        osmt_label_extent* o = a.sum + label;
        if (n) atomicAdd(&o->n_segs, n);
        if (ry0 <= ry1) {
            atomicMin(&o->ry0, ry0);
            atomicMax(&o->ry1, ry1);
            atomicMin(&o->cx0, cx0);
            atomicMax(&o->cx1, cx1);
        }
        if (err) atomicOr(a.err, err);
    }
}

/* exclusive scan of cnt[0 .. n) in blocks of 1024: out = prefix inside the block, blk[b] = the block's total */
__global__ __launch_bounds__(1024) void k_glyph_scan_blocks(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ blk) {
    __shared__ uint32_t ws[16];
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t v = i < n ? cnt[i] : 0u;
    const uint32_t incl = wave_incl_scan(v, lane);
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    if (w == 0) {
        const uint32_t t = lane < 16 ? ws[lane] : 0u;
        const uint32_t ti = wave_incl_scan(t, lane);
        if (lane < 16) ws[lane] = ti - t;
        if (lane == 15) blk[blockIdx.x] = ti;
    }
    __syncthreads();
    if (i < n) out[i] = ws[w] + incl - v;
}

/* blk[0 .. nb) -> its exclusive scan, one workgroup */
__global__ __launch_bounds__(1024) void k_glyph_scan_top(uint32_t* __restrict__ blk, uint32_t nb) {
    __shared__ uint32_t ws[16];
    __shared__ uint32_t carry;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0u;
    for (uint32_t b0 = 0; b0 < nb; b0 += 1024u) {
        __syncthreads();
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? blk[i] : 0u;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (lane == 63) ws[w] = incl;
        __syncthreads();
        if (w == 0) {
            const uint32_t t = lane < 16 ? ws[lane] : 0u;
            const uint32_t ti = wave_incl_scan(t, lane);
            if (lane < 16) ws[lane] = ti - t;
        }
        __syncthreads();
        const uint32_t c = carry;
        if (i < nb) blk[i] = c + ws[w] + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + ws[w] + incl;
    }
}

__global__ __launch_bounds__(256) void k_glyph_emit(osmt_glyph_pass a) {
    const uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * GLYPH_WAVES + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= a.n_pairs) return;
    const osmt_glyph_instance& in = a.inst[a.pair_inst[p]];
    const uint32_t form = in.form;
    /* OSMT_GLYPH_NONE (a text k_text_place skipped): no call */
    const uint32_t v0 = a.voff[in.glyph_id], nv = form == OSMT_GLYPH_NONE ? 0u : a.voff[in.glyph_id + 1] - v0;
    const double scale = in.scale;
    double prm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) prm[k] = in.p[k];
    uint32_t base = a.pair_base[p] + a.blk[p >> 10];
    uint32_t err = 0u;
    for (uint32_t c0 = 0; c0 < nv; c0 += 64u) {
        const uint32_t i = c0 + lane;
        tally_sink t{0u};
        if (i < nv) (void)osmt_glyph_vertex_walk(a.verts + v0, i, scale, form, prm, t);
        const uint32_t incl = wave_incl_scan(t.n, lane);
        write_sink s{a.segs, base + incl - t.n, a.n_segs, 0u};
        if (i < nv) (void)osmt_glyph_vertex_walk(a.verts + v0, i, scale, form, prm, s);
        err |= s.err;
        base += __shfl(incl, 63, 64);
    }
    if (err) atomicOr(a.err, err);
}

__global__ __launch_bounds__(256) void k_glyph_hypot(const double* __restrict__ xy, uint32_t n, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = osmt_hypot(xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
}

}  // namespace

hipError_t osmt_launch_glyph_count(const osmt_glyph_pass& a, uint32_t n_labels, hipStream_t st) {
    hipLaunchKernelGGL(k_glyph_init, dim3((n_labels + 255) / 256), dim3(256), 0, st, a.sum, n_labels, a.err);
    if (a.n_pairs) hipLaunchKernelGGL(k_glyph_count, dim3((a.n_pairs + GLYPH_WAVES - 1) / GLYPH_WAVES), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_glyph_emit(const osmt_glyph_pass& a, hipStream_t st) {
    if (!a.n_pairs) return hipSuccess;
    const uint32_t nb = (a.n_pairs + 1023) / 1024;
    hipLaunchKernelGGL(k_glyph_scan_blocks, dim3(nb), dim3(1024), 0, st, a.pair_cnt, a.n_pairs, a.pair_base, a.blk);
    hipLaunchKernelGGL(k_glyph_scan_top, dim3(1), dim3(1024), 0, st, a.blk, nb);
    hipLaunchKernelGGL(k_glyph_emit, dim3((a.n_pairs + GLYPH_WAVES - 1) / GLYPH_WAVES), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_hypot(const double* xy, uint32_t n, double* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_glyph_hypot, dim3((n + 255) / 256), dim3(256), 0, st, xy, n, out);
    return hipGetLastError();
}
