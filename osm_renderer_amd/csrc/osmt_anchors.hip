/*
 * osmt_anchors.hip — label anchors from tile coordinates (osmt_label_positions_tiles): what Labelable::get_label_position
 * of a Way or Multipolygon does IN FRONT of the search (draw/labelable.rs:26-68) — nodes_to_points over every node of the
 * area, coords_to_xy_tile_relative(node, tile) * scale, unrounded — for a whole batch of (entity, tile) pairs.  The rings
 * and points it writes are what osmt_launch_polylabel (osmt_polylabel.hip) takes, unchanged.  The host twin, and the
 * yardstick of the tests, is osmt::label_rings_of (host/osmt_labelable.hpp).  gfx950 only.
 *
 * The projection is exact because nothing here calls tan or log: the caller registered per node the two Mercator factors
 * (lon_rad + PI) / (2 PI) and (PI - ln(tan(PI / 4 + lat_rad / 2))) / (2 PI) with ITS libm (tile.rs:88-95), and what is left
 * of coords_to_xy (:96-105) and nodes_to_points is a multiplication by a power of two, one subtraction and one
 * multiplication — each rounds once, as IEEE says, on any machine.  This file is compiled with -ffp-contract=off and keeps
 * the three operations in statements of their own.
 *
 *   k_an_count    one lane per request: the rings and the points of its entity (a way: one ring of its nodes; a multipolygon:
 *                 ALL polygon_count() polygons in file order, the empty and the one-node ones too: labelable.rs:41-59).  The
 *                 point count is kept in 64 bits: the low word goes to the scan, what is above it is added to a word of its own.
 *   (scans)       rings per request, points per request (osmt_tq_scan: 32-bit positions, 64-bit totals).  The host reads the
 *                 totals back and launches nothing below before it has seen them fit 32 bits.
 *   k_an_rings    one lane per (request, ring): the ring's node count, where in geo.idx its nodes start, and its request.
 *   (scan)        points per RING: the rings' point bases.  Rings are in request order and points in ring order, so the base
 *                 of a ring is its first_pt.
 *   k_an_records  one lane per ring: its osmt_ring; one lane per request: its osmt_pl_req (a request without rings too).
 *   k_an_points   one lane per point: its ring by bisection over the point bases, the node index, the node's factors, the
 *                 projected point as one double2.  Consecutive lanes walk along a ring: the index loads and the 16-byte
 *                 stores are contiguous over the wave; the factor loads are a gather of 16-byte records (a way's nodes
 *                 are mostly neighbours in the node table).
 *
 * Every index read here was checked on the host when the tables were registered or the batch was validated; every store
 * lands below a total the arrays were sized with; every buffer is written in full before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;

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

__global__ __launch_bounds__(256) void k_an_count(osmt_an_pass P) {
    const uint32_t q = blockIdx.x * WG + threadIdx.x;
    if (q >= P.n_req) return;
    const uint32_t e = P.req[q].entity;
    const uint32_t id = e & ~OSMT_STYLED_MULTIPOLYGON;
    uint32_t rings = 1u;
    unsigned long long pts = 0ull;
    if (e & OSMT_STYLED_MULTIPOLYGON) {
        const uint32_t k0 = P.geo.mp_off[id], k1 = P.geo.mp_off[id + 1u];
        rings = k1 - k0;
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t p = P.geo.mp_polys[k];
            pts += P.geo.poly_off[p + 1u] - P.geo.poly_off[p];
        }
    } else {
        pts = P.geo.way_off[id + 1u] - P.geo.way_off[id];
    }
    P.rpos[q] = rings;
    P.ppos[q] = (uint32_t)pts;
    if (pts >> 32) atomicAdd(P.tot + OSMT_AN_HIGH, pts & 0xFFFFFFFF00000000ull);
}

__global__ __launch_bounds__(256) void k_an_rings(osmt_an_pass P) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= P.n_rings) return;
    const uint32_t q = owner_of(P.rpos, P.n_req, r);
    const uint32_t e = P.req[q].entity;
    const uint32_t id = e & ~OSMT_STYLED_MULTIPOLYGON;
    uint32_t src, n;
    if (e & OSMT_STYLED_MULTIPOLYGON) {
        const uint32_t p = P.geo.mp_polys[P.geo.mp_off[id] + (r - P.rpos[q])];
        src = P.geo.poly_off[p];
        n = P.geo.poly_off[p + 1u] - src;
    } else {
        src = P.geo.way_off[id];
        n = P.geo.way_off[id + 1u] - src;
    }
    P.ring_base[r] = n;
    P.ring_src[r] = src;
    P.ring_req[r] = q;
}

/* grid: max(n_rings, n_req) lanes */
__global__ __launch_bounds__(256) void k_an_records(osmt_an_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < P.n_rings) {
        const uint32_t b = P.ring_base[i];
        osmt_ring ring;
        ring.first_pt = b;
        ring.n_pts = P.ring_base[i + 1u] - b;
        P.rings[i] = ring;
    }
    if (i < P.n_req) {
        const uint32_t r0 = P.rpos[i];
        osmt_pl_req rq;
        rq.ring_off = r0;
        rq.n_rings = P.rpos[i + 1u] - r0;
        rq.keep_off = r0;
        rq._pad = 0u;
        rq.scale = (double)P.scale;
        P.pl_req[i] = rq;
    }
}

__global__ __launch_bounds__(256) void k_an_points(osmt_an_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_pts) return;
    const uint32_t r = owner_of(P.ring_base, P.n_rings, p);
    const uint32_t node = P.geo.idx[P.ring_src[r] + (p - P.ring_base[r])];
    const osmt_query_tile t = P.tiles[P.req[P.ring_req[r]].tile];
    const double2 f = P.factors[node];
    /* coords_to_xy's rescale (tile.rs:94-98): f64::from(TILE_SIZE * (1 << zoom)) is a power of two <= 2^26 */
    const double dim = (double)(OSMT_TILE_SIZE * (1u << t.zoom));
    const double scale = (double)P.scale;
    /* coords_to_xy_tile_relative (tile.rs:103-106): the offset is formed in u32 as project_point forms it */
    const double off_x = (double)(uint32_t)(t.x * OSMT_TILE_SIZE);
    const double off_y = (double)(uint32_t)(t.y * OSMT_TILE_SIZE);
    double x = f.x * dim;
    double y = f.y * dim;
    x = x - off_x;
    y = y - off_y;
    x = x * scale; /* nodes_to_points (labelable.rs:61-68) */
    y = y * scale;
    P.pts[p] = make_double2(x, y);
}

}  // namespace

hipError_t osmt_launch_an_count(const osmt_an_pass& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.tot, 0, OSMT_AN_N * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_an_count, dim3((a.n_req + WG - 1u) / WG), dim3(WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = osmt_tq_scan(a.rpos, a.n_req, a.blk, a.tot + OSMT_AN_RINGS, st);
    if (e != hipSuccess) return e;
    return osmt_tq_scan(a.ppos, a.n_req, a.blk, a.tot + OSMT_AN_POINTS, st);
}

hipError_t osmt_launch_an_expand(const osmt_an_pass& a, hipStream_t st) {
    if (a.n_rings) {
        hipLaunchKernelGGL(k_an_rings, dim3((a.n_rings + WG - 1u) / WG), dim3(WG), 0, st, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    /* n_rings == 0: the scan still writes ring_base[0] = 0 */
    hipError_t e = osmt_tq_scan(a.ring_base, a.n_rings, a.blk, a.tot + OSMT_AN_RING_POINTS, st);
    if (e != hipSuccess) return e;
    const uint32_t n = a.n_rings > a.n_req ? a.n_rings : a.n_req;
    hipLaunchKernelGGL(k_an_records, dim3((n + WG - 1u) / WG), dim3(WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess || !a.n_pts) return e;
    hipLaunchKernelGGL(k_an_points, dim3((a.n_pts + WG - 1u) / WG), dim3(WG), 0, st, a);
    return hipGetLastError();
}
