/*
 * osmt_polylabel.hip — label anchors (osmt_label_positions): Labelable::get_label_position of the reference for ways and
 * multipolygons (src/draw/labelable.rs:191-204: filter_polygons, the bounding box, the centroid and the "polylabel" search
 * of :125-189) on the GPU, one wave per request, bit for bit.  gfx950 only; -ffp-contract=off: every f64 operation is the
 * reference's, in its association (host statement of the same function: host/osmt_labelable.hpp).
 *
 * What runs in parallel and why it may:
 *   - the signed distance of a point to the rings (point_to_polygon_dist, :296-311).  Per edge the crossing test and
 *     segment_dist_sq are independent; the parity is an XOR and the minimum is taken over values that are never NaN
 *     (squares of finite numbers; a NaN `t` only fails both of its comparisons), so both reductions are order-free.
 *     The wave works on FOUR points at a time, one per 16-lane row: lane (row, sub) takes edges sub, sub + 16, ... of
 *     every kept ring for the point of its row; four xor-shuffles inside the row and one ballot finish it.  The four
 *     children of a popped cell are such a group of four (most labelled polygons are buildings of 5 .. 20 edges: a wave
 *     per cell would idle 50 lanes), so are four consecutive cells of the initial grid and four points of a ring under
 *     filter_polygons' inside test.  The row count of passes over E edges, ceil(E / 16), is never more than the
 *     4 * ceil(E / 64) of four whole-wave passes, so large rings take the same path.
 *   - the per-edge products of the area and centroid sums; the ADDITIONS are made by every lane in edge order (the
 *     products are handed round with v_readlane), because their order changes bits.
 * What is serial per request, exactly as the reference runs it: the grid walk (x += cell_size in f64, x outer, y inner),
 * the first best cell at the centroid with half = 0, the pop order, the strict `>` for a new best, the stop rule against
 * the best fitness SO FAR, the four children in dx-outer, dy-inner order.
 *
 * The queue is std::collections::BinaryHeap<Cell> restated (Rust std 1.70 .. 1.80, library/alloc/src/collections/
 * binary_heap/mod.rs; the reference's Ord compares max_fitness alone and calls unordered pairs equal, :99-119, so std's
 * `a <= b` is !(a.key > b.key)):
 *   push            append, then sift_up(0, last): the element climbs while it is NOT <= its parent;
 *   pop             the last element replaces the root, then sift_down_to_bottom(0): the hole walks to the bottom, taking
 *                   the RIGHT child when left <= right, takes a lone last child, and the element sifts up from there.
 * Equal keys are the rule for symmetric shapes, and another tie order returns the mirrored position there.  Heap moves are
 * uniform over the wave (every lane makes the same loads and stores) and tiny next to the distance passes.
 *
 * Two tiers.  k_polylabel keeps the queue of a request in LDS (PL_LDS_CELLS cells per wave).  A request whose queue
 * outgrows it is abandoned there and put on a list; k_polylabel_big — launched behind it with a fixed number of waves, no
 * host round trip — runs the listed requests again from the start with a queue of OSMT_PL_GLOBAL_CELLS cells in device
 * memory.  A request is answered OSMT_LABEL_TOO_LARGE exactly when a push would make the queue hold more than
 * OSMT_LABEL_MAX_CELLS cells or when more than OSMT_LABEL_MAX_CELLS cells would be popped, so neither the initial grid of
 * a degenerate strip (ceil(w / c) * ceil(h / c) cells) nor the search can run away.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t PL_WAVES = 4;       /* requests (waves) per workgroup of k_polylabel */
constexpr uint32_t PL_LDS_CELLS = 256; /* queue cells per wave in LDS */
constexpr uint32_t PL_WG_PER_CU = 3;   /* workgroups of k_polylabel meant to share a CU */
static_assert(PL_WAVES * PL_LDS_CELLS * OSMT_PL_CELL_DOUBLES * sizeof(double) <= 160u * 1024u / PL_WG_PER_CU,
              "the LDS queues of k_polylabel must leave room for PL_WG_PER_CU workgroups per CU (160 KB)");

enum : uint32_t { PL_DONE = 0u, PL_QUEUE_FULL = 1u, PL_POP_CAP = 2u, PL_INTERNAL = 3u };
/* Loops that are bounded by construction carry a bound of their own all the same (a kernel on a shared machine): a wave
 * that passes one stops and reports OSMT_PL_ERR_* through cnt[3]; the host turns it into OSMT_HIP_ERROR. */

struct pl_cell {
    double cx, cy, half, fit, maxfit;
};

/* the value lane `src` holds, in every lane (src uniform): two v_readlane_b32 */
__device__ __forceinline__ double bcast(double v, uint32_t src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), (int)src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), (int)src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint32_t bcast_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

/* a binary max-heap of cells in structure-of-arrays form: field f of cell i at d[f * cap + i] (LDS or device memory) */
struct pl_heap {
    double* d;
    uint32_t cap, n;
    uint32_t err;
    __device__ __forceinline__ double key(uint32_t i) const { return d[4u * cap + i]; }
    __device__ __forceinline__ void move(uint32_t to, uint32_t from) {
#pragma unroll
        for (uint32_t f = 0; f < OSMT_PL_CELL_DOUBLES; ++f) d[f * cap + to] = d[f * cap + from];
    }
    __device__ __forceinline__ void put(uint32_t i, const pl_cell& c) {
        d[i] = c.cx;
        d[cap + i] = c.cy;
        d[2u * cap + i] = c.half;
        d[3u * cap + i] = c.fit;
        d[4u * cap + i] = c.maxfit;
    }
    __device__ __forceinline__ pl_cell get(uint32_t i) const { return {d[i], d[cap + i], d[2u * cap + i], d[3u * cap + i], d[4u * cap + i]}; }
    /* sift_up(0, pos) of the element e (not yet stored) */
    __device__ __forceinline__ void sift_up(uint32_t pos, const pl_cell& e) {
        uint32_t levels = 0u;
        while (pos > 0u) {
            if (++levels > 40u) {
                err |= OSMT_PL_ERR_HEAP;
                break;
            }
            const uint32_t parent = (pos - 1u) >> 1;
            if (!(e.maxfit > key(parent))) break; /* e <= parent */
            move(pos, parent);
            pos = parent;
        }
        put(pos, e);
    }
    __device__ __forceinline__ bool push(const pl_cell& c) {
        if (n >= cap) return false;
        sift_up(n, c);
        ++n;
        return true;
    }
    __device__ __forceinline__ pl_cell pop() { /* n > 0 */
        --n;
        const pl_cell last = get(n);
        if (n == 0u) return last;
        const pl_cell top = get(0u);
        uint32_t pos = 0u, child = 1u, levels = 0u;
        while (child + 1u < n) {
            if (++levels > 40u) {
                err |= OSMT_PL_ERR_HEAP;
                break;
            }
            child += !(key(child) > key(child + 1u)) ? 1u : 0u; /* left <= right: the right one */
            move(pos, child);
            pos = child;
            child = 2u * pos + 1u;
        }
        if (child + 1u == n) {
            move(pos, child);
            pos = child;
        }
        sift_up(pos, last);
        return top;
    }
};

struct pl_geom {
    const osmt_ring* rings;
    const double2* pts;
    const uint32_t* keep; /* the request's kept rings (absolute ring indices), keep[0] = the largest */
    uint32_t n_keep;
    uint32_t first0, n0; /* ring keep[0] */
    uint32_t n_rings_total;
    uint32_t err;
};

/* point_to_polygon_dist of (px, py) — the point of this lane's 16-lane row — to the first n_keep kept rings; every lane of
 * the row returns the row's value */
__device__ __forceinline__ double dist_rows(double px, double py, pl_geom& g, uint32_t n_keep, uint32_t lane) {
    const uint32_t sub = lane & 15u;
    bool inside = false;
    double m = __longlong_as_double(0x7FF0000000000000ll);
    for (uint32_t k = 0; k < n_keep; ++k) {
        uint32_t first = g.first0, n = g.n0;
        if (k) {
            const uint32_t ri = g.keep[k];
            if (ri >= g.n_rings_total) {
                g.err |= OSMT_PL_ERR_KEEP;
                break;
            }
            const osmt_ring r = g.rings[ri];
            first = r.first_pt;
            n = r.n_pts;
        }
        for (uint32_t i = 1u + sub; i < n; i += 16u) {
            const double2 a = g.pts[first + i], b = g.pts[first + i - 1u];
            if ((a.y > py) != (b.y > py) && (px < (b.x - a.x) * (py - a.y) / (b.y - a.y) + a.x)) inside = !inside;
            /* segment_dist_sq(point, a, b) */
            double x = a.x, y = a.y;
            double dx = b.x - x, dy = b.y - y;
            if (dx != 0.0 || dy != 0.0) {
                const double t = ((px - x) * dx + (py - y) * dy) / (dx * dx + dy * dy);
                if (t > 1.0) {
                    x = b.x;
                    y = b.y;
                } else if (t > 0.0) {
                    x += dx * t;
                    y += dy * t;
                }
            }
            dx = px - x;
            dy = py - y;
            const double d = dx * dx + dy * dy;
            m = d < m ? d : m;
        }
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) {
        const double o = __shfl_xor(m, s, 64);
        m = o < m ? o : m;
    }
    const unsigned long long bal = __ballot(inside);
    const uint32_t odd = (uint32_t)__popcll((bal >> (lane & 48u)) & 0xFFFFull) & 1u;
    return (odd ? 1.0 : -1.0) * sqrt(m);
}

struct pl_shape {
    double cen_x, cen_y, max_size;
};

__device__ __forceinline__ double fitness(const pl_shape& s, double cx, double cy, double d) {
    if (d <= 0.0) return d;
    const double dx = cx - s.cen_x, dy = cy - s.cen_y;
    return d * (1.0 - sqrt(dx * dx + dy * dy) / s.max_size);
}

/* Cell::new for the point of this lane's row */
__device__ __forceinline__ pl_cell cell_rows(pl_geom& g, const pl_shape& s, double cx, double cy, double half, uint32_t lane) {
    const double d = dist_rows(cx, cy, g, g.n_keep, lane);
    const double dmax = d + half * 1.4142135623730951; /* std::f64::consts::SQRT_2 */
    return {cx, cy, half, fitness(s, cx, cy, d), fitness(s, cx, cy, dmax)};
}

__device__ __forceinline__ pl_cell cell_of_row(const pl_cell& c, uint32_t row) {
    return {bcast(c.cx, 16u * row), bcast(c.cy, 16u * row), bcast(c.half, 16u * row), bcast(c.fit, 16u * row), bcast(c.maxfit, 16u * row)};
}

/* sum of cross products of a ring in edge order (get_polygon_area before .abs()): products by the lanes, additions in order */
__device__ __forceinline__ double ring_area(const double2* pts, uint32_t first, uint32_t n, uint32_t lane) {
    double s = 0.0;
    for (uint32_t base = 1u; base < n; base += 64u) {
        const uint32_t i = base + lane;
        double c = 0.0;
        if (i < n) {
            const double2 a = pts[first + i], b = pts[first + i - 1u];
            c = a.x * b.y - b.x * a.y;
        }
        const uint32_t cnt = min(64u, n - base);
        for (uint32_t j = 0; j < cnt; ++j) s += bcast(c, j);
    }
    return fabs(s);
}

/* the whole of get_label_position for one request; every value that steers control flow is uniform over the wave */
__device__ __forceinline__ uint32_t label_position(const osmt_polylabel_args& a, uint32_t r, pl_heap& heap, uint32_t lane, double* out_x,
                                                   double* out_y, uint32_t* err) {
    const osmt_pl_req rq = a.req[r];
    const uint32_t row = lane >> 4;
    *out_x = 0.0;
    *out_y = 0.0;
    /* (n_rings == 0 and an empty first ring were answered OSMT_LABEL_NONE by the caller) */

    /* filter_polygons: the first ring of the largest area */
    uint32_t largest = 0u;
    {
        const osmt_ring r0 = a.rings[rq.ring_off];
        double largest_area = ring_area(a.pts, r0.first_pt, r0.n_pts, lane);
        for (uint32_t i = 1u; i < rq.n_rings; ++i) {
            const osmt_ring ri = a.rings[rq.ring_off + i];
            const double ar = ring_area(a.pts, ri.first_pt, ri.n_pts, lane);
            if (ar > largest_area) {
                largest = i;
                largest_area = ar;
            }
        }
    }
    pl_geom g;
    g.rings = a.rings;
    g.pts = a.pts;
    g.n_rings_total = a.n_rings;
    g.err = 0u;
    uint32_t* keep = a.keep + rq.keep_off;
    g.keep = keep;
    {
        const osmt_ring rl = a.rings[rq.ring_off + largest];
        g.first0 = rl.first_pt;
        g.n0 = rl.n_pts;
    }
    /* every lane stores the same word and later reads back what it stored itself */
    keep[0] = rq.ring_off + largest;
    uint32_t n_keep = 1u;
    for (uint32_t i = 0u; i < rq.n_rings; ++i) {
        if (i == largest) continue;
        const osmt_ring ri = a.rings[rq.ring_off + i];
        bool all = true;
        for (uint32_t base = 0u; base < ri.n_pts; base += 4u) {
            const uint32_t k = base + row;
            const bool valid = k < ri.n_pts;
            const double2 p = a.pts[ri.first_pt + (valid ? k : base)];
            const double d = dist_rows(p.x, p.y, g, 1u, lane);
            if (__ballot(valid && !(d >= 0.0)) != 0ull) {
                all = false;
                break;
            }
        }
        if (all) keep[n_keep++] = rq.ring_off + i;
    }
    g.n_keep = n_keep;

    /* get_bounding_box of the leading ring: min / max are order-free except for the sign of a zero minimum, which is the
     * first zero coordinate's in point order (host/osmt_labelable.hpp) */
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double min_x = inf, max_x = -inf, min_y = inf, max_y = -inf;
    for (uint32_t i = lane; i < g.n0; i += 64u) {
        const double2 p = a.pts[g.first0 + i];
        min_x = p.x < min_x ? p.x : min_x;
        max_x = p.x > max_x ? p.x : max_x;
        min_y = p.y < min_y ? p.y : min_y;
        max_y = p.y > max_y ? p.y : max_y;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ax = __shfl_xor(min_x, s, 64), bx = __shfl_xor(max_x, s, 64), ay = __shfl_xor(min_y, s, 64), by = __shfl_xor(max_y, s, 64);
        min_x = ax < min_x ? ax : min_x;
        max_x = bx > max_x ? bx : max_x;
        min_y = ay < min_y ? ay : min_y;
        max_y = by > max_y ? by : max_y;
    }
    min_x = bcast(min_x, 0u);
    max_x = bcast(max_x, 0u);
    min_y = bcast(min_y, 0u);
    max_y = bcast(max_y, 0u);
    if (min_x == 0.0 || min_y == 0.0) {
        bool seen_x = !(min_x == 0.0), seen_y = !(min_y == 0.0);
        for (uint32_t i = 0u; i < g.n0 && !(seen_x && seen_y); ++i) {
            const double2 p = a.pts[g.first0 + i];
            if (!seen_x && p.x == 0.0) {
                min_x = p.x;
                seen_x = true;
            }
            if (!seen_y && p.y == 0.0) {
                min_y = p.y;
                seen_y = true;
            }
        }
    }
    const double w = max_x - min_x, h = max_y - min_y;
    const double precision = (w > h ? w : h) / 100.0 * rq.scale;
    const double cell_size = w < h ? w : h;
    pl_shape s;
    s.max_size = w > h ? w : h;
    if (cell_size == 0.0) {
        *out_x = min_x;
        *out_y = min_y;
        return PL_DONE;
    }

    /* get_centroid */
    {
        double area = 0.0, sx = 0.0, sy = 0.0;
        for (uint32_t base = 1u; base < g.n0; base += 64u) {
            const uint32_t i = base + lane;
            double tx = 0.0, ty = 0.0, ta = 0.0;
            if (i < g.n0) {
                const double2 pa = a.pts[g.first0 + i], pb = a.pts[g.first0 + i - 1u];
                const double c = pa.x * pb.y - pb.x * pa.y;
                tx = (pa.x + pb.x) * c;
                ty = (pa.y + pb.y) * c;
                ta = c * 3.0;
            }
            const uint32_t cnt = min(64u, g.n0 - base);
            for (uint32_t j = 0; j < cnt; ++j) {
                sx += bcast(tx, j);
                sy += bcast(ty, j);
                area += bcast(ta, j);
            }
        }
        const double2 p0 = a.pts[g.first0];
        s.cen_x = area == 0.0 ? p0.x : sx / area;
        s.cen_y = area == 0.0 ? p0.y : sy / area;
    }

    /* the initial grid, four cells at a time */
    heap.n = 0u;
    double half = cell_size / 2.0;
    {
        double qx = 0.0, qy = 0.0; /* the pending point of this lane's row */
        uint32_t pending = 0u, walked = 0u;
        for (double x = min_x; x < max_x; x += cell_size) {
            for (double y = min_y; y < max_y; y += cell_size) {
                if (++walked > OSMT_LABEL_MAX_CELLS + 8u) {
                    *err |= OSMT_PL_ERR_GRID;
                    return PL_INTERNAL;
                }
                if (row == pending || pending == 0u) { /* unused rows repeat the first pending point */
                    qx = x + half;
                    qy = y + half;
                }
                if (++pending == 4u) {
                    const pl_cell c = cell_rows(g, s, qx, qy, half, lane);
                    for (uint32_t k = 0; k < 4u; ++k)
                        if (!heap.push(cell_of_row(c, k))) return PL_QUEUE_FULL;
                    pending = 0u;
                }
            }
        }
        if (pending) {
            const pl_cell c = cell_rows(g, s, qx, qy, half, lane);
            for (uint32_t k = 0; k < pending; ++k)
                if (!heap.push(cell_of_row(c, k))) return PL_QUEUE_FULL;
        }
    }

    pl_cell best = cell_of_row(cell_rows(g, s, s.cen_x, s.cen_y, 0.0, lane), 0u);
    uint32_t pops = 0u;
    while (heap.n > 0u) {
        if (pops >= OSMT_LABEL_MAX_CELLS) return PL_POP_CAP;
        if (g.err | heap.err) {
            *err |= g.err | heap.err;
            return PL_INTERNAL;
        }
        const pl_cell cur = heap.pop();
        ++pops;
        if (cur.fit > best.fit) best = cur;
        if (cur.maxfit - best.fit <= precision) continue;
        half = cur.half / 2.0;
        /* child k = 2 * (dx > 0) + (dy > 0): dx outer, dy inner; row k evaluates child k */
        const double ccx = cur.cx + ((row & 2u) ? half : -half), ccy = cur.cy + ((row & 1u) ? half : -half);
        const pl_cell c = cell_rows(g, s, ccx, ccy, half, lane);
        for (uint32_t k = 0; k < 4u; ++k)
            if (!heap.push(cell_of_row(c, k))) return PL_QUEUE_FULL;
    }
    *err |= g.err | heap.err;
    if (*err) return PL_INTERNAL;
    *out_x = best.cx;
    *out_y = best.cy;
    return PL_DONE;
}

__device__ __forceinline__ void write_out(const osmt_polylabel_args& a, uint32_t r, uint32_t status, double x, double y, uint32_t lane) {
    if (lane == 0u) {
        osmt_label_position o;
        o.x = x;
        o.y = y;
        o.status = status;
        o._pad = 0u;
        a.out[r] = o;
    }
}

__global__ __launch_bounds__(64 * PL_WAVES) void k_polylabel(osmt_polylabel_args a) {
    __shared__ double lds[PL_WAVES][OSMT_PL_CELL_DOUBLES * PL_LDS_CELLS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t r = bcast_u32(blockIdx.x * PL_WAVES + wv);
    if (r >= a.n_req) return; /* whole wave; the kernel has no barrier */
    const osmt_pl_req rq = a.req[r];
    if (rq.n_rings == 0u || a.rings[rq.ring_off].n_pts == 0u) {
        write_out(a, r, OSMT_LABEL_NONE, 0.0, 0.0, lane);
        return;
    }
    pl_heap heap{lds[wv], PL_LDS_CELLS, 0u, 0u};
    double x, y;
    uint32_t err = 0u;
    const uint32_t rc = label_position(a, r, heap, lane, &x, &y, &err);
    if (rc == PL_INTERNAL) {
        if (lane == 0u) atomicOr(&a.cnt[3], err | OSMT_PL_ERR_TIER1);
        write_out(a, r, OSMT_LABEL_TOO_LARGE, 0.0, 0.0, lane);
        return;
    }
    if (rc == PL_QUEUE_FULL) {
        if (lane == 0u) a.over[atomicAdd(&a.cnt[0], 1u)] = r;
        return;
    }
    if (rc == PL_POP_CAP && lane == 0u) atomicAdd(&a.cnt[2], 1u);
    write_out(a, r, rc == PL_DONE ? OSMT_LABEL_OK : OSMT_LABEL_TOO_LARGE, x, y, lane);
}

/* second tier: wave b owns queue slot b and takes listed requests until the list is empty */
__global__ __launch_bounds__(64) void k_polylabel_big(osmt_polylabel_args a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t n_over = min(a.cnt[0], a.n_req);
    pl_heap heap{a.ws + (size_t)blockIdx.x * OSMT_PL_CELL_DOUBLES * OSMT_PL_GLOBAL_CELLS, OSMT_PL_GLOBAL_CELLS, 0u, 0u};
    for (uint32_t round = 0u;; ++round) {
        if (round > a.n_req) {
            if (lane == 0u) atomicOr(&a.cnt[3], OSMT_PL_ERR_LIST);
            return;
        }
        uint32_t i = 0u;
        if (lane == 0u) i = atomicAdd(&a.cnt[1], 1u);
        i = bcast_u32(i);
        if (i >= n_over) return;
        const uint32_t r = bcast_u32(a.over[i]);
        if (r >= a.n_req) return; /* cannot happen: k_polylabel wrote the list */
        double x, y;
        uint32_t err = 0u;
        const uint32_t rc = label_position(a, r, heap, lane, &x, &y, &err);
        if (rc == PL_INTERNAL && lane == 0u) atomicOr(&a.cnt[3], err | OSMT_PL_ERR_TIER2);
        if (rc != PL_DONE && rc != PL_INTERNAL && lane == 0u) atomicAdd(&a.cnt[2], 1u);
        write_out(a, r, rc == PL_DONE ? OSMT_LABEL_OK : OSMT_LABEL_TOO_LARGE, rc == PL_DONE ? x : 0.0, rc == PL_DONE ? y : 0.0, lane);
    }
}

}  // namespace

hipError_t osmt_launch_polylabel(const osmt_polylabel_args& a, hipStream_t st) {
    if (!a.n_req) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.cnt, 0, 4 * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_polylabel, dim3((a.n_req + PL_WAVES - 1) / PL_WAVES), dim3(64 * PL_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_polylabel_big, dim3(a.n_slots), dim3(64), 0, st, a);
    return hipGetLastError();
}
