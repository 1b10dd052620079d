/*
 * osmt_polygons.hip — multipolygon rings assembled on the device from relations' member ways (osmt_assemble_multipolygons):
 * find_polygons_in_multipolygon (find_polygons.rs) over RawRelation::to_segments (importer.rs:516-537), relation by relation,
 * bit for bit.  The host twin, and the yardstick of the tests, is osmt::assemble_multipolygons_host (host/osmt_polygons.hpp).
 * gfx950 only.
 *
 *   k_mpa_count      one lane per way reference: max(len - 1, 0) segments; the exact 64-bit total is summed per wave and
 *                    added once.  The host reads it back before anything is sized.
 *   k_mpa_reloff     a relation's first segment, from the scanned counts: relations own contiguous segment ranges.
 *   k_mpa_segments   one lane per segment, its way reference by bisection: the two node indices, the relation, and the state
 *                    byte (role | 2: available).  An ENDPOINT is e = 2 * segment + side.
 *   k_mpa_vertices   the vertex of an endpoint is the lowest endpoint OF ITS RELATION at the same (lat, lon) bits.  An
 *                    open-addressing table of endpoints keyed by (relation, bits): atomicCAS into an empty slot, atomicMin on a
 *                    resident of the same relation and bits, otherwise probe on.  atomicMin never changes a resident's key, so
 *                    concurrent probes stay correct and the table's CONTENT is deterministic (which slot holds what is not, and
 *                    nothing reads that).  k_mpa_canon looks every endpoint up and writes the pair (vertex, endpoint).
 *   (sort)           the pyramid's radix sort, unchanged, over those pairs.  Sorted by (vertex, endpoint) a vertex's run IS the
 *                    reference's connection list (order 2 * idx + side).  Because a vertex is an endpoint number of its own
 *                    relation, the sorted pairs of relation r are exactly the slice [2 * first, 2 * end) of the array: a
 *                    relation's whole adjacency is contiguous and relation-local, and
 *                    the head of a run is the entry whose endpoint equals its vertex — no mark / scan is needed to number the
 *                    (vertex, relation) groups, and a stamp is one word per endpoint number.
 *   k_mpa_adjacency  one lane per sorted pair: the entry {endpoint, vertex of the other side}, relation-local, and by endpoint
 *                    where its list starts if it is a vertex (all ones if not).
 *   k_mpa_walk       the hot kernel: one wave per relation, a dependent chain of one step per segment.  A step reads the
 *                    current vertex's list start, then up to 64 entries at once, then per entry the segment's state byte, the
 *                    other side's stamp and whether the entry heads another list; a ballot and its lowest set bit give the
 *                    FIRST usable entry.  The relation's slices are read where they lie, in device memory: staging them in
 *                    LDS was built and measured and bought nothing, so the simpler walk stays.  The walk
 *                    only RECORDS the ring's segments; k_mpa_emit derives the node ids.  Every step consumes one segment; the
 *                    loops carry that bound.
 *   k_mpa_emit       after the scans of (accepted, rings, nodes): one wave per accepted relation.  Per ring 64 segments at a
 *                    time: the lanes load their segments' node pairs, the recurrence "node2 if the last id pushed equals node1,
 *                    else node1" runs over the lanes by shuffles, the store is coalesced.
 *
 * Every store lands below a count its array was sized with; every word is written before it is read.  No kernel here uses
 * scratch (profiles/polygons_kernel_resources.txt).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"
#include "osmt_probe_slots.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t AVAILABLE = 2u;

typedef unsigned long long u64;

/* the smallest i with off[i + 1] > r; off[0] <= r < off[n] */
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

__global__ __launch_bounds__(256) void k_mpa_count(const uint32_t* __restrict__ way_off, const uint32_t* __restrict__ rel_ways, uint32_t n_refs,
                                                   uint32_t* __restrict__ cnt, u64* __restrict__ total) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    u64 c = 0ull;
    if (j < n_refs) {
        const uint32_t w = rel_ways[j], len = way_off[w + 1u] - way_off[w];
        c = len ? len - 1u : 0u;
        cnt[j] = (uint32_t)c;
    }
    for (uint32_t d = 32u; d; d >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)c, d), hi = __shfl_down((uint32_t)(c >> 32), d);
        c += ((u64)hi << 32) | lo; /* lanes beyond the wave give their own value: only lane 0's sum is used */
    }
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(total, c);
}

/* ref_off: scanned, [n_refs + 1] */
__global__ __launch_bounds__(256) void k_mpa_reloff(const uint32_t* __restrict__ ref_off, const uint32_t* __restrict__ rel_way_off, uint32_t n_rels,
                                                    uint32_t* __restrict__ rel_seg) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r <= n_rels) rel_seg[r] = ref_off[rel_way_off[r]];
}

__global__ __launch_bounds__(256) void k_mpa_segments(osmt_mpa_pass P) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= P.n_segs) return;
    const uint32_t j = owner_of(P.ref_off, P.n_refs, s);
    const uint32_t at = P.way_off[P.rel_ways[j]] + (s - P.ref_off[j]);
    P.seg_nodes[2u * s] = P.way_nodes[at];
    P.seg_nodes[2u * s + 1u] = P.way_nodes[at + 1u];
    P.seg_rel[s] = owner_of(P.rel_way_off, P.n_rels, j);
    P.seg_state[s] = (uint8_t)((P.rel_inner[j] & 1u) | AVAILABLE);
}

__global__ __launch_bounds__(256) void k_mpa_fill(uint32_t* __restrict__ a, uint32_t n_minus_1, uint32_t v) {
    const u64 i = (u64)blockIdx.x * WG + threadIdx.x;
    if (i <= (u64)n_minus_1) a[i] = v;
}

__device__ __forceinline__ bool same_vertex(const osmt_mpa_pass& P, uint32_t e, uint32_t rel, ulonglong2 pos) {
    if (P.seg_rel[e >> 1] != rel) return false;
    const ulonglong2 q = P.node_bits[P.seg_nodes[e]];
    return q.x == pos.x && q.y == pos.y;
}

/* the vertex hash and where a probe starts: osmt_probe_slots.h, shared with the host test that counts which probes wrap */
__device__ __forceinline__ uint32_t first_slot(const osmt_mpa_pass& P, ulonglong2 pos, uint32_t rel) {
    return osmt_vertex_first_slot(pos.x, pos.y, rel, P.hash_bits, P.table_mask);
}

/* The table has at least twice as many slots as there are endpoints, so a probe meets an empty slot or its own vertex within
 * table_mask + 1 steps; the loops say so. */
__global__ __launch_bounds__(256) void k_mpa_vertices(osmt_mpa_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= 2u * P.n_segs) return;
    const uint32_t rel = P.seg_rel[e >> 1];
    const ulonglong2 pos = P.node_bits[P.seg_nodes[e]];
    uint32_t slot = first_slot(P, pos, rel);
    for (u64 n = 0; n <= (u64)P.table_mask; ++n) {
        uint32_t cur = __hip_atomic_load(&P.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == NONE) {
            cur = atomicCAS(&P.table[slot], NONE, e);
            if (cur == NONE) return;
        }
        if (same_vertex(P, cur, rel, pos)) {
            atomicMin(&P.table[slot], e);
            return;
        }
        slot = (slot + 1u) & P.table_mask;
    }
}

__global__ __launch_bounds__(256) void k_mpa_canon(osmt_mpa_pass P, u64* __restrict__ key, uint32_t* __restrict__ id) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= 2u * P.n_segs) return;
    const uint32_t rel = P.seg_rel[e >> 1];
    const ulonglong2 pos = P.node_bits[P.seg_nodes[e]];
    uint32_t slot = first_slot(P, pos, rel), v = e;
    for (u64 n = 0; n <= (u64)P.table_mask; ++n) {
        const uint32_t cur = P.table[slot];
        if (cur == NONE) break; /* not reached: k_mpa_vertices entered every endpoint */
        if (same_vertex(P, cur, rel, pos)) {
            v = cur;
            break;
        }
        slot = (slot + 1u) & P.table_mask;
    }
    P.canon[e] = v;
    key[e] = (u64)v;
    id[e] = e;
}

/* key, id: sorted */
__global__ __launch_bounds__(256) void k_mpa_adjacency(osmt_mpa_pass P, const u64* __restrict__ key, const uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= 2u * P.n_segs) return;
    const uint32_t e = id[i], v = (uint32_t)key[i];
    const uint32_t base = 2u * P.rel_seg[P.seg_rel[e >> 1]];
    P.ent[i] = make_uint2(e - base, P.canon[e ^ 1u] - base);
    P.gstart[e] = e == v ? i - base : NONE;
}

/* One relation of S segments, walked by one wave.  ent, gstart, stamp [2 * S], state [S]: the relation's slices; canon
 * [2 * S]: its endpoints' vertices, still with the relation's `base` = 2 * first segment on them; ring_seg [S], ring_end
 * [S / 3].  Lane 0 writes what the next step's lanes read: the barrier of the one-wave workgroup waits for the stores. */
__device__ __forceinline__ void walk_relation(const uint2* __restrict__ ent, const uint32_t* __restrict__ gstart, uint32_t* stamp, uint8_t* state, uint32_t S,
                                              const uint32_t* __restrict__ canon, uint32_t base, uint32_t* __restrict__ ring_seg, uint32_t* __restrict__ ring_end, uint32_t* out_acc,
                                              uint32_t* out_rings, uint32_t* out_unmatched) {
    const uint32_t lane = threadIdx.x & 63u, E = 2u * S;
    uint32_t rings = 0u, unmatched = S, walked = 0u, serial = 0u;
    bool accepted = true;
    for (uint32_t start = 0u; start < S && accepted; ++start) {
        const uint32_t st0 = state[start];
        if (!(st0 & AVAILABLE)) continue;
        ++serial;
        const uint32_t want = st0; /* the start segment's role, available */
        const uint32_t first = canon[2u * start] - base, second = canon[2u * start + 1u] - base; /* one load per ring, off the per-step chain */
        if (lane == 0u) {
            state[start] = (uint8_t)(st0 & 1u);
            stamp[first] = serial;
            stamp[second] = serial;
            ring_seg[walked] = start;
        }
        __syncthreads();
        uint32_t count = 1u, cur = second;
        bool closed = false;
        /* at most S steps: each consumes a segment */
        for (uint32_t budget = S; budget && !closed; --budget) {
            const uint32_t p = gstart[cur];
            uint32_t got_e = NONE, got_o = 0u;
            for (uint32_t at = p; at < E; at += 64u) {
                const uint32_t i = at + lane;
                const bool in = i < E;
                const uint2 en = in ? ent[i] : make_uint2(0u, 0u);
                const bool head = in && i > p && gstart[en.x] == i;
                const bool ok = in && state[en.x >> 1] == want && !(stamp[en.y] == serial && en.y != first);
                const u64 stop = __ballot(!in || head);
                u64 okm = __ballot(ok);
                if (stop) okm &= (1ull << __builtin_ctzll(stop)) - 1ull;
                if (okm) {
                    const int l = __builtin_ctzll(okm);
                    got_e = __shfl(en.x, l);
                    got_o = __shfl(en.y, l);
                    break;
                }
                if (stop) break;
            }
            if (got_e == NONE) break; /* no candidate */
            if (lane == 0u) {
                state[got_e >> 1] = (uint8_t)(want & 1u);
                stamp[got_o] = serial;
                ring_seg[walked + count] = got_e >> 1;
            }
            __syncthreads();
            ++count;
            if (got_o == first)
                closed = true;
            else
                cur = got_o;
        }
        if (!closed || count < 3u) {
            accepted = false;
            break;
        }
        walked += count;
        unmatched -= count;
        if (lane == 0u) ring_end[rings] = walked; /* rings < S / 3: every ring before it took at least 3 segments, and so did this one */
        ++rings;
    }
    *out_acc = accepted ? 1u : 0u;
    *out_rings = rings;
    *out_unmatched = unmatched;
}

__global__ __launch_bounds__(64) void k_mpa_walk(osmt_mpa_pass P) {
    const uint32_t r = blockIdx.y * gridDim.x + blockIdx.x, lane = threadIdx.x;
    if (r >= P.n_rels) return;
    const uint32_t s0 = P.rel_seg[r], S = P.rel_seg[r + 1u] - s0;
    uint32_t acc, rings, unmatched;
    walk_relation(P.ent + 2u * s0, P.gstart + 2u * s0, P.stamp + 2u * s0, P.seg_state + s0, S, P.canon + 2u * s0, 2u * s0, P.ring_seg + s0, P.ring_end + s0 / 3u, &acc, &rings,
                  &unmatched);
    if (lane == 0u) {
        osmt_relation_status s;
        s.accepted = acc, s.rings_built = rings, s.unmatched = unmatched;
        P.status[r] = s;
        P.rel_acc[r] = acc;
        P.rel_rings[r] = acc ? rings : 0u;
        P.rel_nodes[r] = acc ? S + rings : 0u; /* an accepted relation's rings hold every segment once, and one id more each */
    }
}

/* rel_acc, rel_rings, rel_nodes: scanned.  Block n_rels writes the closing offsets. */
__global__ __launch_bounds__(64) void k_mpa_emit(osmt_mpa_pass P) {
    const uint32_t r = blockIdx.y * gridDim.x + blockIdx.x, lane = threadIdx.x;
    if (r > P.n_rels) return;
    const uint32_t m = P.rel_acc[r], pb = P.rel_rings[r], nb = P.rel_nodes[r];
    if (r == P.n_rels) {
        if (lane == 0u) P.mp_poly_off[m] = pb, P.poly_node_off[pb] = nb;
        return;
    }
    if (P.rel_acc[r + 1u] == m) return; /* rejected */
    const uint32_t rings = P.rel_rings[r + 1u] - pb, s0 = P.rel_seg[r];
    if (lane == 0u) P.mp_ids[m] = P.rel_ids[r], P.mp_rel[m] = r, P.mp_poly_off[m] = pb;
    for (uint32_t k = lane; k < rings; k += 64u) P.mp_polys[pb + k] = pb + k;
    const uint32_t* ring_end = P.ring_end + s0 / 3u;
    for (uint32_t k = 0u; k < rings; ++k) {
        const uint32_t b = k ? ring_end[k - 1u] : 0u, e = ring_end[k];
        const uint32_t out = nb + b + k; /* k rings before it: one id more each */
        if (lane == 0u) P.poly_node_off[pb + k] = out;
        uint32_t last = 0u;
        for (uint32_t c = b; c < e; c += 64u) {
            const uint32_t n = e - c < 64u ? e - c : 64u;
            uint32_t n1 = 0u, n2 = 0u;
            if (lane < n) {
                const uint32_t s = s0 + P.ring_seg[s0 + c + lane];
                n1 = P.seg_nodes[2u * s], n2 = P.seg_nodes[2u * s + 1u];
            }
            if (c == b) {
                last = __shfl(n1, 0);
                if (lane == 0u) P.poly_nodes[out] = last;
            }
            uint32_t mine = 0u;
            for (uint32_t j = 0u; j < n; ++j) {
                const uint32_t x = __shfl(n1, (int)j), y = __shfl(n2, (int)j);
                last = last == x ? y : x;
                if (lane == j) mine = last;
            }
            if (lane < n) P.poly_nodes[out + 1u + (c - b) + lane] = mine;
        }
    }
}

/* one block per relation; n < 2^31 */
inline dim3 rel_grid(uint32_t n) { return n <= 65536u ? dim3(n) : dim3(65536u, (n + 65535u) / 65536u); }

inline dim3 grid_of(u64 n) { return dim3((uint32_t)((n + WG - 1u) / WG)); }

}  // namespace

hipError_t osmt_launch_mpa_count(const osmt_mpa_pass& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.words, 0, OSMT_MPA_WORDS * 8u, st);
    if (e != hipSuccess) return e;
    if (a.n_refs) hipLaunchKernelGGL(k_mpa_count, grid_of(a.n_refs), dim3(WG), 0, st, a.way_off, a.rel_ways, a.n_refs, a.ref_off, a.words + OSMT_MPA_SEGMENTS);
    e = osmt_tq_scan(a.ref_off, a.n_refs, a.blk, a.words + OSMT_MPA_SCAN, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mpa_reloff, grid_of((u64)a.n_rels + 1u), dim3(WG), 0, st, a.ref_off, a.rel_way_off, a.n_rels, a.rel_seg);
    return hipGetLastError();
}

hipError_t osmt_launch_mpa_vertices(const osmt_mpa_pass& a, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (!a.n_segs) return hipSuccess;
    hipLaunchKernelGGL(k_mpa_segments, grid_of(a.n_segs), dim3(WG), 0, st, a);
    hipLaunchKernelGGL(k_mpa_fill, grid_of((u64)a.table_mask + 1u), dim3(WG), 0, st, a.table, a.table_mask, NONE);
    hipLaunchKernelGGL(k_mpa_vertices, grid_of(2ull * a.n_segs), dim3(WG), 0, st, a);
    hipLaunchKernelGGL(k_mpa_canon, grid_of(2ull * a.n_segs), dim3(WG), 0, st, a, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_mpa_walk(const osmt_mpa_pass& a, const unsigned long long* key, const uint32_t* id, hipStream_t st) {
    if (a.n_segs) {
        hipLaunchKernelGGL(k_mpa_adjacency, grid_of(2ull * a.n_segs), dim3(WG), 0, st, a, key, id);
        const hipError_t e = hipMemsetAsync(a.stamp, 0, 8ull * a.n_segs, st);
        if (e != hipSuccess) return e;
    }
    if (a.n_rels) hipLaunchKernelGGL(k_mpa_walk, rel_grid(a.n_rels), dim3(64), 0, st, a);
    hipError_t e = osmt_tq_scan(a.rel_acc, a.n_rels, a.blk, a.words + OSMT_MPA_MPS, st);
    if (e == hipSuccess) e = osmt_tq_scan(a.rel_rings, a.n_rels, a.blk, a.words + OSMT_MPA_POLYS, st);
    if (e == hipSuccess) e = osmt_tq_scan(a.rel_nodes, a.n_rels, a.blk, a.words + OSMT_MPA_NODES, st);
    return e;
}

hipError_t osmt_launch_mpa_emit(const osmt_mpa_pass& a, hipStream_t st) {
    hipLaunchKernelGGL(k_mpa_emit, rel_grid(a.n_rels + 1u), dim3(64), 0, st, a);
    return hipGetLastError();
}
