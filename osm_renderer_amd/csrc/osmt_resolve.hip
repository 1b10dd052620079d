/*
 * osmt_resolve.hip — OSM ids resolved on the device (osmt_resolve_refs): OsmEntityStorage::translate_id
 * (importer.rs:45-71), the silent drop of references that do not resolve (importer.rs:365-400) and postprocess_node_refs
 * (importer.rs:334-353).  The host twin, and the yardstick of the tests, is osmt::resolve_refs_host (host/osmt_resolve.hpp).
 * gfx950 only.
 *
 *   (id tables)      (key = global id, id = index) of the nodes, and of the ways, sorted by the pyramid's radix sort on the
 *                    key's bytes alone (k_pyr_keydigits, osmt_launch_pyr_pass): the indices go in ascending and the sort is
 *                    stable, so equal ids stay in index order without a pass over the index.
 *   k_res_translate  one lane per reference: its owner by bisection over the offsets, then the LAST table entry <=
 *                    (g, seen - 1) by bisection; it resolves iff that entry's key is g.  The largest index below `seen` wins:
 *                    HashMap::insert overwrites, and an element not yet read does not exist.
 *   k_res_compact    after the scan of the resolved flags: the references that resolved, in order, with their role bytes; an
 *                    owner's new offset is the scan at its old one.  One kernel family serves ways and relations.
 *   k_res_short      the dedup of a way of up to short_max resolved references: one wave per way, an open-addressing table in
 *                    LDS keyed by the unordered pair (min << 32 | max, never all ones: an index is below 2^32 - 1).
 *                    ds atomicCAS claims a slot for a pair, ds atomicMin leaves the lowest position of the pair in it; after
 *                    the barrier position idx is kept iff it is that lowest position.  Which slot holds what depends on the
 *                    lanes' order; what a pair's slot holds does not.  A way of n references has n - 1 pairs and a table of at
 *                    least 2 (n - 1) slots, so a probe ends within the table; the loops say so.
 *   k_res_longcount  one lane per way: position 0 of a longer way is kept, its other positions are pairs for the sort.
 *   k_res_longpairs  one lane per such pair: (min << 32 | max, position).  Positions ascend by way, so after ONE stable sort on
 *                    the key equal keys stand grouped by way, lowest position first.
 *   k_res_longmark   one lane per sorted pair: kept iff its predecessor differs in key or in owning way.
 *   k_res_emit       after the scan of the kept flags: the kept references and the ways' offsets.
 *
 * "Kept iff first occurrence of the unordered pair in its way" IS the importer's running HashSet.
 * Every store lands below a count its array was sized with; every word is written before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"
#include "osmt_probe_slots.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t NONE = 0xFFFFFFFFu;

typedef unsigned long long u64;

constexpr u64 EMPTY = ~0ull;

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

__global__ __launch_bounds__(256) void k_res_iota(uint32_t* __restrict__ id, uint32_t n) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) id[i] = i;
}

__global__ __launch_bounds__(256) void k_res_translate(osmt_res_refs A) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= A.n_refs) return;
    const u64 g = A.refs[r];
    const uint32_t lim = A.seen ? A.seen[owner_of(A.off, A.n_owners, r)] : A.n_table;
    uint32_t found = NONE;
    if (lim) {
        /* how many entries are <= (g, lim - 1) */
        uint32_t lo = 0u, hi = A.n_table;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const u64 k = A.table_key[mid];
            if (k < g || (k == g && A.table_id[mid] < lim))
                lo = mid + 1u;
            else
                hi = mid;
        }
        if (lo && A.table_key[lo - 1u] == g) found = A.table_id[lo - 1u];
    }
    A.local[r] = found;
    A.pos[r] = found != NONE ? 1u : 0u;
}

/* pos: scanned, [n_refs + 1].  Lanes [0, n_refs): the references; lanes [0, n_owners]: the offsets. */
__global__ __launch_bounds__(256) void k_res_compact(osmt_res_refs A) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r < A.n_refs) {
        const uint32_t p = A.pos[r];
        if (A.pos[r + 1u] != p) {
            A.out_local[p] = A.local[r];
            if (A.role) A.out_role[p] = A.role[r];
        }
    }
    if (r <= A.n_owners) A.out_off[r] = A.pos[A.off[r]];
}

/* the pair key, its hash and a way's table size: osmt_probe_slots.h, shared with the host test that counts which probes wrap */
__device__ __forceinline__ u64 pair_key(uint32_t a, uint32_t b) { return osmt_pair_key(a, b); }

__device__ __forceinline__ uint32_t hash_of(u64 k) { return osmt_pair_hash(k); }

/* One wave per way.  lds: tkey [slots_cap] then tpos [slots_cap], slots_cap a power of two >= 2 * short_max. */
__global__ __launch_bounds__(64) void k_res_short(osmt_res_dedup A, uint32_t slots_cap) {
    extern __shared__ u64 lds[];
    u64* tkey = lds;
    uint32_t* tpos = (uint32_t*)(lds + slots_cap);
    const uint32_t w = blockIdx.y * gridDim.x + blockIdx.x, lane = threadIdx.x;
    if (w >= A.n_ways) return;
    const uint32_t b = A.off[w], len = A.off[w + 1u] - b;
    if (len == 0u || len > A.short_max) return; /* uniform over the workgroup */
    if (len <= 2u) { /* nothing to compare */
        if (lane < len) A.keep[b + lane] = 1u;
        return;
    }
    const uint32_t slots = osmt_pair_slots(len); /* <= slots_cap: len <= short_max */
    const uint32_t mask = slots - 1u;
    for (uint32_t s = lane; s < slots; s += 64u) tkey[s] = EMPTY, tpos[s] = NONE;
    __syncthreads();
    for (uint32_t i = 1u + lane; i < len; i += 64u) {
        const u64 k = pair_key(A.refs[b + i - 1u], A.refs[b + i]);
        uint32_t slot = hash_of(k) & mask;
        for (uint32_t n = 0u; n < slots; ++n) {
            const u64 cur = atomicCAS(&tkey[slot], EMPTY, k);
            if (cur == EMPTY || cur == k) {
                atomicMin(&tpos[slot], i);
                break;
            }
            slot = (slot + 1u) & mask;
        }
    }
    __syncthreads();
    if (lane == 0u) A.keep[b] = 1u;
    for (uint32_t i = 1u + lane; i < len; i += 64u) {
        const u64 k = pair_key(A.refs[b + i - 1u], A.refs[b + i]);
        uint32_t slot = hash_of(k) & mask, first = i;
        for (uint32_t n = 0u; n < slots; ++n) {
            if (tkey[slot] == k) {
                first = tpos[slot];
                break;
            }
            slot = (slot + 1u) & mask;
        }
        A.keep[b + i] = first == i ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_res_longcount(osmt_res_dedup A) {
    const uint32_t w = blockIdx.x * WG + threadIdx.x;
    if (w >= A.n_ways) return;
    const uint32_t b = A.off[w], len = A.off[w + 1u] - b;
    const bool is_long = len > A.short_max;
    if (is_long) A.keep[b] = 1u;
    A.long_pos[w] = is_long ? len - 1u : 0u;
}

/* long_pos: scanned, [n_ways + 1] */
__global__ __launch_bounds__(256) void k_res_longpairs(osmt_res_dedup A, uint32_t n_pairs, u64* __restrict__ key, uint32_t* __restrict__ id) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t w = owner_of(A.long_pos, A.n_ways, p);
    const uint32_t g = A.off[w] + 1u + (p - A.long_pos[w]);
    key[p] = pair_key(A.refs[g - 1u], A.refs[g]);
    id[p] = g;
}

/* key, id: sorted by key, positions ascending among equal keys */
__global__ __launch_bounds__(256) void k_res_longmark(osmt_res_dedup A, uint32_t n_pairs, const u64* __restrict__ key, const uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t g = id[i];
    bool repeat = false;
    if (i && key[i - 1u] == key[i]) repeat = owner_of(A.off, A.n_ways, id[i - 1u]) == owner_of(A.off, A.n_ways, g);
    A.keep[g] = repeat ? 0u : 1u;
}

/* keep: scanned, [n_refs + 1].  Lanes [0, n_refs): the references; lanes [0, n_ways]: the offsets. */
__global__ __launch_bounds__(256) void k_res_emit(osmt_res_dedup A, uint32_t n_refs, uint32_t* __restrict__ out_off, uint32_t* __restrict__ out_nodes) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n_refs) {
        const uint32_t p = A.keep[i];
        if (A.keep[i + 1u] != p) out_nodes[p] = A.refs[i];
    }
    if (i <= A.n_ways) out_off[i] = A.keep[A.off[i]];
}

/* one block per way; n < 2^32 - 1 */
inline dim3 way_grid(uint32_t n) { return n <= 65536u ? dim3(n) : dim3(65536u, (n + 65535u) / 65536u); }

inline dim3 grid_of(u64 n) { return dim3((uint32_t)((n + WG - 1u) / WG)); }

inline uint32_t max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }

}  // namespace

hipError_t osmt_launch_res_iota(uint32_t* id, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_res_iota, grid_of(n), dim3(WG), 0, st, id, n);
    return hipGetLastError();
}

hipError_t osmt_launch_res_translate(const osmt_res_refs& a, hipStream_t st) {
    if (a.n_refs) hipLaunchKernelGGL(k_res_translate, grid_of(a.n_refs), dim3(WG), 0, st, a);
    const hipError_t e = osmt_tq_scan(a.pos, a.n_refs, a.blk, a.tot, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_res_compact, grid_of((u64)max_u32(a.n_refs, a.n_owners) + 1u), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_res_short(const osmt_res_dedup& a, hipStream_t st) {
    if (a.n_ways && a.short_max) {
        uint32_t slots_cap = 64u;
        while (slots_cap < 2u * a.short_max) slots_cap <<= 1;
        hipLaunchKernelGGL(k_res_short, way_grid(a.n_ways), dim3(64), slots_cap * 12u, st, a, slots_cap);
    }
    if (a.n_ways) hipLaunchKernelGGL(k_res_longcount, grid_of(a.n_ways), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.long_pos, a.n_ways, a.blk, a.tot, st);
}

hipError_t osmt_launch_res_longpairs(const osmt_res_dedup& a, uint32_t n_pairs, unsigned long long* key, uint32_t* id, hipStream_t st) {
    if (n_pairs) hipLaunchKernelGGL(k_res_longpairs, grid_of(n_pairs), dim3(WG), 0, st, a, n_pairs, key, id);
    return hipGetLastError();
}

hipError_t osmt_launch_res_mark(const osmt_res_dedup& a, uint32_t n_pairs, const unsigned long long* key, const uint32_t* id, uint32_t n_refs, hipStream_t st) {
    if (n_pairs) hipLaunchKernelGGL(k_res_longmark, grid_of(n_pairs), dim3(WG), 0, st, a, n_pairs, key, id);
    return osmt_tq_scan(a.keep, n_refs, a.blk, a.tot + 1, st);
}

hipError_t osmt_launch_res_emit(const osmt_res_dedup& a, uint32_t n_refs, uint32_t* out_off, uint32_t* out_nodes, hipStream_t st) {
    hipLaunchKernelGGL(k_res_emit, grid_of((u64)max_u32(n_refs, a.n_ways) + 1u), dim3(WG), 0, st, a, n_refs, out_off, out_nodes);
    return hipGetLastError();
}
