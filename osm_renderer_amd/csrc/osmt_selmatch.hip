/*
 * osmt_selmatch.hip — MapCSS selector matching for every entity of a registered geodata file (osmt_match_selectors): what
 * Styler::style_area -> area_matches -> matches_by_tags (mapcss/styler.rs:205-242,450-520) decide per entity and rule on the
 * reference's worker thread, zoom left aside, and the entities' classes (cache slot, layer, matched selectors).  The host
 * twin, and the yardstick of the tests, is osmt::match_selectors_host (host/osmt_selmatch.hpp).  gfx950 only.
 *
 *   k_sm_tags         one lane per tag: its key bisected among the set's sorted test keys -> a code that is monotonic along
 *                     an entity's (strictly ascending) keys, so the match bisects codes instead of comparing strings; its
 *                     value bisected among that key's sorted test values -> a value id; the true-value flag; where a
 *                     numeric test names the key, the f64 from the override list or the exact fast path, or "declined".
 *   k_sm_declined     one lane per tag: the declined values compacted (the host sorts and dedups the few there are).
 *   k_sm_match        one lane per entity, once to count and once to emit: slot and object types from the geometry, then the
 *                     selectors in order with wave-uniform selector and test records; each test is a bisection of the lane's
 *                     codes.  The emit pass also parses tags["layer"] and hashes the entity's class key.
 *   k_sm_class_insert one lane per entity: open addressing over REPRESENTATIVE ENTITY NUMBERS.  An empty slot is claimed by
 *                     atomicCAS; an occupied one is compared in full (slot, layer, list) against its representative and
 *                     probed past when they differ, so a hash collision costs time and never merges two classes.  The slot's
 *                     lowest member is kept by an atomicMin that is only issued when it can succeed.
 *   k_sm_class_mark   one lane per entity: 1 where it is the lowest member of its slot.  The scan of the marks numbers the
 *                     classes by lowest member: a pure function of the input, whatever order the lanes ran in.
 *   k_sm_class_count, k_sm_class_emit, k_sm_ent_class: the class records, their pooled selector ids, the entities' classes.
 *   k_sm_bind_count, k_sm_bind_emit: per-class style lists expanded over the entities of one kind.
 *
 * The scans are 32-bit with 64-bit block totals (osmt_tq_scan): the host reads the totals back and launches nothing that
 * stores through an offset before it has seen them fit.  Every index read here was checked on the host when the tables were
 * registered; every store lands below a total the arrays were sized with; every buffer is written before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"
#include "osmt_numparse.h"

namespace {

constexpr uint32_t WG = 256u;

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

/* key[0 .. n) against "layer" in &str order; the word sits in a register, not in an array */
__device__ __forceinline__ int cmp_layer(const uint8_t* __restrict__ key, uint32_t n) {
    const unsigned long long word = 0x726579616CULL; /* "layer", first byte lowest */
    const uint32_t m = n < 5u ? n : 5u;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t c = (uint32_t)(word >> (8u * i)) & 0xFFu;
        if (key[i] != c) return key[i] < c ? -1 : 1;
    }
    return n < 5u ? -1 : (n > 5u ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_sm_tags(osmt_sm_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.tg.n_tags) return;
    const uint4 q = P.tg.tags[t];
    const uint8_t* key = P.tg.strings + q.x;
    const uint8_t* val = P.tg.strings + q.z;
    /* the first test key >= the tag's key */
    uint32_t lo = 0u, hi = P.ss.n_keys;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const osmt_sm_key k = P.ss.keys[mid];
        if (osmt_bytes_cmp(P.ss.strings + k.off, k.len, key, q.y) < 0)
            lo = mid + 1u;
        else
            hi = mid;
    }
    bool hit = false;
    osmt_sm_key k;
    if (lo < P.ss.n_keys) {
        k = P.ss.keys[lo];
        hit = osmt_bytes_cmp(P.ss.strings + k.off, k.len, key, q.y) == 0;
    }
    uint32_t vid = OSMT_SM_NONE, flags = 0u, declined = 0u;
    double num = 0.0;
    if (hit) {
        uint32_t a = 0u, b = k.n_vals;
        while (a < b) {
            const uint32_t mid = a + ((b - a) >> 1);
            const uint2 v = P.ss.vals[k.val_first + mid];
            const int c = osmt_bytes_cmp(P.ss.strings + v.x, v.y, val, q.w);
            if (c == 0) {
                vid = mid;
                break;
            }
            if (c < 0)
                a = mid + 1u;
            else
                b = mid;
        }
        if (osmt_is_true_value(val, q.w)) flags |= OSMT_SM_TRUE;
        if (k.numeric) {
            /* a listed value is not parsed here */
            uint32_t oa = 0u, ob = P.n_ov;
            bool listed = false;
            while (oa < ob) {
                const uint32_t mid = oa + ((ob - oa) >> 1);
                const osmt_number_override o = P.ov[mid];
                if (o.v_off == q.z && o.v_len == q.w) {
                    listed = true;
                    if (o.has_value) {
                        flags |= OSMT_SM_NUM;
                        num = o.value;
                    }
                    break;
                }
                if (o.v_off < q.z || (o.v_off == q.z && o.v_len < q.w))
                    oa = mid + 1u;
                else
                    ob = mid;
            }
            if (!listed) {
                const int rc = osmt_parse_f64_fast(val, q.w, &num);
                if (rc == OSMT_NUM_OK) flags |= OSMT_SM_NUM;
                if (rc == OSMT_NUM_DECLINED) flags |= OSMT_SM_DECLINED, declined = 1u;
                if (rc != OSMT_NUM_OK) num = 0.0;
            }
        }
    }
    P.tag_code[t] = 2u * lo + (hit ? 1u : 0u);
    P.tag_vf[t] = make_uint2(vid, flags);
    P.tag_num[t] = num;
    P.decl_pos[t] = declined;
}

__global__ __launch_bounds__(256) void k_sm_declined(osmt_sm_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.tg.n_tags) return;
    if (P.decl_pos[t + 1u] == P.decl_pos[t]) return;
    const uint4 q = P.tg.tags[t];
    osmt_declined_number d;
    d.v_off = q.z, d.v_len = q.w;
    P.declined[P.decl_pos[t]] = d;
}

/* the entity's tag with test key `key` among codes[t0 .. t1): its index or NONE */
__device__ __forceinline__ uint32_t find_tag(const uint32_t* __restrict__ codes, uint32_t t0, uint32_t t1, uint32_t key) {
    const uint32_t want = 2u * key + 1u;
    uint32_t lo = t0, hi = t1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (codes[mid] < want)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return (lo < t1 && codes[lo] == want) ? lo : OSMT_SM_NONE;
}

/* matches_by_tags (styler.rs:450-499) */
__device__ __forceinline__ bool test_holds(const osmt_sm_pass& P, const osmt_sm_test T, uint32_t t0, uint32_t t1) {
    const uint32_t i = find_tag(P.tag_code, t0, t1, T.key);
    const bool present = i != OSMT_SM_NONE;
    if (T.kind == OSMT_TEST_EXISTS) return present;
    if (T.kind == OSMT_TEST_NOT_EXISTS) return !present;
    const uint2 vf = present ? P.tag_vf[i] : make_uint2(OSMT_SM_NONE, 0u);
    switch (T.kind) {
        case OSMT_TEST_TRUE: return (vf.y & OSMT_SM_TRUE) != 0u;
        case OSMT_TEST_FALSE: return (vf.y & OSMT_SM_TRUE) == 0u;
        case OSMT_TEST_EQUAL: return present && vf.x == T.vid;
        case OSMT_TEST_NOT_EQUAL: return !(present && vf.x == T.vid);
        default: break;
    }
    if (!(vf.y & OSMT_SM_NUM)) return false; /* absent, a parse error, or declined (the call then fails as a whole) */
    const double v = P.tag_num[i];
    switch (T.kind) {
        case OSMT_TEST_LESS: return v < T.value;
        case OSMT_TEST_LESS_OR_EQUAL: return v <= T.value;
        case OSMT_TEST_GREATER: return v > T.value;
        default: return v >= T.value;
    }
}

/* cache slot (styler.rs:559-579) and the object types the entity matches (styler.rs:531-557), as a mask over OSMT_SEL_* */
__device__ __forceinline__ void kind_of(const osmt_sm_pass& P, uint32_t e, uint32_t* slot, uint32_t* types) {
    if (e < P.tg.n_nodes) {
        *slot = 0u, *types = 1u << OSMT_SEL_NODE;
        return;
    }
    const uint32_t w = e - P.tg.n_nodes;
    if (w >= P.tg.n_ways) {
        *slot = 3u, *types = (1u << OSMT_SEL_WAY) | (1u << OSMT_SEL_AREA);
        return;
    }
    /* OsmArea::is_closed of a way (reader.rs:475-482): more than 2 nodes, first and last equal as f64 coordinates */
    const uint32_t a = P.geo.way_off[w], n = P.geo.way_off[w + 1u] - a;
    bool closed = false;
    if (n > 2u) {
        const uint32_t f = P.geo.idx[a], l = P.geo.idx[a + n - 1u];
        closed = P.geo.nodes[2u * f] == P.geo.nodes[2u * l] && P.geo.nodes[2u * f + 1u] == P.geo.nodes[2u * l + 1u];
    }
    *slot = closed ? 1u : 2u;
    *types = (1u << OSMT_SEL_WAY) | (closed ? 1u << OSMT_SEL_AREA : 0u);
}

__device__ __forceinline__ uint32_t mix(uint32_t h, uint32_t v) {
    h ^= v;
    h *= 0x01000193u;
    return h ^ (h >> 15);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_sm_match(osmt_sm_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_ent) return;
    uint32_t slot, types;
    kind_of(P, e, &slot, &types);
    const uint32_t t0 = P.tg.tag_off[e], t1 = P.tg.tag_off[e + 1u];
    uint32_t n = 0u, h = 0x811C9DC5u;
    uint32_t* out = EMIT ? P.ent_sels + P.sel_pos[e] : nullptr;
    for (uint32_t s = 0; s < P.ss.n_sels; ++s) {
        const osmt_sm_sel S = P.ss.sels[s];
        if (!((types >> S.type) & 1u)) continue;
        bool ok = true;
        for (uint32_t j = 0; ok && j < S.n_tests; ++j) ok = test_holds(P, P.ss.tests[S.test_off + j], t0, t1);
        if (!ok) continue;
        if (EMIT) {
            out[n] = s;
            h = mix(h, s);
        }
        ++n;
    }
    if (!EMIT) {
        P.sel_pos[e] = n;
        return;
    }
    /* layer = tags["layer"].parse::<i64>().ok() (styler.rs:367-370): the tags bisected by key */
    long long layer = 0;
    uint32_t has_layer = 0u;
    {
        uint32_t lo = t0, hi = t1;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const uint4 q = P.tg.tags[mid];
            if (cmp_layer(P.tg.strings + q.x, q.y) < 0)
                lo = mid + 1u;
            else
                hi = mid;
        }
        if (lo < t1) {
            const uint4 q = P.tg.tags[lo];
            int64_t v = 0;
            if (cmp_layer(P.tg.strings + q.x, q.y) == 0 && osmt_parse_i64(P.tg.strings + q.z, q.w, &v)) {
                has_layer = 1u;
                layer = (long long)v;
            }
        }
    }
    const uint32_t key = slot | (has_layer << 2);
    h = mix(h, key);
    h = mix(h, (uint32_t)(unsigned long long)layer);
    h = mix(h, (uint32_t)((unsigned long long)layer >> 32));
    P.ent_layer[e] = layer;
    P.ent_key[e] = key;
    P.ent_hash[e] = h;
}

/* the class keys of entities a and b in full */
__device__ __forceinline__ bool same_class(const osmt_sm_pass& P, uint32_t a, uint32_t b) {
    if (P.ent_key[a] != P.ent_key[b] || P.ent_layer[a] != P.ent_layer[b]) return false;
    const uint32_t a0 = P.sel_pos[a], b0 = P.sel_pos[b], n = P.sel_pos[a + 1u] - a0;
    if (P.sel_pos[b + 1u] - b0 != n) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (P.ent_sels[a0 + i] != P.ent_sels[b0 + i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_sm_class_insert(osmt_sm_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_ent) return;
    uint32_t i = (P.ent_hash[e] & P.hash_mask) & P.table_mask;
    /* the table has at least twice as many slots as there are entities: an empty slot is always reached */
    for (;;) {
        /* most entities fall into a handful of classes: look before the CAS, same-address atomics are served one by one */
        uint32_t cur = __hip_atomic_load(P.table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == OSMT_SM_NONE) {
            cur = atomicCAS(P.table + i, OSMT_SM_NONE, e);
            if (cur == OSMT_SM_NONE) cur = e;
        }
        if (cur == e || same_class(P, e, cur)) {
            P.ent_tslot[e] = i;
            if (__hip_atomic_load(P.lowest + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > e) atomicMin(P.lowest + i, e);
            return;
        }
        i = (i + 1u) & P.table_mask;
    }
}

__global__ __launch_bounds__(256) void k_sm_class_mark(osmt_sm_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_ent) return;
    P.first_pos[e] = P.lowest[P.ent_tslot[e]] == e ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_sm_class_count(osmt_sm_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_ent) return;
    const uint32_t c = P.first_pos[e];
    if (P.first_pos[e + 1u] == c) return;
    P.cls_pos[c] = P.sel_pos[e + 1u] - P.sel_pos[e];
    P.cls_first[c] = e;
}

__global__ __launch_bounds__(256) void k_sm_class_emit(osmt_sm_pass P) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= P.n_classes) return;
    const uint32_t e = P.cls_first[c], src = P.sel_pos[e], dst = P.cls_pos[c], n = P.cls_pos[c + 1u] - dst;
    const uint32_t key = P.ent_key[e];
    osmt_match_class r;
    r.layer = P.ent_layer[e];
    r.sel_off = dst;
    r.n_sels = n;
    r.first_entity = e;
    r.slot = (uint8_t)(key & 3u);
    r.has_layer = (uint8_t)(key >> 2);
    r._pad[0] = r._pad[1] = 0;
    P.classes[c] = r;
    for (uint32_t i = 0; i < n; ++i) P.class_sels[dst + i] = P.ent_sels[src + i];
}

__global__ __launch_bounds__(256) void k_sm_ent_class(osmt_sm_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_ent) return;
    P.ent_class[e] = P.first_pos[P.lowest[P.ent_tslot[e]]];
}

__global__ __launch_bounds__(256) void k_sm_bind_count(const uint32_t* __restrict__ ent_class, const uint32_t* __restrict__ class_off, uint32_t n,
                                                      uint32_t* __restrict__ pos) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ent_class[i];
    pos[i] = class_off[c + 1u] - class_off[c];
}

__global__ __launch_bounds__(256) void k_sm_bind_emit(const uint32_t* __restrict__ ent_class, const uint32_t* __restrict__ class_off,
                                                     const uint32_t* __restrict__ class_styles, uint32_t n, const uint32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ent_class[i], src = class_off[c], dst = pos[i], k = pos[i + 1u] - dst;
    for (uint32_t j = 0; j < k; ++j) out[dst + j] = class_styles[src + j];
}

}  // namespace

hipError_t osmt_launch_sm_tags(const osmt_sm_pass& a, hipStream_t st) {
    if (a.tg.n_tags) hipLaunchKernelGGL(k_sm_tags, grid_of(a.tg.n_tags), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.decl_pos, a.tg.n_tags, a.blk, a.tot + OSMT_SM_T_DECLINED, st);
}

hipError_t osmt_launch_sm_declined(const osmt_sm_pass& a, hipStream_t st) {
    if (a.tg.n_tags) hipLaunchKernelGGL(k_sm_declined, grid_of(a.tg.n_tags), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_sm_count(const osmt_sm_pass& a, hipStream_t st) {
    if (a.n_ent) hipLaunchKernelGGL(k_sm_match<false>, grid_of(a.n_ent), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.sel_pos, a.n_ent, a.blk, a.tot + OSMT_SM_T_MATCHED, st);
}

hipError_t osmt_launch_sm_classes(const osmt_sm_pass& a, hipStream_t st) {
    if (a.n_ent) {
        const size_t bytes = ((size_t)a.table_mask + 1u) * 4u;
        hipError_t e = hipMemsetAsync(a.table, 0xFF, bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(a.lowest, 0xFF, bytes, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_sm_match<true>, grid_of(a.n_ent), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_sm_class_insert, grid_of(a.n_ent), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_sm_class_mark, grid_of(a.n_ent), dim3(WG), 0, st, a);
    }
    return osmt_tq_scan(a.first_pos, a.n_ent, a.blk, a.tot + OSMT_SM_T_CLASSES, st);
}

hipError_t osmt_launch_sm_class_count(const osmt_sm_pass& a, hipStream_t st) {
    if (a.n_ent) hipLaunchKernelGGL(k_sm_class_count, grid_of(a.n_ent), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.cls_pos, a.n_classes, a.blk, a.tot + OSMT_SM_T_CLASS_SELS, st);
}

hipError_t osmt_launch_sm_emit(const osmt_sm_pass& a, hipStream_t st) {
    if (a.n_classes) hipLaunchKernelGGL(k_sm_class_emit, grid_of(a.n_classes), dim3(WG), 0, st, a);
    if (a.n_ent) hipLaunchKernelGGL(k_sm_ent_class, grid_of(a.n_ent), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_sm_bind_count(const uint32_t* ent_class, const uint32_t* class_off, uint32_t n, uint32_t* pos, unsigned long long* blk,
                                     unsigned long long* tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_sm_bind_count, grid_of(n), dim3(WG), 0, st, ent_class, class_off, n, pos);
    return osmt_tq_scan(pos, n, blk, tot, st);
}

hipError_t osmt_launch_sm_bind_emit(const uint32_t* ent_class, const uint32_t* class_off, const uint32_t* class_styles, uint32_t n, const uint32_t* pos,
                                    uint32_t* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_sm_bind_emit, grid_of(n), dim3(WG), 0, st, ent_class, class_off, class_styles, n, pos, out);
    return hipGetLastError();
}
