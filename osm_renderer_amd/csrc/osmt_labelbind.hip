/*
 * osmt_labelbind.hip — label bindings per class (osmt_register_label_bindings_matched, osmt_register_area_label_bindings_matched):
 * what Styler::style_entities pushes for every member of a class, with the text Tags::get_by_key(&text_style.text) finds
 * (text_placer.rs:42-45, reader.rs:351-373) decoded into the table's text pool.  The host twin, and the yardstick of the
 * tests, is osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host (host/osmt_selmatch.hpp).  gfx950 only.
 *
 *   k_lb_count        one lane per entity of one kind: the length of its class's list (then the scan: the *_off array).
 *   k_lb_emit         one lane per entity: its class's bindings copied; for a binding with a key the entity's strictly
 *                     ascending tag keys are bisected by bytes, the tag's number in the table is the provisional text and
 *                     used[tag] = 1 (an idempotent store).
 *   k_lb_text_insert  one lane per used tag: open addressing over REPRESENTATIVE TAG NUMBERS, keyed by the value range
 *                     (v_off, v_len).  An empty slot is claimed by atomicCAS, an occupied one is compared in full; the hash
 *                     only chooses where to start.  The slot's lowest member is kept by an atomicMin that is only issued
 *                     when it can succeed.
 *   k_lb_text_mark    one lane per tag: 1 where it is the lowest member of its slot.  The scan numbers the texts by their
 *                     lowest user: a pure function of the input, whatever order the lanes ran in.
 *   k_lb_text_list    one lane per tag: text_tag[text] = its lowest user.
 *   k_lb_measure      one lane per text: the value validated (csrc/osmt_utf8.h) and its scalars counted; an ill-formed one
 *                     does atomicMin on the first-bad-tag word.  Then the scan: text_off.
 *   k_lb_decode       one lane per text: its scalars.
 *   k_lb_patch        one lane per binding: the provisional tag number replaced by the text id of its tag's representative.
 *
 * The scans are 32-bit with 64-bit block totals (osmt_tq_scan): the host reads the totals back and launches nothing that
 * stores through an offset before it has seen them fit.  Every index read here was checked on the host (the descriptor by
 * osmt_validate_class_label_bindings, the tags by osmt_validate_tags); every store lands below a total the arrays were sized
 * with; every buffer is written before it is read.  Integer work only, no LDS.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"
#include "osmt_utf8.h"

namespace {

constexpr uint32_t WG = 256u;

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

/* a[0 .. na) against b[0 .. nb) in &str order.  b is a key of the descriptor's device copy, which starts every key on a
 * 4-byte boundary; where a is aligned too, whole dwords are compared first (big-endian order of a dword is byte order). */
__device__ __forceinline__ int cmp_key(const uint8_t* __restrict__ a, uint32_t na, const uint8_t* __restrict__ b, uint32_t nb) {
    const uint32_t n = na < nb ? na : nb;
    uint32_t i = 0u;
    if (((uintptr_t)a & 3u) == 0u)
        for (; i + 4u <= n; i += 4u) {
            const uint32_t x = *(const uint32_t*)(a + i), y = *(const uint32_t*)(b + i);
            if (x != y) return __builtin_bswap32(x) < __builtin_bswap32(y) ? -1 : 1;
        }
    for (; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : (na > nb ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_lb_count(const uint32_t* __restrict__ ent_class, const uint32_t* __restrict__ class_off, uint32_t n,
                                                  uint32_t* __restrict__ pos) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ent_class[i];
    pos[i] = class_off[c + 1u] - class_off[c];
}

__global__ __launch_bounds__(256) void k_lb_emit(osmt_lb_pass P, uint32_t first, uint32_t n, const uint32_t* __restrict__ pos,
                                                 osmt_label_binding* __restrict__ out) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = first + i;
    const uint32_t c = P.ent_class[e], src = P.class_off[c], dst = pos[i], k = pos[i + 1u] - dst;
    if (k == 0u) return;
    const uint32_t t0 = P.tg.tag_off[e], t1 = P.tg.tag_off[e + 1u];
    for (uint32_t j = 0; j < k; ++j) {
        const uint2 b = P.class_bind[src + j];
        osmt_label_binding r;
        r.style = b.x;
        r.text = OSMT_TEXT_NONE;
        if (b.y != OSMT_TEXT_NONE) {
            const uint2 key = P.keys[b.y];
            /* the first tag whose key is >= the key (Tags::get_by_key over strictly ascending keys) */
            uint32_t lo = t0, hi = t1;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                const uint4 q = P.tg.tags[mid];
                if (cmp_key(P.tg.strings + q.x, q.y, P.key_bytes + key.x, key.y) < 0)
                    lo = mid + 1u;
                else
                    hi = mid;
            }
            if (lo < t1) {
                const uint4 q = P.tg.tags[lo];
                if (cmp_key(P.tg.strings + q.x, q.y, P.key_bytes + key.x, key.y) == 0) {
                    r.text = lo - P.tag_base;
                    P.used[lo - P.tag_base] = 1u;
                }
            }
        }
        out[dst + j] = r;
    }
}

__device__ __forceinline__ uint32_t mix(uint32_t h, uint32_t v) {
    h ^= v;
    h *= 0x01000193u;
    return h ^ (h >> 15);
}

__global__ __launch_bounds__(256) void k_lb_text_insert(osmt_lb_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tt || P.used[t] == 0u) return;
    const uint4 q = P.tg.tags[P.tag_base + t];
    uint32_t i = (mix(mix(0x811C9DC5u, q.z), q.w) & P.hash_mask) & P.table_mask;
    /* the table has at least twice as many slots as the table has tags: an empty slot is always reached */
    for (;;) {
        /* one name serves many entities: look before the CAS, same-address atomics are served one by one */
        uint32_t cur = __hip_atomic_load(P.table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == OSMT_SM_NONE) {
            cur = atomicCAS(P.table + i, OSMT_SM_NONE, t);
            if (cur == OSMT_SM_NONE) cur = t;
        }
        bool same = cur == t;
        if (!same) {
            const uint4 r = P.tg.tags[P.tag_base + cur];
            same = r.z == q.z && r.w == q.w;
        }
        if (same) {
            P.tslot[t] = i;
            if (__hip_atomic_load(P.lowest + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > t) atomicMin(P.lowest + i, t);
            return;
        }
        i = (i + 1u) & P.table_mask;
    }
}

__global__ __launch_bounds__(256) void k_lb_text_mark(osmt_lb_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tt) return;
    P.first_pos[t] = (P.used[t] != 0u && P.lowest[P.tslot[t]] == t) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_lb_text_list(osmt_lb_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tt) return;
    const uint32_t x = P.first_pos[t];
    if (P.first_pos[t + 1u] != x) P.text_tag[x] = t;
}

__global__ __launch_bounds__(256) void k_lb_measure(osmt_lb_pass P) {
    const uint32_t x = blockIdx.x * WG + threadIdx.x;
    if (x >= P.n_texts) return;
    const uint32_t t = P.text_tag[x];
    const uint4 q = P.tg.tags[P.tag_base + t];
    uint32_t n = 0u;
    if (osmt_utf8_validate(P.tg.strings + q.z, q.w, &n) != q.w) atomicMin(P.tot + OSMT_LB_T_FIRST_BAD, (unsigned long long)t);
    P.text_off[x] = n;
}

__global__ __launch_bounds__(256) void k_lb_decode(osmt_lb_pass P) {
    const uint32_t x = blockIdx.x * WG + threadIdx.x;
    if (x >= P.n_texts) return;
    const uint4 q = P.tg.tags[P.tag_base + P.text_tag[x]];
    (void)osmt_utf8_decode(P.tg.strings + q.z, q.w, P.chars + P.text_off[x]);
}

__global__ __launch_bounds__(256) void k_lb_patch(osmt_lb_pass P, osmt_label_binding* __restrict__ bind, uint32_t n) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = bind[i].text;
    if (t == OSMT_TEXT_NONE) return;
    bind[i].text = P.first_pos[P.lowest[P.tslot[t]]];
}

}  // namespace

hipError_t osmt_launch_lb_begin(const osmt_lb_pass& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.tot + OSMT_LB_T_FIRST_BAD, 0xFF, 8, st);
    if (e == hipSuccess && a.n_tt) e = hipMemsetAsync(a.used, 0, (size_t)a.n_tt * 4u, st);
    return e;
}

hipError_t osmt_launch_lb_count(const osmt_lb_pass& a, uint32_t first, uint32_t n, uint32_t* pos, unsigned long long* tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_lb_count, grid_of(n), dim3(WG), 0, st, a.ent_class + first, a.class_off, n, pos);
    return osmt_tq_scan(pos, n, a.blk, tot, st);
}

hipError_t osmt_launch_lb_emit(const osmt_lb_pass& a, uint32_t first, uint32_t n, const uint32_t* pos, osmt_label_binding* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_lb_emit, grid_of(n), dim3(WG), 0, st, a, first, n, pos, out);
    return hipGetLastError();
}

hipError_t osmt_launch_lb_texts(const osmt_lb_pass& a, hipStream_t st) {
    if (a.n_tt) {
        const size_t bytes = ((size_t)a.table_mask + 1u) * 4u;
        hipError_t e = hipMemsetAsync(a.table, 0xFF, bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(a.lowest, 0xFF, bytes, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_lb_text_insert, grid_of(a.n_tt), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_lb_text_mark, grid_of(a.n_tt), dim3(WG), 0, st, a);
    }
    return osmt_tq_scan(a.first_pos, a.n_tt, a.blk, a.tot + OSMT_LB_T_TEXTS, st);
}

hipError_t osmt_launch_lb_measure(const osmt_lb_pass& a, hipStream_t st) {
    if (a.n_tt) hipLaunchKernelGGL(k_lb_text_list, grid_of(a.n_tt), dim3(WG), 0, st, a);
    if (a.n_texts) hipLaunchKernelGGL(k_lb_measure, grid_of(a.n_texts), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.text_off, a.n_texts, a.blk, a.tot + OSMT_LB_T_CHARS, st);
}

hipError_t osmt_launch_lb_decode(const osmt_lb_pass& a, hipStream_t st) {
    if (a.n_texts) hipLaunchKernelGGL(k_lb_decode, grid_of(a.n_texts), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_lb_patch(const osmt_lb_pass& a, osmt_label_binding* bind, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_lb_patch, grid_of(n), dim3(WG), 0, st, a, bind, n);
    return hipGetLastError();
}
