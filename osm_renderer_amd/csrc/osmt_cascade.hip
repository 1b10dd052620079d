/*
 * osmt_cascade.hip — the cascade on the device: from the classes of a match and a registered rule set to the distinct styles
 * and label styles, the zoom ranges and the per-class lists of every range (include/osmtile.h, "the cascade").
 *
 * Stages (count / scan / emit, as k_sm_bind_* and k_lb_*):
 *   k_cs_class_layers  (a set registered with OSMT_RULES_CLASS_LAYERS only) one lane per class: the layers of the class's
 *                      selectors numbered 0 .. 15 by first appearance, the class's own "*" and "default", its layer count; a
 *                      class of more than 16 layers reports itself and the cascade is refused
 *   k_cs_count         one lane per (class, zoom): the layers the kept selectors create, "*" left out  -> scan: the styles
 *   k_cs_fold          32 lanes per (class, zoom), lane = property name: style_area (styler.rs:205-242) with the per-layer
 *                      last writers in 8 registers indexed by the set's layer number, or in 16 indexed by the class's
 *                      (CLASS_LAYERS); the layer bookkeeping (which layers exist, insertion order, the copy
 *                      from "*") is computed identically by every lane.  Writes one row of last writers per style.
 *   k_cs_records       one lane per style: property_map_to_style (osmt_cs_style_of, shared with the host mirror), the two
 *                      records, the text key, the hashes; 1 where the style is a label binding             -> scan
 *   k_cs_insert<K>     open addressing over representative style numbers, the scheme of k_sm_class_insert: load before CAS,
 *                      full comparison on an occupied slot, atomicMin only when it can succeed
 *   k_cs_mark<K>       1 at the style that is the lowest user of its record, 0 elsewhere                  -> scan: at a marked
 *                      style, the id of its record
 *   k_cs_rank          the record ids of every style (through its table slot's lowest user); per distinct record its lowest
 *                      user, per distinct area record the number of its dashes                             -> scan
 *   k_cs_compact       the distinct records, dashes re-pooled per record
 *   k_cs_zoom_differs  one lane per (class, zoom >= 1): do the lists of both kinds equal those of the zoom below
 *   k_cs_range_count   one lane per (range, class): list lengths                                          -> two scans
 *   k_cs_range_emit    the lists, offsets rebased to their range
 *
 * Style numbers follow (class, zoom, position), so "lowest style number" is "lowest user" and every id is a pure function
 * of the input.  No kernel reads a string.  All indices are checked on the host at registration (osmt_validate_rules) or
 * are results of the scans.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "osmt_cascade_rule.h"
#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t GROUP = 32u; /* lanes per (class, zoom) in k_cs_fold */
constexpr uint32_t Z = OSMT_CS_ZOOMS;
constexpr uint32_t L = OSMT_CASCADE_MAX_LAYERS;
constexpr uint32_t LC = OSMT_CASCADE_MAX_CLASS_LAYERS;
static_assert(L == 8u && LC == 16u, "k_cs_fold packs a layer's insertion slot into 4 bits and `exists` into the low bits of a word");

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

__device__ __forceinline__ uint32_t mix(uint32_t h, uint32_t v) {
    h ^= v;
    h *= 0x9E3779B1u;
    return h ^ (h >> 15);
}

/* does selector s admit the zoom (area_matches, styler.rs:505-515) */
__device__ __forceinline__ bool admits(const osmt_cs_rules_dev& R, uint32_t s, uint32_t zoom) { return zoom >= R.sel_zoom[2u * s] && zoom <= R.sel_zoom[2u * s + 1u]; }

/* One lane per class of a set registered with OSMT_RULES_CLASS_LAYERS: one walk of the class's selectors, no zoom filter, that
 * numbers the distinct set-wide layer numbers (0 .. 254) by first appearance.  The numbers met are a set of 256 bits and the
 * set-wide number of every local layer a byte of two words, both in registers and indexed by unrolled selects.  A class of
 * more than LC layers keeps its exact count, gets the local number LC - 1 for what does not fit (so that k_cs_count, which
 * runs before the host has looked, stays inside its 16 bits) and reports itself; the host refuses the cascade. */
__global__ __launch_bounds__(256) void k_cs_class_layers(osmt_cs_pass P) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= P.n_classes) return;
    const uint32_t s0 = P.classes[c].sel_off, n = P.classes[c].n_sels;
    uint64_t seen[4] = {0ull, 0ull, 0ull, 0ull};
    uint64_t ids[LC / 8u] = {0ull, 0ull};
    uint32_t n_layers = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = P.R.sel_layer[P.class_sels[s0 + i]];
        const uint64_t bit = 1ull << (g & 63u);
        bool known = false;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w)
            if (w == g >> 6) {
                known = (seen[w] & bit) != 0ull;
                seen[w] |= bit;
            }
        if (!known) {
#pragma unroll
            for (uint32_t w = 0; w < LC / 8u; ++w)
                if (n_layers < LC && w == n_layers >> 3) ids[w] |= (uint64_t)g << (8u * (n_layers & 7u));
            ++n_layers;
        }
        uint32_t local = LC - 1u;
#pragma unroll
        for (uint32_t k = 0; k < LC; ++k)
            if (k < n_layers && (uint32_t)((ids[k >> 3] >> (8u * (k & 7u))) & 0xFFull) == g) local = k;
        P.sel_local[s0 + i] = (uint8_t)local;
    }
    uint32_t star = 0xFFu, base = 0xFFu;
#pragma unroll
    for (uint32_t k = 0; k < LC; ++k) {
        const uint32_t g = (uint32_t)((ids[k >> 3] >> (8u * (k & 7u))) & 0xFFull);
        if (k < n_layers && g == P.R.star) star = k;
        if (k < n_layers && g == P.R.base) base = k;
    }
    P.class_info[c] = star | (base << 8) | (n_layers << 16);
    if (n_layers > LC) atomicMin(P.tot + OSMT_CS_T_BAD_CLASS, (unsigned long long)c);
}

/* the class's own "*" / "default" of a CLASS_LAYERS set, as the layer number k_cs_count and k_cs_fold compare with */
__device__ __forceinline__ uint32_t local_or_none(uint32_t byte) { return byte == 0xFFu ? OSMT_CS_NONE : byte; }

/* LOCAL: the set is registered with OSMT_RULES_CLASS_LAYERS, layer numbers are the class's (sel_local, class_info); otherwise they
 * are the set's (R.sel_layer, R.star, R.base), below 8 */
template <bool LOCAL>
__global__ __launch_bounds__(256) void k_cs_count(osmt_cs_pass P) {
    const uint32_t pair = blockIdx.x * WG + threadIdx.x;
    if (pair >= P.n_pairs) return;
    const uint32_t c = pair / Z, zoom = pair % Z;
    const uint32_t s0 = P.classes[c].sel_off, n = P.classes[c].n_sels;
    const uint32_t star = LOCAL ? local_or_none(OSMT_CS_CI_STAR(P.class_info[c])) : P.R.star;
    uint32_t exists = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = P.class_sels[s0 + i];
        if (admits(P.R, s, zoom)) exists |= 1u << (LOCAL ? (uint32_t)P.sel_local[s0 + i] : (uint32_t)P.R.sel_layer[s]);
    }
    if (star != OSMT_CS_NONE) exists &= ~(1u << star);
    P.pair_pos[pair] = (uint32_t)__popc(exists);
}

template <uint32_t LAYERS>
struct order_of {
    typedef uint32_t type;
};
template <>
struct order_of<16u> {
    typedef uint64_t type;
};

template <uint32_t LAYERS, bool LOCAL>
__global__ __launch_bounds__(256) void k_cs_fold(osmt_cs_pass P) {
    typedef typename order_of<LAYERS>::type order_t;
    const uint32_t lane = threadIdx.x % GROUP;
    const uint32_t pair = (blockIdx.x * WG + threadIdx.x) / GROUP;
    const bool live = pair < P.n_pairs;
    const uint32_t c = live ? pair / Z : 0u, zoom = pair % Z;
    const uint32_t s0 = live ? P.classes[c].sel_off : 0u, n = live ? P.classes[c].n_sels : 0u;
    const uint32_t name = lane < OSMT_PROP_NAMES ? lane : 0u; /* lanes 20 .. 31 shadow name 0 and write nothing */
    const uint32_t info = LOCAL && live ? P.class_info[c] : 0xFFFFu;
    const uint32_t star = LOCAL ? local_or_none(OSMT_CS_CI_STAR(info)) : P.R.star;
    const uint32_t base = LOCAL ? local_or_none(OSMT_CS_CI_BASE(info)) : P.R.base;
    uint32_t last[LAYERS];
#pragma unroll
    for (uint32_t l = 0; l < LAYERS; ++l) last[l] = OSMT_CS_NONE;
    uint32_t exists = 0u, n_layers = 0u;
    order_t order = 0u; /* 4 bits per layer, in insertion order */
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = P.class_sels[s0 + i];
        if (!admits(P.R, s, zoom)) continue;
        const uint32_t g = LOCAL ? (uint32_t)P.sel_local[s0 + i] : (uint32_t)P.R.sel_layer[s];
        const uint32_t v = P.R.rule_last[P.R.sel_rule[s] * OSMT_PROP_NAMES + name];
        if (!(exists & (1u << g))) {
            /* a new layer starts as a copy of "*", if that exists (styler.rs:225-228) */
            uint32_t init = OSMT_CS_NONE;
            if (star != OSMT_CS_NONE && (exists & (1u << star))) {
#pragma unroll
                for (uint32_t l = 0; l < LAYERS; ++l)
                    if (l == star) init = last[l];
            }
#pragma unroll
            for (uint32_t l = 0; l < LAYERS; ++l)
                if (l == g) last[l] = init;
            exists |= 1u << g;
            order |= (order_t)g << (4u * n_layers);
            ++n_layers;
        }
        if (v != OSMT_CS_NONE) {
            /* the rule's properties go to the layer, and from "*" to every layer that exists (230-237) */
            const uint32_t to = g == star ? exists : 1u << g;
#pragma unroll
            for (uint32_t l = 0; l < LAYERS; ++l)
                if (to & (1u << l)) last[l] = v;
        }
    }
    uint32_t base_width = OSMT_CS_NONE;
    if (base != OSMT_CS_NONE && (exists & (1u << base))) {
#pragma unroll
        for (uint32_t l = 0; l < LAYERS; ++l)
            if (l == base) base_width = last[l];
    }
    /* every lane of the wave is here: the width lane of the group hands its "default" writer to lane 20 */
    base_width = __shfl(base_width, (int)((threadIdx.x & 63u) - lane + OSMT_PROP_WIDTH));
    if (!live) return;
    const uint32_t out0 = P.pair_pos[pair];
    uint32_t position = 0u;
    for (uint32_t k = 0; k < n_layers; ++k) {
        const uint32_t g = (uint32_t)(order >> (4u * k)) & 15u;
        if (g == star) continue;
        uint32_t v = OSMT_CS_NONE;
#pragma unroll
        for (uint32_t l = 0; l < LAYERS; ++l)
            if (l == g) v = last[l];
        uint32_t* row = P.rows + (size_t)(out0 + position) * OSMT_CS_ROW_WORDS;
        if (lane < OSMT_PROP_NAMES) row[lane] = v;
        if (lane == OSMT_CS_ROW_BASE_WIDTH) row[lane] = base_width;
        if (lane == OSMT_CS_ROW_PAIR) row[lane] = pair;
        if (lane == OSMT_CS_ROW_POSITION) row[lane] = position;
        ++position;
    }
}

__device__ __forceinline__ uint32_t hash_words(uint32_t h, const void* p, uint32_t n_words) {
    const uint32_t* w = (const uint32_t*)p;
    for (uint32_t i = 0; i < n_words; ++i) h = mix(h, w[i]);
    return h;
}

__global__ __launch_bounds__(256) void k_cs_records(osmt_cs_pass P) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= P.n_styles) return;
    const uint32_t* row = P.rows + (size_t)s * OSMT_CS_ROW_WORDS;
    osmt_cs_env E;
    E.props = P.R.props;
    E.casing_width_multiplier = P.R.casing_width_multiplier;
    E.font_size_multiplier = P.R.font_size_multiplier;
    E.font_id = P.R.font_id;
    osmt_style_rec a;
    osmt_label_style_rec l;
    uint32_t key;
    const bool draws = osmt_cs_style_of(E, row, P.classes[row[OSMT_CS_ROW_PAIR] / Z], &a, &l, &key);
    P.area[s] = a;
    P.label[s] = l;
    P.text_key[s] = key;
    P.bind_pos[s] = (P.labels_all || draws) ? 1u : 0u;
    /* the hash of an area record leaves the dash offsets out and takes the dashes in */
    osmt_style_rec b = a;
    b.dashes_off = b.casing_dashes_off = 0u;
    uint32_t h = hash_words(0x811C9DC5u, &b, sizeof b / 4u);
    h = hash_words(h, P.R.numbers + a.dashes_off, 2u * a.n_dashes);
    h = hash_words(h, P.R.numbers + a.casing_dashes_off, 2u * a.n_casing_dashes);
    P.hash[0][s] = h;
    P.hash[1][s] = hash_words(0x811C9DC5u, &l, sizeof l / 4u);
}

template <int K>
__device__ __forceinline__ bool same_record(const osmt_cs_pass& P, uint32_t a, uint32_t b) {
    if (K == 0) return osmt_cs_same_area(P.area[a], P.area[b], P.R.numbers);
    return osmt_cs_same_label(P.label[a], P.label[b]);
}

/* is style s a user of kind K: every style uses its area record, a label binding its label record */
template <int K>
__device__ __forceinline__ bool uses(const osmt_cs_pass& P, uint32_t s) {
    return K == 0 || P.bind_pos[s + 1u] != P.bind_pos[s];
}

template <int K>
__global__ __launch_bounds__(256) void k_cs_insert(osmt_cs_pass P) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= P.n_styles || !uses<K>(P, s)) return;
    uint32_t* table = P.table[K];
    uint32_t* lowest = P.lowest[K];
    uint32_t i = (P.hash[K][s] & P.hash_mask) & P.table_mask;
    /* the table has at least twice as many slots as there are styles: an empty slot is always reached */
    for (;;) {
        uint32_t cur = __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == OSMT_CS_NONE) {
            cur = atomicCAS(table + i, OSMT_CS_NONE, s);
            if (cur == OSMT_CS_NONE) cur = s;
        }
        if (cur == s || same_record<K>(P, s, cur)) {
            P.tslot[K][s] = i;
            if (__hip_atomic_load(lowest + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > s) atomicMin(lowest + i, s);
            return;
        }
        i = (i + 1u) & P.table_mask;
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_cs_mark(osmt_cs_pass P) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= P.n_styles) return;
    P.first_pos[K][s] = uses<K>(P, s) && P.lowest[K][P.tslot[K][s]] == s ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_cs_rank(osmt_cs_pass P) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= P.n_styles) return;
    P.id[0][s] = P.first_pos[0][P.lowest[0][P.tslot[0][s]]];
    const bool binds = uses<1>(P, s);
    P.id[1][s] = binds ? P.first_pos[1][P.lowest[1][P.tslot[1][s]]] : OSMT_CS_NONE;
    const uint32_t d = P.first_pos[0][s];
    if (P.first_pos[0][s + 1u] != d) {
        P.rep[0][d] = s;
        P.dash_pos[d] = P.area[s].n_dashes + P.area[s].n_casing_dashes;
    }
    const uint32_t e = P.first_pos[1][s];
    if (P.first_pos[1][s + 1u] != e) P.rep[1][e] = s;
}

/* An area record is six 16-byte words; words 13 .. 16 are dashes_off, n_dashes, casing_dashes_off, n_casing_dashes.  The record
 * is copied word by word with the two offsets patched on the way: a local osmt_style_rec whose fields are written would become
 * a private array (scratch, or LDS by promotion). */
static_assert(sizeof(osmt_style_rec) == 96 && offsetof(osmt_style_rec, dashes_off) == 52 && offsetof(osmt_style_rec, n_dashes) == 56 &&
                  offsetof(osmt_style_rec, casing_dashes_off) == 60 && offsetof(osmt_style_rec, n_casing_dashes) == 64,
              "k_cs_compact patches the dash ranges by word");

__global__ __launch_bounds__(256) void k_cs_compact(osmt_cs_pass P) {
    const uint32_t d = blockIdx.x * WG + threadIdx.x;
    if (d < P.n_area) {
        const uint32_t* in = (const uint32_t*)(P.area + P.rep[0][d]);
        uint32_t* out = (uint32_t*)(P.out_area + d);
        const uint32_t dashes_off = in[13], n_dashes = in[14], casing_off = in[15], n_casing = in[16];
        const uint32_t o = P.dash_pos[d];
        const double* src = P.R.numbers + dashes_off;
        for (uint32_t i = 0; i < n_dashes; ++i) P.out_dashes[o + i] = src[i];
        src = P.R.numbers + casing_off;
        for (uint32_t i = 0; i < n_casing; ++i) P.out_dashes[o + n_dashes + i] = src[i];
#pragma unroll
        for (uint32_t k = 0; k < sizeof(osmt_style_rec) / 4u; ++k) {
            uint32_t v = in[k];
            if (k == 13u && n_dashes) v = o;
            if (k == 15u && n_casing) v = o + n_dashes;
            out[k] = v;
        }
    }
    if (d < P.n_label) {
        const uint4* in = (const uint4*)(P.label + P.rep[1][d]);
        uint4* out = (uint4*)(P.out_label + d);
        out[0] = in[0], out[1] = in[1], out[2] = in[2];
    }
}

__global__ __launch_bounds__(256) void k_cs_zoom_differs(osmt_cs_pass P) {
    const uint32_t pair = blockIdx.x * WG + threadIdx.x;
    if (pair >= P.n_pairs || pair % Z == 0u) return;
    const uint32_t a0 = P.pair_pos[pair - 1u], b0 = P.pair_pos[pair], b1 = P.pair_pos[pair + 1u];
    bool differs = b0 - a0 != b1 - b0;
    for (uint32_t i = 0; i < b1 - b0 && !differs; ++i) differs = P.id[0][a0 + i] != P.id[0][b0 + i];
    /* the label lists: the styles that bind, in order, as (record, key) */
    uint32_t i = a0, j = b0;
    while (!differs) {
        while (i < b0 && P.id[1][i] == OSMT_CS_NONE) ++i;
        while (j < b1 && P.id[1][j] == OSMT_CS_NONE) ++j;
        if (i == b0 || j == b1) {
            differs = (i == b0) != (j == b1);
            break;
        }
        differs = P.id[1][i] != P.id[1][j] || P.text_key[i] != P.text_key[j];
        ++i, ++j;
    }
    if (differs) P.zoom_differs[pair % Z] = 1u; /* every writer writes the same word */
}

__global__ __launch_bounds__(256) void k_cs_range_count(osmt_cs_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_ranges * P.n_classes) return;
    const uint32_t pair = (i % P.n_classes) * Z + P.range_zoom[i / P.n_classes];
    const uint32_t s0 = P.pair_pos[pair], s1 = P.pair_pos[pair + 1u];
    P.rs_pos[i] = s1 - s0;
    P.rb_pos[i] = P.bind_pos[s1] - P.bind_pos[s0];
}

__global__ __launch_bounds__(256) void k_cs_range_emit(osmt_cs_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_ranges * P.n_classes) return;
    const uint32_t r = i / P.n_classes, c = i % P.n_classes;
    const uint32_t pair = c * Z + P.range_zoom[r];
    const uint32_t s0 = P.pair_pos[pair], s1 = P.pair_pos[pair + 1u];
    const uint32_t sb = P.rs_pos[r * P.n_classes], bb = P.rb_pos[r * P.n_classes]; /* the range's bases */
    uint32_t so = P.rs_pos[i], bo = P.rb_pos[i];
    uint32_t* style_off = P.out_style_off + (size_t)r * (P.n_classes + 1u);
    uint32_t* bind_off = P.out_bind_off + (size_t)r * (P.n_classes + 1u);
    style_off[c] = so - sb;
    bind_off[c] = bo - bb;
    if (c == P.n_classes - 1u) {
        style_off[c + 1u] = P.rs_pos[i + 1u] - sb;
        bind_off[c + 1u] = P.rb_pos[i + 1u] - bb;
    }
    for (uint32_t s = s0; s < s1; ++s) {
        P.out_styles[so++] = P.id[0][s];
        if (P.id[1][s] != OSMT_CS_NONE) P.out_binds[bo++] = osmt_class_label_binding{P.id[1][s], P.text_key[s]};
    }
}

}  // namespace

hipError_t osmt_launch_cs_class_layers(const osmt_cs_pass& a, hipStream_t st) {
    if (!(a.R.flags & OSMT_RULES_CLASS_LAYERS)) return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.tot + OSMT_CS_T_BAD_CLASS, 0xFF, 8u, st);
    if (e != hipSuccess) return e;
    if (a.n_classes) hipLaunchKernelGGL(k_cs_class_layers, grid_of(a.n_classes), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_cs_count(const osmt_cs_pass& a, hipStream_t st) {
    if (a.n_pairs) {
        if (a.R.flags & OSMT_RULES_CLASS_LAYERS)
            hipLaunchKernelGGL(k_cs_count<true>, grid_of(a.n_pairs), dim3(WG), 0, st, a);
        else
            hipLaunchKernelGGL(k_cs_count<false>, grid_of(a.n_pairs), dim3(WG), 0, st, a);
    }
    return osmt_tq_scan(a.pair_pos, a.n_pairs, a.blk, a.tot + OSMT_CS_T_STYLES, st);
}

hipError_t osmt_launch_cs_fold(const osmt_cs_pass& a, hipStream_t st) {
    if (a.n_pairs && a.n_styles) {
        const uint32_t blocks = (uint32_t)(((unsigned long long)a.n_pairs * GROUP + WG - 1u) / WG);
        if (a.R.flags & OSMT_RULES_CLASS_LAYERS)
            hipLaunchKernelGGL((k_cs_fold<LC, true>), dim3(blocks), dim3(WG), 0, st, a);
        else
            hipLaunchKernelGGL((k_cs_fold<L, false>), dim3(blocks), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_cs_records, grid_of(a.n_styles), dim3(WG), 0, st, a);
    }
    return osmt_tq_scan(a.bind_pos, a.n_styles, a.blk, a.tot + OSMT_CS_T_BINDINGS, st);
}

hipError_t osmt_launch_cs_distinct(const osmt_cs_pass& a, hipStream_t st) {
    if (a.n_styles) {
        const size_t bytes = ((size_t)a.table_mask + 1u) * 4u;
        for (int k = 0; k < 2; ++k) {
            hipError_t e = hipMemsetAsync(a.table[k], 0xFF, bytes, st);
            if (e == hipSuccess) e = hipMemsetAsync(a.lowest[k], 0xFF, bytes, st);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_cs_insert<0>, grid_of(a.n_styles), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_cs_insert<1>, grid_of(a.n_styles), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_cs_mark<0>, grid_of(a.n_styles), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_cs_mark<1>, grid_of(a.n_styles), dim3(WG), 0, st, a);
    }
    hipError_t e = osmt_tq_scan(a.first_pos[0], a.n_styles, a.blk, a.tot + OSMT_CS_T_AREA, st);
    if (e == hipSuccess) e = osmt_tq_scan(a.first_pos[1], a.n_styles, a.blk, a.tot + OSMT_CS_T_LABEL, st);
    return e;
}

hipError_t osmt_launch_cs_rank(const osmt_cs_pass& a, hipStream_t st) {
    if (a.n_styles) hipLaunchKernelGGL(k_cs_rank, grid_of(a.n_styles), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.dash_pos, a.n_area, a.blk, a.tot + OSMT_CS_T_DASHES, st);
}

hipError_t osmt_launch_cs_compact(const osmt_cs_pass& a, hipStream_t st) {
    const uint32_t n = a.n_area > a.n_label ? a.n_area : a.n_label;
    if (n) hipLaunchKernelGGL(k_cs_compact, grid_of(n), dim3(WG), 0, st, a);
    hipError_t e = hipMemsetAsync(a.zoom_differs, 0, Z * 4u, st);
    if (e != hipSuccess) return e;
    if (a.n_pairs) hipLaunchKernelGGL(k_cs_zoom_differs, grid_of(a.n_pairs), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_cs_range_count(const osmt_cs_pass& a, hipStream_t st) {
    const uint32_t n = a.n_ranges * a.n_classes;
    if (n) hipLaunchKernelGGL(k_cs_range_count, grid_of(n), dim3(WG), 0, st, a);
    hipError_t e = osmt_tq_scan(a.rs_pos, n, a.blk, a.tot + OSMT_CS_T_RANGE_STYLES, st);
    if (e == hipSuccess) e = osmt_tq_scan(a.rb_pos, n, a.blk, a.tot + OSMT_CS_T_RANGE_BINDINGS, st);
    return e;
}

hipError_t osmt_launch_cs_range_emit(const osmt_cs_pass& a, hipStream_t st) {
    const uint32_t n = a.n_ranges * a.n_classes;
    if (n) {
        hipLaunchKernelGGL(k_cs_range_emit, grid_of(n), dim3(WG), 0, st, a);
        return hipGetLastError();
    }
    /* no class: every range's offsets are the one entry 0 */
    const hipError_t e = hipMemsetAsync(a.out_style_off, 0, (size_t)a.n_ranges * 4u, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.out_bind_off, 0, (size_t)a.n_ranges * 4u, st);
}
