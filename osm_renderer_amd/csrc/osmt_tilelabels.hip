/*
 * osmt_tilelabels.hip — node labels of scenes built from tile coordinates (osmt_scene_build_tile_labels): what
 * Styler::style_entities(nodes, zoom, true) (mapcss/styler.rs:128-165) and Labeler::label_entity (draw/labeler.rs:16-106,
 * font/text_placer.rs:24-58) do per node of a tile on the reference's worker thread, for a whole batch.  The query in front —
 * span, columns, gather, sort of the 3 x 3 neighbourhood's node lists — is the k_tq_* stages of osmt_tilequery.hip over
 * the node pools.  The host twin, and the yardstick of the tests, is osmt::node_labels_of_tile (host/osmt_tilelabels.hpp).
 * gfx950 only.
 *
 *   k_tl_mark    one lane per sorted candidate: 0 for a repeat of its predecessor and for a node an id filter does not
 *                list (reader.rs:95-99), else the number of bindings of the node under the tile's zoom.  A scan turns the
 *                counts into label positions.
 *   k_tl_tiles   one lane per tile: job_label_off, the most labels of a tile, the first tile over OSMT_TILE_LABELS_MAX.
 *   k_tl_expand  one lane per candidate again: per (node, binding) a 16-byte key rank:32 | gid:64 | position in the tile:32
 *                and, by that position, the binding and the node.  The rank is the style's dense rank under (layer or 0,
 *                z_index); the position makes the order total and is what the stability of sort_by preserves: elements
 *                arrive in (node id ascending, push order).
 *   k_tl_sort    one workgroup per tile: the bitonic network of osmt_bitonic.h, in LDS up to OSMT_STYLED_LDS_AREAS keys and
 *                in place in device memory beyond.
 *   k_tl_count   one lane per sorted label: the chars of its text (0 without text).  A scan gives the char positions.
 *   k_tl_emit    one lane per sorted label: its osmt_label and osmt_string_run.
 *   k_tl_chars   one lane per char: its label by bisection over the char positions, the code point copied.
 *
 * The scans are 32-bit with 64-bit block totals (osmt_tq_scan): the host reads the totals back and launches nothing that
 * stores through an offset before it has seen them fit.  Every index read here was checked on the host when the tables were
 * registered; every store lands below a total the arrays were sized with; every buffer is written before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_bitonic.h"
#include "osmt_internal.h"
#include "osmt_project.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t SORT_WG = 1024u;

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

__global__ __launch_bounds__(256) void k_tl_mark(osmt_tl_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p == 0u) {
        P.tot[OSMT_TL_MAX_LABELS] = 0ull;
        P.tot[OSMT_TL_OVER] = ~0ull;
    }
    if (p >= P.n_cand) return;
    const uint32_t t = owner_of(P.t_base, P.n_tiles, p);
    const uint32_t id = P.cand[p];
    bool first = p == P.t_base[t] || P.cand[p - 1u] != id;
    if (P.keep_node && !((P.keep_node[id >> 5] >> (id & 31u)) & 1u)) first = false; /* filter_entities_by_ids; uniform: a kernel argument */
    const osmt_tl_bind_dev B = P.bind[P.q[t].zoom];
    P.lpos[p] = first ? B.node_off[id + 1u] - B.node_off[id] : 0u;
}

/* a tile's unique nodes are counted once each and a table holds fewer than 2^32 bindings: its count is exact even where
 * the positions wrapped */
__global__ __launch_bounds__(256) void k_tl_tiles(osmt_tl_pass P) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= P.n_tiles) return;
    const uint32_t a0 = P.lpos[P.t_base[t]], a1 = P.lpos[P.t_base[t + 1u]];
    const uint32_t n = a1 - a0;
    P.job_label_off[t] = a0;
    if (t == P.n_tiles - 1u) P.job_label_off[P.n_tiles] = a1;
    if (n) atomicMax(P.tot + OSMT_TL_MAX_LABELS, (unsigned long long)n);
    if (n > OSMT_TILE_LABELS_MAX) atomicMin(P.tot + OSMT_TL_OVER, (unsigned long long)t);
}

__global__ __launch_bounds__(256) void k_tl_expand(osmt_tl_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_cand) return;
    const uint32_t a0 = P.lpos[p], n = P.lpos[p + 1u] - a0;
    if (n == 0u) return;
    const uint32_t t = owner_of(P.t_base, P.n_tiles, p);
    const uint32_t id = P.cand[p];
    const osmt_tl_bind_dev B = P.bind[P.q[t].zoom];
    const uint32_t b0 = B.node_off[id], base = P.job_label_off[t];
    const unsigned long long gid = P.node_gid[id];
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t e = a0 + j;
        const unsigned long long rank = P.style_rank[B.bindings[b0 + j].style];
        P.keys[e] = make_ulonglong2((rank << 32) | (gid >> 32), (gid << 32) | (unsigned long long)(e - base));
        P.el_bind[e] = b0 + j;
        P.el_node[e] = id;
    }
}

struct key_lt {
    __device__ __forceinline__ bool operator()(const ulonglong2& a, const ulonglong2& b) const { return a.x < b.x || (a.x == b.x && a.y < b.y); }
};

__global__ __launch_bounds__(1024) void k_tl_sort(osmt_tl_pass P) {
    __shared__ ulonglong2 lds_keys[OSMT_STYLED_LDS_AREAS];
    const uint32_t t = blockIdx.x;
    const uint32_t base = P.job_label_off[t], n = P.job_label_off[t + 1u] - base;
    if (n < 2u) return; /* uniform over the workgroup */
    ulonglong2* gk = P.keys + base;
    uint32_t N = 1u;
    while (N < n) N <<= 1;
    if (n <= OSMT_STYLED_LDS_AREAS) {
        for (uint32_t i = threadIdx.x; i < n; i += SORT_WG) lds_keys[i] = gk[i];
        __syncthreads();
        osmt_bitonic<SORT_WG>(lds_keys, n, N, key_lt{});
        for (uint32_t i = threadIdx.x; i < n; i += SORT_WG) gk[i] = lds_keys[i];
    } else {
        osmt_bitonic<SORT_WG>(gk, n, N, key_lt{}); /* a workgroup sees its own global stores behind a barrier */
    }
}

/* sorted label e: whose it is and what Labeler::label_entity does with it */
struct label_of {
    uint32_t tile, node, text_src, n_chars;
    osmt_label_style_rec style;
    bool has_text;
};

__device__ __forceinline__ void eval(const osmt_tl_pass& P, uint32_t e, label_of& o) {
    const uint32_t t = owner_of(P.job_label_off, P.n_tiles, e);
    const uint32_t u = P.job_label_off[t] + (uint32_t)P.keys[e].y; /* the element's position before the sort */
    const osmt_tl_bind_dev B = P.bind[P.q[t].zoom];
    const osmt_label_binding b = B.bindings[P.el_bind[u]];
    o.tile = t;
    o.node = P.el_node[u];
    o.style = P.styles[b.style];
    /* text_placer.rs:37-47: a font size, the tag, and a position that is Center for a node */
    o.has_text = o.style.has_text_style && o.style.has_font_size && b.text != OSMT_TEXT_NONE && o.style.text_position != OSMT_LABEL_POSITION_LINE;
    o.text_src = o.has_text ? B.text_off[b.text] : 0u;
    o.n_chars = o.has_text ? B.text_off[b.text + 1u] - o.text_src : 0u;
}

__global__ __launch_bounds__(256) void k_tl_count(osmt_tl_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_labels) return;
    label_of o;
    eval(P, e, o);
    P.chpos[e] = o.n_chars;
    P.ch_src[e] = o.text_src;
}

__global__ __launch_bounds__(256) void k_tl_emit(osmt_tl_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_labels) return;
    label_of o;
    eval(P, e, o);
    const osmt_query_tile q = P.q[o.tile];
    int32_t x, y;
    project_point(P.nodes[2u * o.node], P.nodes[2u * o.node + 1u], q.zoom, q.x, q.y, (double)P.scale, &x, &y);
    const bool icon = o.style.has_icon != 0;
    osmt_label l;
    l.has_icon = icon ? 1 : 0;
    l.has_text = o.has_text ? 1 : 0;
    const bool col = o.has_text && o.style.has_text_color;
    l.text_color[0] = col ? o.style.text_color[0] : 0;
    l.text_color[1] = col ? o.style.text_color[1] : 0;
    l.text_color[2] = col ? o.style.text_color[2] : 0;
    l._pad[0] = l._pad[1] = l._pad[2] = 0;
    l.image_id = icon ? o.style.icon_image : 0u;
    l.seg_off = P.chpos[e];
    l.n_segs = o.n_chars;
    l._reserved = 0u;
    l.icon_center_x = (double)x;
    l.icon_center_y = (double)y;
    P.labels[e] = l;
    osmt_string_run r;
    r.position = OSMT_TEXT_CENTER;
    r.y_offset = icon ? P.icon_h[o.style.icon_image] / 2u : 0u; /* labeler.rs:61-62 */
    r.pt_off = r.n_pts = 0u;
    r.font_id = o.has_text ? o.style.font_id : 0u;
    r._pad = 0u;
    r.font_size = o.has_text ? o.style.font_size * (double)P.scale : 0.0;
    r.center_x = (double)x;
    r.center_y = (double)y;
    r._reserved[0] = r._reserved[1] = 0.0;
    P.runs[e] = r;
}

__global__ __launch_bounds__(256) void k_tl_chars(osmt_tl_pass P) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= P.n_chars) return;
    const uint32_t e = owner_of(P.chpos, P.n_labels, c);
    const uint32_t t = owner_of(P.job_label_off, P.n_tiles, e);
    P.chars[c] = P.bind[P.q[t].zoom].chars[P.ch_src[e] + (c - P.chpos[e])];
}

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

}  // namespace

hipError_t osmt_launch_tl_mark(const osmt_tl_pass& a, hipStream_t st) {
    hipLaunchKernelGGL(k_tl_mark, a.n_cand ? grid_of(a.n_cand) : dim3(1), dim3(WG), 0, st, a);
    const hipError_t e = osmt_tq_scan(a.lpos, a.n_cand, a.blk, a.tot + OSMT_TL_LABELS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tl_tiles, grid_of(a.n_tiles), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tl_order(const osmt_tl_pass& a, hipStream_t st) {
    if (a.n_labels) {
        hipLaunchKernelGGL(k_tl_expand, grid_of(a.n_cand), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_tl_sort, dim3(a.n_tiles), dim3(SORT_WG), 0, st, a);
        hipLaunchKernelGGL(k_tl_count, grid_of(a.n_labels), dim3(WG), 0, st, a);
    }
    return osmt_tq_scan(a.chpos, a.n_labels, a.blk, a.tot + OSMT_TL_CHARS, st);
}

hipError_t osmt_launch_tl_sort(const osmt_tl_pass& a, hipStream_t st) {
    if (a.n_tiles) hipLaunchKernelGGL(k_tl_sort, dim3(a.n_tiles), dim3(SORT_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_tl_emit(const osmt_tl_pass& a, hipStream_t st) {
    if (a.n_labels) hipLaunchKernelGGL(k_tl_emit, grid_of(a.n_labels), dim3(WG), 0, st, a);
    if (a.n_chars) hipLaunchKernelGGL(k_tl_chars, grid_of(a.n_chars), dim3(WG), 0, st, a);
    return hipGetLastError();
}
