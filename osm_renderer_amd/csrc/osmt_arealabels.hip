/*
 * osmt_arealabels.hip — labels of ways and multipolygons of scenes built from tile coordinates
 * (osmt_scene_build_tile_labels_all): what Styler::style_areas(ways, multipolygons, zoom, true) (mapcss/styler.rs:168-203) and
 * Labeler::label_entity (draw/labeler.rs:16-106, font/text_placer.rs:24-168) do per area of a tile on the reference's worker
 * thread, for a whole batch.  In front of these kernels run the k_tq_* stages of osmt_tilequery.hip over the way and
 * multipolygon pools — span, columns, gather, sort, and mark + tiles with the LABEL bindings' offsets, which number every
 * (entity, binding) of a tile — between them the k_an_* stages and the search of osmt_polylabel.hip, fed with requests that
 * never leave the device, and k_tl_sort of osmt_tilelabels.hip.  The host twin, and the yardstick of the tests, is
 * osmt::area_labels_of_tile (host/osmt_arealabels.hpp).  gfx950 only.
 *
 *   k_al_expand    one lane per sorted candidate: per (entity, binding) the 16-byte key rank:32 | gid:64 | position:32 of
 *                  k_tl_expand and, by that position, the binding and the candidate.  A tile's multipolygon elements are
 *                  numbered in front of its way elements (the query numbers them behind): with the position as the last
 *                  key word ONE sort is the two stable sorts and the merge of style_areas, in which a multipolygon goes first
 *                  unless it compares Greater.  Also per candidate: whether any of its labels asks for the anchor (an icon,
 *                  or a text that reaches Center) and, by bisection, whether the caller handed that anchor in.
 *   k_al_requests  one lane per candidate: the osmt_label_tile_request of a pair that is searched, at its scanned position.
 *   k_al_declined  one lane per request, behind the search: how many were answered TOO_LARGE, and the first.
 *   k_al_count     one lane per sorted label: its chars and, for a text along a way, the way's points.  Two scans.
 *   k_al_project   one lane per way point: project_point of its node under the label's tile, in the way's own order.
 *   k_al_waypts    one lane per way point again: the run in walking order — reversed iff first.x > last.x of the projected
 *                  points (text_placer.rs:65-67); it reads the pool k_al_project wrote and writes another.
 *   k_al_emit      one lane per sorted label: its osmt_label and osmt_string_run.
 *   k_al_chars     one lane per char: its label by bisection over the char positions, the code point copied.
 *
 * The scans are 32-bit with 64-bit block totals (osmt_tq_scan): the host reads the totals back and launches nothing that
 * stores through an offset before it has seen them fit.  Every index read here was checked on the host when the tables were
 * registered; every store lands below a total the arrays were sized with; every buffer is written before it is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"
#include "osmt_project.h"

namespace {

constexpr uint32_t WG = 256u;
constexpr uint32_t NONE = 0xFFFFFFFFu;

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

/* candidate slot p: its tile, kind and id */
struct cand_of {
    uint32_t tile, id, first, n_ways; /* first: the tile's first slot; n_ways: its way candidates */
    bool mp;
};

__device__ __forceinline__ void slot_eval(const osmt_al_pass& P, uint32_t p, cand_of& o) {
    uint32_t lo = 0u, hi = P.n_tiles - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.t_wbase[mid + 1u] + P.t_mbase[mid + 1u] > p)
            hi = mid;
        else
            lo = mid + 1u;
    }
    const uint32_t tw = P.t_wbase[lo];
    o.tile = lo;
    o.first = tw + P.t_mbase[lo];
    o.n_ways = P.t_wbase[lo + 1u] - tw;
    o.mp = p - o.first >= o.n_ways;
    o.id = P.cand[p];
}

/* text_placer.rs:37-47: a text style, a font size and the tag */
__device__ __forceinline__ bool text_ok(const osmt_label_style_rec& s, const osmt_label_binding& b) {
    return s.has_text_style && s.has_font_size && b.text != OSMT_TEXT_NONE;
}
/* drawer.rs:233-250: Line for a way, Center for a multipolygon, unless the style says otherwise */
__device__ __forceinline__ bool is_line(const osmt_label_style_rec& s, bool mp) {
    return s.text_position == OSMT_LABEL_POSITION_NONE ? !mp : s.text_position == OSMT_LABEL_POSITION_LINE;
}
/* labeler.rs:55-57 and text_placer.rs:113: the two callers of get_label_position */
__device__ __forceinline__ bool wants_anchor(const osmt_label_style_rec& s, const osmt_label_binding& b, bool mp) {
    return s.has_icon || (text_ok(s, b) && !is_line(s, mp));
}

/* the entry of (tile, entity) in the caller's anchors, or NONE */
__device__ __forceinline__ uint32_t find_anchor(const osmt_al_pass& P, uint32_t tile, uint32_t entity) {
    uint32_t lo = 0u, hi = P.n_anchors;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const osmt_area_anchor a = P.anchors[mid];
        if (a.tile < tile || (a.tile == tile && a.entity < entity))
            lo = mid + 1u;
        else
            hi = mid;
    }
    if (lo < P.n_anchors && P.anchors[lo].tile == tile && P.anchors[lo].entity == entity) return lo;
    return NONE;
}

__global__ __launch_bounds__(256) void k_al_expand(osmt_al_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_cand) return;
    const uint32_t a0 = P.apos[p], n = P.apos[p + 1u] - a0;
    uint32_t need = 0u, ov = NONE;
    if (n) {
        cand_of c;
        slot_eval(P, p, c);
        const osmt_al_bind_dev B = P.bind[P.q[c.tile].zoom];
        const uint32_t b0 = c.mp ? B.mp_off[c.id] : B.way_off[c.id];
        const osmt_label_binding* bb = c.mp ? B.mp_bind : B.way_bind;
        const uint32_t base = P.job_label_off[c.tile];
        const uint32_t wl = P.apos[c.first + c.n_ways] - base;           /* the tile's way labels */
        const uint32_t ml = P.job_label_off[c.tile + 1u] - base - wl;    /* its multipolygon labels */
        const uint32_t pos0 = c.mp ? a0 - base - wl : a0 - base + ml;    /* multipolygons in front */
        const unsigned long long gid = c.mp ? P.geo.mp_gid[c.id] : P.geo.way_gid[c.id];
        bool wants = false;
        for (uint32_t j = 0; j < n; ++j) {
            const osmt_label_binding b = bb[b0 + j];
            const unsigned long long rank = P.style_rank[b.style];
            const uint32_t e = base + pos0 + j;
            P.keys[e] = make_ulonglong2((rank << 32) | (gid >> 32), (gid << 32) | (unsigned long long)(pos0 + j));
            P.el_bind[e] = b0 + j;
            P.el_slot[e] = p;
            wants = wants || wants_anchor(P.styles[b.style], b, c.mp);
        }
        if (wants) {
            ov = find_anchor(P, c.tile, c.id | (c.mp ? OSMT_STYLED_MULTIPOLYGON : 0u));
            need = ov == NONE ? 1u : 0u;
        }
    }
    P.need[p] = need;
    P.ov[p] = ov;
}

__global__ __launch_bounds__(256) void k_al_requests(osmt_al_pass P) {
    const uint32_t p = blockIdx.x * WG + threadIdx.x;
    if (p >= P.n_cand) return;
    const uint32_t r = P.need[p];
    if (P.need[p + 1u] == r) return;
    cand_of c;
    slot_eval(P, p, c);
    P.req[r] = osmt_label_tile_request{c.id | (c.mp ? OSMT_STYLED_MULTIPOLYGON : 0u), c.tile};
}

__global__ __launch_bounds__(256) void k_al_declined(osmt_al_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_req) return;
    if (P.pos[i].status != OSMT_LABEL_TOO_LARGE) return;
    atomicAdd(P.tot + OSMT_AL_DECLINED, 1ull);
    atomicMin(P.tot + OSMT_AL_FIRST_DECLINED, (unsigned long long)i);
}

/* sorted label e: whose it is and what Labeler::label_entity does with it */
struct label_of {
    uint32_t tile, id, text_src, n_chars, n_pts;
    osmt_label_style_rec style;
    bool icon, has_text, line;
    double ax, ay; /* the anchor where this label asked for one and it is Some, else 0 */
};

__device__ __forceinline__ void eval(const osmt_al_pass& P, uint32_t e, label_of& o) {
    const uint32_t t = owner_of(P.job_label_off, P.n_tiles, e);
    const uint32_t u = P.job_label_off[t] + (uint32_t)P.keys[e].y; /* the element's position before the sort */
    const uint32_t p = P.el_slot[u];
    const uint32_t tw = P.t_wbase[t];
    const bool mp = p - (tw + P.t_mbase[t]) >= P.t_wbase[t + 1u] - tw;
    const osmt_al_bind_dev B = P.bind[P.q[t].zoom];
    const osmt_label_binding b = (mp ? B.mp_bind : B.way_bind)[P.el_bind[u]];
    o.tile = t;
    o.id = P.cand[p];
    o.style = P.styles[b.style];
    const bool txt = text_ok(o.style, b), line = is_line(o.style, mp);
    uint32_t status = OSMT_AL_NO_ANCHOR;
    o.ax = o.ay = 0.0;
    if (wants_anchor(o.style, b, mp)) {
        const uint32_t ov = P.ov[p];
        if (ov != NONE) {
            const osmt_area_anchor a = P.anchors[ov];
            status = a.status, o.ax = a.x, o.ay = a.y;
        } else {
            const osmt_label_position a = P.pos[P.need[p]]; /* the pair asked, so it has a request */
            status = a.status, o.ax = a.x, o.ay = a.y;
        }
        if (status != OSMT_LABEL_OK) o.ax = o.ay = 0.0;
    }
    const bool ok = status == OSMT_LABEL_OK;
    o.icon = o.style.has_icon && ok;
    /* Center needs the anchor (text_placer.rs:113-116), Line the way points: a multipolygon has none (labelable.rs:53-55) */
    o.has_text = txt && (line ? !mp : ok);
    o.line = o.has_text && line;
    o.text_src = o.has_text ? B.text_off[b.text] : 0u;
    o.n_chars = o.has_text ? B.text_off[b.text + 1u] - o.text_src : 0u;
    o.n_pts = o.line ? P.geo.way_off[o.id + 1u] - P.geo.way_off[o.id] : 0u;
}

__global__ __launch_bounds__(256) void k_al_count(osmt_al_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_labels) return;
    label_of o;
    eval(P, e, o);
    P.chpos[e] = o.n_chars;
    P.ch_src[e] = o.text_src;
    P.ptpos[e] = o.n_pts;
    P.pt_src[e] = o.line ? P.geo.way_off[o.id] : 0u;
}

__global__ __launch_bounds__(256) void k_al_project(osmt_al_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_pts) return;
    const uint32_t e = owner_of(P.ptpos, P.n_labels, i);
    const osmt_query_tile q = P.q[owner_of(P.job_label_off, P.n_tiles, e)];
    const uint32_t node = P.geo.idx[P.pt_src[e] + (i - P.ptpos[e])];
    int32_t x, y;
    project_point(P.geo.nodes[2u * node], P.geo.nodes[2u * node + 1u], q.zoom, q.x, q.y, (double)P.scale, &x, &y);
    P.pts_fwd[i] = make_int2(x, y);
}

__global__ __launch_bounds__(256) void k_al_waypts(osmt_al_pass P) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= P.n_pts) return;
    const uint32_t e = owner_of(P.ptpos, P.n_labels, i);
    const uint32_t a = P.ptpos[e], last = P.ptpos[e + 1u] - 1u;
    const bool rev = P.pts_fwd[a].x > P.pts_fwd[last].x; /* text_placer.rs:65-67 */
    P.pts[i] = P.pts_fwd[rev ? last - (i - a) : i];
}

__global__ __launch_bounds__(256) void k_al_emit(osmt_al_pass P) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= P.n_labels) return;
    label_of o;
    eval(P, e, o);
    osmt_label l;
    l.has_icon = o.icon ? 1 : 0;
    l.has_text = o.has_text ? 1 : 0;
    const bool col = o.has_text && o.style.has_text_color;
    l.text_color[0] = col ? o.style.text_color[0] : 0;
    l.text_color[1] = col ? o.style.text_color[1] : 0;
    l.text_color[2] = col ? o.style.text_color[2] : 0;
    l._pad[0] = l._pad[1] = l._pad[2] = 0;
    l.image_id = o.icon ? o.style.icon_image : 0u;
    l.seg_off = P.chpos[e];
    l.n_segs = o.n_chars;
    l._reserved = 0u;
    l.icon_center_x = o.ax;
    l.icon_center_y = o.ay;
    P.labels[e] = l;
    osmt_string_run r;
    r.position = o.line ? OSMT_TEXT_LINE : OSMT_TEXT_CENTER;
    r.y_offset = o.icon ? P.icon_h[o.style.icon_image] / 2u : 0u; /* labeler.rs:61-62 */
    r.pt_off = o.line ? P.ptpos[e] : 0u;
    r.n_pts = o.n_pts;
    r.font_id = o.has_text ? o.style.font_id : 0u;
    r._pad = 0u;
    r.font_size = o.has_text ? o.style.font_size * (double)P.scale : 0.0;
    r.center_x = o.ax;
    r.center_y = o.ay;
    r._reserved[0] = r._reserved[1] = 0.0;
    P.runs[e] = r;
}

__global__ __launch_bounds__(256) void k_al_chars(osmt_al_pass P) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= P.n_chars) return;
    const uint32_t e = owner_of(P.chpos, P.n_labels, c);
    const uint32_t t = owner_of(P.job_label_off, P.n_tiles, e);
    P.chars[c] = P.bind[P.q[t].zoom].chars[P.ch_src[e] + (c - P.chpos[e])];
}

inline dim3 grid_of(uint32_t n) { return dim3((n + WG - 1u) / WG); }

}  // namespace

hipError_t osmt_launch_al_expand(const osmt_al_pass& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.tot, 0, OSMT_AL_N * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.tot + OSMT_AL_FIRST_DECLINED, 0xFF, 8, st);
    if (e != hipSuccess) return e;
    if (a.n_cand) hipLaunchKernelGGL(k_al_expand, grid_of(a.n_cand), dim3(WG), 0, st, a);
    return osmt_tq_scan(a.need, a.n_cand, a.blk, a.tot + OSMT_AL_REQS, st);
}

hipError_t osmt_launch_al_requests(const osmt_al_pass& a, hipStream_t st) {
    if (a.n_req) hipLaunchKernelGGL(k_al_requests, grid_of(a.n_cand), dim3(WG), 0, st, a);
    return hipGetLastError();
}

hipError_t osmt_launch_al_count(const osmt_al_pass& a, hipStream_t st) {
    if (a.n_req) hipLaunchKernelGGL(k_al_declined, grid_of(a.n_req), dim3(WG), 0, st, a);
    if (a.n_labels) hipLaunchKernelGGL(k_al_count, grid_of(a.n_labels), dim3(WG), 0, st, a);
    const hipError_t e = osmt_tq_scan(a.chpos, a.n_labels, a.blk, a.tot + OSMT_AL_CHARS, st);
    if (e != hipSuccess) return e;
    return osmt_tq_scan(a.ptpos, a.n_labels, a.blk, a.tot + OSMT_AL_PTS, st);
}

hipError_t osmt_launch_al_emit(const osmt_al_pass& a, hipStream_t st) {
    if (a.n_pts) {
        hipLaunchKernelGGL(k_al_project, grid_of(a.n_pts), dim3(WG), 0, st, a);
        hipLaunchKernelGGL(k_al_waypts, grid_of(a.n_pts), dim3(WG), 0, st, a);
    }
    if (a.n_labels) hipLaunchKernelGGL(k_al_emit, grid_of(a.n_labels), dim3(WG), 0, st, a);
    if (a.n_chars) hipLaunchKernelGGL(k_al_chars, grid_of(a.n_chars), dim3(WG), 0, st, a);
    return hipGetLastError();
}
