/*
 * osmt_host_polygons.cpp — host side of libosmtile.so: multipolygon rings assembled from relations' member ways
 * (include/osmtile.h, osmt_polygons.hip).  One call uploads the caller's arrays, reads the segment total back before anything
 * is sized, sorts the (vertex, endpoint) pairs with the pyramid's radix sort, walks every relation and compacts the accepted
 * ones into the arrays osmt_geodata_desc takes.  Shares osmt_host.h with the other host files.
 */
#include "osmt_host.h"
#include "osmt_probe_slots.h" /* osmt_vertex_slots: the vertex table's size */

using namespace osmt_host;

/* an assembly's result: one dev_alloc buffer, given back by osmt_polygons_free */
struct osmt_polygons {
    osmt_ctx* ctx = nullptr;
    char* pool = nullptr;
    const uint32_t *poly_node_off = nullptr, *poly_nodes = nullptr, *mp_poly_off = nullptr, *mp_polys = nullptr, *mp_rel = nullptr;
    const uint64_t* mp_ids = nullptr;
    const osmt_relation_status* status = nullptr;
    size_t n_polys = 0, n_poly_nodes = 0, n_mps = 0, n_rels = 0;
};

namespace {

const uint32_t ZERO_OFF[1] = {0u}; /* the offsets of no ways / no relations, where the caller gave none */

int validate_relations(const osmt_relations_desc* d, uint64_t* out_segments = nullptr) {
    if (!d) return fail(OSMT_INVALID_ARG, "NULL argument");
    const struct {
        const void* p;
        size_t n;
        const char* name;
    } arrays[] = {{d->nodes, d->n_nodes, "nodes"},
                  {d->way_node_off, d->n_ways, "way_node_off"},
                  {d->way_nodes, d->n_way_nodes, "way_nodes"},
                  {d->relation_ids, d->n_relations, "relation_ids"},
                  {d->relation_way_off, d->n_relations, "relation_way_off"},
                  {d->relation_ways, d->n_relation_ways, "relation_ways"},
                  {d->relation_way_inner, d->n_relation_ways, "relation_way_inner"}};
    for (const auto& a : arrays)
        if (!a.p && a.n) return fail(OSMT_INVALID_ARG, "relations: %s is NULL with a count of %zu", a.name, a.n);
    if (d->n_nodes >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "relations: %zu nodes do not fit 32-bit indices (at most %llu)", d->n_nodes, 0xFFFFFFFEull);
    if (d->n_relations >= 0x80000000ull) return fail(OSMT_UNSUPPORTED, "relations: %zu relations (at most 2^31 - 1)", d->n_relations);
    const uint32_t *way_off = d->way_node_off ? d->way_node_off : ZERO_OFF, *rel_off = d->relation_way_off ? d->relation_way_off : ZERO_OFF;
    if (!d->way_node_off && d->n_way_nodes) return fail(OSMT_INVALID_ARG, "relations: %zu way nodes and no ways", d->n_way_nodes);
    if (!d->relation_way_off && d->n_relation_ways) return fail(OSMT_INVALID_ARG, "relations: %zu way references and no relations", d->n_relation_ways);
    int rc = check_offsets_of("relations", "way_node_off", way_off, d->n_ways, d->n_way_nodes);
    if (rc == OSMT_OK) rc = check_offsets_of("relations", "relation_way_off", rel_off, d->n_relations, d->n_relation_ways);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < d->n_way_nodes; ++i)
        if (d->way_nodes[i] >= d->n_nodes) return fail(OSMT_INVALID_ARG, "relations: way_nodes[%zu] = %u is not a node (%zu nodes)", i, d->way_nodes[i], d->n_nodes);
    uint64_t segments = 0;
    for (size_t i = 0; i < d->n_relation_ways; ++i) {
        const uint32_t w = d->relation_ways[i];
        if (w >= d->n_ways) return fail(OSMT_INVALID_ARG, "relations: relation_ways[%zu] = %u is not a way (%zu ways)", i, w, d->n_ways);
        if (d->relation_way_inner[i] > 1u)
            return fail(OSMT_INVALID_ARG, "relations: relation_way_inner[%zu] = %u is not a role (0: outer, 1: inner)", i, (unsigned)d->relation_way_inner[i]);
        const uint32_t len = way_off[w + 1] - way_off[w];
        segments += len ? len - 1u : 0u;
    }
    if (segments >= 0x80000000ull)
        return fail(OSMT_UNSUPPORTED, "relations: %llu segments (at most 2^31 - 1: an endpoint is 2 * segment + side in 32 bits)", (unsigned long long)segments);
    if (out_segments) *out_segments = segments;
    return OSMT_OK;
}

/* the pyramid's radix sort over n pairs in (key[0], id[0]); returns which of the two buffers holds them sorted */
int sort_pairs(hipStream_t st, unsigned long long* key[2], uint32_t* id[2], uint32_t n, uint32_t* counts, uint32_t* d_hist, unsigned long long* blk,
               unsigned long long* tot, int* at) {
    *at = 0;
    if (n < 2u) return OSMT_OK;
    std::vector<uint32_t> hist(OSMT_PYR_DIGITS * 256);
    HIP_TRY(osmt_launch_pyr_digits(key[0], id[0], n, d_hist, st));
    HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, hist.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) { /* a digit whose histogram has one non-empty bin is not sorted on */
        bool one_bin = false;
        for (uint32_t b = 0; b < 256; ++b) one_bin = one_bin || hist[d * 256 + b] == n;
        if (one_bin) continue;
        HIP_TRY(osmt_launch_pyr_pass(key[*at], id[*at], n, d, counts, blk, tot, key[*at ^ 1], id[*at ^ 1], st));
        *at ^= 1;
    }
    return OSMT_OK;
}

enum { EV_START, EV_COUNT, EV_VERTICES, EV_SORT, EV_WALK, EV_EMIT, EV_N };

int assemble_body(osmt_ctx* ctx, const osmt_relations_desc* d, osmt_polygons** out) {
    if (!ctx || !d || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = validate_relations(d);
    if (rc != OSMT_OK) return rc;
    uint32_t hash_bits;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        hash_bits = ctx->vertex_hash_bits;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    call_work wg(ctx, "multipolygon assembly");
    rc = wg.begin(EV_N);
    if (rc != OSMT_OK) return rc;
    hipStream_t st = wg.st;
    const auto t_start = std::chrono::steady_clock::now();
    const size_t n_nodes = d->n_nodes, n_ways = d->n_ways, n_rels = d->n_relations, n_refs = d->n_relation_ways;
    osmt_mpa_pass P{};
    P.n_nodes = (uint32_t)n_nodes, P.n_ways = (uint32_t)n_ways, P.n_rels = (uint32_t)n_rels, P.n_refs = (uint32_t)n_refs, P.hash_bits = hash_bits;
    /* work buffer 0: the caller's arrays and everything sized by them */
    {
        pool_layout pl;
        const size_t o_nodes = pl.add(n_nodes * 16), o_woff = pl.add((n_ways + 1) * 4), o_wn = pl.add(d->n_way_nodes * 4), o_ids = pl.add(n_rels * 8);
        const size_t o_roff = pl.add((n_rels + 1) * 4), o_rw = pl.add(n_refs * 4), o_in = pl.add(n_refs), o_ref = pl.add((n_refs + 1) * 4);
        const size_t o_rs = pl.add((n_rels + 1) * 4), o_acc = pl.add((n_rels + 1) * 4), o_rr = pl.add((n_rels + 1) * 4), o_rn = pl.add((n_rels + 1) * 4);
        const size_t o_blk = pl.add((std::max(n_refs, n_rels) / 256 + 2) * 8), o_words = pl.add(OSMT_MPA_WORDS * 8), o_status = pl.add(n_rels * sizeof(osmt_relation_status));
        rc = wg.alloc(0, pl, "relations");
        if (rc != OSMT_OK) return rc;
        char* w = wg.work[0];
        const struct {
            size_t o;
            const void* src;
            size_t bytes;
        } up[] = {{o_nodes, d->nodes, n_nodes * 16},
                  {o_woff, d->way_node_off ? d->way_node_off : ZERO_OFF, (n_ways + 1) * 4},
                  {o_wn, d->way_nodes, d->n_way_nodes * 4},
                  {o_ids, d->relation_ids, n_rels * 8},
                  {o_roff, d->relation_way_off ? d->relation_way_off : ZERO_OFF, (n_rels + 1) * 4},
                  {o_rw, d->relation_ways, n_refs * 4},
                  {o_in, d->relation_way_inner, n_refs}};
        for (const auto& u : up)
            if (u.bytes) HIP_TRY(hipMemcpyAsync(w + u.o, u.src, u.bytes, hipMemcpyHostToDevice, st));
        P.node_bits = (const ulonglong2*)(w + o_nodes), P.way_off = (const uint32_t*)(w + o_woff), P.way_nodes = (const uint32_t*)(w + o_wn);
        P.rel_ids = (const uint64_t*)(w + o_ids), P.rel_way_off = (const uint32_t*)(w + o_roff), P.rel_ways = (const uint32_t*)(w + o_rw);
        P.rel_inner = (const uint8_t*)(w + o_in), P.ref_off = (uint32_t*)(w + o_ref), P.rel_seg = (uint32_t*)(w + o_rs);
        P.rel_acc = (uint32_t*)(w + o_acc), P.rel_rings = (uint32_t*)(w + o_rr), P.rel_nodes = (uint32_t*)(w + o_rn);
        P.blk = (unsigned long long*)(w + o_blk), P.words = (unsigned long long*)(w + o_words), P.status = (osmt_relation_status*)(w + o_status);
    }
    HIP_TRY(wg.mark(EV_START));
    HIP_TRY(osmt_launch_mpa_count(P, st));
    HIP_TRY(wg.mark(EV_COUNT));
    unsigned long long words[OSMT_MPA_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(words, P.words, sizeof words, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    /* the limit, from the 64-bit total, before any pair has a buffer */
    if (words[OSMT_MPA_SEGMENTS] >= 0x80000000ull)
        return fail(OSMT_UNSUPPORTED, "relations: %llu segments (at most 2^31 - 1: an endpoint is 2 * segment + side in 32 bits)", words[OSMT_MPA_SEGMENTS]);
    const size_t S = (size_t)words[OSMT_MPA_SEGMENTS], E = 2 * S;
    P.n_segs = (uint32_t)S;
    unsigned long long* key[2] = {nullptr, nullptr};
    uint32_t* id[2] = {nullptr, nullptr};
    int at = 0;
    if (S) {
        /* at least twice as many slots as endpoints: a power of two, 2^32 at the most (then still more slots than endpoints) */
        const uint64_t slots = osmt_vertex_slots(E);
        P.table_mask = (uint32_t)(slots - 1);
        const size_t n_wg = (E + OSMT_PYR_SORT_BLOCK - 1) / OSMT_PYR_SORT_BLOCK;
        pool_layout pl;
        const size_t o_sn = pl.add(E * 4), o_sr = pl.add(S * 4), o_ss = pl.add(S), o_canon = pl.add(E * 4), o_ent = pl.add(E * 8), o_gs = pl.add(E * 4);
        const size_t o_stamp = pl.add(E * 4), o_rseg = pl.add(S * 4), o_rend = pl.add((S / 3 + 1) * 4);
        rc = wg.alloc(1, pl, "segments");
        if (rc != OSMT_OK) return rc;
        char* w = wg.work[1];
        P.seg_nodes = (uint32_t*)(w + o_sn), P.seg_rel = (uint32_t*)(w + o_sr), P.seg_state = (uint8_t*)(w + o_ss), P.canon = (uint32_t*)(w + o_canon);
        P.ent = (uint2*)(w + o_ent), P.gstart = (uint32_t*)(w + o_gs), P.stamp = (uint32_t*)(w + o_stamp), P.ring_seg = (uint32_t*)(w + o_rseg);
        P.ring_end = (uint32_t*)(w + o_rend);
        pool_layout tl;
        tl.add((size_t)slots * 4);
        rc = wg.alloc(2, tl, "vertex table");
        if (rc != OSMT_OK) return rc;
        P.table = (uint32_t*)wg.work[2];
        pool_layout sl;
        const size_t o_k0 = sl.add(E * 8), o_k1 = sl.add(E * 8), o_i0 = sl.add(E * 4), o_i1 = sl.add(E * 4), o_cnt = sl.add((256 * n_wg + 1) * 4);
        const size_t o_hist = sl.add(OSMT_PYR_DIGITS * 256 * 4), o_blk = sl.add((n_wg + 2) * 8), o_tot = sl.add(8);
        rc = wg.alloc(3, sl, "pairs");
        if (rc != OSMT_OK) return rc;
        char* s = wg.work[3];
        key[0] = (unsigned long long*)(s + o_k0), key[1] = (unsigned long long*)(s + o_k1), id[0] = (uint32_t*)(s + o_i0), id[1] = (uint32_t*)(s + o_i1);
        HIP_TRY(osmt_launch_mpa_vertices(P, key[0], id[0], st));
        HIP_TRY(wg.mark(EV_VERTICES));
        rc = sort_pairs(st, key, id, (uint32_t)E, (uint32_t*)(s + o_cnt), (uint32_t*)(s + o_hist), (unsigned long long*)(s + o_blk), (unsigned long long*)(s + o_tot), &at);
        if (rc != OSMT_OK) return rc;
    } else {
        HIP_TRY(wg.mark(EV_VERTICES));
    }
    HIP_TRY(wg.mark(EV_SORT));
    HIP_TRY(osmt_launch_mpa_walk(P, key[at], id[at], st));
    HIP_TRY(wg.mark(EV_WALK));
    HIP_TRY(hipMemcpyAsync(words, P.words, sizeof words, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t n_mps = (size_t)words[OSMT_MPA_MPS], n_polys = (size_t)words[OSMT_MPA_POLYS], n_poly_nodes = (size_t)words[OSMT_MPA_NODES];
    std::unique_ptr<osmt_polygons> res(new osmt_polygons);
    pool_layout pl;
    const size_t o_po = pl.add((n_polys + 1) * 4), o_pn = pl.add(n_poly_nodes * 4), o_ids = pl.add(n_mps * 8), o_mo = pl.add((n_mps + 1) * 4);
    const size_t o_mp = pl.add(n_polys * 4), o_rel = pl.add(n_mps * 4), o_status = pl.add(n_rels * sizeof(osmt_relation_status));
    char* pool = nullptr;
    rc = wg.alloc(&pool, pl, "result");
    if (rc != OSMT_OK) return rc;
    P.poly_node_off = (uint32_t*)(pool + o_po), P.poly_nodes = (uint32_t*)(pool + o_pn), P.mp_ids = (uint64_t*)(pool + o_ids);
    P.mp_poly_off = (uint32_t*)(pool + o_mo), P.mp_polys = (uint32_t*)(pool + o_mp), P.mp_rel = (uint32_t*)(pool + o_rel);
    hipError_t e = osmt_launch_mpa_emit(P, st);
    if (e == hipSuccess && n_rels) e = hipMemcpyAsync(pool + o_status, P.status, n_rels * sizeof(osmt_relation_status), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = wg.mark(EV_EMIT);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        dev_free(ctx, pool);
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "multipolygon assembly: the emit stage failed: %s", hipGetErrorString(e));
    }
    if (wg.trace)
        fprintf(stderr,
                "osmt multipolygon assembly: %.1f us in all; count %.1f us, segments + vertices %.1f us, sort %.1f us, adjacency + walk %.1f us, emit %.1f us "
                "on the device (%zu relations, %zu segments, %zu multipolygons, %zu polygons, %zu polygon nodes)\n",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(), wg.us(EV_START, EV_COUNT), wg.us(EV_COUNT, EV_VERTICES),
                wg.us(EV_VERTICES, EV_SORT), wg.us(EV_SORT, EV_WALK), wg.us(EV_WALK, EV_EMIT), n_rels, S, n_mps, n_polys, n_poly_nodes);
    res->ctx = ctx, res->pool = pool;
    res->poly_node_off = P.poly_node_off, res->poly_nodes = P.poly_nodes, res->mp_ids = P.mp_ids, res->mp_poly_off = P.mp_poly_off, res->mp_polys = P.mp_polys;
    res->mp_rel = P.mp_rel, res->status = (const osmt_relation_status*)(pool + o_status);
    res->n_polys = n_polys, res->n_poly_nodes = n_poly_nodes, res->n_mps = n_mps, res->n_rels = n_rels;
    ctx->refs.fetch_add(1);
    *out = res.release();
    return OSMT_OK;
}

int read_body(osmt_ctx* ctx, const osmt_polygons* p, uint32_t* polygon_node_off, uint32_t* polygon_nodes, uint64_t* multipolygon_ids,
              uint32_t* multipolygon_polygon_off, uint32_t* multipolygon_polygons, osmt_relation_status* status, uint32_t* multipolygon_relation) {
    if (!ctx || !p) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (p->ctx != ctx) return fail(OSMT_INVALID_ARG, "polygons: the result belongs to another context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (polygon_node_off) HIP_TRY(copy_back(ctx, polygon_node_off, p->poly_node_off, (p->n_polys + 1) * 4));
    if (polygon_nodes && p->n_poly_nodes) HIP_TRY(copy_back(ctx, polygon_nodes, p->poly_nodes, p->n_poly_nodes * 4));
    if (multipolygon_ids && p->n_mps) HIP_TRY(copy_back(ctx, multipolygon_ids, p->mp_ids, p->n_mps * 8));
    if (multipolygon_polygon_off) HIP_TRY(copy_back(ctx, multipolygon_polygon_off, p->mp_poly_off, (p->n_mps + 1) * 4));
    if (multipolygon_polygons && p->n_polys) HIP_TRY(copy_back(ctx, multipolygon_polygons, p->mp_polys, p->n_polys * 4));
    if (status && p->n_rels) HIP_TRY(copy_back(ctx, status, p->status, p->n_rels * sizeof(osmt_relation_status)));
    if (multipolygon_relation && p->n_mps) HIP_TRY(copy_back(ctx, multipolygon_relation, p->mp_rel, p->n_mps * 4));
    return OSMT_OK;
}

}  // namespace

int osmt_validate_relations(const osmt_relations_desc* relations) {
    return guarded([&] { return validate_relations(relations); });
}

int osmt_assemble_multipolygons(osmt_ctx* ctx, const osmt_relations_desc* relations, osmt_polygons** out) {
    return guarded([&] { return assemble_body(ctx, relations, out); });
}

int osmt_polygons_counts(const osmt_polygons* p, size_t counts[4]) {
    return guarded([&] {
        if (!p || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
        counts[0] = p->n_polys, counts[1] = p->n_poly_nodes, counts[2] = p->n_mps, counts[3] = p->n_polys; /* every polygon belongs to one multipolygon */
        return (int)OSMT_OK;
    });
}

int osmt_polygons_read(osmt_ctx* ctx, const osmt_polygons* p, uint32_t* polygon_node_off, uint32_t* polygon_nodes, uint64_t* multipolygon_ids,
                       uint32_t* multipolygon_polygon_off, uint32_t* multipolygon_polygons, osmt_relation_status* status,
                       uint32_t* multipolygon_relation) {
    return guarded([&] {
        return read_body(ctx, p, polygon_node_off, polygon_nodes, multipolygon_ids, multipolygon_polygon_off, multipolygon_polygons, status, multipolygon_relation);
    });
}

void osmt_polygons_free(osmt_polygons* p) {
    if (!p) return;
    osmt_ctx* ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    dev_free(ctx, p->pool);
    delete p;
    ctx_release(ctx);
}

int osmt_debug_vertex_hash_bits(osmt_ctx* ctx, uint32_t bits) {
    return guarded([&] {
        if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
        if (bits > 32u) return fail(OSMT_INVALID_ARG, "hash bits %u (0..32)", bits);
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->vertex_hash_bits = bits;
        return (int)OSMT_OK;
    });
}
