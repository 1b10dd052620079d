/*
 * osmt_host_resolve.cpp — host side of libosmtile.so: OSM ids resolved to local indices (include/osmtile.h,
 * osmt_resolve.hip).  One call uploads the parser's arrays, sorts the two id tables with the pyramid's radix sort, translates
 * and compacts the references of ways and relations, dedups the ways' references on two paths (LDS for short ways, the sort
 * for long ones) and leaves the arrays osmt_relations_desc and osmt_geodata_desc take on the device.  Shares osmt_host.h with
 * the other host files.
 */
#include "osmt_host.h"

using namespace osmt_host;

/* a resolution's result: one dev_alloc buffer, given back by osmt_resolved_free */
struct osmt_resolved {
    osmt_ctx* ctx = nullptr;
    char* pool = nullptr;
    const uint32_t *way_node_off = nullptr, *way_nodes = nullptr, *relation_way_off = nullptr, *relation_ways = nullptr;
    const uint8_t* relation_way_inner = nullptr;
    size_t n_ways = 0, n_relations = 0;
    size_t counts[5] = {0, 0, 0, 0, 0};
};

namespace {

const uint32_t ZERO_OFF[1] = {0u}; /* the offsets of no ways / no relations, where the caller gave none */

int validate_resolve(const osmt_raw_osm_desc* d) {
    if (!d) return fail(OSMT_INVALID_ARG, "NULL argument");
    const struct {
        const void* p;
        size_t n;
        const char* name;
    } arrays[] = {{d->node_ids, d->n_nodes, "node_ids"},
                  {d->way_ids, d->n_ways, "way_ids"},
                  {d->way_ref_off, d->n_ways, "way_ref_off"},
                  {d->way_refs, d->n_way_refs, "way_refs"},
                  {d->relation_ref_off, d->n_relations, "relation_ref_off"},
                  {d->relation_refs, d->n_relation_refs, "relation_refs"},
                  {d->relation_ref_inner, d->n_relation_refs, "relation_ref_inner"}};
    for (const auto& a : arrays)
        if (!a.p && a.n) return fail(OSMT_INVALID_ARG, "resolve: %s is NULL with a count of %zu", a.name, a.n);
    if (d->n_nodes >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "resolve: %zu nodes do not fit 32-bit indices (at most %llu)", d->n_nodes, 0xFFFFFFFEull);
    if (d->n_ways >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "resolve: %zu ways do not fit 32-bit indices (at most %llu)", d->n_ways, 0xFFFFFFFEull);
    if (d->n_relations >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "resolve: %zu relations do not fit 32-bit offsets (at most %llu)", d->n_relations, 0xFFFFFFFEull);
    if (d->n_way_refs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "resolve: %zu node references (at most %llu)", d->n_way_refs, 0xFFFFFFFEull);
    if (d->n_relation_refs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "resolve: %zu way references (at most %llu)", d->n_relation_refs, 0xFFFFFFFEull);
    if (!d->way_ref_off && d->n_way_refs) return fail(OSMT_INVALID_ARG, "resolve: %zu node references and no ways", d->n_way_refs);
    if (!d->relation_ref_off && d->n_relation_refs) return fail(OSMT_INVALID_ARG, "resolve: %zu way references and no relations", d->n_relation_refs);
    int rc = check_offsets_of("resolve", "way_ref_off", d->way_ref_off ? d->way_ref_off : ZERO_OFF, d->n_ways, d->n_way_refs);
    if (rc == OSMT_OK) rc = check_offsets_of("resolve", "relation_ref_off", d->relation_ref_off ? d->relation_ref_off : ZERO_OFF, d->n_relations, d->n_relation_refs);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < d->n_relation_refs; ++i)
        if (d->relation_ref_inner[i] > 1u)
            return fail(OSMT_INVALID_ARG, "resolve: relation_ref_inner[%zu] = %u is not a role (0: outer, 1: inner)", i, (unsigned)d->relation_ref_inner[i]);
    if (d->way_nodes_seen)
        for (size_t i = 0; i < d->n_ways; ++i)
            if (d->way_nodes_seen[i] > d->n_nodes) return fail(OSMT_INVALID_ARG, "resolve: way_nodes_seen[%zu] = %u is above the %zu nodes", i, d->way_nodes_seen[i], d->n_nodes);
    if (d->relation_ways_seen)
        for (size_t i = 0; i < d->n_relations; ++i)
            if (d->relation_ways_seen[i] > d->n_ways)
                return fail(OSMT_INVALID_ARG, "resolve: relation_ways_seen[%zu] = %u is above the %zu ways", i, d->relation_ways_seen[i], d->n_ways);
    return OSMT_OK;
}

/* n pairs to sort by the key alone, and what the passes need */
struct sort_job {
    unsigned long long* key[2] = {nullptr, nullptr};
    uint32_t* id[2] = {nullptr, nullptr};
    uint32_t *counts = nullptr, *hist = nullptr;
    unsigned long long *blk = nullptr, *tot = nullptr;
    uint32_t n = 0;
    int at = 0; /* which of the two buffers holds the pairs */
};

struct sort_layout {
    size_t o_k0, o_k1, o_i0, o_i1, o_cnt, o_hist, o_blk, o_tot;
};

sort_layout add_sort(pool_layout& pl, size_t n) {
    const size_t n_wg = (n + OSMT_PYR_SORT_BLOCK - 1) / OSMT_PYR_SORT_BLOCK;
    sort_layout s;
    s.o_k0 = pl.add(n * 8), s.o_k1 = pl.add(n * 8), s.o_i0 = pl.add(n * 4), s.o_i1 = pl.add(n * 4), s.o_cnt = pl.add((256 * n_wg + 1) * 4);
    s.o_hist = pl.add(OSMT_PYR_KEY_DIGITS * 256 * 4), s.o_blk = pl.add((n_wg + 2) * 8), s.o_tot = pl.add(8);
    return s;
}

sort_job sort_at(char* w, const sort_layout& s, size_t n) {
    sort_job j;
    j.key[0] = (unsigned long long*)(w + s.o_k0), j.key[1] = (unsigned long long*)(w + s.o_k1), j.id[0] = (uint32_t*)(w + s.o_i0), j.id[1] = (uint32_t*)(w + s.o_i1);
    j.counts = (uint32_t*)(w + s.o_cnt), j.hist = (uint32_t*)(w + s.o_hist), j.blk = (unsigned long long*)(w + s.o_blk), j.tot = (unsigned long long*)(w + s.o_tot);
    j.n = (uint32_t)n;
    return j;
}

/* The pyramid's radix sort over the bytes of the key alone: the pairs went in with ascending ids and every pass is stable.
 * hist: the jobs' histograms as k_pyr_keydigits left them, read back by the caller. */
int sort_by_key(hipStream_t st, sort_job& j, const uint32_t* hist) {
    if (j.n < 2u) return OSMT_OK;
    for (uint32_t b = 0; b < OSMT_PYR_KEY_DIGITS; ++b) { /* a byte whose histogram has one non-empty bin is not sorted on */
        bool one_bin = false;
        for (uint32_t v = 0; v < 256; ++v) one_bin = one_bin || hist[b * 256 + v] == j.n;
        if (one_bin) continue;
        HIP_TRY(osmt_launch_pyr_pass(j.key[j.at], j.id[j.at], j.n, 4u + b, j.counts, j.blk, j.tot, j.key[j.at ^ 1], j.id[j.at ^ 1], st));
        j.at ^= 1;
    }
    return OSMT_OK;
}

enum { EV_START, EV_TABLES, EV_TRANSLATE, EV_SHORT, EV_LONG, EV_EMIT, EV_N };
enum { W_NODES, W_PAIRS, W_KEPT, W_MEMBERS, W_N }; /* the words read back: node references resolved, pairs to sort, node references kept, members resolved */

int resolve_body(osmt_ctx* ctx, const osmt_raw_osm_desc* d, osmt_resolved** out) {
    if (!ctx || !d || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = validate_resolve(d);
    if (rc != OSMT_OK) return rc;
    uint32_t short_max;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        short_max = ctx->resolve_short_way_max;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    call_work wg(ctx, "id resolution");
    rc = wg.begin(EV_N);
    if (rc != OSMT_OK) return rc;
    hipStream_t st = wg.st;
    const auto t_start = std::chrono::steady_clock::now();
    const size_t n_nodes = d->n_nodes, n_ways = d->n_ways, n_rels = d->n_relations, n_wrefs = d->n_way_refs, n_rrefs = d->n_relation_refs;
    /* work buffers 0, 1: the id tables */
    sort_job tab[2];
    const size_t tab_n[2] = {n_nodes, n_ways};
    const uint64_t* tab_ids[2] = {d->node_ids, d->way_ids};
    HIP_TRY(wg.mark(EV_START));
    for (int k = 0; k < 2; ++k) {
        pool_layout pl;
        const sort_layout sl = add_sort(pl, tab_n[k]);
        rc = wg.alloc(k, pl, k ? "way ids" : "node ids");
        if (rc != OSMT_OK) return rc;
        tab[k] = sort_at(wg.work[k], sl, tab_n[k]);
        if (tab_n[k]) HIP_TRY(hipMemcpyAsync(tab[k].key[0], tab_ids[k], tab_n[k] * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(osmt_launch_res_iota(tab[k].id[0], tab[k].n, st));
        HIP_TRY(osmt_launch_pyr_keydigits(tab[k].key[0], tab[k].n, tab[k].hist, st));
    }
    /* work buffer 2: the references and everything sized by them */
    osmt_res_refs R[2] = {};
    osmt_res_dedup D{};
    unsigned long long* d_words = nullptr;
    {
        const size_t n_scan = std::max(std::max(n_wrefs, n_rrefs), std::max(n_ways, n_rels));
        pool_layout pl;
        const size_t o_woff = pl.add((n_ways + 1) * 4), o_wrefs = pl.add(n_wrefs * 8), o_wseen = pl.add(d->way_nodes_seen ? n_ways * 4 : 0);
        const size_t o_roff = pl.add((n_rels + 1) * 4), o_rrefs = pl.add(n_rrefs * 8), o_rseen = pl.add(d->relation_ways_seen ? n_rels * 4 : 0), o_role = pl.add(n_rrefs);
        const size_t o_wloc = pl.add(n_wrefs * 4), o_wpos = pl.add((n_wrefs + 1) * 4), o_toff = pl.add((n_ways + 1) * 4), o_trefs = pl.add(n_wrefs * 4);
        const size_t o_rloc = pl.add(n_rrefs * 4), o_rpos = pl.add((n_rrefs + 1) * 4);
        const size_t o_keep = pl.add((n_wrefs + 1) * 4), o_lpos = pl.add((n_ways + 1) * 4), o_blk = pl.add((n_scan / 256 + 2) * 8), o_words = pl.add(W_N * 8);
        rc = wg.alloc(2, pl, "references");
        if (rc != OSMT_OK) return rc;
        char* w = wg.work[2];
        const struct {
            size_t o;
            const void* src;
            size_t bytes;
        } up[] = {{o_woff, d->way_ref_off ? d->way_ref_off : ZERO_OFF, (n_ways + 1) * 4},
                  {o_wrefs, d->way_refs, n_wrefs * 8},
                  {o_wseen, d->way_nodes_seen, d->way_nodes_seen ? n_ways * 4 : 0},
                  {o_roff, d->relation_ref_off ? d->relation_ref_off : ZERO_OFF, (n_rels + 1) * 4},
                  {o_rrefs, d->relation_refs, n_rrefs * 8},
                  {o_rseen, d->relation_ways_seen, d->relation_ways_seen ? n_rels * 4 : 0},
                  {o_role, d->relation_ref_inner, n_rrefs}};
        for (const auto& u : up)
            if (u.bytes) HIP_TRY(hipMemcpyAsync(w + u.o, u.src, u.bytes, hipMemcpyHostToDevice, st));
        d_words = (unsigned long long*)(w + o_words);
        R[0].off = (const uint32_t*)(w + o_woff), R[0].refs = (const unsigned long long*)(w + o_wrefs);
        R[0].seen = d->way_nodes_seen && n_ways ? (const uint32_t*)(w + o_wseen) : nullptr;
        R[0].n_owners = (uint32_t)n_ways, R[0].n_refs = (uint32_t)n_wrefs, R[0].local = (uint32_t*)(w + o_wloc), R[0].pos = (uint32_t*)(w + o_wpos);
        R[0].out_off = (uint32_t*)(w + o_toff), R[0].out_local = (uint32_t*)(w + o_trefs), R[0].tot = d_words + W_NODES;
        R[1].off = (const uint32_t*)(w + o_roff), R[1].refs = (const unsigned long long*)(w + o_rrefs);
        R[1].seen = d->relation_ways_seen && n_rels ? (const uint32_t*)(w + o_rseen) : nullptr;
        R[1].role = (const uint8_t*)(w + o_role), R[1].n_owners = (uint32_t)n_rels, R[1].n_refs = (uint32_t)n_rrefs;
        R[1].local = (uint32_t*)(w + o_rloc), R[1].pos = (uint32_t*)(w + o_rpos), R[1].tot = d_words + W_MEMBERS;
        R[0].blk = R[1].blk = D.blk = (unsigned long long*)(w + o_blk);
        D.off = R[0].out_off, D.refs = R[0].out_local, D.n_ways = (uint32_t)n_ways, D.short_max = short_max;
        D.keep = (uint32_t*)(w + o_keep), D.long_pos = (uint32_t*)(w + o_lpos), D.tot = d_words + W_PAIRS;
    }
    /* the tables' histograms, then their passes */
    std::vector<uint32_t> hist(2 * OSMT_PYR_KEY_DIGITS * 256);
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemcpyAsync(hist.data() + k * OSMT_PYR_KEY_DIGITS * 256, tab[k].hist, OSMT_PYR_KEY_DIGITS * 256 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) {
        rc = sort_by_key(st, tab[k], hist.data() + k * OSMT_PYR_KEY_DIGITS * 256);
        if (rc != OSMT_OK) return rc;
        R[k].table_key = tab[k].key[tab[k].at], R[k].table_id = tab[k].id[tab[k].at], R[k].n_table = tab[k].n;
    }
    HIP_TRY(wg.mark(EV_TABLES));
    /* the ways' references: translated and compacted into work buffer 2, where the dedup reads them */
    HIP_TRY(osmt_launch_res_translate(R[0], st));
    HIP_TRY(wg.mark(EV_TRANSLATE));
    HIP_TRY(osmt_launch_res_short(D, st));
    HIP_TRY(wg.mark(EV_SHORT));
    unsigned long long words[W_N] = {};
    HIP_TRY(hipMemcpyAsync(words, d_words, 2 * 8, hipMemcpyDeviceToHost, st)); /* W_NODES, W_PAIRS: the others are not written yet */
    HIP_TRY(hipStreamSynchronize(st));
    const size_t T = (size_t)words[W_NODES], L = (size_t)words[W_PAIRS];
    sort_job lj;
    if (L) {
        pool_layout pl;
        const sort_layout sl = add_sort(pl, L);
        rc = wg.alloc(3, pl, "pairs of long ways");
        if (rc != OSMT_OK) return rc;
        lj = sort_at(wg.work[3], sl, L);
        HIP_TRY(osmt_launch_res_longpairs(D, lj.n, lj.key[0], lj.id[0], st));
        HIP_TRY(osmt_launch_pyr_keydigits(lj.key[0], lj.n, lj.hist, st));
        HIP_TRY(hipMemcpyAsync(hist.data(), lj.hist, OSMT_PYR_KEY_DIGITS * 256 * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rc = sort_by_key(st, lj, hist.data());
        if (rc != OSMT_OK) return rc;
    }
    HIP_TRY(osmt_launch_res_mark(D, lj.n, lj.key[lj.at], lj.id[lj.at], (uint32_t)T, st));
    HIP_TRY(wg.mark(EV_LONG));
    std::unique_ptr<osmt_resolved> res(new osmt_resolved);
    /* The relations' members are compacted straight into the result.  Its relation arrays are sized by the members that came
     * in and its way nodes by T, the total before the dedup: neither final total is known yet, and sizing by them would cost a
     * read-back each for a result at most the dropped references smaller. */
    pool_layout pl;
    const size_t o_wo = pl.add((n_ways + 1) * 4), o_wn = pl.add(T * 4), o_ro = pl.add((n_rels + 1) * 4), o_rw = pl.add(n_rrefs * 4), o_ri = pl.add(n_rrefs);
    char* pool = nullptr;
    rc = wg.alloc(&pool, pl, "result");
    if (rc != OSMT_OK) return rc;
    R[1].out_off = (uint32_t*)(pool + o_ro), R[1].out_local = (uint32_t*)(pool + o_rw), R[1].out_role = (uint8_t*)(pool + o_ri);
    hipError_t e = osmt_launch_res_translate(R[1], st);
    if (e == hipSuccess) e = osmt_launch_res_emit(D, (uint32_t)T, (uint32_t*)(pool + o_wo), (uint32_t*)(pool + o_wn), st);
    if (e == hipSuccess) e = wg.mark(EV_EMIT);
    if (e == hipSuccess) e = hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        dev_free(ctx, pool);
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "id resolution: the emit stage failed: %s", hipGetErrorString(e));
    }
    const size_t kept = (size_t)words[W_KEPT], members = (size_t)words[W_MEMBERS];
    if (wg.trace)
        fprintf(stderr,
                "osmt id resolution: %.1f us in all; id tables %.1f us, translate %.1f us, short ways %.1f us, long ways + mark %.1f us, relations + emit %.1f us "
                "on the device (%zu nodes, %zu ways, %zu + %zu references, %zu pairs through the sort, short way bound %u)\n",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(), wg.us(EV_START, EV_TABLES), wg.us(EV_TABLES, EV_TRANSLATE),
                wg.us(EV_TRANSLATE, EV_SHORT), wg.us(EV_SHORT, EV_LONG), wg.us(EV_LONG, EV_EMIT), n_nodes, n_ways, n_wrefs, n_rrefs, L, short_max);
    res->ctx = ctx, res->pool = pool;
    res->way_node_off = (const uint32_t*)(pool + o_wo), res->way_nodes = (const uint32_t*)(pool + o_wn);
    res->relation_way_off = R[1].out_off, res->relation_ways = R[1].out_local, res->relation_way_inner = R[1].out_role;
    res->n_ways = n_ways, res->n_relations = n_rels;
    res->counts[0] = kept, res->counts[1] = members, res->counts[2] = n_wrefs - T, res->counts[3] = T - kept, res->counts[4] = n_rrefs - members;
    ctx->refs.fetch_add(1);
    *out = res.release();
    return OSMT_OK;
}

int read_body(osmt_ctx* ctx, const osmt_resolved* r, uint32_t* way_node_off, uint32_t* way_nodes, uint32_t* relation_way_off, uint32_t* relation_ways,
              uint8_t* relation_way_inner) {
    if (!ctx || !r) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (r->ctx != ctx) return fail(OSMT_INVALID_ARG, "resolve: the result belongs to another context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (way_node_off) HIP_TRY(copy_back(ctx, way_node_off, r->way_node_off, (r->n_ways + 1) * 4));
    if (way_nodes && r->counts[0]) HIP_TRY(copy_back(ctx, way_nodes, r->way_nodes, r->counts[0] * 4));
    if (relation_way_off) HIP_TRY(copy_back(ctx, relation_way_off, r->relation_way_off, (r->n_relations + 1) * 4));
    if (relation_ways && r->counts[1]) HIP_TRY(copy_back(ctx, relation_ways, r->relation_ways, r->counts[1] * 4));
    if (relation_way_inner && r->counts[1]) HIP_TRY(copy_back(ctx, relation_way_inner, r->relation_way_inner, r->counts[1]));
    return OSMT_OK;
}

}  // namespace

int osmt_validate_resolve(const osmt_raw_osm_desc* raw) {
    return guarded([&] { return validate_resolve(raw); });
}

int osmt_resolve_refs(osmt_ctx* ctx, const osmt_raw_osm_desc* raw, osmt_resolved** out) {
    return guarded([&] { return resolve_body(ctx, raw, out); });
}

int osmt_resolved_counts(const osmt_resolved* r, size_t counts[5]) {
    return guarded([&] {
        if (!r || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
        for (int i = 0; i < 5; ++i) counts[i] = r->counts[i];
        return (int)OSMT_OK;
    });
}

int osmt_resolved_read(osmt_ctx* ctx, const osmt_resolved* r, uint32_t* way_node_off, uint32_t* way_nodes, uint32_t* relation_way_off, uint32_t* relation_ways,
                       uint8_t* relation_way_inner) {
    return guarded([&] { return read_body(ctx, r, way_node_off, way_nodes, relation_way_off, relation_ways, relation_way_inner); });
}

void osmt_resolved_free(osmt_resolved* r) {
    if (!r) return;
    osmt_ctx* ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    dev_free(ctx, r->pool);
    delete r;
    ctx_release(ctx);
}

int osmt_debug_resolve_short_way_max(osmt_ctx* ctx, uint32_t n) {
    return guarded([&] {
        if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
        if (n > OSMT_RES_SHORT_WAY_CAP) return fail(OSMT_INVALID_ARG, "short way bound %u (0..%u)", n, OSMT_RES_SHORT_WAY_CAP);
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->resolve_short_way_max = n;
        return (int)OSMT_OK;
    });
}
