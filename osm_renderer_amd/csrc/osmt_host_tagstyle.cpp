/*
 * osmt_host_tagstyle.cpp — host side of libosmtile.so: from tags to styles.  Selector matching (osmt_selmatch.hip), label
 * bindings per class (osmt_labelbind.hip) and the cascade (osmt_cascade.hip); the three share osmt_match, which nothing else
 * in the library uses.  Shares osmt_host.h with the other host files.
 */
#include "osmt_host.h"

using namespace osmt_host;

/* ---- selector matching (include/osmtile.h, csrc/osmt_selmatch.hip) ------------------------------------------------ */
struct osmt_match {
    osmt_ctx* ctx = nullptr;
    uint32_t geodata_id = 0;
    uint32_t selectors_id = 0;
    bool complete = false; /* false: the declined state, only the declined values can be read */
    std::vector<osmt_declined_number> declined;
    size_t n_nodes = 0, n_ways = 0, n_mps = 0, n_classes = 0, n_class_sels = 0;
    char* d_keep = nullptr; /* one allocation: the three arrays below */
    const uint32_t* d_ent_class = nullptr;
    const osmt_match_class* d_classes = nullptr;
    const uint32_t* d_class_sels = nullptr;
};

namespace {

struct sm_tag_kind {
    const char *off_name, *what;
    const uint32_t *off, *tags;
    size_t n, n_tags;
};

int validate_tags(const osmt_tags_desc* t, uint32_t geodata_id, osmt_ctx* ctx) {
    if (!t) return fail(OSMT_INVALID_ARG, "tags are NULL");
    const sm_tag_kind kinds[3] = {{"node_tag_off", "node", t->node_tag_off, t->node_tags, t->n_nodes, t->n_node_tags},
                                  {"way_tag_off", "way", t->way_tag_off, t->way_tags, t->n_ways, t->n_way_tags},
                                  {"multipolygon_tag_off", "multipolygon", t->multipolygon_tag_off, t->multipolygon_tags, t->n_multipolygons,
                                   t->n_multipolygon_tags}};
    for (const sm_tag_kind& k : kinds)
        if (!k.off || (k.n_tags && !k.tags)) return fail(OSMT_INVALID_ARG, "tags: NULL %s array (every offset array has at least its first entry)", k.what);
    if (t->n_string_bytes && !t->strings) return fail(OSMT_INVALID_ARG, "tags: NULL strings with %zu bytes", t->n_string_bytes);
    if (t->n_nodes + t->n_ways + t->n_multipolygons > ((size_t)1 << 30))
        return fail(OSMT_UNSUPPORTED, "tags: %zu entities (> 2^30)", t->n_nodes + t->n_ways + t->n_multipolygons);
    if (t->n_node_tags + t->n_way_tags + t->n_multipolygon_tags >= 0xFFFFFFFFull || t->n_string_bytes >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "tags: too large for 32-bit indices");
    for (const sm_tag_kind& k : kinds) {
        const int rc = check_offsets_of("tags", k.off_name, k.off, k.n, k.n_tags);
        if (rc != OSMT_OK) return rc;
    }
    for (const sm_tag_kind& k : kinds)
        for (size_t i = 0; i < k.n; ++i)
            for (uint32_t j = k.off[i]; j < k.off[i + 1]; ++j) {
                const uint32_t* q = k.tags + 4 * (size_t)j;
                if ((size_t)q[0] + q[1] > t->n_string_bytes || (size_t)q[2] + q[3] > t->n_string_bytes)
                    return fail(OSMT_INVALID_ARG, "tags: tag %u of %s %zu = (%u, %u, %u, %u) leaves the %zu string bytes", j - k.off[i], k.what, i, q[0], q[1],
                                q[2], q[3], t->n_string_bytes);
                if (j > k.off[i] && osmt_bytes_cmp(t->strings + q[-4], q[-3], t->strings + q[0], q[1]) >= 0)
                    return fail(OSMT_INVALID_ARG, "tags: the keys of %s %zu are not strictly ascending as unsigned bytes (tag %u against the one before)",
                                k.what, i, j - k.off[i]);
            }
    if (!ctx) return OSMT_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "tags: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    const osmt_ctx::geodata_host& g = ctx->geodata[geodata_id];
    if (g.n_nodes != t->n_nodes || g.n_ways != t->n_ways || g.n_mps != t->n_multipolygons)
        return fail(OSMT_INVALID_ARG, "tags: %zu nodes, %zu ways, %zu multipolygons, but geodata id %u has %zu, %zu, %zu", t->n_nodes, t->n_ways,
                    t->n_multipolygons, geodata_id, g.n_nodes, g.n_ways, g.n_mps);
    return OSMT_OK;
}

int register_tags_body(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tags_desc* t) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id < ctx->geodata.size() && ctx->geodata[geodata_id].d_tags)
            return fail(OSMT_INVALID_ARG, "geodata id %u has tags already (one table per file)", geodata_id);
    }
    const int rc = validate_tags(t, geodata_id, ctx);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_ent = t->n_nodes + t->n_ways + t->n_multipolygons, n_tags = t->n_node_tags + t->n_way_tags + t->n_multipolygon_tags;
    std::vector<uint32_t> tag_off(n_ent + 1);
    {
        size_t e = 0;
        for (size_t i = 0; i < t->n_nodes; ++i) tag_off[e++] = t->node_tag_off[i];
        for (size_t i = 0; i < t->n_ways; ++i) tag_off[e++] = (uint32_t)(t->n_node_tags + t->way_tag_off[i]);
        for (size_t i = 0; i < t->n_multipolygons; ++i) tag_off[e++] = (uint32_t)(t->n_node_tags + t->n_way_tags + t->multipolygon_tag_off[i]);
        tag_off[e] = (uint32_t)n_tags;
    }
    pool_layout pl;
    const size_t o_off = pl.add((n_ent + 1) * 4), o_tags = pl.add(n_tags * 16), o_str = pl.add(t->n_string_bytes);
    table_upload up("tags", pl);
    char* pool = up.pool;
    up.put(o_off, tag_off.data(), (n_ent + 1) * 4);
    up.put(o_tags, t->node_tags, t->n_node_tags * 16);
    up.put(o_tags + t->n_node_tags * 16, t->way_tags, t->n_way_tags * 16);
    up.put(o_tags + (t->n_node_tags + t->n_way_tags) * 16, t->multipolygon_tags, t->n_multipolygon_tags * 16);
    up.put(o_str, t->strings, t->n_string_bytes);
    if (up.done() != OSMT_OK) return up.done();
    osmt_sm_tags_dev d{};
    d.tag_off = (const uint32_t*)(pool + o_off);
    d.tags = (const uint4*)(pool + o_tags);
    d.strings = (const uint8_t*)(pool + o_str);
    d.n_nodes = (uint32_t)t->n_nodes, d.n_ways = (uint32_t)t->n_ways, d.n_mps = (uint32_t)t->n_multipolygons, d.n_tags = (uint32_t)n_tags;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->geodata[geodata_id].d_tags) return fail(OSMT_INVALID_ARG, "geodata id %u has tags already (one table per file)", geodata_id); /* another thread was first */
    ctx->geodata[geodata_id].d_tags = pool;
    ctx->geodata[geodata_id].tags = d;
    ctx->geodata[geodata_id].tags_string_bytes = t->n_string_bytes;
    ctx->geodata[geodata_id].n_node_tags = t->n_node_tags, ctx->geodata[geodata_id].n_way_tags = t->n_way_tags;
    up.release();
    return OSMT_OK;
}

int validate_selectors(const osmt_selectors_desc* d) {
    if (!d) return fail(OSMT_INVALID_ARG, "selectors are NULL");
    if ((d->n_selectors && !d->selectors) || (d->n_tests && !d->tests) || (d->n_string_bytes && !d->strings))
        return fail(OSMT_INVALID_ARG, "selectors: NULL array with non-zero count");
    if (d->n_selectors > OSMT_MATCH_MAX_SELECTORS)
        return fail(OSMT_UNSUPPORTED, "selectors: %zu selectors (> OSMT_MATCH_MAX_SELECTORS = %u)", d->n_selectors, OSMT_MATCH_MAX_SELECTORS);
    if (d->n_tests >= 0xFFFFFFFFull || d->n_string_bytes >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "selectors: too large for 32-bit indices");
    for (size_t i = 0; i < d->n_selectors; ++i) {
        const osmt_selector_rec& s = d->selectors[i];
        if (s.object_type > OSMT_SEL_OTHER) return fail(OSMT_INVALID_ARG, "selector %zu: object type %u is not an OSMT_SEL_* value", i, s.object_type);
        if (s.has_min_zoom > 1 || s.has_max_zoom > 1) return fail(OSMT_INVALID_ARG, "selector %zu: a zoom flag that is not 0 or 1", i);
        if (s.n_tests > OSMT_MATCH_MAX_SELECTOR_TESTS)
            return fail(OSMT_UNSUPPORTED, "selector %zu has %u tests (> OSMT_MATCH_MAX_SELECTOR_TESTS = %u)", i, s.n_tests, OSMT_MATCH_MAX_SELECTOR_TESTS);
        if ((size_t)s.test_off + s.n_tests > d->n_tests)
            return fail(OSMT_INVALID_ARG, "selector %zu: tests %u..%u leave the %zu tests", i, s.test_off, s.test_off + s.n_tests, d->n_tests);
    }
    for (size_t i = 0; i < d->n_tests; ++i) {
        const osmt_selector_test& t = d->tests[i];
        if (t.kind >= OSMT_TEST_KINDS) return fail(OSMT_INVALID_ARG, "test %zu: kind %u is not an OSMT_TEST_* value", i, t.kind);
        if ((size_t)t.key_off + t.key_len > d->n_string_bytes || (size_t)t.value_off + t.value_len > d->n_string_bytes)
            return fail(OSMT_INVALID_ARG, "test %zu: a string range leaves the %zu string bytes", i, d->n_string_bytes);
    }
    return OSMT_OK;
}

int register_selectors_body(osmt_ctx* ctx, const osmt_selectors_desc* d, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = validate_selectors(d);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    /* the distinct test keys in &str order (std::string compares as unsigned bytes) and per key its distinct string values */
    struct key_info {
        std::vector<std::string> vals;
        bool numeric = false;
        uint32_t id = 0;
    };
    std::map<std::string, key_info> keys;
    auto str = [&](uint32_t off, uint32_t len) { return std::string((const char*)d->strings + off, len); };
    for (size_t i = 0; i < d->n_tests; ++i) {
        const osmt_selector_test& t = d->tests[i];
        key_info& k = keys[str(t.key_off, t.key_len)];
        if (t.kind == OSMT_TEST_EQUAL || t.kind == OSMT_TEST_NOT_EQUAL) k.vals.push_back(str(t.value_off, t.value_len));
        if (t.kind >= OSMT_TEST_LESS) k.numeric = true;
    }
    std::vector<osmt_sm_key> h_keys;
    std::vector<uint2> h_vals;
    std::string blob;
    for (auto& kv : keys) {
        key_info& k = kv.second;
        std::sort(k.vals.begin(), k.vals.end());
        k.vals.erase(std::unique(k.vals.begin(), k.vals.end()), k.vals.end());
        k.id = (uint32_t)h_keys.size();
        osmt_sm_key r{};
        r.off = (uint32_t)blob.size(), r.len = (uint32_t)kv.first.size();
        blob += kv.first;
        r.val_first = (uint32_t)h_vals.size(), r.n_vals = (uint32_t)k.vals.size();
        r.numeric = k.numeric ? 1u : 0u;
        for (const std::string& v : k.vals) {
            h_vals.push_back(make_uint2((uint32_t)blob.size(), (uint32_t)v.size()));
            blob += v;
        }
        h_keys.push_back(r);
    }
    if (blob.size() >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "selectors: too large for 32-bit indices");
    std::vector<osmt_sm_test> h_tests(d->n_tests);
    for (size_t i = 0; i < d->n_tests; ++i) {
        const osmt_selector_test& t = d->tests[i];
        const key_info& k = keys[str(t.key_off, t.key_len)];
        osmt_sm_test r{};
        r.kind = t.kind, r.key = k.id, r.vid = OSMT_SM_NONE, r.value = t.value;
        if (t.kind == OSMT_TEST_EQUAL || t.kind == OSMT_TEST_NOT_EQUAL)
            r.vid = (uint32_t)(std::lower_bound(k.vals.begin(), k.vals.end(), str(t.value_off, t.value_len)) - k.vals.begin());
        h_tests[i] = r;
    }
    std::vector<osmt_sm_sel> h_sels(d->n_selectors);
    for (size_t i = 0; i < d->n_selectors; ++i) {
        osmt_sm_sel r{};
        r.type = d->selectors[i].object_type, r.test_off = d->selectors[i].test_off, r.n_tests = d->selectors[i].n_tests;
        h_sels[i] = r;
    }
    pool_layout pl;
    const size_t o_k = pl.add(h_keys.size() * sizeof(osmt_sm_key)), o_v = pl.add(h_vals.size() * sizeof(uint2)), o_s = pl.add(blob.size());
    const size_t o_sel = pl.add(h_sels.size() * sizeof(osmt_sm_sel)), o_t = pl.add(h_tests.size() * sizeof(osmt_sm_test));
    table_upload up("selectors", pl);
    char* pool = up.pool;
    up.put(o_k, h_keys.data(), h_keys.size() * sizeof(osmt_sm_key));
    up.put(o_v, h_vals.data(), h_vals.size() * sizeof(uint2));
    up.put(o_s, blob.data(), blob.size());
    up.put(o_sel, h_sels.data(), h_sels.size() * sizeof(osmt_sm_sel));
    up.put(o_t, h_tests.data(), h_tests.size() * sizeof(osmt_sm_test));
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::selectors_host h;
    h.d_pool = pool;
    h.dev.keys = (const osmt_sm_key*)(pool + o_k);
    h.dev.vals = (const uint2*)(pool + o_v);
    h.dev.strings = (const uint8_t*)(pool + o_s);
    h.dev.sels = (const osmt_sm_sel*)(pool + o_sel);
    h.dev.tests = (const osmt_sm_test*)(pool + o_t);
    h.dev.n_keys = (uint32_t)h_keys.size(), h.dev.n_sels = (uint32_t)h_sels.size();
    {
        auto zooms = std::make_shared<std::vector<uint8_t>>(2 * d->n_selectors);
        for (size_t i = 0; i < d->n_selectors; ++i) {
            (*zooms)[2 * i] = d->selectors[i].has_min_zoom ? d->selectors[i].min_zoom : 0;
            (*zooms)[2 * i + 1] = d->selectors[i].has_max_zoom ? d->selectors[i].max_zoom : 255;
        }
        h.zooms = zooms;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out_id = (uint32_t)ctx->selectors.size();
    ctx->selectors.push_back(h);
    up.release();
    return OSMT_OK;
}

int match_selectors_body(osmt_ctx* ctx, uint32_t geodata_id, uint32_t selectors_id, const osmt_number_override* ov, size_t n_ov, osmt_match** out) {
    if (!ctx || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out = nullptr;
    osmt_ctx::geodata_host geo;
    osmt_ctx::selectors_host sel;
    uint32_t hash_bits = 32;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
        if (!ctx->geodata[geodata_id].d_tags) return fail(OSMT_INVALID_ARG, "geodata id %u has no tags (osmt_register_tags)", geodata_id);
        if (selectors_id >= ctx->selectors.size())
            return fail(OSMT_INVALID_ARG, "selectors id %u is not registered (%zu sets)", selectors_id, ctx->selectors.size());
        geo = ctx->geodata[geodata_id];
        sel = ctx->selectors[selectors_id];
        hash_bits = ctx->match_hash_bits;
    }
    if (n_ov && !ov) return fail(OSMT_INVALID_ARG, "number overrides: NULL array with non-zero count");
    if (n_ov >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "number overrides: too many");
    for (size_t i = 0; i < n_ov; ++i) {
        const osmt_number_override& o = ov[i];
        if ((size_t)o.v_off + o.v_len > geo.tags_string_bytes)
            return fail(OSMT_INVALID_ARG, "number overrides: entry %zu = (%u, %u) leaves the %zu string bytes of the tags", i, o.v_off, o.v_len,
                        geo.tags_string_bytes);
        if (o.has_value > 1u) return fail(OSMT_INVALID_ARG, "number overrides: entry %zu has has_value = %u (0 or 1)", i, o.has_value);
        if (i && !(ov[i - 1].v_off < o.v_off || (ov[i - 1].v_off == o.v_off && ov[i - 1].v_len < o.v_len)))
            return fail(OSMT_INVALID_ARG, "number overrides: entry %zu = (%u, %u) does not come after entry %zu (strictly ascending by (v_off, v_len))", i,
                        o.v_off, o.v_len, i - 1);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    /* the trace: the device time of the stages */
    enum { EV_TAGS0, EV_TAGS1, EV_COUNT0, EV_COUNT1, EV_CLASS0, EV_CLASS1, EV_EMIT0, EV_EMIT1, EV_N };
    call_work wg(ctx, "selector match");
    const int brc = wg.begin(EV_N);
    if (brc != OSMT_OK) return brc;
    hipStream_t st = wg.st;
    const bool trace = wg.trace;
    pool_layout pl;

    const size_t n_ent = (size_t)geo.tags.n_nodes + geo.tags.n_ways + geo.tags.n_mps, n_tags = geo.tags.n_tags;
    unsigned long long tot[OSMT_SM_T_N] = {};
    osmt_sm_pass P;
    memset(&P, 0, sizeof P);
    P.geo = geo.dev;
    P.tg = geo.tags;
    P.ss = sel.dev;
    P.n_ov = (uint32_t)n_ov;
    P.n_ent = (uint32_t)n_ent;
    P.hash_mask = hash_bits >= 32u ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
    /* 1. tags */
    pl = pool_layout();
    const size_t o_ov = pl.add(n_ov * sizeof(osmt_number_override)), o_code = pl.add(n_tags * 4), o_vf = pl.add(n_tags * 8), o_num = pl.add(n_tags * 8);
    const size_t o_dp = pl.add((n_tags + 1) * 4), o_blk = pl.add((std::max(n_tags, n_ent) / 256 + 1) * 8), o_tot = pl.add(OSMT_SM_T_N * 8);
    int rc = wg.alloc(0, pl, "tags");
    if (rc != OSMT_OK) return rc;
    char* w0 = wg.work[0];
    if (n_ov) HIP_TRY(hipMemcpyAsync(w0 + o_ov, ov, n_ov * sizeof(osmt_number_override), hipMemcpyHostToDevice, st));
    P.ov = (const osmt_number_override*)(w0 + o_ov);
    P.tag_code = (uint32_t*)(w0 + o_code);
    P.tag_vf = (uint2*)(w0 + o_vf);
    P.tag_num = (double*)(w0 + o_num);
    P.decl_pos = (uint32_t*)(w0 + o_dp);
    P.blk = (unsigned long long*)(w0 + o_blk);
    P.tot = (unsigned long long*)(w0 + o_tot);
    HIP_TRY(wg.mark(EV_TAGS0));
    HIP_TRY(osmt_launch_sm_tags(P, st));
    HIP_TRY(wg.mark(EV_TAGS1));
    HIP_TRY(hipMemcpyAsync(tot, P.tot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[OSMT_SM_T_DECLINED]) {
        const size_t n_decl = (size_t)tot[OSMT_SM_T_DECLINED];
        pl = pool_layout();
        (void)pl.add(n_decl * sizeof(osmt_declined_number));
        rc = wg.alloc(1, pl, "declined values");
        if (rc != OSMT_OK) return rc;
        P.n_declined = (uint32_t)n_decl;
        P.declined = (osmt_declined_number*)wg.work[1];
        HIP_TRY(osmt_launch_sm_declined(P, st));
        std::unique_ptr<osmt_match> m(new osmt_match);
        m->declined.resize(n_decl);
        HIP_TRY(hipMemcpyAsync(m->declined.data(), P.declined, n_decl * sizeof(osmt_declined_number), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        auto lt = [](const osmt_declined_number& a, const osmt_declined_number& b) { return a.v_off < b.v_off || (a.v_off == b.v_off && a.v_len < b.v_len); };
        std::sort(m->declined.begin(), m->declined.end(), lt);
        m->declined.erase(std::unique(m->declined.begin(), m->declined.end(),
                                      [](const osmt_declined_number& a, const osmt_declined_number& b) { return a.v_off == b.v_off && a.v_len == b.v_len; }),
                          m->declined.end());
        const osmt_declined_number first = m->declined[0];
        char text[49] = {};
        const size_t shown = std::min<size_t>(first.v_len, sizeof text - 1);
        if (shown) HIP_TRY(copy_back(ctx, text, geo.tags.strings + first.v_off, shown));
        m->ctx = ctx;
        m->geodata_id = geodata_id;
        ctx->refs.fetch_add(1);
        const size_t n_distinct = m->declined.size();
        *out = m.release();
        return fail(OSMT_UNSUPPORTED,
                    "the exact number parse declines %zu distinct tag values, the first is \"%s\"%s (v_off %u, v_len %u): read them with "
                    "osmt_match_read_declined_numbers and pass their values as overrides",
                    n_distinct, text, shown < first.v_len ? "..." : "", first.v_off, first.v_len);
    }
    /* 2. count */
    size_t table = 2;
    while (table < 2 * n_ent) table <<= 1;
    P.table_mask = (uint32_t)(table - 1);
    pl = pool_layout();
    const size_t o_sp = pl.add((n_ent + 1) * 4), o_lay = pl.add(n_ent * 8), o_key = pl.add(n_ent * 4), o_hash = pl.add(n_ent * 4), o_ts = pl.add(n_ent * 4);
    const size_t o_fp = pl.add((n_ent + 1) * 4), o_tab = pl.add(table * 4), o_low = pl.add(table * 4);
    rc = wg.alloc(1, pl, "entities");
    if (rc != OSMT_OK) return rc;
    char* w1 = wg.work[1];
    P.sel_pos = (uint32_t*)(w1 + o_sp);
    P.ent_layer = (long long*)(w1 + o_lay);
    P.ent_key = (uint32_t*)(w1 + o_key);
    P.ent_hash = (uint32_t*)(w1 + o_hash);
    P.ent_tslot = (uint32_t*)(w1 + o_ts);
    P.first_pos = (uint32_t*)(w1 + o_fp);
    P.table = (uint32_t*)(w1 + o_tab);
    P.lowest = (uint32_t*)(w1 + o_low);
    HIP_TRY(wg.mark(EV_COUNT0));
    HIP_TRY(osmt_launch_sm_count(P, st));
    HIP_TRY(wg.mark(EV_COUNT1));
    HIP_TRY(hipMemcpyAsync(tot + OSMT_SM_T_MATCHED, P.tot + OSMT_SM_T_MATCHED, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[OSMT_SM_T_MATCHED] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "the match has %llu (entity, selector) pairs (> 2^32 - 2): split the selector set", tot[OSMT_SM_T_MATCHED]);
    P.n_matched = (uint32_t)tot[OSMT_SM_T_MATCHED];
    /* 3. lists and classes */
    pl = pool_layout();
    (void)pl.add((size_t)P.n_matched * 4);
    rc = wg.alloc(2, pl, "selector lists");
    if (rc != OSMT_OK) return rc;
    P.ent_sels = (uint32_t*)wg.work[2];
    HIP_TRY(wg.mark(EV_CLASS0));
    HIP_TRY(osmt_launch_sm_classes(P, st));
    HIP_TRY(wg.mark(EV_CLASS1));
    HIP_TRY(hipMemcpyAsync(tot + OSMT_SM_T_CLASSES, P.tot + OSMT_SM_T_CLASSES, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    P.n_classes = (uint32_t)tot[OSMT_SM_T_CLASSES]; /* at most n_ent */
    pl = pool_layout();
    const size_t o_cp = pl.add(((size_t)P.n_classes + 1) * 4), o_cf = pl.add((size_t)P.n_classes * 4);
    rc = wg.alloc(3, pl, "classes");
    if (rc != OSMT_OK) return rc;
    P.cls_pos = (uint32_t*)(wg.work[3] + o_cp);
    P.cls_first = (uint32_t*)(wg.work[3] + o_cf);
    HIP_TRY(wg.mark(EV_EMIT0));
    HIP_TRY(osmt_launch_sm_class_count(P, st));
    HIP_TRY(hipMemcpyAsync(tot + OSMT_SM_T_CLASS_SELS, P.tot + OSMT_SM_T_CLASS_SELS, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    P.n_class_sels = (uint32_t)tot[OSMT_SM_T_CLASS_SELS]; /* at most n_matched */
    /* 4. the result: one allocation that goes to the match */
    pl = pool_layout();
    const size_t o_ec = pl.add(n_ent * 4), o_cl = pl.add((size_t)P.n_classes * sizeof(osmt_match_class)), o_cs = pl.add((size_t)P.n_class_sels * 4);
    rc = wg.alloc(4, pl, "result");
    if (rc != OSMT_OK) return rc;
    char* keep = wg.work[4];
    P.ent_class = (uint32_t*)(keep + o_ec);
    P.classes = (osmt_match_class*)(keep + o_cl);
    P.class_sels = (uint32_t*)(keep + o_cs);
    HIP_TRY(osmt_launch_sm_emit(P, st));
    HIP_TRY(wg.mark(EV_EMIT1));
    HIP_TRY(hipStreamSynchronize(st));
    std::unique_ptr<osmt_match> m(new osmt_match);
    m->ctx = ctx;
    m->geodata_id = geodata_id;
    m->selectors_id = selectors_id;
    m->complete = true;
    m->n_nodes = geo.tags.n_nodes, m->n_ways = geo.tags.n_ways, m->n_mps = geo.tags.n_mps;
    m->n_classes = P.n_classes, m->n_class_sels = P.n_class_sels;
    m->d_keep = keep;
    m->d_ent_class = P.ent_class, m->d_classes = P.classes, m->d_class_sels = P.class_sels;
    wg.work[4] = nullptr;
    ctx->refs.fetch_add(1);
    *out = m.release();
    if (trace) {
        fprintf(stderr,
                "osmt selector match: tags %.1f us, count %.1f us, lists + classes %.1f us, records %.1f us (%zu entities, %zu tags, %u selectors, "
                "%u pairs, %u classes)\n",
                wg.us(EV_TAGS0, EV_TAGS1), wg.us(EV_COUNT0, EV_COUNT1), wg.us(EV_CLASS0, EV_CLASS1), wg.us(EV_EMIT0, EV_EMIT1), n_ent, n_tags, sel.dev.n_sels,
                P.n_matched, P.n_classes);
    }
    return OSMT_OK;
}

int match_read_body(osmt_match* m, uint32_t* ent_class, osmt_match_class* classes, uint32_t* class_sels, const size_t caps[3], size_t counts[3]) {
    if (!m || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (!m->complete) return fail(OSMT_INVALID_ARG, "the match is in the declined state: it answers only osmt_match_read_declined_numbers");
    const size_t n_ent = m->n_nodes + m->n_ways + m->n_mps;
    counts[0] = n_ent, counts[1] = m->n_classes, counts[2] = m->n_class_sels;
    if (!ent_class && !classes && !class_sels) return OSMT_OK;
    if (!caps) return fail(OSMT_INVALID_ARG, "NULL caps with an output");
    if ((ent_class && caps[0] < counts[0]) || (classes && caps[1] < counts[1]) || (class_sels && caps[2] < counts[2]))
        return fail(OSMT_INVALID_ARG, "caps (%zu, %zu, %zu) are less than the match's (%zu, %zu, %zu)", caps[0], caps[1], caps[2], counts[0], counts[1],
                    counts[2]);
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (ent_class) HIP_TRY(copy_back(m->ctx, ent_class, m->d_ent_class, n_ent * 4));
    if (classes) HIP_TRY(copy_back(m->ctx, classes, m->d_classes, m->n_classes * sizeof(osmt_match_class)));
    if (class_sels) HIP_TRY(copy_back(m->ctx, class_sels, m->d_class_sels, m->n_class_sels * 4));
    return OSMT_OK;
}

int bindings_matched_body(osmt_ctx* ctx, osmt_match* m, uint8_t zoom_lo, uint8_t zoom_hi, const uint32_t* class_off, const uint32_t* class_styles, size_t n,
                          uint32_t* out_id) {
    if (!ctx || !m || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (m->ctx != ctx) return fail(OSMT_INVALID_ARG, "bindings per class: the match belongs to another context");
    if (!m->complete) return fail(OSMT_INVALID_ARG, "bindings per class: the match is in the declined state");
    if (zoom_lo > zoom_hi || zoom_hi > OSMT_MAX_ZOOM)
        return fail(OSMT_INVALID_ARG, "bindings per class: zoom range %u..%u (zoom_lo <= zoom_hi <= %u)", zoom_lo, zoom_hi, OSMT_MAX_ZOOM);
    if (n != m->n_classes) return fail(OSMT_INVALID_ARG, "bindings per class: %zu classes, the match has %zu", n, m->n_classes);
    if (!class_off) return fail(OSMT_INVALID_ARG, "bindings per class: NULL class_style_off (it has at least its first entry)");
    int rc = check_offsets_of("bindings per class", "class_style_off", class_off, n, class_off[n]);
    if (rc != OSMT_OK) return rc;
    const size_t n_styles_in = class_off[n];
    if (n_styles_in && !class_styles) return fail(OSMT_INVALID_ARG, "bindings per class: NULL class_styles with %zu entries", n_styles_in);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (size_t i = 0; i < n_styles_in; ++i)
            if (class_styles[i] >= ctx->styles.size())
                return fail(OSMT_INVALID_ARG, "bindings per class: class_styles[%zu] = %u is not a registered style (%zu styles)", i, class_styles[i],
                            ctx->styles.size());
    }
    HIP_TRY(hipSetDevice(ctx->device));
    call_work wg(ctx, "bindings per class"); /* wg.pool: the table, until it is registered */
    const int brc = wg.begin(0);
    if (brc != OSMT_OK) return brc;
    hipStream_t st = wg.st;
    const size_t n_ways = m->n_ways, n_mps = m->n_mps;
    pool_layout pl;
    const size_t o_co = pl.add((n + 1) * 4), o_cs = pl.add(n_styles_in * 4), o_pw = pl.add((n_ways + 1) * 4), o_pm = pl.add((n_mps + 1) * 4);
    const size_t o_blk = pl.add((std::max(n_ways, n_mps) / 256 + 1) * 8), o_tot = pl.add(16);
    const int arc = wg.alloc(0, pl);
    if (arc != OSMT_OK) return arc;
    char* w = wg.work[0];
    HIP_TRY(hipMemcpyAsync(w + o_co, class_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_styles_in) HIP_TRY(hipMemcpyAsync(w + o_cs, class_styles, n_styles_in * 4, hipMemcpyHostToDevice, st));
    const uint32_t* d_co = (const uint32_t*)(w + o_co);
    const uint32_t* d_cs = (const uint32_t*)(w + o_cs);
    uint32_t *pw = (uint32_t*)(w + o_pw), *pm = (uint32_t*)(w + o_pm);
    unsigned long long* d_tot = (unsigned long long*)(w + o_tot);
    const uint32_t* way_class = m->d_ent_class + m->n_nodes;
    const uint32_t* mp_class = way_class + n_ways;
    HIP_TRY(osmt_launch_sm_bind_count(way_class, d_co, (uint32_t)n_ways, pw, (unsigned long long*)(w + o_blk), d_tot, st));
    HIP_TRY(osmt_launch_sm_bind_count(mp_class, d_co, (uint32_t)n_mps, pm, (unsigned long long*)(w + o_blk), d_tot + 1, st));
    unsigned long long tot[2] = {};
    HIP_TRY(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[0] >= 0xFFFFFFFFull || tot[1] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "bindings per class: %llu way and %llu multipolygon bindings (> 2^32 - 2 of one kind)", tot[0], tot[1]);
    /* the table, laid out as osmt_register_style_bindings lays it out */
    pl = pool_layout();
    const size_t o_wo = pl.add((n_ways + 1) * 4), o_w = pl.add((size_t)tot[0] * 4), o_mo = pl.add((n_mps + 1) * 4), o_m = pl.add((size_t)tot[1] * 4);
    const int prc = wg.alloc_pool(pl);
    if (prc != OSMT_OK) return prc;
    char* pool = wg.pool;
    HIP_TRY(hipMemcpyAsync(pool + o_wo, pw, (n_ways + 1) * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(pool + o_mo, pm, (n_mps + 1) * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(osmt_launch_sm_bind_emit(way_class, d_co, d_cs, (uint32_t)n_ways, pw, (uint32_t*)(pool + o_w), st));
    HIP_TRY(osmt_launch_sm_bind_emit(mp_class, d_co, d_cs, (uint32_t)n_mps, pm, (uint32_t*)(pool + o_m), st));
    HIP_TRY(hipStreamSynchronize(st));
    osmt_ctx::bindings_host h;
    h.geodata_id = m->geodata_id, h.zoom_lo = zoom_lo, h.zoom_hi = zoom_hi;
    h.d_pool = pool;
    h.dev.way_off = (const uint32_t*)(pool + o_wo);
    h.dev.way_styles = (const uint32_t*)(pool + o_w);
    h.dev.mp_off = (const uint32_t*)(pool + o_mo);
    h.dev.mp_styles = (const uint32_t*)(pool + o_m);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "bindings table too large");
    *out_id = (uint32_t)ctx->bindings.size();
    ctx->bindings.push_back(h);
    wg.pool = nullptr;
    return OSMT_OK;
}

}  // namespace

int osmt_validate_tags(const osmt_tags_desc* tags, uint32_t geodata_id, osmt_ctx* ctx) {
    return guarded([&] { return validate_tags(tags, geodata_id, ctx); });
}
int osmt_register_tags(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tags_desc* tags) {
    return guarded([&] { return register_tags_body(ctx, geodata_id, tags); });
}
int osmt_validate_selectors(const osmt_selectors_desc* selectors) {
    return guarded([&] { return validate_selectors(selectors); });
}
int osmt_register_selectors(osmt_ctx* ctx, const osmt_selectors_desc* selectors, uint32_t* out_selectors_id) {
    return guarded([&] { return register_selectors_body(ctx, selectors, out_selectors_id); });
}
int osmt_match_selectors(osmt_ctx* ctx, uint32_t geodata_id, uint32_t selectors_id, const osmt_number_override* ov, size_t n_ov, osmt_match** out) {
    return guarded([&] { return match_selectors_body(ctx, geodata_id, selectors_id, ov, n_ov, out); });
}
void osmt_match_free(osmt_match* m) {
    if (!m) return;
    osmt_ctx* ctx = m->ctx;
    (void)hipSetDevice(ctx->device);
    dev_free(ctx, m->d_keep);
    delete m;
    ctx_release(ctx);
}
int osmt_match_read_declined_numbers(osmt_match* m, osmt_declined_number* out, size_t cap, size_t* n) {
    return guarded([&] {
        if (!m || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
        *n = m->declined.size();
        if (out && cap < *n) return fail(OSMT_INVALID_ARG, "cap %zu is less than the %zu declined values", cap, *n);
        if (out && *n) memcpy(out, m->declined.data(), *n * sizeof(osmt_declined_number));
        return (int)OSMT_OK;
    });
}
int osmt_match_read(osmt_match* m, uint32_t* entity_class, osmt_match_class* classes, uint32_t* class_selectors, const size_t caps[3], size_t counts[3]) {
    return guarded([&] { return match_read_body(m, entity_class, classes, class_selectors, caps, counts); });
}
int osmt_register_style_bindings_matched(osmt_ctx* ctx, osmt_match* match, uint8_t zoom_lo, uint8_t zoom_hi, const uint32_t* class_style_off,
                                         const uint32_t* class_styles, size_t n, uint32_t* out_bindings_id) {
    return guarded([&] { return bindings_matched_body(ctx, match, zoom_lo, zoom_hi, class_style_off, class_styles, n, out_bindings_id); });
}
int osmt_debug_match_hash_bits(osmt_ctx* ctx, uint32_t bits) {
    return guarded([&] {
        if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
        if (bits > 32u) return fail(OSMT_INVALID_ARG, "hash bits %u (0..32)", bits);
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->match_hash_bits = bits;
        return (int)OSMT_OK;
    });
}

/* ---- label bindings per class (include/osmtile.h, csrc/osmt_labelbind.hip) ----------------------------------------- */
namespace {

int validate_class_label_bindings(const osmt_class_label_bindings_desc* d, osmt_match* m, osmt_ctx* ctx) {
    const char* who = "label bindings per class";
    if (!d) return fail(OSMT_INVALID_ARG, "%s: the descriptor is NULL", who);
    if (m) {
        if (ctx && m->ctx != ctx) return fail(OSMT_INVALID_ARG, "%s: the match belongs to another context", who);
        if (!m->complete) return fail(OSMT_INVALID_ARG, "%s: the match is in the declined state", who);
    }
    if (d->zoom_lo > d->zoom_hi || d->zoom_hi > OSMT_MAX_ZOOM)
        return fail(OSMT_INVALID_ARG, "%s: zoom range %u..%u (zoom_lo <= zoom_hi <= %u)", who, d->zoom_lo, d->zoom_hi, OSMT_MAX_ZOOM);
    if (m && d->n_classes != m->n_classes) return fail(OSMT_INVALID_ARG, "%s: %zu classes, the match has %zu", who, d->n_classes, m->n_classes);
    if (d->n_keys > OSMT_LABEL_TEXT_KEYS_MAX)
        return fail(OSMT_UNSUPPORTED, "%s: %zu keys (> OSMT_LABEL_TEXT_KEYS_MAX = %u)", who, d->n_keys, OSMT_LABEL_TEXT_KEYS_MAX);
    if (d->n_classes >= 0xFFFFFFFFull || d->n_bindings >= 0xFFFFFFFFull || d->n_key_bytes >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "%s: %zu classes, %zu bindings, %zu key bytes: too large for 32-bit indices", who, d->n_classes, d->n_bindings,
                    d->n_key_bytes);
    if (!d->class_off || !d->key_off || (d->n_bindings && !d->bindings) || (d->n_key_bytes && !d->key_bytes))
        return fail(OSMT_INVALID_ARG, "%s: NULL array (every offset array has at least its first entry)", who);
    int rc = check_offsets_of(who, "class_off", d->class_off, d->n_classes, d->n_bindings);
    if (rc == OSMT_OK) rc = check_offsets_of(who, "key_off", d->key_off, d->n_keys, d->n_key_bytes);
    if (rc != OSMT_OK) return rc;
    size_t n_styles = SIZE_MAX;
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        n_styles = ctx->label_styles.size();
    }
    for (size_t i = 0; i < d->n_bindings; ++i) {
        const osmt_class_label_binding& b = d->bindings[i];
        if (b.style >= n_styles)
            return fail(OSMT_INVALID_ARG, "%s: bindings[%zu].style = %u is not a registered label style (%zu styles)", who, i, b.style, n_styles);
        if (b.text_key != OSMT_TEXT_NONE && b.text_key >= d->n_keys)
            return fail(OSMT_INVALID_ARG, "%s: bindings[%zu].text_key = %u is neither one of the %zu keys nor OSMT_TEXT_NONE", who, i, b.text_key, d->n_keys);
    }
    return OSMT_OK;
}

int label_bindings_matched_body(osmt_ctx* ctx, osmt_match* m, const osmt_class_label_bindings_desc* d, uint32_t* out_id, bool area) {
    const char* who = area ? "area label bindings per class" : "label bindings per class";
    if (!ctx || !m || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    int rc = validate_class_label_bindings(d, m, ctx);
    if (rc != OSMT_OK) return rc;
    osmt_ctx::geodata_host geo;
    uint32_t hash_bits = 32;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geo = ctx->geodata[m->geodata_id]; /* a match exists only for a registered file with tags */
        hash_bits = ctx->match_hash_bits;
    }
    if (area && !geo.d_index) return fail(OSMT_INVALID_ARG, "%s: geodata id %u has no tile index (osmt_register_tile_index)", who, m->geodata_id);
    if (area && !geo.d_factors)
        return fail(OSMT_INVALID_ARG, "%s: geodata id %u has no Mercator factors (osmt_register_node_mercator)", who, m->geodata_id);
    HIP_TRY(hipSetDevice(ctx->device));
    /* the device copy of the keys starts every key on a 4-byte boundary (k_lb_emit compares whole dwords); declared in front of
     * the guard, whose destructor waits for the stream that may still read them */
    std::vector<uint2> h_keys(d->n_keys);
    std::vector<uint8_t> h_key_bytes;
    /* the trace: the device time of the stages */
    enum { EV_COUNT0, EV_COUNT1, EV_EMIT0, EV_EMIT1, EV_TEXTS1, EV_MEASURE0, EV_MEASURE1, EV_DECODE0, EV_DECODE1, EV_PATCH1, EV_N };
    call_work wg(ctx, who);
    const int brc = wg.begin(EV_N);
    if (brc != OSMT_OK) return brc;
    hipStream_t st = wg.st;
    const bool trace = wg.trace;
    pool_layout pl;

    /* the kinds of the table and its tags: the node table numbers the node tags, the area table the way tags, then the
     * multipolygon tags */
    const size_t first0 = area ? m->n_nodes : 0, n0 = area ? m->n_ways : m->n_nodes, first1 = m->n_nodes + m->n_ways, n1 = area ? m->n_mps : 0;
    const size_t tag_base = area ? geo.n_node_tags : 0, n_tt = area ? (size_t)geo.tags.n_tags - geo.n_node_tags : geo.n_node_tags;
    const size_t n_cls = d->n_classes, n_keys = d->n_keys;
    for (size_t k = 0; k < n_keys; ++k) {
        const uint32_t a = d->key_off[k], len = d->key_off[k + 1] - a;
        h_keys[k] = make_uint2((uint32_t)h_key_bytes.size(), len);
        h_key_bytes.insert(h_key_bytes.end(), d->key_bytes + a, d->key_bytes + a + len);
        h_key_bytes.resize(align_up(h_key_bytes.size(), 4), 0);
    }
    size_t table = 2;
    while (table < 2 * n_tt) table <<= 1;
    const size_t o_co = pl.add((n_cls + 1) * 4), o_cb = pl.add(d->n_bindings * 8), o_k = pl.add(n_keys * 8), o_kb = pl.add(h_key_bytes.size());
    const size_t o_p0 = pl.add((n0 + 1) * 4), o_p1 = pl.add((n1 + 1) * 4), o_blk = pl.add((std::max(std::max(n0, n1), n_tt) / 256 + 1) * 8);
    const size_t o_tot = pl.add(OSMT_LB_T_N * 8), o_used = pl.add(n_tt * 4), o_ts = pl.add(n_tt * 4), o_fp = pl.add((n_tt + 1) * 4);
    const size_t o_tab = pl.add(table * 4), o_low = pl.add(table * 4);
    rc = wg.alloc(0, pl, "classes and tags");
    if (rc != OSMT_OK) return rc;
    char* w = wg.work[0];
    HIP_TRY(hipMemcpyAsync(w + o_co, d->class_off, (n_cls + 1) * 4, hipMemcpyHostToDevice, st));
    if (d->n_bindings) HIP_TRY(hipMemcpyAsync(w + o_cb, d->bindings, d->n_bindings * 8, hipMemcpyHostToDevice, st));
    if (n_keys) HIP_TRY(hipMemcpyAsync(w + o_k, h_keys.data(), n_keys * 8, hipMemcpyHostToDevice, st));
    if (!h_key_bytes.empty()) HIP_TRY(hipMemcpyAsync(w + o_kb, h_key_bytes.data(), h_key_bytes.size(), hipMemcpyHostToDevice, st));
    osmt_lb_pass P;
    memset(&P, 0, sizeof P);
    P.tg = geo.tags;
    P.ent_class = m->d_ent_class;
    P.class_off = (const uint32_t*)(w + o_co);
    P.class_bind = (const uint2*)(w + o_cb);
    P.keys = (const uint2*)(w + o_k);
    P.key_bytes = (const uint8_t*)(w + o_kb);
    P.tag_base = (uint32_t)tag_base, P.n_tt = (uint32_t)n_tt;
    P.hash_mask = hash_bits >= 32u ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
    P.table_mask = (uint32_t)(table - 1);
    P.used = (uint32_t*)(w + o_used);
    P.tslot = (uint32_t*)(w + o_ts);
    P.first_pos = (uint32_t*)(w + o_fp);
    P.table = (uint32_t*)(w + o_tab);
    P.lowest = (uint32_t*)(w + o_low);
    P.blk = (unsigned long long*)(w + o_blk);
    P.tot = (unsigned long long*)(w + o_tot);
    uint32_t *pos0 = (uint32_t*)(w + o_p0), *pos1 = (uint32_t*)(w + o_p1);
    unsigned long long tot[OSMT_LB_T_N] = {};
    /* 1. count */
    HIP_TRY(wg.mark(EV_COUNT0));
    HIP_TRY(osmt_launch_lb_begin(P, st));
    HIP_TRY(osmt_launch_lb_count(P, (uint32_t)first0, (uint32_t)n0, pos0, P.tot + OSMT_LB_T_BIND0, st));
    HIP_TRY(osmt_launch_lb_count(P, (uint32_t)first1, (uint32_t)n1, pos1, P.tot + OSMT_LB_T_BIND1, st));
    HIP_TRY(wg.mark(EV_COUNT1));
    HIP_TRY(hipMemcpyAsync(tot, P.tot, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[OSMT_LB_T_BIND0] >= 0xFFFFFFFFull || tot[OSMT_LB_T_BIND1] >= 0xFFFFFFFFull) {
        if (area)
            return fail(OSMT_UNSUPPORTED, "%s: %llu way and %llu multipolygon bindings (> 2^32 - 2 of one kind)", who, tot[OSMT_LB_T_BIND0],
                        tot[OSMT_LB_T_BIND1]);
        return fail(OSMT_UNSUPPORTED, "%s: %llu node bindings (> 2^32 - 2)", who, tot[OSMT_LB_T_BIND0]);
    }
    const size_t nb0 = (size_t)tot[OSMT_LB_T_BIND0], nb1 = (size_t)tot[OSMT_LB_T_BIND1];
    /* 2. emit with provisional texts, 3. texts */
    pl = pool_layout();
    const size_t o_b0 = pl.add(nb0 * 8), o_b1 = pl.add(nb1 * 8);
    rc = wg.alloc(1, pl, "bindings");
    if (rc != OSMT_OK) return rc;
    osmt_label_binding *bind0 = (osmt_label_binding*)(wg.work[1] + o_b0), *bind1 = (osmt_label_binding*)(wg.work[1] + o_b1);
    HIP_TRY(wg.mark(EV_EMIT0));
    HIP_TRY(osmt_launch_lb_emit(P, (uint32_t)first0, (uint32_t)n0, pos0, bind0, st));
    HIP_TRY(osmt_launch_lb_emit(P, (uint32_t)first1, (uint32_t)n1, pos1, bind1, st));
    HIP_TRY(wg.mark(EV_EMIT1));
    HIP_TRY(osmt_launch_lb_texts(P, st));
    HIP_TRY(wg.mark(EV_TEXTS1));
    HIP_TRY(hipMemcpyAsync(tot + OSMT_LB_T_TEXTS, P.tot + OSMT_LB_T_TEXTS, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[OSMT_LB_T_TEXTS] >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "%s: %llu texts (>= 2^32 - 1)", who, tot[OSMT_LB_T_TEXTS]);
    const size_t n_texts = (size_t)tot[OSMT_LB_T_TEXTS]; /* at most n_tt */
    P.n_texts = (uint32_t)n_texts;
    /* 4. measure */
    pl = pool_layout();
    const size_t o_tt = pl.add(n_texts * 4), o_to = pl.add((n_texts + 1) * 4);
    rc = wg.alloc(2, pl, "texts");
    if (rc != OSMT_OK) return rc;
    P.text_tag = (uint32_t*)(wg.work[2] + o_tt);
    P.text_off = (uint32_t*)(wg.work[2] + o_to);
    HIP_TRY(wg.mark(EV_MEASURE0));
    HIP_TRY(osmt_launch_lb_measure(P, st));
    HIP_TRY(wg.mark(EV_MEASURE1));
    HIP_TRY(hipMemcpyAsync(tot + OSMT_LB_T_CHARS, P.tot + OSMT_LB_T_CHARS, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[OSMT_LB_T_FIRST_BAD] != ~0ull) {
        /* name the tag: its kind and entity from the tag offsets, its value range, the byte the decoder stops at */
        const size_t t = tag_base + (size_t)tot[OSMT_LB_T_FIRST_BAD], n_ent = m->n_nodes + m->n_ways + m->n_mps;
        std::vector<uint32_t> tag_off(n_ent + 1);
        uint32_t q[4] = {};
        HIP_TRY(copy_back(ctx, tag_off.data(), geo.tags.tag_off, (n_ent + 1) * 4));
        HIP_TRY(copy_back(ctx, q, geo.tags.tags + t, 16));
        std::vector<uint8_t> value(q[3]);
        if (q[3]) HIP_TRY(copy_back(ctx, value.data(), geo.tags.strings + q[2], q[3]));
        const size_t e = (size_t)(std::upper_bound(tag_off.begin(), tag_off.end(), (uint32_t)t) - tag_off.begin()) - 1;
        const char* kind = e < m->n_nodes ? "node" : e < m->n_nodes + m->n_ways ? "way" : "multipolygon";
        const size_t local = e < m->n_nodes ? e : e < m->n_nodes + m->n_ways ? e - m->n_nodes : e - m->n_nodes - m->n_ways;
        uint32_t n_scalars = 0;
        const uint32_t bad = osmt_utf8_validate(value.data(), q[3], &n_scalars);
        return fail(OSMT_INVALID_ARG, "%s: the value of tag %zu of %s %zu (v_off %u, v_len %u) is not well-formed UTF-8 at byte %u; nothing is registered", who,
                    t - tag_off[e], kind, local, q[2], q[3], bad);
    }
    if (tot[OSMT_LB_T_CHARS] >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "%s: %llu chars (>= 2^32 - 1)", who, tot[OSMT_LB_T_CHARS]);
    const size_t n_chars = (size_t)tot[OSMT_LB_T_CHARS];
    P.n_chars = (uint32_t)n_chars;
    /* 5. the table, laid out as osmt_register_label_bindings / osmt_register_area_label_bindings lay it out; decode and patch in place */
    pl = pool_layout();
    size_t o_0o, o_1o = 0, o_0b, o_1b = 0, o_txo, o_c;
    if (area) {
        o_0o = pl.add((n0 + 1) * 4), o_1o = pl.add((n1 + 1) * 4), o_0b = pl.add(nb0 * 8), o_1b = pl.add(nb1 * 8), o_txo = pl.add((n_texts + 1) * 4), o_c = pl.add(n_chars * 4);
    } else {
        o_0o = pl.add((n0 + 1) * 4), o_0b = pl.add(nb0 * 8), o_txo = pl.add((n_texts + 1) * 4), o_c = pl.add(n_chars * 4);
    }
    const int prc = wg.alloc_pool(pl);
    if (prc != OSMT_OK) return prc;
    char* pool = wg.pool;
    HIP_TRY(hipMemcpyAsync(pool + o_0o, pos0, (n0 + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (nb0) HIP_TRY(hipMemcpyAsync(pool + o_0b, bind0, nb0 * 8, hipMemcpyDeviceToDevice, st));
    if (area) {
        HIP_TRY(hipMemcpyAsync(pool + o_1o, pos1, (n1 + 1) * 4, hipMemcpyDeviceToDevice, st));
        if (nb1) HIP_TRY(hipMemcpyAsync(pool + o_1b, bind1, nb1 * 8, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(pool + o_txo, P.text_off, (n_texts + 1) * 4, hipMemcpyDeviceToDevice, st));
    P.chars = (uint32_t*)(pool + o_c);
    HIP_TRY(wg.mark(EV_DECODE0));
    HIP_TRY(osmt_launch_lb_decode(P, st));
    HIP_TRY(wg.mark(EV_DECODE1));
    HIP_TRY(osmt_launch_lb_patch(P, (osmt_label_binding*)(pool + o_0b), (uint32_t)nb0, st));
    if (area) HIP_TRY(osmt_launch_lb_patch(P, (osmt_label_binding*)(pool + o_1b), (uint32_t)nb1, st));
    HIP_TRY(wg.mark(EV_PATCH1));
    HIP_TRY(hipStreamSynchronize(st));
    if (trace) {
        fprintf(stderr,
                "osmt %s: count %.1f us, emit %.1f us, texts %.1f us, measure %.1f us, decode %.1f us, patch %.1f us (%zu entities, %zu tags, %zu "
                "bindings, %zu texts, %zu chars)\n",
                who, wg.us(EV_COUNT0, EV_COUNT1), wg.us(EV_EMIT0, EV_EMIT1), wg.us(EV_EMIT1, EV_TEXTS1), wg.us(EV_MEASURE0, EV_MEASURE1), wg.us(EV_DECODE0, EV_DECODE1),
                wg.us(EV_DECODE1, EV_PATCH1), n0 + n1, n_tt, nb0 + nb1, n_texts, n_chars);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (area) {
        osmt_ctx::area_label_bindings_host h;
        h.geodata_id = m->geodata_id, h.zoom_lo = d->zoom_lo, h.zoom_hi = d->zoom_hi;
        h.d_pool = pool;
        h.dev.way_off = (const uint32_t*)(pool + o_0o);
        h.dev.mp_off = (const uint32_t*)(pool + o_1o);
        h.dev.way_bind = (const osmt_label_binding*)(pool + o_0b);
        h.dev.mp_bind = (const osmt_label_binding*)(pool + o_1b);
        h.dev.text_off = (const uint32_t*)(pool + o_txo);
        h.dev.chars = (const uint32_t*)(pool + o_c);
        h.n_ways = n0, h.n_mps = n1, h.n_way_bindings = nb0, h.n_mp_bindings = nb1, h.n_texts = n_texts, h.n_chars = n_chars;
        if (ctx->area_label_bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "area label bindings table too large");
        *out_id = (uint32_t)ctx->area_label_bindings.size();
        ctx->area_label_bindings.push_back(h);
    } else {
        osmt_ctx::label_bindings_host h;
        h.geodata_id = m->geodata_id, h.zoom_lo = d->zoom_lo, h.zoom_hi = d->zoom_hi;
        h.d_pool = pool;
        h.dev.node_off = (const uint32_t*)(pool + o_0o);
        h.dev.bindings = (const osmt_label_binding*)(pool + o_0b);
        h.dev.text_off = (const uint32_t*)(pool + o_txo);
        h.dev.chars = (const uint32_t*)(pool + o_c);
        h.n_nodes = n0, h.n_bindings = nb0, h.n_texts = n_texts, h.n_chars = n_chars;
        if (ctx->label_bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "label bindings table too large");
        *out_id = (uint32_t)ctx->label_bindings.size();
        ctx->label_bindings.push_back(h);
    }
    wg.pool = nullptr;
    return OSMT_OK;
}

/* one array of a read call: refused when its cap is too small, copied when asked for */
struct lb_read_part {
    void* dst;
    const void* src;
    size_t count, elem, cap;
};

int read_bindings_parts(osmt_ctx* ctx, const char* who, const lb_read_part* parts, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (parts[i].dst && parts[i].cap < parts[i].count)
            return fail(OSMT_INVALID_ARG, "%s: a cap of %zu is less than the table's %zu", who, parts[i].cap, parts[i].count);
    HIP_TRY(hipSetDevice(ctx->device));
    for (size_t i = 0; i < n; ++i)
        if (parts[i].dst && parts[i].count) HIP_TRY(copy_back(ctx, parts[i].dst, parts[i].src, parts[i].count * parts[i].elem));
    return OSMT_OK;
}

int read_label_bindings_body(osmt_ctx* ctx, uint32_t id, uint32_t* node_off, osmt_label_binding* bindings, uint32_t* text_off, uint32_t* chars,
                             const size_t caps[3], size_t counts[3]) {
    if (!ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx::label_bindings_host h;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (id >= ctx->label_bindings.size())
            return fail(OSMT_INVALID_ARG, "label bindings id %u is not registered (%zu tables)", id, ctx->label_bindings.size());
        h = ctx->label_bindings[id];
    }
    counts[0] = h.n_bindings, counts[1] = h.n_texts, counts[2] = h.n_chars;
    if (!node_off && !bindings && !text_off && !chars) return OSMT_OK;
    if (!caps) return fail(OSMT_INVALID_ARG, "NULL caps with an output");
    /* the offset arrays have one entry more than their count; they follow the caps of what they index */
    const lb_read_part parts[4] = {{node_off, h.dev.node_off, h.n_nodes + 1, 4, SIZE_MAX},
                                   {bindings, h.dev.bindings, h.n_bindings, sizeof(osmt_label_binding), caps[0]},
                                   {text_off, h.dev.text_off, h.n_texts + 1, 4, text_off && caps[1] < h.n_texts ? 0 : SIZE_MAX},
                                   {chars, h.dev.chars, h.n_chars, 4, caps[2]}};
    return read_bindings_parts(ctx, "osmt_read_label_bindings", parts, 4);
}

int read_area_label_bindings_body(osmt_ctx* ctx, uint32_t id, uint32_t* way_off, osmt_label_binding* way_bindings, uint32_t* mp_off,
                                  osmt_label_binding* mp_bindings, uint32_t* text_off, uint32_t* chars, const size_t caps[4], size_t counts[4]) {
    if (!ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx::area_label_bindings_host h;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (id >= ctx->area_label_bindings.size())
            return fail(OSMT_INVALID_ARG, "area label bindings id %u is not registered (%zu tables)", id, ctx->area_label_bindings.size());
        h = ctx->area_label_bindings[id];
    }
    counts[0] = h.n_way_bindings, counts[1] = h.n_mp_bindings, counts[2] = h.n_texts, counts[3] = h.n_chars;
    if (!way_off && !way_bindings && !mp_off && !mp_bindings && !text_off && !chars) return OSMT_OK;
    if (!caps) return fail(OSMT_INVALID_ARG, "NULL caps with an output");
    const lb_read_part parts[6] = {{way_off, h.dev.way_off, h.n_ways + 1, 4, SIZE_MAX},
                                   {way_bindings, h.dev.way_bind, h.n_way_bindings, sizeof(osmt_label_binding), caps[0]},
                                   {mp_off, h.dev.mp_off, h.n_mps + 1, 4, SIZE_MAX},
                                   {mp_bindings, h.dev.mp_bind, h.n_mp_bindings, sizeof(osmt_label_binding), caps[1]},
                                   {text_off, h.dev.text_off, h.n_texts + 1, 4, text_off && caps[2] < h.n_texts ? 0 : SIZE_MAX},
                                   {chars, h.dev.chars, h.n_chars, 4, caps[3]}};
    return read_bindings_parts(ctx, "osmt_read_area_label_bindings", parts, 6);
}

}  // namespace

int osmt_validate_class_label_bindings(const osmt_class_label_bindings_desc* d, osmt_match* match, osmt_ctx* ctx) {
    return guarded([&] { return validate_class_label_bindings(d, match, ctx); });
}
int osmt_register_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, const osmt_class_label_bindings_desc* d, uint32_t* out_bindings_id) {
    return guarded([&] { return label_bindings_matched_body(ctx, match, d, out_bindings_id, false); });
}
int osmt_register_area_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, const osmt_class_label_bindings_desc* d, uint32_t* out_bindings_id) {
    return guarded([&] { return label_bindings_matched_body(ctx, match, d, out_bindings_id, true); });
}
int osmt_read_label_bindings(osmt_ctx* ctx, uint32_t id, uint32_t* node_off, osmt_label_binding* bindings, uint32_t* text_off, uint32_t* chars,
                             const size_t caps[3], size_t counts[3]) {
    return guarded([&] { return read_label_bindings_body(ctx, id, node_off, bindings, text_off, chars, caps, counts); });
}
int osmt_read_area_label_bindings(osmt_ctx* ctx, uint32_t id, uint32_t* way_off, osmt_label_binding* way_bindings, uint32_t* multipolygon_off,
                                  osmt_label_binding* multipolygon_bindings, uint32_t* text_off, uint32_t* chars, const size_t caps[4],
                                  size_t counts[4]) {
    return guarded([&] {
        return read_area_label_bindings_body(ctx, id, way_off, way_bindings, multipolygon_off, multipolygon_bindings, text_off, chars, caps, counts);
    });
}

/* ---- the cascade (include/osmtile.h, csrc/osmt_cascade.hip, csrc/osmt_cascade_rule.h) ------------------------------ */
struct osmt_cascade {
    osmt_ctx* ctx = nullptr;
    uint32_t geodata_id = 0, selectors_id = 0;
    size_t n_classes = 0;
    std::vector<osmt_style_rec> styles;
    std::vector<double> dashes;
    std::vector<osmt_label_style_rec> label_styles;
    std::shared_ptr<const std::vector<uint32_t>> key_off;
    std::shared_ptr<const std::vector<uint8_t>> key_bytes;
    std::vector<uint8_t> zoom_lo, zoom_hi;
    std::vector<uint32_t> class_style_off, class_styles, range_style_base; /* [ranges][classes + 1], pooled, [ranges + 1] */
    std::vector<uint32_t> class_off, range_binding_base;
    std::vector<osmt_class_label_binding> bindings;
};

namespace {

int validate_rules(const osmt_rules_desc* d, uint32_t flags, osmt_ctx* ctx, osmt_cs_tables* out_tables) {
    if (flags & ~OSMT_RULES_CLASS_LAYERS) return fail(OSMT_INVALID_ARG, "rules: flags = 0x%x (0 or OSMT_RULES_CLASS_LAYERS)", flags);
    if (!d) return fail(OSMT_INVALID_ARG, "rules are NULL");
    if ((d->n_selectors && (!d->selector_rule || !d->selector_layer)) || (d->n_layer_bytes && !d->layer_bytes) || (d->n_props && !d->props) ||
        (d->n_numbers && !d->numbers) || (d->n_string_bytes && !d->strings))
        return fail(OSMT_INVALID_ARG, "rules: NULL array with non-zero count");
    if (!d->layer_off || !d->rule_prop_off) return fail(OSMT_INVALID_ARG, "rules: NULL offset array (every offset array has at least its first entry)");
    if (d->n_props >= 0xFFFFFFFFull || d->n_numbers >= 0xFFFFFFFFull || d->n_string_bytes >= 0xFFFFFFFFull || d->n_layer_bytes >= 0xFFFFFFFFull ||
        d->n_rules >= 0xFFFFFFFFull / OSMT_PROP_NAMES || d->n_layers >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "rules: too large for 32-bit indices");
    int rc = check_offsets_of("rules", "layer_off", d->layer_off, d->n_layers, d->n_layer_bytes);
    if (rc == OSMT_OK) rc = check_offsets_of("rules", "rule_prop_off", d->rule_prop_off, d->n_rules, d->n_props);
    if (rc != OSMT_OK) return rc;
    if (std::isnan(d->casing_width_multiplier)) return fail(OSMT_INVALID_ARG, "rules: casing_width_multiplier is NaN");
    if (d->has_font_size_multiplier > 1u) return fail(OSMT_INVALID_ARG, "rules: has_font_size_multiplier = %u (0 or 1)", d->has_font_size_multiplier);
    if (d->has_font_size_multiplier && std::isnan(d->font_size_multiplier)) return fail(OSMT_INVALID_ARG, "rules: font_size_multiplier is NaN");
    for (size_t i = 0; i < d->n_selectors; ++i) {
        if (d->selector_rule[i] >= d->n_rules)
            return fail(OSMT_INVALID_ARG, "rules: selector_rule[%zu] = %u is not below the %zu rules", i, d->selector_rule[i], d->n_rules);
        if (i && d->selector_rule[i] < d->selector_rule[i - 1])
            return fail(OSMT_INVALID_ARG, "rules: selector_rule[%zu] = %u decreases (selectors are in stylesheet order)", i, d->selector_rule[i]);
        if (d->selector_layer[i] != OSMT_LAYER_DEFAULT && d->selector_layer[i] >= d->n_layers)
            return fail(OSMT_INVALID_ARG, "rules: selector_layer[%zu] = %u is neither below the %zu layer names nor OSMT_LAYER_DEFAULT", i,
                        d->selector_layer[i], d->n_layers);
    }
    size_t n_images = 0, n_fonts = 0;
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        n_images = ctx->images.size(), n_fonts = ctx->fonts.size();
        if (d->selectors_id >= ctx->selectors.size())
            return fail(OSMT_INVALID_ARG, "rules: selectors id %u is not registered (%zu sets)", d->selectors_id, ctx->selectors.size());
        if (d->n_selectors != ctx->selectors[d->selectors_id].dev.n_sels)
            return fail(OSMT_INVALID_ARG, "rules: %zu selectors, the selector set %u has %u", d->n_selectors, d->selectors_id,
                        ctx->selectors[d->selectors_id].dev.n_sels);
    }
    bool writes_font_size = false;
    for (size_t i = 0; i < d->n_props; ++i) {
        const osmt_rule_prop& p = d->props[i];
        if (p.name > OSMT_PROP_OTHER) return fail(OSMT_INVALID_ARG, "rules: property %zu: name %u is not an OSMT_PROP_* value", i, p.name);
        if (p.kind >= OSMT_PV_KINDS) return fail(OSMT_INVALID_ARG, "rules: property %zu: kind %u is not an OSMT_PV_* value", i, p.kind);
        if (p.has_color > 1 || p.has_image > 1) return fail(OSMT_INVALID_ARG, "rules: property %zu: a flag that is not 0 or 1", i);
        const bool stringy = p.kind == OSMT_PV_IDENTIFIER || p.kind == OSMT_PV_STRING;
        if (p.kind == OSMT_PV_COLOR && !p.has_color) return fail(OSMT_INVALID_ARG, "rules: property %zu: a COLOR value has has_color = 1", i);
        if (p.has_color && p.kind != OSMT_PV_COLOR && p.kind != OSMT_PV_IDENTIFIER)
            return fail(OSMT_INVALID_ARG, "rules: property %zu: has_color on a value that is neither COLOR nor IDENTIFIER", i);
        if (p.has_image && !(stringy && (p.name == OSMT_PROP_ICON_IMAGE || p.name == OSMT_PROP_FILL_IMAGE)))
            return fail(OSMT_INVALID_ARG, "rules: property %zu: has_image on a property that is not an IDENTIFIER or STRING of icon-image / fill-image", i);
        if (stringy && (size_t)p.str_off + p.str_len > d->n_string_bytes)
            return fail(OSMT_INVALID_ARG, "rules: property %zu: string %u..%zu leaves the %zu string bytes", i, p.str_off, (size_t)p.str_off + p.str_len,
                        d->n_string_bytes);
        if (p.kind == OSMT_PV_NUMBERS && (size_t)p.num_off + p.n_nums > d->n_numbers)
            return fail(OSMT_INVALID_ARG, "rules: property %zu: numbers %u..%zu leave the %zu numbers", i, p.num_off, (size_t)p.num_off + p.n_nums, d->n_numbers);
        if (ctx && stringy && (p.name == OSMT_PROP_ICON_IMAGE || p.name == OSMT_PROP_FILL_IMAGE) && p.has_image && p.image >= n_images)
            return fail(OSMT_INVALID_ARG, "rules: property %zu: image %u is not registered (%zu images)", i, p.image, n_images);
        if (p.name == OSMT_PROP_FONT_SIZE) writes_font_size = true;
    }
    if (ctx && writes_font_size && d->font_id >= n_fonts) return fail(OSMT_INVALID_ARG, "rules: font_id %u is not registered (%zu fonts)", d->font_id, n_fonts);
    osmt_cs_tables local;
    osmt_cs_tables& T = out_tables ? *out_tables : local;
    size_t n_names = 0;
    osmt_cs_resolve(*d, T, &n_names);
    if ((flags & OSMT_RULES_CLASS_LAYERS) && n_names > OSMT_CASCADE_MAX_LAYER_NAMES)
        return fail(OSMT_UNSUPPORTED, "rules: %zu distinct layer names (> OSMT_CASCADE_MAX_LAYER_NAMES = %u)", n_names, OSMT_CASCADE_MAX_LAYER_NAMES);
    if (!(flags & OSMT_RULES_CLASS_LAYERS) && n_names > OSMT_CASCADE_MAX_LAYERS)
        return fail(OSMT_UNSUPPORTED, "rules: %zu distinct layer names (> OSMT_CASCADE_MAX_LAYERS = %u)", n_names, OSMT_CASCADE_MAX_LAYERS);
    if (T.key_off.size() - 1 > OSMT_LABEL_TEXT_KEYS_MAX)
        return fail(OSMT_UNSUPPORTED, "rules: %zu distinct text strings (> OSMT_LABEL_TEXT_KEYS_MAX = %u)", T.key_off.size() - 1, OSMT_LABEL_TEXT_KEYS_MAX);
    return OSMT_OK;
}

int register_rules_body(osmt_ctx* ctx, const osmt_rules_desc* d, uint32_t flags, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_cs_tables T;
    const int rc = validate_rules(d, flags, ctx, &T);
    if (rc != OSMT_OK) return rc;
    std::shared_ptr<const std::vector<uint8_t>> zooms;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        zooms = ctx->selectors[d->selectors_id].zooms;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    const size_t o_p = pl.add(T.props.size() * sizeof(osmt_cs_prop)), o_l = pl.add(T.rule_last.size() * 4), o_r = pl.add(d->n_selectors * 4);
    const size_t o_g = pl.add(d->n_selectors), o_z = pl.add(d->n_selectors * 2), o_n = pl.add(d->n_numbers * 8);
    table_upload up("rules", pl);
    char* pool = up.pool;
    up.put(o_p, T.props.data(), T.props.size() * sizeof(osmt_cs_prop));
    up.put(o_l, T.rule_last.data(), T.rule_last.size() * 4);
    up.put(o_r, d->selector_rule, d->n_selectors * 4);
    up.put(o_g, T.sel_layer.data(), d->n_selectors);
    up.put(o_z, zooms->data(), d->n_selectors * 2);
    up.put(o_n, d->numbers, d->n_numbers * 8);
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::rules_host h;
    h.d_pool = pool;
    h.selectors_id = d->selectors_id;
    h.dev.props = (const osmt_cs_prop*)(pool + o_p);
    h.dev.rule_last = (const uint32_t*)(pool + o_l);
    h.dev.sel_rule = (const uint32_t*)(pool + o_r);
    h.dev.sel_layer = (const uint8_t*)(pool + o_g);
    h.dev.sel_zoom = (const uint8_t*)(pool + o_z);
    h.dev.numbers = (const double*)(pool + o_n);
    h.dev.n_sels = (uint32_t)d->n_selectors, h.dev.n_layers = T.n_layers, h.dev.star = T.star, h.dev.base = T.base;
    h.dev.font_id = d->font_id, h.dev.flags = flags;
    h.dev.casing_width_multiplier = d->casing_width_multiplier;
    h.dev.font_size_multiplier = d->has_font_size_multiplier ? d->font_size_multiplier : 1.0;
    h.key_off = std::make_shared<std::vector<uint32_t>>(std::move(T.key_off));
    h.key_bytes = std::make_shared<std::vector<uint8_t>>(std::move(T.key_bytes));
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out_id = (uint32_t)ctx->rules.size();
    ctx->rules.push_back(h);
    up.release();
    return OSMT_OK;
}

int cascade_classes_body(osmt_ctx* ctx, osmt_match* m, uint32_t rules_id, uint32_t labels_all, osmt_cascade** out) {
    if (!ctx || !m || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (m->ctx != ctx) return fail(OSMT_INVALID_ARG, "cascade: the match belongs to another context");
    if (!m->complete) return fail(OSMT_INVALID_ARG, "cascade: the match is in the declined state");
    if (labels_all > 1u) return fail(OSMT_INVALID_ARG, "cascade: labels_all = %u (0 or 1)", labels_all);
    osmt_ctx::rules_host rules;
    uint32_t hash_bits = 32;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (rules_id >= ctx->rules.size()) return fail(OSMT_INVALID_ARG, "cascade: rules id %u is not registered (%zu sets)", rules_id, ctx->rules.size());
        rules = ctx->rules[rules_id];
        hash_bits = ctx->match_hash_bits;
    }
    if (rules.selectors_id != m->selectors_id)
        return fail(OSMT_INVALID_ARG, "cascade: the match was made with selector set %u, the rules are over set %u", m->selectors_id, rules.selectors_id);
    const size_t n_classes = m->n_classes;
    if (n_classes * (size_t)OSMT_CS_ZOOMS >= 0xFFFFFFFFull / 32u)
        return fail(OSMT_UNSUPPORTED, "cascade: %zu classes x %u zooms do not fit the 32-bit lane index", n_classes, OSMT_CS_ZOOMS);
    HIP_TRY(hipSetDevice(ctx->device));
    /* the trace: the device time of the stages */
    enum { EV_0, EV_LAYERS, EV_FOLD, EV_DISTINCT, EV_COMPACT, EV_RANGES, EV_N };
    call_work wg(ctx, "cascade");
    const int brc = wg.begin(EV_N);
    if (brc != OSMT_OK) return brc;
    hipStream_t st = wg.st;
    const bool trace = wg.trace;
    pool_layout pl;
    /* the stages' buffers: one slot each, `base` the newest, and the layout starts over behind every one */
    char* base = nullptr;
    int n_work = 0;
    auto alloc = [&](const char* what) {
        const int arc = wg.alloc(n_work, pl, what);
        if (arc != OSMT_OK) return arc;
        base = wg.work[n_work++];
        pl = pool_layout();
        return (int)OSMT_OK;
    };

    unsigned long long tot[OSMT_CS_T_N] = {};
    osmt_cs_pass P;
    memset(&P, 0, sizeof P);
    P.R = rules.dev;
    const bool class_layers = (rules.dev.flags & OSMT_RULES_CLASS_LAYERS) != 0u;
    P.classes = m->d_classes, P.class_sels = m->d_class_sels;
    P.n_classes = (uint32_t)n_classes, P.n_pairs = (uint32_t)(n_classes * OSMT_CS_ZOOMS);
    P.labels_all = labels_all;
    P.hash_mask = hash_bits >= 32u ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
    auto read_tot = [&](int first, int n) {
        hipError_t e = hipMemcpyAsync(tot + first, P.tot + first, (size_t)n * 8, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };
    /* 1. count */
    const size_t n_pairs = P.n_pairs;
    const size_t o_pp = pl.add((n_pairs + 1) * 4), o_tot = pl.add(OSMT_CS_T_N * 8), o_zd = pl.add(OSMT_CS_ZOOMS * 4), o_blk0 = pl.add((n_pairs / 256 + 1) * 8);
    const size_t o_sl = class_layers ? pl.add(m->n_class_sels) : 0, o_ci = class_layers ? pl.add(n_classes * 4) : 0;
    int rc = alloc("pairs");
    if (rc != OSMT_OK) return rc;
    if (class_layers) P.sel_local = (uint8_t*)(base + o_sl), P.class_info = (uint32_t*)(base + o_ci);
    P.pair_pos = (uint32_t*)(base + o_pp);
    P.tot = (unsigned long long*)(base + o_tot);
    P.zoom_differs = (uint32_t*)(base + o_zd);
    P.blk = (unsigned long long*)(base + o_blk0);
    HIP_TRY(wg.mark(EV_0));
    HIP_TRY(osmt_launch_cs_class_layers(P, st));
    HIP_TRY(wg.mark(EV_LAYERS));
    HIP_TRY(osmt_launch_cs_count(P, st));
    HIP_TRY(read_tot(class_layers ? OSMT_CS_T_BAD_CLASS : OSMT_CS_T_STYLES, class_layers ? 2 : 1));
    if (class_layers && tot[OSMT_CS_T_BAD_CLASS] != ~0ull) {
        /* the lowest class over the bound; its exact count is in its word */
        const size_t bad = (size_t)tot[OSMT_CS_T_BAD_CLASS];
        uint32_t info = 0;
        HIP_TRY(hipMemcpyAsync(&info, P.class_info + bad, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return fail(OSMT_UNSUPPORTED, "cascade: the selectors of class %zu name %u distinct layers (> OSMT_CASCADE_MAX_CLASS_LAYERS = %u)", bad,
                    OSMT_CS_CI_LAYERS(info), OSMT_CASCADE_MAX_CLASS_LAYERS);
    }
    if (tot[OSMT_CS_T_STYLES] > 0x80000000ull)
        return fail(OSMT_UNSUPPORTED, "cascade: %llu styles over all classes and zooms (the table of distinct records holds at most 2^31)", tot[OSMT_CS_T_STYLES]);
    const size_t n_styles = (size_t)tot[OSMT_CS_T_STYLES];
    P.n_styles = (uint32_t)n_styles;
    /* 2. fold and records */
    size_t table = 2;
    while (table < 2 * n_styles) table <<= 1;
    P.table_mask = (uint32_t)(table - 1);
    const size_t o_rows = pl.add(n_styles * OSMT_CS_ROW_WORDS * 4), o_area = pl.add(n_styles * sizeof(osmt_style_rec)), o_lab = pl.add(n_styles * sizeof(osmt_label_style_rec));
    const size_t o_key = pl.add(n_styles * 4), o_bp = pl.add((n_styles + 1) * 4), o_blk = pl.add((std::max(n_styles, n_pairs) / 256 + 1) * 8);
    size_t o_hash[2], o_ts[2], o_fp[2], o_id[2], o_tab[2], o_low[2];
    for (int k = 0; k < 2; ++k) {
        o_hash[k] = pl.add(n_styles * 4), o_ts[k] = pl.add(n_styles * 4), o_fp[k] = pl.add((n_styles + 1) * 4), o_id[k] = pl.add(n_styles * 4);
        o_tab[k] = pl.add(table * 4), o_low[k] = pl.add(table * 4);
    }
    rc = alloc("styles");
    if (rc != OSMT_OK) return rc;
    P.rows = (uint32_t*)(base + o_rows);
    P.area = (osmt_style_rec*)(base + o_area);
    P.label = (osmt_label_style_rec*)(base + o_lab);
    P.text_key = (uint32_t*)(base + o_key);
    P.bind_pos = (uint32_t*)(base + o_bp);
    P.blk = (unsigned long long*)(base + o_blk);
    for (int k = 0; k < 2; ++k) {
        P.hash[k] = (uint32_t*)(base + o_hash[k]), P.tslot[k] = (uint32_t*)(base + o_ts[k]), P.first_pos[k] = (uint32_t*)(base + o_fp[k]);
        P.id[k] = (uint32_t*)(base + o_id[k]), P.table[k] = (uint32_t*)(base + o_tab[k]), P.lowest[k] = (uint32_t*)(base + o_low[k]);
    }
    HIP_TRY(osmt_launch_cs_fold(P, st));
    HIP_TRY(wg.mark(EV_FOLD));
    /* 3. distinct records */
    HIP_TRY(osmt_launch_cs_distinct(P, st));
    HIP_TRY(read_tot(OSMT_CS_T_BINDINGS, 3));
    P.n_bindings = (uint32_t)tot[OSMT_CS_T_BINDINGS], P.n_area = (uint32_t)tot[OSMT_CS_T_AREA], P.n_label = (uint32_t)tot[OSMT_CS_T_LABEL];
    const size_t n_area = P.n_area, n_label = P.n_label;
    const size_t o_dp = pl.add((n_area + 1) * 4), o_r0 = pl.add(n_area * 4), o_r1 = pl.add(n_label * 4);
    const size_t o_oa = pl.add(n_area * sizeof(osmt_style_rec)), o_ol = pl.add(n_label * sizeof(osmt_label_style_rec));
    rc = alloc("distinct records");
    if (rc != OSMT_OK) return rc;
    P.dash_pos = (uint32_t*)(base + o_dp);
    P.rep[0] = (uint32_t*)(base + o_r0), P.rep[1] = (uint32_t*)(base + o_r1);
    P.out_area = (osmt_style_rec*)(base + o_oa);
    P.out_label = (osmt_label_style_rec*)(base + o_ol);
    HIP_TRY(osmt_launch_cs_rank(P, st));
    HIP_TRY(read_tot(OSMT_CS_T_DASHES, 1));
    HIP_TRY(wg.mark(EV_DISTINCT));
    const size_t n_dashes = (size_t)tot[OSMT_CS_T_DASHES]; /* at most 2 x 2^32 per record sum: checked against 32 bits below */
    if (n_dashes >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "cascade: %zu dashes of the distinct styles (> 2^32 - 2)", n_dashes);
    (void)pl.add(n_dashes * 8);
    rc = alloc("dashes");
    if (rc != OSMT_OK) return rc;
    P.out_dashes = (double*)base;
    HIP_TRY(osmt_launch_cs_compact(P, st));
    uint32_t differs[OSMT_CS_ZOOMS] = {};
    HIP_TRY(hipMemcpyAsync(differs, P.zoom_differs, sizeof differs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(wg.mark(EV_COMPACT));
    /* 4. zoom ranges: the maximal runs */
    std::unique_ptr<osmt_cascade> c(new osmt_cascade);
    for (uint32_t z = 0; z < OSMT_CS_ZOOMS; ++z) {
        if (z == 0 || differs[z]) {
            P.range_zoom[c->zoom_lo.size()] = (uint8_t)z;
            c->zoom_lo.push_back((uint8_t)z);
            c->zoom_hi.push_back((uint8_t)z);
        } else {
            c->zoom_hi.back() = (uint8_t)z;
        }
    }
    const size_t n_ranges = c->zoom_lo.size(), n_rc = n_ranges * n_classes;
    P.n_ranges = (uint32_t)n_ranges;
    const size_t o_rs = pl.add((n_rc + 1) * 4), o_rb = pl.add((n_rc + 1) * 4), o_so = pl.add(n_ranges * (n_classes + 1) * 4), o_bo = pl.add(n_ranges * (n_classes + 1) * 4);
    const size_t o_blk2 = pl.add((n_rc / 256 + 1) * 8);
    rc = alloc("ranges");
    if (rc != OSMT_OK) return rc;
    P.rs_pos = (uint32_t*)(base + o_rs), P.rb_pos = (uint32_t*)(base + o_rb);
    P.out_style_off = (uint32_t*)(base + o_so), P.out_bind_off = (uint32_t*)(base + o_bo);
    P.blk = (unsigned long long*)(base + o_blk2);
    HIP_TRY(osmt_launch_cs_range_count(P, st));
    HIP_TRY(read_tot(OSMT_CS_T_RANGE_STYLES, 2));
    if (tot[OSMT_CS_T_RANGE_STYLES] >= 0xFFFFFFFFull || tot[OSMT_CS_T_RANGE_BINDINGS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "cascade: %llu class styles and %llu class label bindings over the %zu zoom ranges (> 2^32 - 2)", tot[OSMT_CS_T_RANGE_STYLES],
                    tot[OSMT_CS_T_RANGE_BINDINGS], n_ranges);
    const size_t n_rs = (size_t)tot[OSMT_CS_T_RANGE_STYLES], n_rb = (size_t)tot[OSMT_CS_T_RANGE_BINDINGS];
    const size_t o_os = pl.add(n_rs * 4), o_ob = pl.add(n_rb * sizeof(osmt_class_label_binding));
    rc = alloc("lists");
    if (rc != OSMT_OK) return rc;
    P.out_styles = (uint32_t*)(base + o_os);
    P.out_binds = (osmt_class_label_binding*)(base + o_ob);
    HIP_TRY(osmt_launch_cs_range_emit(P, st));
    HIP_TRY(wg.mark(EV_RANGES));
    /* 5. the result comes to the host: the registrations take host arrays */
    c->ctx = ctx, c->geodata_id = m->geodata_id, c->selectors_id = m->selectors_id, c->n_classes = n_classes;
    c->key_off = rules.key_off, c->key_bytes = rules.key_bytes;
    c->styles.resize(n_area), c->dashes.resize(n_dashes), c->label_styles.resize(n_label);
    c->class_style_off.resize(n_ranges * (n_classes + 1)), c->class_off.resize(n_ranges * (n_classes + 1));
    c->class_styles.resize(n_rs), c->bindings.resize(n_rb);
    c->range_style_base.resize(n_ranges + 1), c->range_binding_base.resize(n_ranges + 1);
    auto back = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    HIP_TRY(back(c->styles.data(), P.out_area, n_area * sizeof(osmt_style_rec)));
    HIP_TRY(back(c->dashes.data(), P.out_dashes, n_dashes * 8));
    HIP_TRY(back(c->label_styles.data(), P.out_label, n_label * sizeof(osmt_label_style_rec)));
    HIP_TRY(back(c->class_style_off.data(), P.out_style_off, c->class_style_off.size() * 4));
    HIP_TRY(back(c->class_off.data(), P.out_bind_off, c->class_off.size() * 4));
    HIP_TRY(back(c->class_styles.data(), P.out_styles, n_rs * 4));
    HIP_TRY(back(c->bindings.data(), P.out_binds, n_rb * sizeof(osmt_class_label_binding)));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t r = 0; r <= n_ranges; ++r) {
        /* a range's base is the sum of the ranges before it: the last offset of each */
        c->range_style_base[r] = r ? c->range_style_base[r - 1] + c->class_style_off[(r - 1) * (n_classes + 1) + n_classes] : 0u;
        c->range_binding_base[r] = r ? c->range_binding_base[r - 1] + c->class_off[(r - 1) * (n_classes + 1) + n_classes] : 0u;
    }
    /* what the registrations would refuse of a produced record is refused here, naming its lowest user */
    for (int k = 0; k < 2; ++k) {
        const size_t n = k == 0 ? n_area : n_label;
        size_t bad = n;
        int vrc = OSMT_OK;
        for (size_t i = 0; i < n && vrc == OSMT_OK; ++i) {
            vrc = k == 0 ? validate_styles(&c->styles[i], 1, c->dashes.data(), n_dashes, ctx_image_count(ctx)) : validate_label_styles(&c->label_styles[i], 1, ctx);
            if (vrc != OSMT_OK) bad = i;
        }
        if (vrc == OSMT_OK) continue;
        const std::string why = osmt_last_error(); /* the thread-local itself is private to osmt_api.cpp */
        uint32_t s = 0, user[2] = {};
        HIP_TRY(copy_back(ctx, &s, P.rep[k] + bad, 4));
        HIP_TRY(copy_back(ctx, user, P.rows + (size_t)s * OSMT_CS_ROW_WORDS + OSMT_CS_ROW_PAIR, 8));
        return fail(vrc == OSMT_UNSUPPORTED ? OSMT_UNSUPPORTED : OSMT_INVALID_ARG,
                    "cascade: distinct %s %zu is refused (%s); it is produced first by class %u at zoom %u, layer position %u", k == 0 ? "style" : "label style", bad,
                    why.c_str(), user[0] / OSMT_CS_ZOOMS, user[0] % OSMT_CS_ZOOMS, user[1]);
    }
    ctx->refs.fetch_add(1);
    *out = c.release();
    if (trace) {
        fprintf(stderr,
                "osmt cascade: count + fold + records %.1f us, distinct %.1f us, compact + zooms %.1f us, ranges %.1f us (%zu classes, %zu styles, %zu + %zu "
                "distinct, %zu ranges), class layers %.1f us\n",
                wg.us(EV_LAYERS, EV_FOLD), wg.us(EV_FOLD, EV_DISTINCT), wg.us(EV_DISTINCT, EV_COMPACT), wg.us(EV_COMPACT, EV_RANGES), n_classes, n_styles, n_area, n_label, n_ranges,
                wg.us(EV_0, EV_LAYERS));
    }
    return OSMT_OK;
}

int cascade_read_body(osmt_cascade* c, osmt_style_rec* styles, double* dashes, osmt_label_style_rec* label_styles, uint8_t* key_bytes, uint32_t* key_off,
                      uint8_t* zoom_lo, uint8_t* zoom_hi, uint32_t* class_style_off, uint32_t* class_styles, uint32_t* range_style_base, uint32_t* class_off,
                      osmt_class_label_binding* bindings, uint32_t* range_binding_base, const size_t caps[8], size_t counts[9]) {
    if (!c || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    const size_t n_ranges = c->zoom_lo.size();
    counts[0] = c->styles.size(), counts[1] = c->dashes.size(), counts[2] = c->label_styles.size(), counts[3] = c->key_bytes->size();
    counts[4] = c->key_off->size() - 1, counts[5] = n_ranges, counts[6] = c->class_styles.size(), counts[7] = c->bindings.size(), counts[8] = c->n_classes;
    const bool any = styles || dashes || label_styles || key_bytes || key_off || zoom_lo || zoom_hi || class_style_off || class_styles || range_style_base ||
                     class_off || bindings || range_binding_base;
    if (!any) return OSMT_OK;
    if (!caps) return fail(OSMT_INVALID_ARG, "NULL caps with an output");
    const bool wants[8] = {styles != nullptr,
                           dashes != nullptr,
                           label_styles != nullptr,
                           key_bytes != nullptr,
                           key_off != nullptr,
                           zoom_lo || zoom_hi || class_style_off || range_style_base || class_off || range_binding_base,
                           class_styles != nullptr,
                           bindings != nullptr};
    for (int i = 0; i < 8; ++i)
        if (wants[i] && caps[i] < counts[i]) return fail(OSMT_INVALID_ARG, "cascade read: caps[%d] = %zu is less than %zu", i, caps[i], counts[i]);
    auto put = [](void* dst, const void* src, size_t bytes) {
        if (dst && bytes) memcpy(dst, src, bytes);
    };
    put(styles, c->styles.data(), c->styles.size() * sizeof(osmt_style_rec));
    put(dashes, c->dashes.data(), c->dashes.size() * 8);
    put(label_styles, c->label_styles.data(), c->label_styles.size() * sizeof(osmt_label_style_rec));
    put(key_bytes, c->key_bytes->data(), c->key_bytes->size());
    put(key_off, c->key_off->data(), c->key_off->size() * 4);
    put(zoom_lo, c->zoom_lo.data(), n_ranges);
    put(zoom_hi, c->zoom_hi.data(), n_ranges);
    put(class_style_off, c->class_style_off.data(), c->class_style_off.size() * 4);
    put(class_styles, c->class_styles.data(), c->class_styles.size() * 4);
    put(range_style_base, c->range_style_base.data(), c->range_style_base.size() * 4);
    put(class_off, c->class_off.data(), c->class_off.size() * 4);
    put(bindings, c->bindings.data(), c->bindings.size() * sizeof(osmt_class_label_binding));
    put(range_binding_base, c->range_binding_base.data(), c->range_binding_base.size() * 4);
    return OSMT_OK;
}

int cascade_register_body(osmt_ctx* ctx, osmt_cascade* c, osmt_match* m, uint32_t what, uint32_t* bind_of_zoom, uint32_t* label_of_zoom, uint32_t* area_label_of_zoom) {
    if (!ctx || !c || !m) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (c->ctx != ctx || m->ctx != ctx) return fail(OSMT_INVALID_ARG, "cascade register: the cascade or the match belongs to another context");
    if (!m->complete || m->n_classes != c->n_classes || m->geodata_id != c->geodata_id || m->selectors_id != c->selectors_id)
        return fail(OSMT_INVALID_ARG, "cascade register: the match is not the one the cascade was made from");
    const uint32_t all = OSMT_CASCADE_AREA_STYLES | OSMT_CASCADE_NODE_LABELS | OSMT_CASCADE_AREA_LABELS;
    if (what == 0u || (what & ~all)) return fail(OSMT_INVALID_ARG, "cascade register: what = 0x%x (a non-empty set of OSMT_CASCADE_* bits)", what);
    if (((what & OSMT_CASCADE_AREA_STYLES) && !bind_of_zoom) || ((what & OSMT_CASCADE_NODE_LABELS) && !label_of_zoom) ||
        ((what & OSMT_CASCADE_AREA_LABELS) && !area_label_of_zoom))
        return fail(OSMT_INVALID_ARG, "cascade register: NULL id array for a table `what` asks for");
    for (uint32_t* a : {bind_of_zoom, label_of_zoom, area_label_of_zoom})
        if (a) std::fill(a, a + OSMT_MAX_ZOOM + 1, OSMT_BINDINGS_NONE);
    const size_t n = c->n_classes, n_ranges = c->zoom_lo.size();
    int rc = OSMT_OK;
    if (what & OSMT_CASCADE_AREA_STYLES) {
        uint32_t first = 0;
        rc = register_styles_body(ctx, c->styles.data(), c->styles.size(), c->dashes.data(), c->dashes.size(), &first);
        std::vector<uint32_t> ids;
        for (size_t r = 0; r < n_ranges && rc == OSMT_OK; ++r) {
            ids.assign(c->class_styles.begin() + c->range_style_base[r], c->class_styles.begin() + c->range_style_base[r + 1]);
            for (uint32_t& v : ids) v += first;
            uint32_t id = 0;
            rc = bindings_matched_body(ctx, m, c->zoom_lo[r], c->zoom_hi[r], c->class_style_off.data() + r * (n + 1), ids.data(), n, &id);
            for (uint32_t z = c->zoom_lo[r]; rc == OSMT_OK && z <= c->zoom_hi[r]; ++z) bind_of_zoom[z] = id;
        }
        if (rc != OSMT_OK) return rc;
    }
    if (what & (OSMT_CASCADE_NODE_LABELS | OSMT_CASCADE_AREA_LABELS)) {
        uint32_t first = 0;
        rc = register_label_styles_body(ctx, c->label_styles.data(), c->label_styles.size(), &first);
        std::vector<osmt_class_label_binding> b;
        for (size_t r = 0; r < n_ranges && rc == OSMT_OK; ++r) {
            b.assign(c->bindings.begin() + c->range_binding_base[r], c->bindings.begin() + c->range_binding_base[r + 1]);
            for (osmt_class_label_binding& v : b) v.style += first;
            osmt_class_label_bindings_desc d{};
            d.zoom_lo = c->zoom_lo[r], d.zoom_hi = c->zoom_hi[r];
            d.class_off = c->class_off.data() + r * (n + 1);
            d.bindings = b.data();
            d.n_classes = n, d.n_bindings = b.size();
            d.key_off = c->key_off->data(), d.key_bytes = c->key_bytes->data();
            d.n_keys = c->key_off->size() - 1, d.n_key_bytes = c->key_bytes->size();
            uint32_t id = 0;
            if (what & OSMT_CASCADE_NODE_LABELS) {
                rc = label_bindings_matched_body(ctx, m, &d, &id, false);
                for (uint32_t z = d.zoom_lo; rc == OSMT_OK && z <= d.zoom_hi; ++z) label_of_zoom[z] = id;
            }
            if (rc == OSMT_OK && (what & OSMT_CASCADE_AREA_LABELS)) {
                rc = label_bindings_matched_body(ctx, m, &d, &id, true);
                for (uint32_t z = d.zoom_lo; rc == OSMT_OK && z <= d.zoom_hi; ++z) area_label_of_zoom[z] = id;
            }
        }
    }
    return rc;
}

}  // namespace

int osmt_validate_rules_ex(const osmt_rules_desc* rules, uint32_t flags, osmt_ctx* ctx) {
    return guarded([&] { return validate_rules(rules, flags, ctx, nullptr); });
}
int osmt_validate_rules(const osmt_rules_desc* rules, osmt_ctx* ctx) { return osmt_validate_rules_ex(rules, 0u, ctx); }
int osmt_register_rules_ex(osmt_ctx* ctx, const osmt_rules_desc* rules, uint32_t flags, uint32_t* out_rules_id) {
    return guarded([&] { return register_rules_body(ctx, rules, flags, out_rules_id); });
}
int osmt_register_rules(osmt_ctx* ctx, const osmt_rules_desc* rules, uint32_t* out_rules_id) { return osmt_register_rules_ex(ctx, rules, 0u, out_rules_id); }
int osmt_cascade_classes(osmt_ctx* ctx, osmt_match* match, uint32_t rules_id, uint32_t labels_all, osmt_cascade** out) {
    return guarded([&] { return cascade_classes_body(ctx, match, rules_id, labels_all, out); });
}
void osmt_cascade_free(osmt_cascade* c) {
    if (!c) return;
    osmt_ctx* ctx = c->ctx;
    delete c;
    ctx_release(ctx);
}
int osmt_cascade_read(osmt_cascade* cascade, osmt_style_rec* styles, double* dashes, osmt_label_style_rec* label_styles, uint8_t* key_bytes,
                      uint32_t* key_off, uint8_t* zoom_lo, uint8_t* zoom_hi, uint32_t* class_style_off, uint32_t* class_styles,
                      uint32_t* range_style_base, uint32_t* class_off, osmt_class_label_binding* bindings, uint32_t* range_binding_base,
                      const size_t caps[8], size_t counts[9]) {
    return guarded([&] {
        return cascade_read_body(cascade, styles, dashes, label_styles, key_bytes, key_off, zoom_lo, zoom_hi, class_style_off, class_styles, range_style_base,
                                 class_off, bindings, range_binding_base, caps, counts);
    });
}
int osmt_cascade_register(osmt_ctx* ctx, osmt_cascade* cascade, osmt_match* match, uint32_t what, uint32_t bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                          uint32_t label_bindings_of_zoom[OSMT_MAX_ZOOM + 1], uint32_t area_label_bindings_of_zoom[OSMT_MAX_ZOOM + 1]) {
    return guarded([&] { return cascade_register_body(ctx, cascade, match, what, bindings_of_zoom, label_bindings_of_zoom, area_label_bindings_of_zoom); });
}
