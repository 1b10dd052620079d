/*
 * osmt_host_pyramid.cpp — host side of libosmtile.so: the tile index pyramid (include/osmtile.h, osmt_tilepyramid.hip).
 * Registration builds the levels on the device, finest first, each from the one before; the tile queries of the other host
 * files ask tq_bind_levels which index a tile of each zoom reads.  The z18 index itself can be built the same way from the
 * nodes' Mercator factors and the topology (osmt_build_tile_index, osmt_tileindex.hip): level 18 from geometry, through the
 * same sort, mark and emit stages.  Shares osmt_host.h with the other host files.
 */
#include "osmt_host.h"

using namespace osmt_host;

namespace {

typedef osmt_ctx::geodata_host geodata_host;
typedef geodata_host::pyramid_level pyramid_level;
typedef geodata_host::pyramid_host pyramid_host;

int validate_pyramid(uint32_t geodata_id, uint32_t mask, osmt_ctx* ctx) {
    if (mask == 0u) return fail(OSMT_INVALID_ARG, "tile pyramid: level mask 0 names no level");
    if (mask & ~(uint32_t)OSMT_PYRAMID_ALL_LEVELS)
        return fail(OSMT_INVALID_ARG, "tile pyramid: level mask 0x%x has bits above level %u", mask, OSMT_MAX_ZOOM);
    if (!ctx) return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u is not registered (no context)", geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size())
        return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    const geodata_host& g = ctx->geodata[geodata_id];
    if (!g.d_index) return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u has no tile index (osmt_register_tile_index)", geodata_id);
    if (g.pyramid || g.pyramid_building) return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u has a tile pyramid already (one per file)", geodata_id);
    return OSMT_OK;
}

/* one sort job of a level: its pairs in two buffers, the scans' arrays and the totals, carved from one work buffer */
struct job {
    unsigned long long* key[2] = {};
    uint32_t* id[2] = {};
    uint32_t *pos = nullptr, *cpos = nullptr, *counts = nullptr, *hist = nullptr;
    unsigned long long *blk = nullptr, *tot = nullptr;
    uint32_t n = 0;
    int at = 0;           /* which buffer holds the pairs */
    uint64_t distinct = 0, cols = 0;
    double wait_us = 0.0; /* host time blocked in the job's read-backs, and their number (OSMT_TRACE_UPLOAD) */
    uint32_t n_waits = 0;
};

/* the stream synchronised, the time the host was blocked added to *us */
hipError_t timed_sync(hipStream_t st, double* us, uint32_t* n) {
    ++*n;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipStreamSynchronize(st);
    *us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return e;
}

const char* const KIND[4] = {"tile", "way", "multipolygon", "node"};

/* where a job's pairs come from: `n` pairs written into (key, id) on the stream — an osmt_pyr_src of a finer level, or pairs
 * some other stage has ready */
struct pair_source {
    size_t n = 0;
    std::function<hipError_t(unsigned long long* key, uint32_t* id, hipStream_t st)> emit;
};

pair_source source_pairs(const osmt_pyr_src& src, bool tiles) {
    pair_source p;
    p.n = tiles ? src.n_tiles : src.n_refs;
    p.emit = [src, tiles](unsigned long long* key, uint32_t* id, hipStream_t st) {
        return tiles ? osmt_launch_pyr_tilekeys(src, key, id, st) : osmt_launch_pyr_pairs(src, key, id, st);
    };
    return p;
}

/* takes the pairs of `src` (tiles: tile keys), sorts them, numbers the distinct ones; reads the totals back.  who: "tile pyramid:
 * level 12" in the refusal.  ev >= 0: trace events ev and ev + 1 of `wg` go around the sort passes */
int run_job(call_work& wg, int slot, const pair_source& src, bool tiles, const char* who, const char* kind, job& j, int ev = -1) {
    hipStream_t st = wg.st;
    const size_t n = src.n, n_wg = (n + OSMT_PYR_SORT_BLOCK - 1) / OSMT_PYR_SORT_BLOCK;
    pool_layout pl;
    const size_t o_k0 = pl.add(n * 8), o_k1 = pl.add(n * 8), o_i0 = pl.add(n * 4), o_i1 = pl.add(n * 4), o_pos = pl.add((n + 1) * 4);
    const size_t o_cpos = pl.add(tiles ? (n + 1) * 4 : 0), o_cnt = pl.add((256 * n_wg + 1) * 4), o_hist = pl.add(OSMT_PYR_DIGITS * 256 * 4);
    const size_t o_blk = pl.add((std::max(n_wg, n / 256) + 1) * 8), o_tot = pl.add(2 * 8);
    const int rc = wg.alloc(slot, pl, kind);
    if (rc != OSMT_OK) return rc;
    char* w = wg.work[slot];
    j.key[0] = (unsigned long long*)(w + o_k0), j.key[1] = (unsigned long long*)(w + o_k1);
    j.id[0] = (uint32_t*)(w + o_i0), j.id[1] = (uint32_t*)(w + o_i1);
    j.pos = (uint32_t*)(w + o_pos), j.cpos = tiles ? (uint32_t*)(w + o_cpos) : nullptr;
    j.counts = (uint32_t*)(w + o_cnt), j.hist = (uint32_t*)(w + o_hist);
    j.blk = (unsigned long long*)(w + o_blk), j.tot = (unsigned long long*)(w + o_tot);
    j.n = (uint32_t)n, j.at = 0;
    HIP_TRY(src.emit(j.key[0], j.id[0], st));
    /* the digits that differ among the pairs: a digit whose histogram has one non-empty bin is not sorted on */
    std::vector<uint32_t> hist(OSMT_PYR_DIGITS * 256);
    if (n > 1) {
        HIP_TRY(osmt_launch_pyr_digits(j.key[0], j.id[0], j.n, j.hist, st));
        HIP_TRY(hipMemcpyAsync(hist.data(), j.hist, hist.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(timed_sync(st, &j.wait_us, &j.n_waits));
        if (ev >= 0) HIP_TRY(wg.mark(ev));
        for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) {
            bool one_bin = false;
            for (uint32_t b = 0; b < 256; ++b) one_bin = one_bin || hist[d * 256 + b] == n;
            if (one_bin) continue;
            HIP_TRY(osmt_launch_pyr_pass(j.key[j.at], j.id[j.at], j.n, d, j.counts, j.blk, j.tot, j.key[j.at ^ 1], j.id[j.at ^ 1], st));
            j.at ^= 1;
        }
        if (ev >= 0) HIP_TRY(wg.mark(ev + 1));
    }
    HIP_TRY(osmt_launch_pyr_mark(j.key[j.at], j.id[j.at], j.n, j.pos, j.cpos, j.blk, j.tot, st));
    unsigned long long tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, j.tot, tiles ? 16 : 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(timed_sync(st, &j.wait_us, &j.n_waits));
    j.distinct = tot[0], j.cols = tot[1];
    if (j.distinct >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "%s has %llu %s references (> 2^32)", who, (unsigned long long)j.distinct, kind);
    return OSMT_OK;
}

/* the source of one kind for the level below `lv` */
osmt_pyr_src source_of(const pyramid_level& lv, int kind, uint32_t shift) {
    osmt_pyr_src s{};
    s.col_x = lv.ix.col_x, s.col_first = lv.ix.col_first, s.tile_y = lv.ix.tile_y;
    s.n_cols = lv.ix.n_cols, s.n_tiles = lv.ix.n_tiles, s.shift = shift;
    if (kind == 1) s.off = lv.ix.way_off, s.pool = lv.ix.ways, s.n_refs = (uint32_t)lv.n_way_refs;
    if (kind == 2) s.off = lv.ix.mp_off, s.pool = lv.ix.mps, s.n_refs = (uint32_t)lv.n_mp_refs;
    if (kind == 3) s.off = lv.node_off, s.pool = lv.nodes, s.n_refs = (uint32_t)lv.n_node_refs;
    return s;
}

/* level `level` from `from` (the registered index as a level, or the level built before) */
int build_level(osmt_ctx* ctx, hipStream_t st, const pyramid_level& from, uint32_t level, bool with_nodes, pyramid_level& out, void** out_pool) {
    call_work wg(ctx, "tile pyramid", st);
    int rc = wg.begin(0);
    if (rc != OSMT_OK) return rc;
    const uint32_t shift = from.ix.level - level;
    const int n_kinds = with_nodes ? 4 : 3;
    job jobs[4];
    char who[48];
    snprintf(who, sizeof who, "tile pyramid: level %u", level);
    for (int k = 0; k < n_kinds; ++k) {
        const osmt_pyr_src src = source_of(from, k, shift);
        const uint64_t pairs = k ? src.n_refs : src.n_tiles; /* both below 2^32 - 1: checked when the source was made */
        if (pairs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "tile pyramid: level %u sorts %llu %s pairs (> 2^32)", level, (unsigned long long)pairs, KIND[k]);
        rc = run_job(wg, k, source_pairs(src, k == 0), k == 0, who, KIND[k], jobs[k]);
        if (rc != OSMT_OK) return rc;
    }
    const size_t n_tiles = (size_t)jobs[0].distinct, n_cols = (size_t)jobs[0].cols;
    const size_t nw = (size_t)jobs[1].distinct, nm = (size_t)jobs[2].distinct, nn = with_nodes ? (size_t)jobs[3].distinct : 0;
    pool_layout pl;
    const size_t o_cx = pl.add(n_cols * 4), o_cf = pl.add((n_cols + 1) * 4), o_tx = pl.add(n_tiles * 4), o_ty = pl.add(n_tiles * 4);
    const size_t o_wo = pl.add((n_tiles + 1) * 4), o_w = pl.add(nw * 4), o_mo = pl.add((n_tiles + 1) * 4), o_m = pl.add(nm * 4);
    const size_t o_no = pl.add(with_nodes ? (n_tiles + 1) * 4 : 0), o_n = pl.add(nn * 4), o_z = pl.add(with_nodes ? (n_tiles + 1) * 4 : 0);
    char* pool = nullptr;
    rc = wg.alloc(&pool, pl, "level");
    if (rc != OSMT_OK) return rc;
    *out_pool = pool; /* the caller's from here on: given back if the registration fails */
    uint32_t *tile_x = (uint32_t*)(pool + o_tx), *tile_y = (uint32_t*)(pool + o_ty);
    const job& t = jobs[0];
    HIP_TRY(osmt_launch_pyr_emit_tiles(t.key[t.at], t.n, t.pos, t.cpos, (uint32_t)n_tiles, (uint32_t)n_cols, tile_x, tile_y, (uint32_t*)(pool + o_cx),
                                       (uint32_t*)(pool + o_cf), st));
    const size_t o_off[4] = {0, o_wo, o_mo, o_no}, o_pool[4] = {0, o_w, o_m, o_n};
    for (int k = 1; k < n_kinds; ++k) {
        const job& j = jobs[k];
        HIP_TRY(osmt_launch_pyr_emit_lists(j.key[j.at], j.id[j.at], j.n, j.pos, tile_x, tile_y, (uint32_t)n_tiles, (uint32_t*)(pool + o_off[k]),
                                           (uint32_t*)(pool + o_pool[k]), st));
    }
    if (with_nodes) HIP_TRY(hipMemsetAsync(pool + o_z, 0, (n_tiles + 1) * 4, st));
    HIP_TRY(hipStreamSynchronize(st));
    out = pyramid_level();
    out.ix.col_x = (const uint32_t*)(pool + o_cx), out.ix.col_first = (const uint32_t*)(pool + o_cf), out.ix.tile_y = tile_y;
    out.ix.way_off = (const uint32_t*)(pool + o_wo), out.ix.ways = (const uint32_t*)(pool + o_w);
    out.ix.mp_off = (const uint32_t*)(pool + o_mo), out.ix.mps = (const uint32_t*)(pool + o_m);
    out.ix.n_cols = (uint32_t)n_cols, out.ix.n_tiles = (uint32_t)n_tiles, out.ix.level = level;
    out.tile_x = tile_x;
    if (with_nodes) out.node_off = (const uint32_t*)(pool + o_no), out.nodes = (const uint32_t*)(pool + o_n), out.zero_off = (const uint32_t*)(pool + o_z);
    out.n_way_refs = nw, out.n_mp_refs = nm, out.n_node_refs = nn;
    return OSMT_OK;
}

int register_pyramid_body(osmt_ctx* ctx, uint32_t geodata_id, uint32_t mask) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    int rc = validate_pyramid(geodata_id, mask, ctx);
    if (rc != OSMT_OK) return rc;
    geodata_host geo;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geodata_host& g = ctx->geodata[geodata_id];
        if (g.pyramid || g.pyramid_building) return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u has a tile pyramid already (one per file)", geodata_id);
        g.pyramid_building = true;
        geo = g;
    }
    std::vector<void*> pools;
    auto built = std::make_shared<pyramid_host>();
    rc = [&]() -> int {
        HIP_TRY(hipSetDevice(ctx->device));
        call_work wg(ctx, "tile pyramid");
        int r = wg.begin(0);
        if (r != OSMT_OK) return r;
        hipStream_t st = wg.st;
        const bool with_nodes = geo.d_node_index != nullptr;
        /* the registered index as the source of the finest level: its reference totals are its last offsets */
        pyramid_level from;
        from.ix = geo.ix;
        uint32_t last[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(&last[0], geo.ix.way_off + geo.ix.n_tiles, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last[1], geo.ix.mp_off + geo.ix.n_tiles, 4, hipMemcpyDeviceToHost, st));
        if (with_nodes) HIP_TRY(hipMemcpyAsync(&last[2], geo.d_node_off + geo.ix.n_tiles, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        from.n_way_refs = last[0], from.n_mp_refs = last[1], from.n_node_refs = last[2];
        if (with_nodes) from.node_off = geo.d_node_off, from.nodes = geo.d_node_refs;
        for (int level = OSMT_MAX_ZOOM; level >= 0; --level) {
            if (!((mask >> level) & 1u)) continue;
            void* pool = nullptr;
            r = build_level(ctx, st, from, (uint32_t)level, with_nodes, built->level[level], &pool);
            if (pool) pools.push_back(pool);
            if (r != OSMT_OK) return r;
            from = built->level[level];
        }
        built->mask = mask;
        built->node_mask = with_nodes ? mask : 0u;
        /* the index of each zoom, resident: a query binds a pointer and uploads nothing */
        osmt_tq_index_dev table[2][OSMT_MAX_ZOOM + 1];
        osmt_tq_index_dev z18_nodes = geo.ix;
        z18_nodes.way_off = geo.d_node_off, z18_nodes.ways = geo.d_node_refs, z18_nodes.mp_off = geo.d_zero_off, z18_nodes.mps = geo.d_node_refs;
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) {
            table[0][z] = geo.ix, table[1][z] = z18_nodes;
            if (!(mask >> z)) continue;
            const pyramid_level& lv = built->level[z + (uint32_t)__builtin_ctz(mask >> z)]; /* the smallest level >= z */
            table[0][z] = table[1][z] = lv.ix;
            table[1][z].way_off = lv.node_off, table[1][z].ways = lv.nodes, table[1][z].mp_off = lv.zero_off, table[1][z].mps = lv.nodes;
        }
        pool_layout pl;
        (void)pl.add(sizeof table);
        char* d_table = nullptr;
        r = wg.alloc(&d_table, pl, "zoom table");
        if (r != OSMT_OK) return r;
        pools.push_back(d_table);
        HIP_TRY(hipMemcpyAsync(d_table, table, sizeof table, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        built->area_table = (const osmt_tq_index_dev*)d_table;
        if (with_nodes) built->node_table = built->area_table + (OSMT_MAX_ZOOM + 1);
        return OSMT_OK;
    }();
    if (rc != OSMT_OK)
        for (void* p : pools) dev_free(ctx, p);
    std::lock_guard<std::mutex> lk(ctx->mu);
    geodata_host& g = ctx->geodata[geodata_id];
    g.pyramid_building = false;
    if (rc == OSMT_OK) g.pyramid = built;
    return rc;
}

int pyramid_of(osmt_ctx* ctx, uint32_t geodata_id, std::shared_ptr<const pyramid_host>* out) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size())
        return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    *out = ctx->geodata[geodata_id].pyramid;
    return OSMT_OK;
}

int read_pyramid_body(osmt_ctx* ctx, uint32_t geodata_id, uint32_t level, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways, uint32_t* mp_off, uint32_t* mps,
                      uint32_t* node_off, uint32_t* nodes, const size_t* caps, size_t* counts) {
    if (!counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    std::shared_ptr<const pyramid_host> p;
    const int rc = pyramid_of(ctx, geodata_id, &p);
    if (rc != OSMT_OK) return rc;
    if (level > OSMT_MAX_ZOOM || !p || !((p->mask >> level) & 1u))
        return fail(OSMT_INVALID_ARG, "tile pyramid: geodata id %u has no level %u (registered levels: mask 0x%x)", geodata_id, level, p ? p->mask : 0u);
    const pyramid_level& lv = p->level[level];
    const size_t n = lv.ix.n_tiles;
    counts[0] = n, counts[1] = lv.n_way_refs, counts[2] = lv.n_mp_refs, counts[3] = lv.n_node_refs;
    if (caps) {
        const void* outs[4] = {tile_xy, ways, mps, nodes};
        for (int k = 0; k < 4; ++k)
            if (outs[k] && caps[k] < counts[k]) return fail(OSMT_INVALID_ARG, "tile pyramid: caps[%d] = %zu is less than the level's %zu", k, caps[k], counts[k]);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (tile_xy && n) {
        std::vector<uint32_t> x(n), y(n);
        HIP_TRY(copy_back(ctx, x.data(), lv.tile_x, n * 4));
        HIP_TRY(copy_back(ctx, y.data(), lv.ix.tile_y, n * 4));
        for (size_t i = 0; i < n; ++i) tile_xy[2 * i] = x[i], tile_xy[2 * i + 1] = y[i];
    }
    if (way_off) HIP_TRY(copy_back(ctx, way_off, lv.ix.way_off, (n + 1) * 4));
    if (ways && lv.n_way_refs) HIP_TRY(copy_back(ctx, ways, lv.ix.ways, lv.n_way_refs * 4));
    if (mp_off) HIP_TRY(copy_back(ctx, mp_off, lv.ix.mp_off, (n + 1) * 4));
    if (mps && lv.n_mp_refs) HIP_TRY(copy_back(ctx, mps, lv.ix.mps, lv.n_mp_refs * 4));
    if (node_off) {
        if (lv.node_off)
            HIP_TRY(copy_back(ctx, node_off, lv.node_off, (n + 1) * 4));
        else
            memset(node_off, 0, (n + 1) * 4);
    }
    if (nodes && lv.n_node_refs) HIP_TRY(copy_back(ctx, nodes, lv.nodes, lv.n_node_refs * 4));
    return OSMT_OK;
}

/* ---- the z18 index itself, built from geometry (osmt_build_tile_index, osmt_tileindex.hip) ---------------------------- */
int validate_index_build(uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes, osmt_ctx* ctx) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u is not registered (no context)", geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size())
        return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    const geodata_host& g = ctx->geodata[geodata_id];
    if (!g.d_factors) return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has no Mercator factors (osmt_register_node_mercator)", geodata_id);
    if (g.d_index || g.index_building) return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has a tile index already (one per file)", geodata_id);
    if (node_ids && n_nodes != g.n_nodes)
        return fail(OSMT_INVALID_ARG, "tile index build: n_nodes = %zu, the geodata has %zu nodes", n_nodes, g.n_nodes);
    if (node_ids && g.d_node_index) return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has a node index already (one per file)", geodata_id);
    return OSMT_OK;
}

/* what a successful build hands to the registration */
struct built_index {
    char* pool = nullptr;
    osmt_tq_index_dev ix{};
    const uint32_t *node_off = nullptr, *nodes = nullptr, *zero_off = nullptr;
    const uint64_t* node_gid = nullptr;
};

int build_index(osmt_ctx* ctx, const geodata_host& geo, const uint64_t* node_ids, built_index& out) {
    HIP_TRY(hipSetDevice(ctx->device));
    call_work wg(ctx, "tile index build");
    int rc = wg.begin(8); /* two per job, around its sort passes */
    if (rc != OSMT_OK) return rc;
    hipStream_t st = wg.st;
    const auto t_start = std::chrono::steady_clock::now();
    double wait_us = 0.0;
    uint32_t n_waits = 0;
    const size_t n_nodes = geo.n_nodes, n_ways = geo.n_ways, n_polys = geo.n_polys, n_mps = geo.n_mps;
    /* nodes' tiles, boxes, per-entity tile counts and their scans: work buffer 4 (0 .. 3 are the jobs') */
    osmt_tix_pass P{};
    {
        pool_layout pl;
        const size_t o_tx = pl.add(n_nodes * 4), o_ty = pl.add(n_nodes * 4), o_wb = pl.add(n_ways * 16), o_pb = pl.add(n_polys * 16), o_mb = pl.add(n_mps * 16);
        const size_t o_wc = pl.add((n_ways + 1) * 4), o_mc = pl.add((n_mps + 1) * 4), o_blk = pl.add((std::max(n_ways, n_mps) / 256 + 2) * 8);
        const size_t o_words = pl.add(OSMT_TIX_WORDS * 8);
        rc = wg.alloc(4, pl, "boxes");
        if (rc != OSMT_OK) return rc;
        char* w = wg.work[4];
        P.geo = geo.dev, P.factors = geo.d_factors;
        P.n_nodes = (uint32_t)n_nodes, P.n_ways = (uint32_t)n_ways, P.n_polys = (uint32_t)n_polys, P.n_mps = (uint32_t)n_mps;
        P.n_way_nodes = (uint32_t)geo.n_way_nodes, P.n_poly_nodes = (uint32_t)geo.n_poly_nodes, P.n_mp_polys = (uint32_t)geo.n_mp_polys;
        P.tx = (uint32_t*)(w + o_tx), P.ty = (uint32_t*)(w + o_ty);
        P.way_box = (uint4*)(w + o_wb), P.poly_box = (uint4*)(w + o_pb), P.mp_box = (uint4*)(w + o_mb);
        P.way_cnt = (uint32_t*)(w + o_wc), P.mp_cnt = (uint32_t*)(w + o_mc);
        P.blk = (unsigned long long*)(w + o_blk), P.words = (unsigned long long*)(w + o_words);
    }
    HIP_TRY(osmt_launch_tix_boxes(P, st));
    unsigned long long words[OSMT_TIX_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(words, P.words, sizeof words, hipMemcpyDeviceToHost, st));
    HIP_TRY(timed_sync(st, &wait_us, &n_waits));
    /* the limits, from 64-bit totals, before any pair has a buffer */
    if (words[OSMT_TIX_OFFENDER] != ~0ull)
        return fail(OSMT_UNSUPPORTED,
                    "tile index build: node %llu: %s factor is exactly 1.0 (coordinate 2^18 is outside the zoom-18 world; never clamped)",
                    words[OSMT_TIX_OFFENDER] >> 1, (words[OSMT_TIX_OFFENDER] & 1ull) ? "y" : "x");
    const unsigned long long pairs[4] = {0ull, words[OSMT_TIX_WAY_REFS], words[OSMT_TIX_MP_REFS], (unsigned long long)n_nodes};
    for (int k = 1; k < 4; ++k)
        if (pairs[k] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile index build: %llu %s references do not fit 32 bits (at most %llu)", pairs[k], KIND[k], 0xFFFFFFFEull);
    /* one job per kind: its pairs sorted, then the first of every key marked for the tiles' job */
    job jobs[4];
    unsigned long long keys[4] = {0ull, 0ull, 0ull, 0ull};
    uint32_t* head[4] = {};
    for (int k = 1; k < 4; ++k) {
        pair_source src;
        src.n = (size_t)pairs[k];
        if (k == 1) src.emit = [&](unsigned long long* key, uint32_t* id, hipStream_t s) { return osmt_launch_tix_pairs(P.way_cnt, P.n_ways, P.way_box, (uint32_t)pairs[1], key, id, s); };
        if (k == 2) src.emit = [&](unsigned long long* key, uint32_t* id, hipStream_t s) { return osmt_launch_tix_pairs(P.mp_cnt, P.n_mps, P.mp_box, (uint32_t)pairs[2], key, id, s); };
        if (k == 3) src.emit = [&](unsigned long long* key, uint32_t* id, hipStream_t s) { return osmt_launch_tix_node_pairs(P.tx, P.ty, P.n_nodes, key, id, s); };
        rc = run_job(wg, k, src, false, "tile index build: the index", KIND[k], jobs[k], 2 * k);
        if (rc != OSMT_OK) return rc;
        job& j = jobs[k];
        head[k] = (uint32_t*)j.key[j.at ^ 1]; /* the sort's other buffer is free: n * 8 bytes (at least 4) hold n + 1 words */
        HIP_TRY(osmt_launch_tix_keymark(j.key[j.at], j.n, head[k], j.blk, j.tot + 1, st));
        HIP_TRY(hipMemcpyAsync(&keys[k], j.tot + 1, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(timed_sync(st, &wait_us, &n_waits));
    /* the tiles' job sorts the kinds' distinct keys */
    const unsigned long long n_keys = keys[1] + keys[2] + keys[3];
    if (n_keys >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "tile index build: %llu tile keys do not fit 32 bits (at most %llu)", n_keys, 0xFFFFFFFEull);
    pair_source tsrc;
    tsrc.n = (size_t)n_keys;
    tsrc.emit = [&](unsigned long long* key, uint32_t* id, hipStream_t s) {
        size_t at = 0;
        for (int k = 1; k < 4; ++k) {
            const job& j = jobs[k];
            const hipError_t e = osmt_launch_tix_keycompact(j.key[j.at], j.n, head[k], key + at, id + at, s);
            if (e != hipSuccess) return e;
            at += (size_t)keys[k];
        }
        return hipSuccess;
    };
    rc = run_job(wg, 0, tsrc, true, "tile index build: the index", KIND[0], jobs[0], 0);
    if (rc != OSMT_OK) return rc;
    const size_t n_tiles = (size_t)jobs[0].distinct, n_cols = (size_t)jobs[0].cols;
    const size_t nw = (size_t)pairs[1], nm = (size_t)pairs[2], nn = n_nodes;
    pool_layout pl;
    const size_t o_cx = pl.add(n_cols * 4), o_cf = pl.add((n_cols + 1) * 4), o_tx = pl.add(n_tiles * 4), o_ty = pl.add(n_tiles * 4);
    const size_t o_wo = pl.add((n_tiles + 1) * 4), o_w = pl.add(nw * 4), o_mo = pl.add((n_tiles + 1) * 4), o_m = pl.add(nm * 4);
    const size_t o_no = pl.add((n_tiles + 1) * 4), o_n = pl.add(nn * 4), o_z = pl.add((n_tiles + 1) * 4), o_gid = pl.add(node_ids ? nn * 8 : 0);
    char* pool = nullptr;
    rc = wg.alloc(&pool, pl, "index");
    if (rc != OSMT_OK) return rc;
    out.pool = pool; /* the caller's from here on: given back if the build fails */
    uint32_t *tile_x = (uint32_t*)(pool + o_tx), *tile_y = (uint32_t*)(pool + o_ty);
    const job& t = jobs[0];
    HIP_TRY(osmt_launch_pyr_emit_tiles(t.key[t.at], t.n, t.pos, t.cpos, (uint32_t)n_tiles, (uint32_t)n_cols, tile_x, tile_y, (uint32_t*)(pool + o_cx),
                                       (uint32_t*)(pool + o_cf), st));
    const size_t o_off[4] = {0, o_wo, o_mo, o_no}, o_pool[4] = {0, o_w, o_m, o_n};
    for (int k = 1; k < 4; ++k) {
        const job& j = jobs[k];
        HIP_TRY(osmt_launch_pyr_emit_lists(j.key[j.at], j.id[j.at], j.n, j.pos, tile_x, tile_y, (uint32_t)n_tiles, (uint32_t*)(pool + o_off[k]),
                                           (uint32_t*)(pool + o_pool[k]), st));
    }
    HIP_TRY(hipMemsetAsync(pool + o_z, 0, (n_tiles + 1) * 4, st));
    if (node_ids && nn) HIP_TRY(hipMemcpyAsync(pool + o_gid, node_ids, nn * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(timed_sync(st, &wait_us, &n_waits));
    if (wg.trace) {
        double sort_us = 0.0;
        for (int k = 0; k < 4; ++k) {
            wait_us += jobs[k].wait_us, n_waits += jobs[k].n_waits;
            if (jobs[k].n > 1) sort_us += wg.us(2 * k, 2 * k + 1);
        }
        fprintf(stderr, "osmt tile index build: %.1f us in all, sort passes %.1f us on the device, %.1f us of host time blocked in %u read-backs (%zu tiles, %zu + %zu + %zu references)\n",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(), sort_us, wait_us, n_waits, n_tiles, nw, nm, nn);
    }
    out.ix.col_x = (const uint32_t*)(pool + o_cx), out.ix.col_first = (const uint32_t*)(pool + o_cf), out.ix.tile_y = tile_y;
    out.ix.way_off = (const uint32_t*)(pool + o_wo), out.ix.ways = (const uint32_t*)(pool + o_w);
    out.ix.mp_off = (const uint32_t*)(pool + o_mo), out.ix.mps = (const uint32_t*)(pool + o_m);
    out.ix.n_cols = (uint32_t)n_cols, out.ix.n_tiles = (uint32_t)n_tiles, out.ix.level = OSMT_MAX_ZOOM;
    out.node_off = (const uint32_t*)(pool + o_no), out.nodes = (const uint32_t*)(pool + o_n), out.zero_off = (const uint32_t*)(pool + o_z);
    out.node_gid = node_ids ? (const uint64_t*)(pool + o_gid) : nullptr;
    return OSMT_OK;
}

int build_index_body(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    int rc = validate_index_build(geodata_id, node_ids, n_nodes, ctx);
    if (rc != OSMT_OK) return rc;
    geodata_host geo;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geodata_host& g = ctx->geodata[geodata_id];
        if (g.d_index || g.index_building) return fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has a tile index already (one per file)", geodata_id);
        g.index_building = true;
        geo = g;
    }
    built_index b;
    try {
        rc = build_index(ctx, geo, node_ids, b);
    } catch (...) { /* a std::bad_alloc of a host table: the id may be built for again, the buffer goes back; guarded() reports it */
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->geodata[geodata_id].index_building = false;
        }
        dev_free(ctx, b.pool);
        throw;
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geodata_host& g = ctx->geodata[geodata_id];
        g.index_building = false;
        /* a registration that came in while the build ran was first */
        if (rc == OSMT_OK && g.d_index) rc = fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has a tile index already (one per file)", geodata_id);
        if (rc == OSMT_OK && node_ids && g.d_node_index)
            rc = fail(OSMT_INVALID_ARG, "tile index build: geodata id %u has a node index already (one per file)", geodata_id);
        if (rc == OSMT_OK) {
            g.d_index = b.pool, g.ix = b.ix, g.index_built = true;
            g.built_node_off = b.node_off, g.built_nodes = b.nodes;
            if (node_ids) {
                g.d_node_index = b.pool, g.node_index_built = true;
                g.d_node_gid = b.node_gid, g.d_node_off = b.node_off, g.d_node_refs = b.nodes, g.d_zero_off = b.zero_off;
            }
        }
    }
    if (rc != OSMT_OK) dev_free(ctx, b.pool);
    return rc;
}

int read_index_body(osmt_ctx* ctx, uint32_t geodata_id, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways, uint32_t* mp_off, uint32_t* mps, uint32_t* node_off,
                    uint32_t* nodes, const size_t* caps, size_t* counts) {
    if (!ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    geodata_host geo;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "tile index: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
        geo = ctx->geodata[geodata_id];
    }
    if (!geo.d_index) return fail(OSMT_INVALID_ARG, "tile index: geodata id %u has no tile index (osmt_register_tile_index, osmt_build_tile_index)", geodata_id);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = geo.ix.n_tiles;
    const uint32_t *d_noff = geo.d_node_index ? geo.d_node_off : geo.built_node_off, *d_nodes = geo.d_node_index ? geo.d_node_refs : geo.built_nodes;
    uint32_t last[3] = {0, 0, 0};
    HIP_TRY(copy_back(ctx, &last[0], geo.ix.way_off + n, 4));
    HIP_TRY(copy_back(ctx, &last[1], geo.ix.mp_off + n, 4));
    if (d_noff) HIP_TRY(copy_back(ctx, &last[2], d_noff + n, 4));
    counts[0] = n, counts[1] = last[0], counts[2] = last[1], counts[3] = last[2];
    if (caps) {
        const void* outs[4] = {tile_xy, ways, mps, nodes};
        for (int k = 0; k < 4; ++k)
            if (outs[k] && caps[k] < counts[k]) return fail(OSMT_INVALID_ARG, "tile index: caps[%d] = %zu is less than the index's %zu", k, caps[k], counts[k]);
    }
    if (tile_xy && n) { /* x from the column directory: a registered index keeps no tile_x */
        std::vector<uint32_t> cx(geo.ix.n_cols), cf(geo.ix.n_cols + 1), y(n);
        HIP_TRY(copy_back(ctx, cx.data(), geo.ix.col_x, cx.size() * 4));
        HIP_TRY(copy_back(ctx, cf.data(), geo.ix.col_first, cf.size() * 4));
        HIP_TRY(copy_back(ctx, y.data(), geo.ix.tile_y, n * 4));
        for (size_t c = 0; c < cx.size(); ++c)
            for (size_t i = cf[c]; i < cf[c + 1] && i < n; ++i) tile_xy[2 * i] = cx[c], tile_xy[2 * i + 1] = y[i];
    }
    if (way_off) HIP_TRY(copy_back(ctx, way_off, geo.ix.way_off, (n + 1) * 4));
    if (ways && last[0]) HIP_TRY(copy_back(ctx, ways, geo.ix.ways, (size_t)last[0] * 4));
    if (mp_off) HIP_TRY(copy_back(ctx, mp_off, geo.ix.mp_off, (n + 1) * 4));
    if (mps && last[1]) HIP_TRY(copy_back(ctx, mps, geo.ix.mps, (size_t)last[1] * 4));
    if (node_off) {
        if (d_noff)
            HIP_TRY(copy_back(ctx, node_off, d_noff, (n + 1) * 4));
        else
            memset(node_off, 0, (n + 1) * 4);
    }
    if (nodes && last[2]) HIP_TRY(copy_back(ctx, nodes, d_nodes, (size_t)last[2] * 4));
    return OSMT_OK;
}

}  // namespace

namespace osmt_host {

void tq_bind_levels(const geodata_host& geo, bool nodes, const osmt_tq_index_dev& z18, osmt_tq_pass& P) {
    const pyramid_host* p = geo.pyramid.get();
    P.ix = z18;
    P.ixz = !p ? nullptr : nodes ? p->node_table : p->area_table; /* a pyramid without node lists: the z18 node index */
}

void tq_stats_set(osmt_ctx* ctx, uint64_t items, uint64_t ways, uint64_t mps, uint64_t nodes) {
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->tq_stats[0] = items, ctx->tq_stats[1] = ways, ctx->tq_stats[2] = mps, ctx->tq_stats[3] = nodes;
}

}  // namespace osmt_host

int osmt_validate_tile_pyramid(uint32_t geodata_id, uint32_t level_mask, osmt_ctx* ctx) {
    return guarded([&] { return validate_pyramid(geodata_id, level_mask, ctx); });
}

int osmt_register_tile_pyramid(osmt_ctx* ctx, uint32_t geodata_id, uint32_t level_mask) {
    return guarded([&] { return register_pyramid_body(ctx, geodata_id, level_mask); });
}

int osmt_tile_pyramid_levels(osmt_ctx* ctx, uint32_t geodata_id, uint32_t* out_mask, uint32_t* out_node_mask) {
    return guarded([&] {
        if (!out_mask || !out_node_mask) return fail(OSMT_INVALID_ARG, "NULL argument");
        std::shared_ptr<const pyramid_host> p;
        const int rc = pyramid_of(ctx, geodata_id, &p);
        if (rc != OSMT_OK) return rc;
        *out_mask = p ? p->mask : 0u;
        *out_node_mask = p ? p->node_mask : 0u;
        return (int)OSMT_OK;
    });
}

int osmt_read_tile_pyramid(osmt_ctx* ctx, uint32_t geodata_id, uint32_t level, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways, uint32_t* mp_off,
                           uint32_t* mps, uint32_t* node_off, uint32_t* nodes, const size_t caps[4], size_t counts[4]) {
    return guarded([&] { return read_pyramid_body(ctx, geodata_id, level, tile_xy, way_off, ways, mp_off, mps, node_off, nodes, caps, counts); });
}

int osmt_validate_tile_index_build(uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes, osmt_ctx* ctx) {
    return guarded([&] { return validate_index_build(geodata_id, node_ids, n_nodes, ctx); });
}

int osmt_build_tile_index(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes) {
    return guarded([&] { return build_index_body(ctx, geodata_id, node_ids, n_nodes); });
}

int osmt_read_tile_index(osmt_ctx* ctx, uint32_t geodata_id, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways, uint32_t* mp_off, uint32_t* mps,
                         uint32_t* node_off, uint32_t* nodes, const size_t caps[4], size_t counts[4]) {
    return guarded([&] { return read_index_body(ctx, geodata_id, tile_xy, way_off, ways, mp_off, mps, node_off, nodes, caps, counts); });
}

int osmt_tile_query_stats(osmt_ctx* ctx, uint64_t stats[4]) {
    return guarded([&] {
        if (!ctx || !stats) return fail(OSMT_INVALID_ARG, "NULL argument");
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        for (int i = 0; i < 4; ++i) stats[i] = ctx->tq_stats[i];
        return (int)OSMT_OK;
    });
}
