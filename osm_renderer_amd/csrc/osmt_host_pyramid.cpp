/*
 * osmt_host_pyramid.cpp — host side of libosmtile.so: the tile index pyramid (include/osmtile.h, osmt_tilepyramid.hip).
 * Registration builds the levels on the device, finest first, each from the one before; the tile queries of the other host
 * files ask tq_bind_levels which index a tile of each zoom reads.  Shares osmt_host.h with the other host files.
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
};

const char* const KIND[4] = {"tile", "way", "multipolygon", "node"};

/* emits the pairs of `src` (tiles: its tile keys), sorts them, numbers the distinct ones; reads the totals back */
int run_job(call_work& wg, int slot, const osmt_pyr_src& src, bool tiles, uint32_t level, const char* kind, job& j) {
    hipStream_t st = wg.st;
    const size_t n = tiles ? src.n_tiles : src.n_refs, n_wg = (n + OSMT_PYR_SORT_BLOCK - 1) / OSMT_PYR_SORT_BLOCK;
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
    HIP_TRY(tiles ? osmt_launch_pyr_tilekeys(src, j.key[0], j.id[0], st) : osmt_launch_pyr_pairs(src, j.key[0], j.id[0], st));
    /* the digits that differ among the pairs: a digit whose histogram has one non-empty bin is not sorted on */
    std::vector<uint32_t> hist(OSMT_PYR_DIGITS * 256);
    if (n > 1) {
        HIP_TRY(osmt_launch_pyr_digits(j.key[0], j.id[0], j.n, j.hist, st));
        HIP_TRY(hipMemcpyAsync(hist.data(), j.hist, hist.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t d = 0; d < OSMT_PYR_DIGITS; ++d) {
            bool one_bin = false;
            for (uint32_t b = 0; b < 256; ++b) one_bin = one_bin || hist[d * 256 + b] == n;
            if (one_bin) continue;
            HIP_TRY(osmt_launch_pyr_pass(j.key[j.at], j.id[j.at], j.n, d, j.counts, j.blk, j.tot, j.key[j.at ^ 1], j.id[j.at ^ 1], st));
            j.at ^= 1;
        }
    }
    HIP_TRY(osmt_launch_pyr_mark(j.key[j.at], j.id[j.at], j.n, j.pos, j.cpos, j.blk, j.tot, st));
    unsigned long long tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, j.tot, tiles ? 16 : 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    j.distinct = tot[0], j.cols = tot[1];
    if (j.distinct >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "tile pyramid: level %u has %llu %s references (> 2^32)", level, (unsigned long long)j.distinct, kind);
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
    for (int k = 0; k < n_kinds; ++k) {
        const osmt_pyr_src src = source_of(from, k, shift);
        const uint64_t pairs = k ? src.n_refs : src.n_tiles; /* both below 2^32 - 1: checked when the source was made */
        if (pairs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "tile pyramid: level %u sorts %llu %s pairs (> 2^32)", level, (unsigned long long)pairs, KIND[k]);
        rc = run_job(wg, k, src, k == 0, level, KIND[k], jobs[k]);
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

int osmt_tile_query_stats(osmt_ctx* ctx, uint64_t stats[4]) {
    return guarded([&] {
        if (!ctx || !stats) return fail(OSMT_INVALID_ARG, "NULL argument");
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        for (int i = 0; i < 4; ++i) stats[i] = ctx->tq_stats[i];
        return (int)OSMT_OK;
    });
}
