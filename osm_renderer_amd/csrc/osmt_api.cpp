/*
 * osmt_api.cpp — host side of libosmtile.so: contexts, HBM-resident scenes, the C ABI
 * of include/osmtile.h.  No CPU rendering path exists here on purpose: every entry point
 * either runs the HIP kernels or fails with an error code.
 */
#include "osmt_host.h"

using namespace osmt_host;

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace osmt_host {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace osmt_host

/* error reporting for the other translation units of the library */
int osmt_fail_public(int code, const char* msg) { return fail(code, "%s", msg); }

namespace {

constexpr double OSMT_MAX_ABS_LAT = 85.06; /* Web-Mercator limit 85.0511..., with a little slack */
/* Idle buffers beyond this are returned to the driver, least recently used first.  hipFree waits for the device: a process
 * that has rendered a few big batches (a 10 000-tile call leaves 5 GB idle) and then runs pipelined jobs must not free —
 * and malloc again — a buffer on every call (round 4: 8 GB, oldest ALLOCATION first: the PNG begin / end leg of bench.py ran
 * at 3.6 ms per batch behind the other legs and at 2.1 ms on its own).  288 GB of HBM: 32 GB, OSMT_CACHE_GB overrides. */
size_t cache_keep_bytes() {
    static const size_t v = [] {
        const char* e = getenv("OSMT_CACHE_GB");
        const long gb = e ? atol(e) : 32;
        return (size_t)std::min<long>(std::max<long>(gb, 0), 256) << 30;
    }();
    return v;
}

}  // namespace

namespace osmt_host {

/* OSMT_POISON_ALLOC=1 (tests/conftest.py, tools/fuzz_parity.py): every device buffer handed out — fresh from the driver or
 * recycled from the cache — is filled with 0xA5 first, and every pinned staging buffer too.  The reference resets every
 * pixel and every pending entry per tile (tile_pixels.rs:89-105); this library recycles its buffers un-zeroed, so whatever a
 * kernel reads it must have been written by this render.  A fresh process sees zero pages from hipMalloc and hides a missing
 * write (round 4's empty-tile list headers); under poison it reads 0xA5A5A5A5 and fails at once. */
bool poison_alloc() {
    static const bool v = [] {
        const char* e = getenv("OSMT_POISON_ALLOC");
        return e && *e && *e != '0';
    }();
    return v;
}

}  // namespace osmt_host

namespace {

hipError_t dev_poison(osmt_ctx* ctx, void* p, size_t bytes) {
    /* The fill is a kernel: on a pooled stream it can share a hardware queue with a caller's long queue of renders and wait
     * for all of them (tests/test_gpu_fullsize_and_errors.py::test_worker_threads_..., once in four runs).  A stream of the
     * highest priority has a queue of its own and its workgroups are dispatched first. */
    hipStream_t st = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        if (!ctx->poison_stream) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi); /* hi = the numerically lowest = greatest priority */
            if (hipStreamCreateWithPriority(&ctx->poison_stream, hipStreamNonBlocking, hi) != hipSuccess) {
                (void)hipGetLastError();
                ctx->poison_stream = nullptr;
            }
        }
        st = ctx->poison_stream;
    }
    const bool pooled = st == nullptr;
    hipError_t e = pooled ? stream_acquire(ctx, &st) : hipSuccess;
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p, 0xA5, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (pooled) stream_release(ctx, st);
    return e;
}

hipError_t dev_alloc_raw(osmt_ctx* ctx, void** out, size_t bytes, size_t* got);

}  // namespace

namespace osmt_host {

hipError_t dev_alloc(osmt_ctx* ctx, void** out, size_t bytes) {
    size_t got = 0;
    hipError_t e = dev_alloc_raw(ctx, out, bytes, &got);
    if (e == hipSuccess && poison_alloc()) e = dev_poison(ctx, *out, got);
    return e;
}

}  // namespace osmt_host

namespace {

hipError_t dev_alloc_raw(osmt_ctx* ctx, void** out, size_t bytes, size_t* got) {
    bytes = align_up(bytes ? bytes : 1, (size_t)2 << 20);
    {
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        osmt_ctx::cached_buf* best = nullptr;
        for (auto& c : ctx->cache)
            if (!c.used && c.bytes >= bytes && c.bytes <= 2 * bytes && (!best || c.bytes < best->bytes)) best = &c;
        if (best) {
            best->used = true;
            best->tick = ++ctx->cache_tick;
            *out = best->p;
            *got = best->bytes;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory) { /* give the idle buffers back and retry once */
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        for (size_t i = 0; i < ctx->cache.size();) {
            if (!ctx->cache[i].used) {
                (void)hipFree(ctx->cache[i].p);
                ctx->cache.erase(ctx->cache.begin() + (long)i);
            } else {
                ++i;
            }
        }
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->cache.push_back({*out, bytes, true, ++ctx->cache_tick});
    *got = bytes;
    return hipSuccess;
}

}  // namespace

namespace osmt_host {

hipError_t stream_acquire(osmt_ctx* ctx, hipStream_t* out) {
    {
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        if (!ctx->idle_streams.empty()) {
            *out = ctx->idle_streams.back();
            ctx->idle_streams.pop_back();
            return hipSuccess;
        }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void stream_release(osmt_ctx* ctx, hipStream_t st) {
    if (!st) return;
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->idle_streams.push_back(st);
}

}  // namespace osmt_host

namespace {

constexpr size_t STAGE_MAX_BYTES = (size_t)4 << 20; /* calls with more input than this copy array by array */
constexpr uint32_t ERR_SLOTS = 1024;

uint32_t* err_slot_acquire(osmt_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    if (!ctx->err_page) {
        void* p = nullptr;
        if (hipHostMalloc(&p, ERR_SLOTS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        memset(p, 0, ERR_SLOTS * sizeof(uint32_t));
        ctx->err_page = (uint32_t*)p;
        ctx->err_free.reserve(ERR_SLOTS);
        for (uint32_t i = ERR_SLOTS; i-- > 0;) ctx->err_free.push_back((uint16_t)i);
    }
    if (ctx->err_free.empty()) return nullptr;
    uint32_t* w = ctx->err_page + ctx->err_free.back();
    ctx->err_free.pop_back();
    *w = 0u;
    return w;
}

void err_slot_release(osmt_ctx* ctx, uint32_t* w) {
    if (!w) return;
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->err_free.push_back((uint16_t)(w - ctx->err_page));
}

}  // namespace

namespace osmt_host {

void* stage_acquire(osmt_ctx* ctx, size_t bytes) {
    bytes = align_up(bytes ? bytes : 1, (size_t)64 << 10);
    {
        /* best fit, and never a buffer more than four times the request: first fit handed the megabyte-sized output
         * staging of a gathered group to the next 20 KB upload, and the next group then had to hipHostMalloc (hundreds of
         * microseconds) a new one — every time */
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        osmt_ctx::cached_buf* best = nullptr;
        for (auto& c : ctx->host_cache)
            if (!c.used && c.bytes >= bytes && c.bytes <= 4 * bytes && (!best || c.bytes < best->bytes)) best = &c;
        if (best) {
            best->used = true;
            if (poison_alloc()) memset(best->p, 0xA5, best->bytes);
            return best->p;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr; /* the caller falls back to per-array copies */
    }
    if (poison_alloc()) memset(p, 0xA5, bytes);
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->host_cache.push_back({p, bytes, true, 0});
    return p;
}

void stage_release(osmt_ctx* ctx, void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    for (auto& c : ctx->host_cache)
        if (c.p == p) c.used = false;
}

void dev_free(osmt_ctx* ctx, void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    size_t idle = 0;
    for (auto& c : ctx->cache) {
        if (c.p == p) c.used = false;
        if (!c.used) idle += c.bytes;
    }
    while (idle > cache_keep_bytes()) {
        size_t lru = ctx->cache.size();
        for (size_t i = 0; i < ctx->cache.size(); ++i)
            if (!ctx->cache[i].used && (lru == ctx->cache.size() || ctx->cache[i].tick < ctx->cache[lru].tick)) lru = i;
        if (lru == ctx->cache.size()) break;
        idle -= ctx->cache[lru].bytes;
        (void)hipFree(ctx->cache[lru].p);
        ctx->cache.erase(ctx->cache.begin() + (long)lru);
    }
}

bool trace_upload() {
    static const bool v = getenv("OSMT_TRACE_UPLOAD") != nullptr;
    return v;
}

}  // namespace osmt_host

namespace {

/* ---- the device copy of a registry that only grows ----
 * A registration followed by a use makes NEW device arrays; the old ones move to osmt_ctx::image_graveyard and live until the
 * context goes, so a kernel launched by another thread with the previous snapshot never reads freed memory.  All of the new
 * arrays are allocated and filled, or none is and the context is as it was.  Called with ctx->mu held. */
struct snap_part {
    void** slot;      /* the context's pointer: replaced */
    const void* src;
    size_t bytes;     /* copied */
    size_t min_bytes; /* allocated at least; 0 with bytes == 0: no allocation, the slot becomes NULL */
};
int snapshot_replace(osmt_ctx* ctx, const char* name, const snap_part* parts, int n) {
    constexpr int MAX_PARTS = 4;
    void* fresh[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};
    if (n > MAX_PARTS) return fail(OSMT_HIP_ERROR, "internal error: the %s has %d arrays (at most %d)", name, n, MAX_PARTS);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        const size_t b = std::max(parts[i].bytes, parts[i].min_bytes);
        if (b) e = hipMalloc(&fresh[i], b);
        if (e != hipSuccess) fresh[i] = nullptr;
    }
    for (int i = 0; i < n && e == hipSuccess; ++i)
        if (parts[i].bytes) e = hipMemcpy(fresh[i], parts[i].src, parts[i].bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (int i = 0; i < n; ++i)
            if (fresh[i]) (void)hipFree(fresh[i]);
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "%s upload failed: %s", name, hipGetErrorString(e));
    }
    for (int i = 0; i < n; ++i) {
        if (*parts[i].slot) ctx->image_graveyard.push_back(*parts[i].slot);
        *parts[i].slot = fresh[i];
    }
    return OSMT_OK;
}

struct image_snapshot {
    const osmt_image_desc* desc = nullptr;
    const double4* pool = nullptr;
    uint32_t n = 0;
};

/* Brings the device copy of the icon registry up to date and returns a consistent (descriptors, pool, count) triple
 * that stays valid for the life of the context. */
int sync_images(osmt_ctx* ctx, image_snapshot* snap) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->images_dirty) {
        /* an empty registry has no device arrays at all */
        const snap_part parts[2] = {{(void**)&ctx->d_images, ctx->images.data(), ctx->images.size() * sizeof(osmt_image_desc), 0},
                                    {(void**)&ctx->d_image_pool, ctx->image_pool_host.data(), ctx->image_pool_host.size() * sizeof(double), 0}};
        const int rc = snapshot_replace(ctx, "icon registry", parts, 2);
        if (rc != OSMT_OK) return rc;
        ctx->d_n_images = (uint32_t)ctx->images.size();
        ctx->images_dirty = false;
    }
    if (snap) {
        snap->desc = ctx->d_images;
        snap->pool = ctx->d_image_pool;
        snap->n = ctx->d_n_images;
    }
    return OSMT_OK;
}

struct glyph_snapshot {
    const osmt_glyph_vertex* verts = nullptr;
    const uint32_t* voff = nullptr;
    uint32_t n = 0;
};

/* Brings the device copy of the glyph table up to date; the snapshot stays valid for the life of the context. */
int sync_glyphs(osmt_ctx* ctx, glyph_snapshot* snap) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->glyphs_dirty) {
        const snap_part parts[2] = {
            {(void**)&ctx->d_glyph_voff, ctx->glyph_voff.data(), ctx->glyph_voff.size() * sizeof(uint32_t), 0}, /* never empty: voff[0] = 0 */
            {(void**)&ctx->d_glyph_verts, ctx->glyph_verts.data(), ctx->glyph_verts.size() * sizeof(osmt_glyph_vertex), sizeof(osmt_glyph_vertex)}};
        const int rc = snapshot_replace(ctx, "glyph table", parts, 2);
        if (rc != OSMT_OK) return rc;
        ctx->d_n_glyphs = (uint32_t)(ctx->glyph_voff.size() - 1);
        ctx->glyphs_dirty = false;
    }
    if (snap) {
        snap->verts = ctx->d_glyph_verts;
        snap->voff = ctx->d_glyph_voff;
        snap->n = ctx->d_n_glyphs;
    }
    return OSMT_OK;
}

struct font_snapshot {
    const osmt_font_dev* fonts = nullptr;
    uint32_t n = 0;
};

/* Brings the device copy of the font table up to date: the tables of fonts not yet uploaded, then a new array of records
 * if one was added.  The snapshot stays valid for the life of the context. */
int sync_fonts(osmt_ctx* ctx, font_snapshot* snap) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->fonts_dirty) {
        for (auto& fp : ctx->fonts) {
            osmt_ctx::font_host& f = *fp;
            if (f.d_pool) continue;
            const size_t b_cmap = f.cmap.size() * sizeof(osmt_cmap_entry), b_adv = f.advance.size() * 4, b_out = f.outline.size() * 4;
            const size_t b_kern = f.kern.size() * sizeof(osmt_kern_pair);
            pool_layout pl;
            const size_t o_cmap = pl.add(b_cmap), o_adv = pl.add(b_adv), o_out = pl.add(b_out), o_kern = pl.add(b_kern);
            table_upload up("font table", pl);
            char* pool = up.pool;
            up.put(o_cmap, f.cmap.data(), b_cmap);
            up.put(o_adv, f.advance.data(), b_adv);
            up.put(o_out, f.outline.data(), b_out);
            up.put(o_kern, f.kern.data(), b_kern);
            if (up.done() != OSMT_OK) return up.done();
            up.release();
            f.d_pool = pool;
            f.dev.cmap = (const osmt_cmap_entry*)(pool + o_cmap);
            f.dev.advance = (const int32_t*)(pool + o_adv);
            f.dev.outline = (const uint32_t*)(pool + o_out);
            f.dev.kern = b_kern ? (const osmt_kern_pair*)(pool + o_kern) : nullptr;
            f.dev.n_cmap = (uint32_t)f.cmap.size();
            f.dev.n_kern = (uint32_t)f.kern.size();
            f.dev.n_glyphs = (uint32_t)f.advance.size();
        }
        std::vector<osmt_font_dev> recs;
        for (const auto& fp : ctx->fonts) recs.push_back(fp->dev);
        /* as for every registry: an allocation the device has no memory for is OSMT_OOM, a failed copy OSMT_HIP_ERROR */
        const snap_part part = {(void**)&ctx->d_fonts, recs.data(), recs.size() * sizeof(osmt_font_dev), sizeof(osmt_font_dev)};
        const int rc = snapshot_replace(ctx, "font table", &part, 1);
        if (rc != OSMT_OK) return rc;
        ctx->d_n_fonts = (uint32_t)recs.size();
        ctx->fonts_dirty = false;
    }
    if (snap) {
        snap->fonts = ctx->d_fonts;
        snap->n = ctx->d_n_fonts;
    }
    return OSMT_OK;
}

void ctx_teardown(osmt_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    comm_destroy(ctx);
    if (ctx->d_images) (void)hipFree(ctx->d_images);
    if (ctx->d_image_pool) (void)hipFree(ctx->d_image_pool);
    if (ctx->d_glyph_verts) (void)hipFree(ctx->d_glyph_verts);
    if (ctx->d_glyph_voff) (void)hipFree(ctx->d_glyph_voff);
    if (ctx->d_fonts) (void)hipFree(ctx->d_fonts);
    for (auto& f : ctx->fonts)
        if (f->d_pool) (void)hipFree(f->d_pool);
    for (auto& g : ctx->geodata)
    {
        if (g.d_pool) (void)hipFree(g.d_pool);
        if (g.d_index && !g.index_built) (void)hipFree(g.d_index); /* a built index is one of ctx->cache's buffers */
        if (g.d_node_index && !g.node_index_built) (void)hipFree(g.d_node_index);
        if (g.d_factors) (void)hipFree((void*)g.d_factors);
        if (g.d_tags) (void)hipFree(g.d_tags);
    }
    for (auto& b : ctx->rules)
        if (b.d_pool) (void)hipFree(b.d_pool);
    for (auto& b : ctx->selectors)
        if (b.d_pool) (void)hipFree(b.d_pool);
    for (auto& b : ctx->bindings)
        if (b.d_pool) (void)hipFree(b.d_pool);
    for (auto& b : ctx->label_bindings)
        if (b.d_pool) (void)hipFree(b.d_pool);
    for (auto& b : ctx->area_label_bindings)
        if (b.d_pool) (void)hipFree(b.d_pool);
    for (auto& b : ctx->id_filters)
        if (b.d_pool) (void)hipFree(b.d_pool);
    if (ctx->d_label_styles) (void)hipFree(ctx->d_label_styles);
    if (ctx->d_label_rank) (void)hipFree(ctx->d_label_rank);
    if (ctx->d_styles) (void)hipFree(ctx->d_styles);
    if (ctx->d_style_rank) (void)hipFree(ctx->d_style_rank);
    if (ctx->d_style_dashes) (void)hipFree(ctx->d_style_dashes);
    for (void* p : ctx->image_graveyard) (void)hipFree(p);
    for (auto& c : ctx->cache) (void)hipFree(c.p);
    for (hipStream_t st : ctx->idle_streams) (void)hipStreamDestroy(st);
    if (ctx->poison_stream) (void)hipStreamDestroy(ctx->poison_stream);
    for (auto& c : ctx->host_cache) (void)hipHostFree(c.p);
    if (ctx->err_page) (void)hipHostFree(ctx->err_page);
    delete ctx;
}

}  // namespace

namespace osmt_host {

void ctx_release(osmt_ctx* ctx) {
    if (ctx->refs.fetch_sub(1) == 1) ctx_teardown(ctx);
}

}  // namespace osmt_host

namespace {

/* The wait at the end of a small request: the work behind it is ~100 us of kernels, and a thread that sleeps in the driver
 * until the completion interrupt wakes it adds a noticeable share of that on top.  Poll the stream for a bounded time
 * first (a request of the per-tile server loop is latency, not throughput), then fall back to the blocking wait.
 * OSMT_SPIN_SYNC=0 turns the polling off. */
hipError_t stream_sync_small(hipStream_t st) {
    static const bool spin = [] {
        const char* v = getenv("OSMT_SPIN_SYNC");
        return !(v && v[0] == '0');
    }();
    /* (Several groups in flight = several threads polling, and hipStreamQuery takes the runtime's lock every time: with six
     * groups in flight a two-tile group takes 520 us instead of 200.  Waiting on a word of pinned memory that the stream
     * writes behind the copy — hipStreamWriteValue32 — removes that contention (6 in flight: 20 k -> 42 k tiles/s) but the
     * write itself is slow: 2 in flight 33 k against 45 k.  Two groups in flight and the query it is.) */
    if (spin) {
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(400);
        for (;;) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) return q;
            if (std::chrono::steady_clock::now() >= t_end) break;
        }
        (void)hipGetLastError(); /* hipErrorNotReady is sticky in hipGetLastError */
    }
    return hipStreamSynchronize(st);
}

}  // namespace

namespace osmt_host {

/* Device -> host copy of finished data on a private pooled stream: a NULL-stream hipMemcpy would order itself against
 * every blocking stream of the process. */
hipError_t copy_back(osmt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    hipStream_t st = nullptr;
    hipError_t e = stream_acquire(ctx, &st);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    stream_release(ctx, st);
    return e;
}

}  // namespace osmt_host

namespace {

/* Host-buffer entry points: an internal error of the label coverage kernels (window overflow) must not return OSMT_OK
 * with wrong pixels.  Called after the call's work was enqueued on `st`; synchronises it. */
/* set by prepass_error_check when the overflow it reports belongs to a scene with guessed arenas: the caller renders again
 * with exact sizing instead of failing */
thread_local bool g_arena_guess_missed = false;

/* the pre-pass kernels' word: valid once the stream(s) the scene was rendered on have been synchronised */
int prepass_error_check(osmt_scene* sc) {
    if (!sc->h_err) return OSMT_OK;
    const uint32_t code = *(volatile uint32_t*)sc->h_err;
    if (!code) return OSMT_OK;
    *(volatile uint32_t*)sc->h_err = 0u;
    if (sc->arena_guess) {
        g_arena_guess_missed = true;
        std::lock_guard<std::mutex> lk(sc->ctx->cache_mu);
        sc->ctx->density[sc->scale].uploads = 0; /* the next big upload measures again */
    }
    return fail(OSMT_HIP_ERROR, "pre-pass arena overflow (internal error %u: %s arena)", code,
                code == OSMT_PREPASS_ERR_FILL_ARENA ? "fill" : code == OSMT_PREPASS_ERR_STROKE_ARENA ? "stroke" : "list");
}

int label_error_check(osmt_scene* sc, hipStream_t st) {
    {
        const int rc = prepass_error_check(sc); /* every caller has synchronised the scene's stream(s) by now */
        if (rc != OSMT_OK) return rc;
    }
    if (!sc->n_labels) return OSMT_OK;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, sc->d_lab_err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err) return fail(OSMT_HIP_ERROR, "label coverage window overflow (internal error %u)", err);
    return OSMT_OK;
}

/* The scene object itself (device buffers are returned by the caller first). */
void scene_delete(osmt_scene* s) {
    for (auto& u : s->last_use) (void)hipEventDestroy(u.second);
    osmt_ctx* ctx = s->ctx;
    if (ctx) err_slot_release(ctx, s->h_err);
    delete s;
    if (ctx) ctx_release(ctx);
}

/* Records "the scene was last read here" behind the launches just issued on `st` (public scenes only). */
hipError_t scene_mark_use(osmt_scene* sc, hipStream_t st) {
    if (sc->own_stream) return hipSuccess; /* per-call scenes live and die on their own stream */
    std::lock_guard<std::mutex> lk(sc->use_mu);
    for (auto& u : sc->last_use)
        if (u.first == st) return hipEventRecord(u.second, st);
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    sc->last_use.emplace_back(st, ev);
    return hipEventRecord(ev, st);
}

/* Blocks the calling thread until every launch that reads or writes the scene has finished — and nothing else. */
hipError_t scene_wait_idle(osmt_scene* sc) {
    if (sc->own_stream) return hipStreamSynchronize(sc->own_stream);
    std::lock_guard<std::mutex> lk(sc->use_mu);
    hipError_t first = hipSuccess;
    for (auto& u : sc->last_use) {
        const hipError_t e = hipEventSynchronize(u.second);
        if (e != hipSuccess && first == hipSuccess) first = e;
    }
    return first;
}

/* the coordinate scan of validate_batch: independent of everything else, O(n_pts) — big uploads run it on a helper thread
 * beside the host-table building and the copies (validate_coords_range is what the thread calls on its slice) */
int validate_coords_range(const osmt_batch* b, size_t lo, size_t hi) {
    if (b->coord_kind == OSMT_COORD_POINT_I32) {
        for (size_t i = 2 * lo; i < 2 * hi; ++i)
            if (b->points[i] > OSMT_COORD_LIMIT || b->points[i] < -OSMT_COORD_LIMIT)
                return fail(OSMT_UNSUPPORTED, "point %zu: |coordinate| > 2^28", i / 2);
    } else {
        /* The closed forms and the Bresenham state of the kernels need |pixel coordinate| <= 2^28 (osmt_geom.h); with
         * zoom <= 18 and scale <= 4 that holds for every (lat, lon) of the Web-Mercator square (|lat| <= 85.0511...).  The
         * band up to OSMT_MAX_ABS_LAT admitted here lies 19 187 px outside it at zoom 18: up to scale 3 still within 2^28
         * under every tile, at scale 4 up to 2^28 + 76 748 under a tile of the opposite edge.  Further out
         * (or for a NaN / infinity) Point::from_node saturates (point.rs:11-19) and the integer walks would overflow. */
        const double* ll = b->coord_kind == OSMT_COORD_NODE_REF ? b->nodes : b->latlon;
        for (size_t i = lo; i < hi; ++i) {
            const double lat = ll[2 * i], lon = ll[2 * i + 1];
            if (!(std::fabs(lat) <= OSMT_MAX_ABS_LAT) || !(std::fabs(lon) <= 180.0))
                return fail(OSMT_UNSUPPORTED, "point %zu: (lat, lon) = (%g, %g) outside the Web-Mercator square (|lat| <= %g, |lon| <= 180)", i, lat,
                            lon, OSMT_MAX_ABS_LAT);
        }
    }
    return OSMT_OK;
}
size_t coord_count(const osmt_batch* b) { return b->coord_kind == OSMT_COORD_NODE_REF ? b->n_nodes : b->n_pts; }

}  // namespace

namespace osmt_host {

/* ---- what Rust's types guarantee has to be checked at a C boundary, in three pieces so that callers can validate in
 * parallel (osmt_render_batch_multi: one thread per GPU; osmt_worker_render: every requester its own request) ----------
 * validate_batch_global: what needs the whole batch — the header, and that the jobs' op ranges PARTITION the op pool
 * (every op of the pool is pre-processed on the device, k_opinfo runs over [0, n_ops): every op must be reachable through
 * exactly one job) and their point ranges do not overlap (a point is projected against the tile of the job that owns it)
 * — in O(n_jobs log n_jobs): two sorts of the ranges.  validate_job: everything about ONE job — its ops, rings, dashes,
 * node references and (with_coords) the coordinates of its points; jobs are independent, any number of threads may run
 * it on disjoint sets of jobs.  validate_nodes: a slice of the shared node table of OSMT_COORD_NODE_REF.  Points no job
 * owns are not looked at: no kernel reads them either (k_project skips them). */
int validate_batch_global(const osmt_batch* b) {
    if (!b) return fail(OSMT_INVALID_ARG, "batch is NULL");
    if (b->scale < 1 || b->scale > OSMT_MAX_SCALE) return fail(OSMT_INVALID_ARG, "scale %u not in 1..%u", b->scale, OSMT_MAX_SCALE);
    if (b->coord_kind != OSMT_COORD_LATLON_F64 && b->coord_kind != OSMT_COORD_POINT_I32 && b->coord_kind != OSMT_COORD_NODE_REF)
        return fail(OSMT_INVALID_ARG, "unknown coord_kind %u", b->coord_kind);
    if (b->n_jobs >= 0x7FFFFFFFull / 64 || b->n_ops >= 0xFFFFFFFFull || b->n_rings >= 0xFFFFFFFFull ||
        b->n_pts >= 0xFFFFFFFFull || b->n_dashes >= 0xFFFFFFFFull)
        return fail(OSMT_INVALID_ARG, "batch too large for 32-bit indices");
    if ((b->n_jobs && !b->jobs) || (b->n_ops && !b->ops) || (b->n_rings && !b->rings) || (b->n_dashes && !b->dashes))
        return fail(OSMT_INVALID_ARG, "NULL pool with non-zero count");
    if (b->n_pts) {
        if (b->coord_kind == OSMT_COORD_LATLON_F64 && !b->latlon) return fail(OSMT_INVALID_ARG, "latlon pool is NULL");
        if (b->coord_kind == OSMT_COORD_POINT_I32 && !b->points) return fail(OSMT_INVALID_ARG, "points pool is NULL");
        if (b->coord_kind == OSMT_COORD_NODE_REF) {
            if (!b->node_refs || !b->nodes) return fail(OSMT_INVALID_ARG, "node table / node_refs is NULL");
            if (b->n_nodes >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "node table too large for 32-bit indices");
        }
    }
    struct range {
        uint64_t lo, hi;
        uint32_t job;
    };
    std::vector<range> ops, pts;
    ops.reserve(b->n_jobs);
    pts.reserve(b->n_jobs);
    for (size_t j = 0; j < b->n_jobs; ++j) {
        const osmt_tile_job& job = b->jobs[j];
        if (job.zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "job %zu: zoom %u > MAX_ZOOM (src/tile.rs:5)", j, job.zoom);
        if ((size_t)job.op_off + job.n_ops > b->n_ops) return fail(OSMT_INVALID_ARG, "job %zu: op range out of bounds", j);
        if ((size_t)job.pt_off + job.n_pts > b->n_pts) return fail(OSMT_INVALID_ARG, "job %zu: point range out of bounds", j);
        if (job.n_ops) ops.push_back({job.op_off, (uint64_t)job.op_off + job.n_ops, (uint32_t)j});
        if (job.n_pts) pts.push_back({job.pt_off, (uint64_t)job.pt_off + job.n_pts, (uint32_t)j});
    }
    auto by_lo = [](const range& x, const range& y) { return x.lo < y.lo; };
    std::sort(ops.begin(), ops.end(), by_lo);
    uint64_t next = 0;
    for (const range& r : ops) {
        if (r.lo < next)
            return fail(OSMT_INVALID_ARG, "job %u: op %llu also belongs to another job (op ranges must not overlap)", r.job, (unsigned long long)r.lo);
        if (r.lo > next)
            return fail(OSMT_INVALID_ARG, "op %llu is not covered by any job (the jobs' op ranges must partition the op pool)", (unsigned long long)next);
        next = r.hi;
    }
    if (next != b->n_ops)
        return fail(OSMT_INVALID_ARG, "op %llu is not covered by any job (the jobs' op ranges must partition the op pool)", (unsigned long long)next);
    std::sort(pts.begin(), pts.end(), by_lo);
    for (size_t i = 1; i < pts.size(); ++i)
        if (pts[i].lo < pts[i - 1].hi) return fail(OSMT_INVALID_ARG, "the point ranges of two jobs overlap at point %llu", (unsigned long long)pts[i].lo);
    return OSMT_OK;
}

int validate_job(const osmt_batch* b, size_t j, bool with_coords) {
    const osmt_tile_job& job = b->jobs[j];
    for (uint32_t k = 0; k < job.n_ops; ++k) {
        const osmt_op& op = b->ops[job.op_off + k];
        if (op.kind > OSMT_OP_STROKE) return fail(OSMT_INVALID_ARG, "job %zu op %u: unknown kind %u", j, k, op.kind);
        if (op.kind == OSMT_OP_NONE) continue;
        if ((size_t)op.ring_off + op.n_rings > b->n_rings) return fail(OSMT_INVALID_ARG, "job %zu op %u: ring range out of bounds", j, k);
        for (uint32_t r = 0; r < op.n_rings; ++r) {
            const osmt_ring& ring = b->rings[op.ring_off + r];
            if (ring.first_pt < job.pt_off || (size_t)ring.first_pt + ring.n_pts > (size_t)job.pt_off + job.n_pts)
                return fail(OSMT_INVALID_ARG, "job %zu op %u ring %u: points outside the job's pool range", j, k, r);
        }
        if (!(op.opacity >= 0.0) || !(op.opacity <= 4503599627370496.0))
            return fail(OSMT_INVALID_ARG, "job %zu op %u: opacity must be in [0, 2^52]", j, k);
        if (op.kind == OSMT_OP_STROKE) {
            if (!std::isfinite(op.width)) return fail(OSMT_INVALID_ARG, "job %zu op %u: width not finite", j, k);
            if (std::fabs(op.width) > 65536.0) return fail(OSMT_UNSUPPORTED, "job %zu op %u: |width| > 65536 px", j, k);
            if (op.cap > OSMT_CAP_SQUARE) return fail(OSMT_INVALID_ARG, "job %zu op %u: unknown cap", j, k);
            if (op.has_dashes) {
                if (op.n_dashes == 0) return fail(OSMT_INVALID_ARG, "job %zu op %u: empty dash list", j, k);
                if (op.n_dashes > OSMT_MAX_DASHES) return fail(OSMT_UNSUPPORTED, "job %zu op %u: more than %u dashes", j, k, OSMT_MAX_DASHES);
                if ((size_t)op.dashes_off + op.n_dashes > b->n_dashes) return fail(OSMT_INVALID_ARG, "job %zu op %u: dash range out of bounds", j, k);
            }
        }
    }
    if (b->coord_kind == OSMT_COORD_NODE_REF) {
        for (size_t i = job.pt_off; i < (size_t)job.pt_off + job.n_pts; ++i)
            if (b->node_refs[i] >= b->n_nodes) return fail(OSMT_INVALID_ARG, "point %zu: node reference %u out of range", i, b->node_refs[i]);
        return OSMT_OK; /* the node table itself: validate_nodes */
    }
    return with_coords ? validate_coords_range(b, job.pt_off, (size_t)job.pt_off + job.n_pts) : OSMT_OK;
}

int validate_nodes(const osmt_batch* b, size_t lo, size_t hi) {
    return b->coord_kind == OSMT_COORD_NODE_REF ? validate_coords_range(b, lo, hi) : OSMT_OK;
}

/* the whole batch on the calling thread; with_coords = false: the caller scans the coordinates itself (big uploads do it
 * on helper threads, validate_coords_range over the whole pool) */
int validate_batch(const osmt_batch* b, bool with_coords) {
    int rc = validate_batch_global(b);
    for (size_t j = 0; rc == OSMT_OK && j < b->n_jobs; ++j) rc = validate_job(b, j, with_coords);
    if (rc == OSMT_OK && with_coords) rc = validate_nodes(b, 0, b->n_nodes);
    return rc;
}

}  // namespace osmt_host

namespace {

/* Arguments of stage 2 (k_opinfo -> k_fill_rows -> k_stroke_bin); sizing: only the arena cursors are produced. */
osmt_prepass_args prepass_args(const osmt_scene* sc, bool sizing) {
    osmt_prepass_args a;
    memset(&a, 0, sizeof a);
    a.jobs = sc->d_jobs;
    a.n_jobs = sc->n_jobs;
    a.ops = sc->d_ops;
    a.n_ops = sc->n_ops;
    a.rings = sc->d_rings;
    a.pts = reinterpret_cast<const int2*>(sc->d_pts);
    a.dashes = sc->d_dashes;
    a.op_aux = sc->d_op_aux;
    a.op_job = sc->d_op_job;
    a.op_blk = sc->d_op_blk;
    a.op_vseg = sc->d_op_vseg;
    a.vseg = sc->d_vseg;
    a.n_vsegs = sc->n_vsegs;
    a.max_job_ops = sc->max_job_ops;
    a.fold_max_ops = sc->n_jobs <= OSMT_FOLD_MAX_JOBS ? OSMT_FOLD_MAX_OPS : 0u;
    a.scale = sc->scale;
    a.sub_rows = OSMT_TILE_SIZE * sc->scale / OSMT_SUB_H;
    a.info = sc->d_info;
    a.aux = sc->d_aux;
    a.dseg = sc->d_dseg;
    a.blk = sc->d_blk;
    a.submask = sc->d_submask;
    a.cursors = sc->d_cursors;
    a.cnt = sc->d_cnt;
    a.hdr = sc->d_hdr;
    a.ent = sc->d_ent;
    a.ent_cap = sizing ? 0ull : sc->ent_cap;
    a.fmask = sc->d_fmask;
    a.srec = sc->d_srec;
    a.skey = sc->d_skey;
    a.fmask_cap = sizing ? 0ull : sc->fmask_cap;
    a.srec_cap = sizing ? 0ull : sc->srec_cap;
    a.slots = sc->d_slots;
    a.slot_cap = sizing ? 0ull : sc->slot_cap;
    a.n_fill_pass = sc->n_fill_pass;
    a.err = sizing ? nullptr : sc->h_err; /* hipHostMallocMapped memory: one address on both sides (unified addressing) */
    return a;
}

/* stages: 1 = project, 2 = per-op pre-pass, 4 = raster (with the label kernels first when the scene has labels),
 * 8 = label kernels only (cover + resolve), 16 = with 4: the label kernels already ran for this scene.
 * [first_job, first_job + n_range) = tiles the raster stage renders into d_out (n_range 0: all). */
int render_impl(osmt_ctx* ctx, osmt_scene* sc, uint32_t stages, void* d_out, size_t stride, bool f64, void* stream,
                uint32_t first_job = 0, uint32_t n_range = 0) {
    if (!ctx || !sc || sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "bad ctx/scene");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t W = OSMT_TILE_SIZE * sc->scale;
    if ((stages & 4u) && !d_out) return fail(OSMT_INVALID_ARG, "output pointer is NULL");
    const bool rgb8 = (stages & 32u) != 0u; /* stage bit 32 (internal): k_raster writes packed RGB8 */
    if ((stages & 4u) && !f64 && !rgb8 && stride < (size_t)W * W * 4) return fail(OSMT_INVALID_ARG, "out_tile_stride_bytes < W*H*4");
    if ((stages & 4u) && rgb8 && (f64 || stride < (size_t)W * W * 3 || (stride & 3u) || ((uintptr_t)d_out & 3u)))
        return fail(OSMT_INVALID_ARG, "RGB8 output: tile stride below W*H*3 or not a multiple of 4");
    bool zeroed = false;
    if ((stages & 1u) && sc->coord_kind != OSMT_COORD_POINT_I32) {
        /* when the pre-pass follows in this call, the projection kernel clears its cursors and list counts on the way */
        const osmt_prepass_args pa = prepass_args(sc, false);
        zeroed = (stages & 2u) != 0u && sc->n_pts != 0u;
        HIP_TRY(osmt_launch_project(sc->d_jobs, sc->d_pt_job, sc->d_latlon, sc->coord_kind == OSMT_COORD_NODE_REF ? sc->d_node_refs : nullptr,
                                    sc->n_pts, (double)sc->scale, sc->d_pts, st, zeroed ? reinterpret_cast<uint32_t*>(pa.cursors) : nullptr,
                                    zeroed ? osmt_prepass_zero_words(pa) : 0));
    }
    if (stages & 2u) HIP_TRY(osmt_launch_prepass(prepass_args(sc, false), st, zeroed));
    const bool want_labels = sc->n_labels && !f64;
    if (want_labels && ((stages & 8u) || ((stages & 4u) && !(stages & 16u)))) {
        /* the label pass does not read the area canvas: coverage + collisions first, then
         * k_raster blends the survivors right before to_rgb_triples */
        int rc = sync_images(ctx, nullptr);
        if (rc != OSMT_OK) return rc;
        osmt_label_launch ll;
        memset(&ll, 0, sizeof ll);
        ll.info = sc->d_lab;
        ll.n_labels = sc->n_labels;
        ll.n_jobs = sc->n_jobs;
        ll.scale = sc->scale;
        ll.n_wide = sc->n_lab_wide;
        ll.bands = sc->d_lab_bands;
        ll.n_bands = sc->n_lab_bands;
        ll.job_label_off = sc->d_job_label_off;
        ll.segs = sc->d_lab_segs;
        ll.wide = sc->d_lab_wide;
        ll.plane_a = sc->d_lab_a;
        ll.cell_bits = sc->d_lab_bits;
        ll.plane_s_wide = sc->d_lab_s_wide;
        ll.bitmap = sc->d_lab_bitmap;
        ll.ok = sc->d_lab_ok;
        ll.err = sc->d_lab_err;
        ll.tile_labels = sc->d_tile_labels;
        ll.tile_label_cnt = sc->d_tile_label_cnt;
        HIP_TRY(osmt_launch_labels(ll, st));
        sc->lab_cover_valid = true;
    }
    if (stages & 4u) {
        image_snapshot img;
        int rc = sync_images(ctx, &img);
        if (rc != OSMT_OK) return rc;
        if (first_job > sc->n_jobs || n_range > sc->n_jobs - first_job) return fail(OSMT_INVALID_ARG, "tile range out of bounds");
        const uint32_t n_render = n_range ? n_range : sc->n_jobs - first_job;
        osmt_raster_args a;
        memset(&a, 0, sizeof a);
        a.jobs = sc->d_jobs + first_job;
        a.n_jobs = n_render;
        a.scale = sc->scale;
        a.aux = sc->d_aux;
        a.dseg = sc->d_dseg;
        {
            const uint32_t Wt = OSMT_TILE_SIZE * sc->scale;
            a.hdr = sc->d_hdr + (size_t)first_job * (Wt / OSMT_SUB_W) * (Wt / OSMT_SUB_H);
        }
        a.ent = sc->d_ent;
        a.fmask = sc->d_fmask;
        a.srec = sc->d_srec;
        a.skey = sc->d_skey;
        a.info = sc->d_info;
        a.submask = sc->d_submask;
        a.fold_max_ops = sc->n_jobs <= OSMT_FOLD_MAX_JOBS ? OSMT_FOLD_MAX_OPS : 0u; /* the same rule as the pre-pass (prepass_args) */
        a.images = img.desc;
        a.image_pool = img.pool;
        a.n_images = img.n;
        a.out = d_out;
        a.out_tile_stride = stride;
        a.out_rgb8 = rgb8 ? 1u : 0u;
        if (want_labels) {
            a.labels.info = sc->d_lab;
            a.labels.n_labels = sc->n_labels;
            a.labels.job_label_off = sc->d_job_label_off + first_job; /* values stay absolute label indices */
            a.labels.tile_labels = sc->d_tile_labels;
            a.labels.tile_label_cnt = sc->d_tile_label_cnt + first_job;
            a.labels.plane = sc->d_lab_a;
        }
        HIP_TRY(osmt_launch_raster(a, f64, st));
    }
    HIP_TRY(scene_mark_use(sc, st));
    return OSMT_OK;
}

}  // namespace

uint32_t osmt_version(void) { return (1u << 16) | 1u; }

const char* osmt_last_error(void) { return g_last_error.c_str(); }

static int osmt_create_body(const osmt_config* cfg, osmt_ctx** out_ctx) {
    if (!out_ctx) return fail(OSMT_INVALID_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(OSMT_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    const int dev = cfg ? cfg->device : 0;
    if (dev < 0 || dev >= n) return fail(OSMT_INVALID_ARG, "device %d out of range (0..%d)", dev, n - 1);
    HIP_TRY(hipSetDevice(dev));
    osmt_ctx* c = new (std::nothrow) osmt_ctx();
    if (!c) return fail(OSMT_OOM, "out of host memory");
    c->device = dev;
    *out_ctx = c;
    return OSMT_OK;
}

int osmt_create(const osmt_config* cfg, osmt_ctx** out_ctx) {
    return guarded([&] { return osmt_create_body(cfg, out_ctx); });
}

void osmt_destroy(osmt_ctx* ctx) {
    if (!ctx) return;
    ctx_release(ctx); /* scenes still alive keep the context (and the device buffers they use) until they are freed */
}

static int osmt_register_image_body(osmt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t* out_id) {
    if (!ctx || !rgba8 || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (width == 0 || height == 0) return fail(OSMT_INVALID_ARG, "empty image");
    std::lock_guard<std::mutex> lk(ctx->mu);
    osmt_image_desc d;
    d.offset = ctx->image_pool_host.size() / 4;
    d.width = width;
    d.height = height;
    const size_t n = (size_t)width * height;
    ctx->image_pool_host.reserve(ctx->image_pool_host.size() + 4 * n);
    for (size_t i = 0; i < n; ++i) {
        /* RgbaColor::from_components (tile_pixels.rs:21-23): from_color(Color{r,g,b}, a/255) */
        const double a = (double)rgba8[4 * i + 3] / 255.0;
        ctx->image_pool_host.push_back(a * ((double)rgba8[4 * i + 0] / 255.0));
        ctx->image_pool_host.push_back(a * ((double)rgba8[4 * i + 1] / 255.0));
        ctx->image_pool_host.push_back(a * ((double)rgba8[4 * i + 2] / 255.0));
        ctx->image_pool_host.push_back(a);
    }
    *out_id = (uint32_t)ctx->images.size();
    ctx->images.push_back(d);
    ctx->images_dirty = true;
    return OSMT_OK;
}

int osmt_register_image(osmt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t* out_id) {
    return guarded([&] { return osmt_register_image_body(ctx, rgba8, width, height, out_id); });
}

static int osmt_register_glyphs_body(osmt_ctx* ctx, const osmt_glyph_vertex* v, const uint32_t* voff, uint32_t n, uint32_t* out_first) {
    if (!ctx || !voff || !out_first) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (voff[0] != 0) return fail(OSMT_INVALID_ARG, "vertex_off[0] must be 0");
    for (uint32_t i = 0; i < n; ++i)
        if (voff[i] > voff[i + 1]) return fail(OSMT_INVALID_ARG, "vertex_off is not monotonic at glyph %u", i);
    const uint32_t nv = voff[n];
    if (nv && !v) return fail(OSMT_INVALID_ARG, "NULL vertex pool");
    for (uint32_t k = 0; k < nv; ++k)
        if (v[k].type < OSMT_GLYPH_MOVE_TO || v[k].type > OSMT_GLYPH_CURVE_TO)
            return fail(OSMT_INVALID_ARG, "glyph vertex %u: type %u is not MoveTo / LineTo / CurveTo", k, (unsigned)v[k].type);
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t base = ctx->glyph_verts.size();
    if (base + nv >= 0xFFFFFFFFull || ctx->glyph_voff.size() + n >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "glyph table too large");
    *out_first = (uint32_t)(ctx->glyph_voff.size() - 1);
    ctx->glyph_verts.insert(ctx->glyph_verts.end(), v, v + nv);
    for (uint32_t i = 1; i <= n; ++i) ctx->glyph_voff.push_back((uint32_t)(base + voff[i]));
    ctx->glyphs_dirty = true;
    return OSMT_OK;
}

int osmt_register_glyphs(osmt_ctx* ctx, const osmt_glyph_vertex* v, const uint32_t* vertex_off, uint32_t n_glyphs, uint32_t* out_first_id) {
    return guarded([&] { return osmt_register_glyphs_body(ctx, v, vertex_off, n_glyphs, out_first_id); });
}

static int osmt_register_font_body(osmt_ctx* ctx, const osmt_font_desc* font, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::string why;
    const int rc = osmt::validate_font(font, ctx->glyph_voff.size() - 1, &why); /* the glyph table is append-only: an id once valid stays valid */
    if (rc != OSMT_OK) return fail(rc, "%s", why.c_str());
    if (ctx->fonts.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "font table too large");
    auto f = std::make_shared<osmt_ctx::font_host>();
    f->cmap.assign(font->cmap, font->cmap + font->n_cmap);
    f->advance.assign(font->advance, font->advance + font->n_glyphs);
    f->outline.assign(font->outline_id, font->outline_id + font->n_glyphs);
    if (font->n_kern) f->kern.assign(font->kern, font->kern + font->n_kern);
    f->view = *font;
    f->view.cmap = f->cmap.data();
    f->view.advance = f->advance.data();
    f->view.outline_id = f->outline.data();
    f->view.kern = f->kern.empty() ? nullptr : f->kern.data();
    *out_id = (uint32_t)ctx->fonts.size();
    ctx->fonts.push_back(std::move(f));
    ctx->fonts_dirty = true;
    return OSMT_OK;
}

int osmt_register_font(osmt_ctx* ctx, const osmt_font_desc* font, uint32_t* out_font_id) {
    return guarded([&] { return osmt_register_font_body(ctx, font, out_font_id); });
}

/* The fonts registered so far, as osmt::validate_string_labels takes them; `keep` holds them alive (a font is never
 * removed, but the vector may grow under another thread). */
static std::vector<const osmt_font_desc*> font_views(osmt_ctx* ctx, std::vector<std::shared_ptr<osmt_ctx::font_host>>* keep) {
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        *keep = ctx->fonts;
    }
    std::vector<const osmt_font_desc*> v;
    for (const auto& f : *keep) v.push_back(&f->view);
    return v;
}

/* The pre-pass writes into two arenas whose sizes depend on the PROJECTED geometry (how many sub-tiles every op
 * reaches).  Small scenes take the worst case — every fill covers the whole tile, every stroke segment reaches every
 * sub-tile — without asking the device (a single-tile request must not pay a round trip); larger ones run the
 * projection and the sizing half of k_opinfo once, read the two totals back and allocate exactly.  Either way the
 * reservation logic of k_opinfo is the same code at render time, so the arenas cannot overflow. */
static int scene_size_arenas(osmt_ctx* ctx, osmt_scene* s, size_t n_fills, bool allow_guess) {
    const size_t W = (size_t)OSMT_TILE_SIZE * s->scale;
    const size_t nsub = (W / OSMT_SUB_W) * (W / OSMT_SUB_H);
    unsigned long long groups = (unsigned long long)n_fills * nsub, recs = (unsigned long long)s->n_vsegs * nsub;
    /* (the list arena at the size its layout gives it: twice the entries for batches whose arena is cut into slices, osmt_list_slices.h) */
    const unsigned long long worst_bytes = groups * 64ull + recs * (sizeof(osmt_srec) + 8ull) +
                                           osmt_list_layout_make(s->n_jobs, ((unsigned long long)n_fills + s->n_strokes) * nsub).total * sizeof(osmt_ent);
    /* (taking the worst case up to 2 GB instead — 1.8 GB for 1024 config-2 tiles — was tried to save this sizing run,
     * 0.14 ms of a 0.84 ms upload: no gain on one thread, and four worker threads' arenas then outgrow the buffer cache) */
    bool guessed = false;
    /* a guess needs the scene's error word: without one (more than ERR_SLOTS live scenes, or no pinned page) an overflow
     * could not be seen and the call would return OSMT_OK with geometry missing — such a scene is sized exactly */
    if (worst_bytes > ((unsigned long long)32 << 20) && allow_guess && s->h_err != nullptr) {
        /* A host-buffer call that follows others of its kind: the arenas from the densities the recent exact runs measured,
         * a quarter on top.  The kernels reserve with the same code as ever; if the guess is too small for this batch they
         * draw nothing for the ops that do not fit and say so in the scene's error word, and the call renders again with
         * exact sizing (g_arena_guess_missed).  Every 64th upload measures again, so the densities follow the workload. */
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        osmt_ctx::arena_density& d = ctx->density[s->scale];
        if (d.uploads != 0 && (d.uploads & 63u) != 0 && d.groups_per_fill > 0.0 && d.recs_per_vseg > 0.0) {
            const unsigned long long g = (unsigned long long)(d.groups_per_fill * 1.25 * (double)n_fills) + 4096ull;
            const unsigned long long r = (unsigned long long)(d.recs_per_vseg * 1.25 * (double)s->n_vsegs) + 4096ull;
            groups = std::min(groups, g);
            recs = std::min(recs, r);
            guessed = true;
            ++d.uploads;
        }
    }
    s->arena_guess = guessed;
    if (worst_bytes > ((unsigned long long)32 << 20) && !guessed) {
        hipStream_t st = s->own_stream;
        if (s->coord_kind != OSMT_COORD_POINT_I32)
            HIP_TRY(osmt_launch_project(s->d_jobs, s->d_pt_job, s->d_latlon, s->coord_kind == OSMT_COORD_NODE_REF ? s->d_node_refs : nullptr,
                                        s->n_pts, (double)s->scale, s->d_pts, st));
        HIP_TRY(osmt_launch_prepass(prepass_args(s, true), st));
        unsigned long long totals[4] = {0ull, 0ull, 0ull, 0ull}; /* [3]: fill slots, whole passes */
        HIP_TRY(hipMemcpyAsync(totals, s->d_cursors, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        groups = totals[0];
        recs = totals[1];
        /* (at least one block: 0 stands for "not counted") */
        s->n_fill_pass = (uint32_t)std::max<unsigned long long>(std::min<unsigned long long>(totals[3] / OSMT_FILL_PASS_SLOTS, 0x7FFFFFFFull), 1ull);
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        osmt_ctx::arena_density& d = ctx->density[s->scale];
        if (n_fills) d.groups_per_fill = std::max(d.groups_per_fill * 0.98, (double)groups / (double)n_fills);
        if (s->n_vsegs) d.recs_per_vseg = std::max(d.recs_per_vseg * 0.98, (double)recs / (double)s->n_vsegs);
        if (d.groups_per_fill <= 0.0) d.groups_per_fill = 1e-9; /* a workload without fills (or strokes) still counts as measured */
        if (d.recs_per_vseg <= 0.0) d.recs_per_vseg = 1e-9;
        ++d.uploads;
    }
    /* A list entry carries a fill's position in the fill arena as a 32-bit WORD index (osmt_ent::arena = group * 16, built by
     * k_sublist and the fold path of k_raster): it holds 2^28 groups = 16 GiB of coverage words, no more.  Such a scene is
     * refused here, before anything is allocated — a 64-bit position would widen osmt_ent and k_raster's register budget. */
    if (groups >= OSMT_MAX_FILL_GROUPS)
        return fail(OSMT_UNSUPPORTED, "scene needs %llu fill groups (>= 2^28 = %llu, the most a list entry's 32-bit word index reaches): split the batch",
                    groups, (unsigned long long)OSMT_MAX_FILL_GROUPS);
    if (groups >= 0xFFFFFFFFull || recs >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "scene needs %llu fill groups / %llu stroke records (> 2^32): split the batch", groups, recs);
    pool_layout pl;
    /* list entries: one per (op, sub-tile the op draws into) — at most one per fill group / stroke slot, and never more
     * than every op in every sub-tile */
    unsigned long long ents = std::min<unsigned long long>(groups + recs, ((unsigned long long)n_fills + s->n_strokes) * nsub);
    if (ents >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "scene needs %llu list entries (> 2^32): split the batch", ents);
    const size_t o_f = pl.add((size_t)(groups + 1) * 64);
    const size_t o_r = pl.add((size_t)(recs + 1) * sizeof(osmt_srec));
    const size_t o_k = pl.add((size_t)(recs + 1) * 8);
    /* batches of many tiles: the arena in slices with a cursor each and an overflow slice behind them (osmt_list_slices.h) */
    const osmt_list_layout lay = osmt_list_layout_make(s->n_jobs, ents + 1);
    const size_t o_e = pl.add((size_t)lay.total * sizeof(osmt_ent));
    /* one descriptor per (fill op, sub-tile row of its window) and the rounding of every k_opinfo workgroup */
    const unsigned long long slot_cap = osmt_fill_slot_capacity(groups, n_fills, (uint32_t)(W / OSMT_SUB_H), s->n_ops);
    const size_t o_q = pl.add((size_t)slot_cap * sizeof(osmt_fill_slot));
    hipError_t e = dev_alloc(ctx, (void**)&s->d_arena, pl.size() + 256);
    if (e != hipSuccess) {
        s->d_arena = nullptr;
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) for the pre-pass arenas failed: %s", pl.size(), hipGetErrorString(e));
    }
    s->d_fmask = (uint32_t*)(s->d_arena + o_f);
    s->d_srec = (osmt_srec*)(s->d_arena + o_r);
    s->d_skey = (uint2*)(s->d_arena + o_k);
    s->d_ent = (osmt_ent*)(s->d_arena + o_e);
    s->ent_cap = ents + 1;
    s->d_slots = (osmt_fill_slot*)(s->d_arena + o_q);
    s->slot_cap = slot_cap;
    /* OSMT_TRACE_UPLOAD=1 (diagnostic): what the arenas take, one line on stderr */
    static const bool trace_arenas = getenv("OSMT_TRACE_UPLOAD") != nullptr;
    if (trace_arenas)
        fprintf(stderr, "osmt arenas: %u tiles, fill groups %llu, stroke records %llu, list entries %llu in %u slice(s) of %llu (+ overflow): "
                        "list arena %.1f MB of %.1f MB%s\n", s->n_jobs, groups, recs, ents + 1, lay.n_slices, lay.slice_cap,
                (double)lay.total * sizeof(osmt_ent) / 1e6, (double)pl.size() / 1e6, guessed ? " (guessed)" : "");
    s->fmask_cap = groups + 1; /* never 0: 0 means "sizing pass" to the kernels */
    s->srec_cap = recs + 1;
    return OSMT_OK;
}

/* The back half of a scene's memory, behind the arrays the caller (osmt_scene_upload) or the build kernels
 * (osmt_scene_build_styled) fill: the work areas of the pre-pass per op, per stroke slot, per 64-edge block, per virtual
 * segment and per sub-tile.  Both paths carve them with this function, right behind their front arrays, and then size the
 * arenas with scene_size_arenas. */
struct scene_back {
    size_t o_info, o_aux, o_dseg, o_submask, o_blk, o_vseg, o_cursors, o_hdr;
};
static scene_back scene_carve_back(pool_layout& pl, size_t n_jobs, size_t n_ops, size_t n_strokes, size_t n_blk, size_t n_vsegs, uint32_t scale) {
    scene_back k;
    k.o_info = pl.add(n_ops * sizeof(osmt_opinfo));
    /* per virtual segment (not per point: two stroke ops may share a ring, e.g. a casing and its stroke) */
    k.o_aux = pl.add((size_t)(n_strokes + 1) * sizeof(osmt_stroke_aux));
    k.o_dseg = pl.add((size_t)(n_strokes + 1) * OSMT_MAX_DASH_SEGS * sizeof(osmt_dash_seg)); /* touched by dashed ops only */
    const size_t sub_rows = (size_t)OSMT_TILE_SIZE * scale / OSMT_SUB_H;
    k.o_submask = pl.add(n_ops * sub_rows * 4);
    k.o_blk = pl.add((n_blk + 1) * sizeof(osmt_blk_bbox));
    k.o_vseg = pl.add((n_vsegs + 1) * sizeof(osmt_vseg));
    const size_t n_sub = ((size_t)OSMT_TILE_SIZE * scale / OSMT_SUB_W) * sub_rows;
    /* cursors + list counts + the cursors of the list arena's slices: zeroed together every frame */
    k.o_cursors = pl.add((osmt_list_cursor_word0(n_jobs * n_sub) + OSMT_LIST_CURSOR_WORDS) * 4);
    k.o_hdr = pl.add(n_jobs * n_sub * sizeof(uint2));
    return k;
}
static void scene_point_back(osmt_scene* s, char* rbase, const scene_back& k) {
    s->d_info = (osmt_opinfo*)(rbase + k.o_info);
    s->d_aux = (osmt_stroke_aux*)(rbase + k.o_aux);
    s->d_dseg = (osmt_dash_seg*)(rbase + k.o_dseg);
    s->d_submask = (uint32_t*)(rbase + k.o_submask);
    s->d_blk = (osmt_blk_bbox*)(rbase + k.o_blk);
    s->d_vseg = (osmt_vseg*)(rbase + k.o_vseg);
    s->d_cursors = (unsigned long long*)(rbase + k.o_cursors);
    s->d_cnt = (uint32_t*)(rbase + k.o_cursors + 32);
    s->d_hdr = (uint2*)(rbase + k.o_hdr);
}

/* st == nullptr: blocking copies (the public osmt_scene_upload); otherwise stream-ordered on `st`, the caller
 * synchronises the stream before the batch's host arrays go away */
/* trusted: the batch was built by the library itself from a batch it has already validated (the shards of osmt_render_batch_multi) */
static int scene_upload_impl(osmt_ctx* ctx, const osmt_batch* b, osmt_scene** out_scene, hipStream_t st, bool trusted = false,
                             bool allow_guess = false) {
    if (!ctx || !out_scene) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_scene = nullptr;
    /* Big uploads: the O(n_pts) coordinate scan runs on helper threads while this one builds the index tables and feeds
     * the copies (they do not depend on it); the verdict is collected before the first kernel can be launched. */
    const bool big = b && coord_count(b) >= ((size_t)1 << 16);
    /* Where the host's own arrays go inside the scene's memory: known from the batch's sizes alone */
    pool_layout pl;
    const bool ll = b && b->coord_kind == OSMT_COORD_LATLON_F64;
    const bool nr = b && b->coord_kind == OSMT_COORD_NODE_REF;
    size_t o_jobs = 0, o_ops = 0, o_rings = 0, o_latlon = 0, o_refs = 0, o_pts = 0, o_dashes = 0, o_ptjob = 0, o_opaux = 0, o_opblk = 0, o_opvseg = 0,
           o_opjob = 0, front_bytes = 0;
    if (b) {
        o_jobs = pl.add(b->n_jobs * sizeof(osmt_tile_job));
        o_ops = pl.add(b->n_ops * sizeof(osmt_op));
        o_rings = pl.add(b->n_rings * sizeof(osmt_ring));
        /* an array the coordinate kind does not have takes no room: a one-tile request stays as small as it was */
        o_latlon = ll ? pl.add(b->n_pts * 16) : nr ? pl.add(b->n_nodes * 16) : pl.size();
        o_refs = nr ? pl.add(b->n_pts * 4) : pl.size();
        o_pts = pl.add(b->n_pts * 8);
        o_dashes = pl.add((b->n_dashes + 1) * 8);
        o_ptjob = pl.add(b->n_pts * 4);
        o_opaux = pl.add(b->n_ops * 4);
        o_opblk = pl.add(b->n_ops * 4);
        o_opvseg = pl.add(b->n_ops * 4);
        o_opjob = pl.add(b->n_ops * 4);
        front_bytes = pl.size(); /* everything the host provides sits in [0, front_bytes) */
    }
    /* SPLIT upload (round 5; big stream-ordered uploads): the caller's arrays — 27 MB for 1024 config-2 tiles, 0.44 ms of
     * pageable copies — go to an allocation of their own and are copied by a helper thread WHILE this thread validates the jobs
     * and builds the index tables (0.3 + 0.19 ms): the host half of a one-piece call was validation -> tables -> copies in a
     * row in front of the GPU half.  Nothing on the device looks at the data before the verdicts are in (the first launch comes
     * after the join below). */
    const bool split = big && st != nullptr && front_bytes > STAGE_MAX_BYTES;
    int rc = OSMT_OK;
    if (!trusted) rc = split ? validate_batch_global(b) : validate_batch(b, !big);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    struct coord_check {
        std::vector<std::thread> th;
        std::vector<int> rc;
        std::vector<std::string> msg;
        int join() { /* first failing slice wins: the message names the lowest point index */
            for (auto& t : th)
                if (t.joinable()) t.join();
            for (size_t i = 0; i < rc.size(); ++i)
                if (rc[i] != OSMT_OK) return fail(rc[i], "%s", msg[i].c_str());
            return OSMT_OK;
        }
        void wait() {
            for (auto& t : th)
                if (t.joinable()) t.join();
        }
        ~coord_check() { wait(); }
    } cc;
    const unsigned n_coord_thr = (big && !trusted) ? (coord_count(b) >= ((size_t)1 << 19) ? 2u : 1u) : 0u;
    cc.rc.assign(n_coord_thr + (split ? 2u : 0u), OSMT_OK); /* sized before any helper runs: they write their own slots */
    cc.msg.resize(n_coord_thr + (split ? 2u : 0u));
    if (big && !trusted) {
        const size_t n = coord_count(b);
        const unsigned n_thr = n_coord_thr;
        for (unsigned t = 0; t < n_thr; ++t) {
            const size_t lo = n * t / n_thr, hi = n * (t + 1) / n_thr;
            try {
                cc.th.emplace_back([&cc, b, t, lo, hi] {
                    cc.rc[t] = guarded([&] { return validate_coords_range(b, lo, hi); });
                    if (cc.rc[t] != OSMT_OK) cc.msg[t] = osmt_last_error();
                });
            } catch (...) { /* no thread to be had: scan here */
                cc.rc[t] = validate_coords_range(b, lo, hi);
                if (cc.rc[t] != OSMT_OK) cc.msg[t] = osmt_last_error();
            }
        }
    }

    char* d_front = nullptr;
    /* Owns d_front until the scene's free path does: whatever way this function is left before that — a refused batch,
     * a failed allocation, an exception out of the table building (bad_alloc, caught by guarded()) — the helpers are joined, THEIR
     * COPIES ON THE STREAM ARE WAITED FOR (joining a helper only means its hipMemcpyAsync calls were issued: up to tens of MB may
     * still be on their way out of the caller's arrays and into a buffer the cache would hand to the next upload at once) and the
     * buffer goes back to the cache.  Declared behind `cc`: destroyed before it. */
    struct front_guard {
        osmt_ctx* ctx;
        coord_check* cc;
        hipStream_t st;
        char* p = nullptr;
        ~front_guard() {
            if (!p) return;
            cc->wait();
            (void)hipStreamSynchronize(st);
            dev_free(ctx, p);
        }
    } fg{ctx, &cc, st ? st : nullptr};
    if (split) {
        hipError_t fe = dev_alloc(ctx, (void**)&d_front, front_bytes + 256);
        if (fe != hipSuccess) {
            cc.wait();
            return fail(fe == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) failed: %s", front_bytes, hipGetErrorString(fe));
        }
        fg.p = d_front;
        /* two helpers: the op side (jobs, ops, rings, dashes) and the coordinate side — 16 + 11 MB for 1024 config-2 tiles */
        auto copy_user_arrays = [&cc, ctx, b, st, d_front, ll, nr, o_jobs, o_ops, o_rings, o_latlon, o_refs, o_pts, o_dashes](unsigned slot, bool coords) {
            cc.rc[slot] = guarded([&] {
                HIP_TRY(hipSetDevice(ctx->device));
                auto put = [&](size_t o, const void* src, size_t bytes) -> hipError_t {
                    return bytes ? hipMemcpyAsync(d_front + o, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
                };
                if (!coords) {
                    HIP_TRY(put(o_jobs, b->jobs, b->n_jobs * sizeof(osmt_tile_job)));
                    HIP_TRY(put(o_ops, b->ops, b->n_ops * sizeof(osmt_op)));
                    HIP_TRY(put(o_rings, b->rings, b->n_rings * sizeof(osmt_ring)));
                    HIP_TRY(put(o_dashes, b->dashes, b->n_dashes * 8));
                } else {
                    if (ll) HIP_TRY(put(o_latlon, b->latlon, b->n_pts * 16));
                    if (nr) HIP_TRY(put(o_latlon, b->nodes, b->n_nodes * 16));
                    if (nr) HIP_TRY(put(o_refs, b->node_refs, b->n_pts * 4));
                    if (!ll && !nr) HIP_TRY(put(o_pts, b->points, b->n_pts * 8));
                }
                return (int)OSMT_OK;
            });
            if (cc.rc[slot] != OSMT_OK) cc.msg[slot] = osmt_last_error();
        };
        for (unsigned h = 0; h < 2u; ++h) {
            try {
                cc.th.emplace_back(copy_user_arrays, n_coord_thr + h, h == 1u);
            } catch (...) { /* no thread to be had: copy here */
                copy_user_arrays(n_coord_thr + h, h == 1u);
            }
        }
        if (!trusted) { /* the per-job half of validate_batch, beside the copies (coordinates: the helpers above) */
            for (size_t j = 0; rc == OSMT_OK && j < b->n_jobs; ++j) rc = validate_job(b, j, false);
            if (rc != OSMT_OK) {
                const std::string msg = osmt_last_error();
                return fail(rc, "%s", msg.c_str()); /* (front_guard: join, wait for the copies, free) */
            }
        }
    }

    /* OSMT_TRACE_UPLOAD=1 (diagnostic): where the host time of this call goes, one line on stderr */
    static const bool trace_upload = getenv("OSMT_TRACE_UPLOAD") != nullptr;
    using tclock = std::chrono::steady_clock;
    tclock::time_point tp[6];
    auto mark = [&](int i) {
        if (trace_upload) tp[i] = tclock::now();
    };
    auto report = [&] {
        if (!trace_upload) return;
        auto us = [&](int a, int b2) { return std::chrono::duration<double, std::micro>(tp[b2] - tp[a]).count(); };
        fprintf(stderr, "osmt upload: tables %.0f us, alloc %.0f us, copies %.0f us, coordinate check join %.0f us, arenas %.0f us\n",
                us(0, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5));
    };
    mark(0);
    osmt_scene* s = new (std::nothrow) osmt_scene();
    if (!s) return fail(OSMT_OOM, "out of host memory");
    s->own_stream = st;
    /* host-side index tables: point -> job (for projection), op -> stroke slot */
    std::vector<uint32_t>& pt_job = s->h_pt_job;
    std::vector<uint32_t>& op_aux = s->h_op_aux;
    std::vector<uint32_t>& op_blk = s->h_op_blk;
    std::vector<uint32_t>& op_vseg = s->h_op_vseg;
    const bool host_pt_job = !big; /* big uploads fill point -> job on the device (k_ptjob): no 4 B/point host loop and copy */
    if (host_pt_job) pt_job.assign(b->n_pts, 0xFFFFFFFFu);
    op_aux.assign(b->n_ops, 0u);
    op_blk.assign(b->n_ops, 0xFFFFFFFFu);
    op_vseg.assign(b->n_ops, 0u);
    /* op -> job; stroke slot -> op; first virtual segment (edges + the two cap stubs of Round/Square caps,
     * line.rs:33-57) of every stroke slot: k_stroke_bin runs one thread per virtual segment of the scene */
    std::vector<uint32_t>& op_job = s->h_op_job;
    op_job.assign(b->n_ops, 0u);
    uint32_t n_strokes = 0;
    size_t n_blk = 0; /* 64-edge blocks of the ops with more than 64 edges */
    size_t n_vsegs = 0, n_fills = 0;
    uint32_t max_job_ops = 0;
    for (size_t j = 0; j < b->n_jobs; ++j) {
        const osmt_tile_job& job = b->jobs[j];
        max_job_ops = std::max(max_job_ops, job.n_ops);
        if (host_pt_job)
            for (uint32_t i = 0; i < job.n_pts; ++i) pt_job[job.pt_off + i] = (uint32_t)j;
        for (uint32_t k = 0; k < job.n_ops; ++k) {
            const osmt_op& op = b->ops[job.op_off + k];
            op_job[job.op_off + k] = (uint32_t)j;
            if (op.kind == OSMT_OP_NONE) continue;
            size_t ne = 0;
            for (uint32_t r = 0; r < op.n_rings; ++r) {
                const uint32_t np = b->rings[op.ring_off + r].n_pts;
                if (np >= 2) ne += np - 1;
            }
            if (ne > 64 && n_blk + (ne + 63) / 64 < 0xFFFFFFFFull) {
                op_blk[job.op_off + k] = (uint32_t)n_blk;
                n_blk += (ne + 63) / 64;
            }
            if (op.kind == OSMT_OP_STROKE) {
                op_aux[job.op_off + k] = n_strokes++;
                const size_t nv = ne + ((op.cap == OSMT_CAP_ROUND || op.cap == OSMT_CAP_SQUARE) ? 2u : 0u);
                op_vseg[job.op_off + k] = (uint32_t)n_vsegs; /* k_opinfo writes the per-segment tables from here on */
                n_vsegs += nv;
            } else {
                ++n_fills;
            }
        }
    }
    if (n_vsegs >= 0xFFFFFFFFull) {
        delete s;
        return fail(OSMT_INVALID_ARG, "batch too large for 32-bit indices (stroke segments)");
    }

    s->ctx = ctx;
    ctx->refs.fetch_add(1);
    s->h_err = err_slot_acquire(ctx);
    s->n_jobs = (uint32_t)b->n_jobs;
    s->max_job_ops = max_job_ops;
    s->n_ops = (uint32_t)b->n_ops;
    s->n_rings = (uint32_t)b->n_rings;
    s->n_pts = (uint32_t)b->n_pts;
    s->n_dashes = (uint32_t)b->n_dashes;
    s->n_strokes = n_strokes;
    s->n_blk = (uint32_t)n_blk;
    s->n_vsegs = (uint32_t)n_vsegs;
    s->scale = b->scale;
    s->coord_kind = b->coord_kind;

    const scene_back bk = scene_carve_back(pl, b->n_jobs, b->n_ops, n_strokes, n_blk, n_vsegs, b->scale);
    s->bytes = pl.size() - (split ? front_bytes : 0) + 256;
    mark(1);
    hipError_t e = dev_alloc(ctx, (void**)&s->d_base, s->bytes);
    mark(2);
    if (e != hipSuccess) {
        scene_delete(s);
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) failed: %s", pl.size(),
                    hipGetErrorString(e));
    }
    /* front offsets live in d_front when the upload is split, everything behind them in d_base */
    char* const fbase = split ? d_front : s->d_base;
    char* const rbase = split ? s->d_base - front_bytes : s->d_base;
    s->d_jobs = (osmt_tile_job*)(fbase + o_jobs);
    s->d_ops = (osmt_op*)(fbase + o_ops);
    s->d_rings = (osmt_ring*)(fbase + o_rings);
    s->d_latlon = (double*)(fbase + o_latlon);
    s->d_node_refs = (uint32_t*)(fbase + o_refs);
    s->d_pts = (int32_t*)(fbase + o_pts);
    s->d_dashes = (double*)(fbase + o_dashes);
    s->d_pt_job = (uint32_t*)(fbase + o_ptjob);
    s->d_op_aux = (uint32_t*)(fbase + o_opaux);
    s->d_op_blk = (uint32_t*)(fbase + o_opblk);
    s->d_op_vseg = (uint32_t*)(fbase + o_opvseg);
    s->d_op_job = (uint32_t*)(fbase + o_opjob);
    scene_point_back(s, rbase, bk);

    auto up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (!bytes) return hipSuccess;
        return st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    hipError_t err = hipSuccess;
    char* stage = (st && front_bytes <= STAGE_MAX_BYTES) ? (char*)stage_acquire(ctx, front_bytes) : nullptr;
    if (stage) {
        /* small call: pack the arrays into pinned staging and move them with ONE copy (a dozen pageable copies cost
         * more host time than the kernels of a single tile) */
        auto put = [&](size_t o, const void* src, size_t bytes) {
            if (bytes) memcpy(stage + o, src, bytes);
        };
        put(o_jobs, b->jobs, b->n_jobs * sizeof(osmt_tile_job));
        put(o_ops, b->ops, b->n_ops * sizeof(osmt_op));
        put(o_rings, b->rings, b->n_rings * sizeof(osmt_ring));
        if (ll) put(o_latlon, b->latlon, b->n_pts * 16);
        if (nr) put(o_latlon, b->nodes, b->n_nodes * 16);
        if (nr) put(o_refs, b->node_refs, b->n_pts * 4);
        if (!ll && !nr) put(o_pts, b->points, b->n_pts * 8);
        put(o_dashes, b->dashes, b->n_dashes * 8);
        if (host_pt_job) put(o_ptjob, pt_job.data(), b->n_pts * 4);
        put(o_opaux, op_aux.data(), b->n_ops * 4);
        put(o_opblk, op_blk.data(), b->n_ops * 4);
        put(o_opvseg, op_vseg.data(), b->n_ops * 4);
        put(o_opjob, op_job.data(), b->n_ops * 4);
        s->h_stage = stage;
        err = hipMemcpyAsync(s->d_base, stage, front_bytes, hipMemcpyHostToDevice, st);
        if (err == hipSuccess && !host_pt_job) err = osmt_launch_ptjob(s->d_jobs, s->n_jobs, s->d_pt_job, s->n_pts, st);
        if (err != hipSuccess) {
            stage_release(ctx, stage);
            dev_free(ctx, s->d_base);
            scene_delete(s);
            return fail(OSMT_HIP_ERROR, "upload failed: %s", hipGetErrorString(err));
        }
        mark(3);
        rc = cc.join(); /* no kernel has seen the coordinates yet */
        mark(4);
        if (rc == OSMT_OK) rc = scene_size_arenas(ctx, s, n_fills, allow_guess);
        mark(5);
        report();
        if (rc != OSMT_OK) {
            osmt_scene_free(s);
            return rc;
        }
        *out_scene = s;
        return OSMT_OK;
    }
    if (!split) { /* (split: the helper thread is copying these) */
        if (err == hipSuccess) err = up(s->d_jobs, b->jobs, b->n_jobs * sizeof(osmt_tile_job));
        if (err == hipSuccess) err = up(s->d_ops, b->ops, b->n_ops * sizeof(osmt_op));
        if (err == hipSuccess) err = up(s->d_rings, b->rings, b->n_rings * sizeof(osmt_ring));
        if (err == hipSuccess && ll) err = up(s->d_latlon, b->latlon, b->n_pts * 16);
        if (err == hipSuccess && nr) err = up(s->d_latlon, b->nodes, b->n_nodes * 16);
        if (err == hipSuccess && nr) err = up(s->d_node_refs, b->node_refs, b->n_pts * 4);
        if (err == hipSuccess && !ll && !nr) err = up(s->d_pts, b->points, b->n_pts * 8);
        if (err == hipSuccess) err = up(s->d_dashes, b->dashes, b->n_dashes * 8);
    }
    if (err == hipSuccess && host_pt_job) err = up(s->d_pt_job, pt_job.data(), b->n_pts * 4);
    if (err == hipSuccess && !host_pt_job && !split) err = osmt_launch_ptjob(s->d_jobs, s->n_jobs, s->d_pt_job, s->n_pts, st ? st : nullptr);
    if (err == hipSuccess) err = up(s->d_op_aux, op_aux.data(), b->n_ops * 4);
    if (err == hipSuccess) err = up(s->d_op_blk, op_blk.data(), b->n_ops * 4);
    if (err == hipSuccess) err = up(s->d_op_vseg, op_vseg.data(), b->n_ops * 4);
    if (err == hipSuccess) err = up(s->d_op_job, op_job.data(), b->n_ops * 4);
    if (err != hipSuccess) {
        cc.wait();
        (void)hipStreamSynchronize(st ? st : nullptr); /* copies into d_base may be on their way too */
        dev_free(ctx, s->d_base);
        scene_delete(s);
        return fail(OSMT_HIP_ERROR, "upload failed: %s", hipGetErrorString(err));
    }
    /* from here on the scene owns the front buffer: every later exit goes through osmt_scene_free (which waits for the stream) */
    s->d_front = d_front;
    fg.p = nullptr;
    mark(3);
    rc = cc.join(); /* no kernel has seen the coordinates yet; the helper's copies are on the stream */
    if (rc == OSMT_OK && split && !host_pt_job) { /* the point -> job kernel reads the jobs the helper copied: behind the join */
        err = osmt_launch_ptjob(s->d_jobs, s->n_jobs, s->d_pt_job, s->n_pts, st);
        if (err != hipSuccess) rc = fail(OSMT_HIP_ERROR, "upload failed: %s", hipGetErrorString(err));
    }
    mark(4);
    if (rc == OSMT_OK) rc = scene_size_arenas(ctx, s, n_fills, allow_guess);
    mark(5);
    report();
    if (rc != OSMT_OK) {
        osmt_scene_free(s);
        return rc;
    }
    *out_scene = s;
    return OSMT_OK;
}

int osmt_validate_batch(const osmt_batch* b) {
    return guarded([&] { return validate_batch(b); });
}

/* Public scenes: the upload runs on a pooled private stream (never the NULL stream, whose copies order themselves
 * against other workers' streams) and is complete when the call returns; the scene is then free to be rendered on any
 * stream of the caller. */
static int osmt_scene_upload_body(osmt_ctx* ctx, const osmt_batch* b, osmt_scene** out_scene) {
    if (!ctx || !out_scene) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = nullptr;
    HIP_TRY(stream_acquire(ctx, &st));
    int rc = scene_upload_impl(ctx, b, out_scene, st);
    if (rc == OSMT_OK) {
        osmt_scene* s = *out_scene;
        const hipError_t e = hipStreamSynchronize(st);
        s->own_stream = nullptr; /* from here on a public scene: waits go through its last-use events */
        stage_release(ctx, s->h_stage);
        s->h_stage = nullptr;
        if (e != hipSuccess) {
            osmt_scene_free(s);
            *out_scene = nullptr;
            rc = fail(OSMT_HIP_ERROR, "upload failed: %s", hipGetErrorString(e));
        }
    }
    stream_release(ctx, st);
    return rc;
}

int osmt_scene_upload(osmt_ctx* ctx, const osmt_batch* b, osmt_scene** out_scene) {
    return guarded([&] { return osmt_scene_upload_body(ctx, b, out_scene); });
}

void osmt_scene_free(osmt_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    /* in-flight kernels may still read the scene and a cached buffer can be handed to the next upload at once:
     * wait for the scene's own stream (internal per-call scenes) or for the last launch on every stream the scene
     * was rendered on (public scenes) — not for the device: other workers' streams keep running */
    (void)scene_wait_idle(s);
    dev_free(s->ctx, s->d_base);
    dev_free(s->ctx, s->d_front);
    dev_free(s->ctx, s->d_arena);
    dev_free(s->ctx, s->d_lab_base);
    dev_free(s->ctx, s->d_text_inst);
    dev_free(s->ctx, s->d_text_glyphs);
    dev_free(s->ctx, s->d_tq);
    dev_free(s->ctx, s->d_tq_areas_buf);
    stage_release(s->ctx, s->h_stage);
    scene_delete(s);
}

/* ---- display lists built on the device (include/osmtile.h "display lists built on the GPU") --------------------------- */
namespace osmt_host {

/* offs: count + 1 entries from 0 to `total`, never decreasing */
int check_offsets_of(const char* who, const char* what, const uint32_t* offs, size_t count, size_t total) {
    if (offs[0] != 0u) return fail(OSMT_INVALID_ARG, "%s: %s[0] is %u, not 0", who, what, offs[0]);
    for (size_t i = 0; i < count; ++i)
        if (offs[i + 1] < offs[i])
            return fail(OSMT_INVALID_ARG, "%s: %s[%zu] = %u is less than the entry before it (%u)", who, what, i + 1, offs[i + 1], offs[i]);
    if ((size_t)offs[count] != total)
        return fail(OSMT_INVALID_ARG, "%s: %s[%zu] = %u does not end at the %zu entries it indexes", who, what, count, offs[count], total);
    return OSMT_OK;
}

}  // namespace osmt_host

namespace {

int validate_geodata(const osmt_geodata_desc* g) {
    if (!g) return fail(OSMT_INVALID_ARG, "geodata is NULL");
    if ((g->n_nodes && !g->nodes) || (g->n_ways && !g->way_ids) || !g->way_node_off || (g->n_way_nodes && !g->way_nodes) || !g->polygon_node_off ||
        (g->n_polygon_nodes && !g->polygon_nodes) || (g->n_multipolygons && !g->multipolygon_ids) || !g->multipolygon_polygon_off ||
        (g->n_multipolygon_polygons && !g->multipolygon_polygons))
        return fail(OSMT_INVALID_ARG, "geodata: NULL array (every offset array has at least its first entry)");
    if (g->n_nodes >= 0xFFFFFFFFull || g->n_ways >= 0x7FFFFFFFull || g->n_multipolygons >= 0x7FFFFFFFull || g->n_polygons >= 0xFFFFFFFFull ||
        g->n_multipolygon_polygons >= 0xFFFFFFFFull || (unsigned long long)g->n_way_nodes + g->n_polygon_nodes >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "geodata: too large for 32-bit indices (ways and multipolygons: 31 bits)");
    int rc = check_offsets_of("geodata", "way_node_off", g->way_node_off, g->n_ways, g->n_way_nodes);
    if (rc == OSMT_OK) rc = check_offsets_of("geodata", "polygon_node_off", g->polygon_node_off, g->n_polygons, g->n_polygon_nodes);
    if (rc == OSMT_OK) rc = check_offsets_of("geodata", "multipolygon_polygon_off", g->multipolygon_polygon_off, g->n_multipolygons, g->n_multipolygon_polygons);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < g->n_way_nodes; ++i)
        if (g->way_nodes[i] >= g->n_nodes) return fail(OSMT_INVALID_ARG, "geodata: way_nodes[%zu] = %u is not a node (%zu nodes)", i, g->way_nodes[i], g->n_nodes);
    for (size_t i = 0; i < g->n_polygon_nodes; ++i)
        if (g->polygon_nodes[i] >= g->n_nodes)
            return fail(OSMT_INVALID_ARG, "geodata: polygon_nodes[%zu] = %u is not a node (%zu nodes)", i, g->polygon_nodes[i], g->n_nodes);
    for (size_t i = 0; i < g->n_multipolygon_polygons; ++i)
        if (g->multipolygon_polygons[i] >= g->n_polygons)
            return fail(OSMT_INVALID_ARG, "geodata: multipolygon_polygons[%zu] = %u is not a polygon (%zu polygons)", i, g->multipolygon_polygons[i],
                        g->n_polygons);
    /* what validate_nodes refuses of the node table of an OSMT_COORD_NODE_REF batch */
    for (size_t i = 0; i < g->n_nodes; ++i) {
        const double lat = g->nodes[2 * i], lon = g->nodes[2 * i + 1];
        if (!(std::fabs(lat) <= OSMT_MAX_ABS_LAT) || !(std::fabs(lon) <= 180.0))
            return fail(OSMT_INVALID_ARG, "geodata: node %zu: (lat, lon) = (%g, %g) outside the Web-Mercator square (|lat| <= %g, |lon| <= 180)", i, lat, lon,
                        OSMT_MAX_ABS_LAT);
    }
    return OSMT_OK;
}

}  // namespace

namespace osmt_host {

int validate_styles(const osmt_style_rec* st, size_t n, const double* dashes, size_t n_dashes, size_t n_images) {
    if (n && !st) return fail(OSMT_INVALID_ARG, "styles is NULL");
    if (n_dashes && !dashes) return fail(OSMT_INVALID_ARG, "the styles' dash pool is NULL");
    for (size_t i = 0; i < n; ++i) {
        const osmt_style_rec& s = st[i];
        if (std::isnan(s.z_index)) return fail(OSMT_INVALID_ARG, "style %zu: z_index is NaN", i);
        auto opacity = [&](const char* what, uint8_t has, double v) {
            if (has && (!(v >= 0.0) || !(v <= 4503599627370496.0))) return fail(OSMT_INVALID_ARG, "style %zu: %s must be in [0, 2^52]", i, what);
            return (int)OSMT_OK;
        };
        auto width = [&](const char* what, uint8_t has, double v) {
            if (!has) return (int)OSMT_OK;
            if (!std::isfinite(v) || !std::isfinite(v * (double)OSMT_MAX_SCALE)) return fail(OSMT_INVALID_ARG, "style %zu: %s not finite", i, what);
            if (std::fabs(v * (double)OSMT_MAX_SCALE) > 65536.0) return fail(OSMT_UNSUPPORTED, "style %zu: |%s| * %u > 65536 px", i, what, OSMT_MAX_SCALE);
            return (int)OSMT_OK;
        };
        auto dash_list = [&](const char* what, uint8_t has, uint32_t off, uint32_t cnt) {
            if (!has) return (int)OSMT_OK;
            if (cnt == 0) return fail(OSMT_INVALID_ARG, "style %zu: empty %s list", i, what);
            if (cnt > OSMT_MAX_DASHES) return fail(OSMT_UNSUPPORTED, "style %zu: more than %u %s", i, OSMT_MAX_DASHES, what);
            if ((size_t)off + cnt > n_dashes) return fail(OSMT_INVALID_ARG, "style %zu: %s range outside the pool", i, what);
            return (int)OSMT_OK;
        };
        int rc = opacity("opacity", s.has_opacity, s.opacity);
        if (rc == OSMT_OK) rc = opacity("fill_opacity", s.has_fill_opacity, s.fill_opacity);
        if (rc == OSMT_OK) rc = width("width", s.has_width, s.width);
        if (rc == OSMT_OK) rc = width("casing_width", s.has_casing_width, s.casing_width);
        if (rc == OSMT_OK && s.line_cap > OSMT_CAP_SQUARE) rc = fail(OSMT_INVALID_ARG, "style %zu: unknown line_cap %u", i, s.line_cap);
        if (rc == OSMT_OK && s.casing_line_cap > OSMT_CAP_SQUARE) rc = fail(OSMT_INVALID_ARG, "style %zu: unknown casing_line_cap %u", i, s.casing_line_cap);
        if (rc == OSMT_OK) rc = dash_list("dashes", s.has_dashes, s.dashes_off, s.n_dashes);
        if (rc == OSMT_OK) rc = dash_list("casing_dashes", s.has_casing_dashes, s.casing_dashes_off, s.n_casing_dashes);
        if (rc == OSMT_OK && s.has_fill_image && s.fill_image >= n_images)
            rc = fail(OSMT_INVALID_ARG, "style %zu: fill_image %u is not registered (%zu images)", i, s.fill_image, n_images);
        if (rc != OSMT_OK) return rc;
    }
    return OSMT_OK;
}

size_t ctx_image_count(osmt_ctx* ctx) {
    if (!ctx) return 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx->images.size();
}

}  // namespace osmt_host

namespace {

/* the part of compare_styled_entities (styler.rs:246-272) that depends on the style alone */
int style_key_cmp(const osmt_style_rec& a, const osmt_style_rec& b) {
    const int64_t la = a.has_layer ? a.layer : 0, lb = b.has_layer ? b.layer : 0;
    if (la != lb) return la < lb ? -1 : 1;
    const bool fa = a.is_foreground_fill != 0, fb = b.is_foreground_fill != 0;
    if (fa != fb) return fa ? 1 : -1; /* false < true */
    if (a.z_index != b.z_index) return a.z_index < b.z_index ? -1 : 1; /* -0.0 == +0.0; never NaN */
    return 0;
}

struct styles_snapshot {
    const osmt_style_rec* styles = nullptr;
    const uint32_t* rank = nullptr;
    const double* dashes = nullptr;
    uint32_t n = 0;
};

/* Brings the device copy of the style table up to date (records, their dense ranks under style_key_cmp, the dash pool);
 * the snapshot stays valid for the life of the context. */
int sync_styles(osmt_ctx* ctx, styles_snapshot* snap) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->styles_dirty) {
        const size_t n = ctx->styles.size();
        std::vector<uint32_t> order(n), rank(n);
        for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return style_key_cmp(ctx->styles[x], ctx->styles[y]) < 0; });
        uint32_t r = 0;
        for (size_t i = 0; i < n; ++i) {
            if (i && style_key_cmp(ctx->styles[order[i - 1]], ctx->styles[order[i]]) != 0) ++r;
            rank[order[i]] = r;
        }
        const snap_part parts[3] = {{(void**)&ctx->d_styles, ctx->styles.data(), n * sizeof(osmt_style_rec), sizeof(osmt_style_rec)},
                                    {(void**)&ctx->d_style_rank, rank.data(), n * 4, 4},
                                    {(void**)&ctx->d_style_dashes, ctx->style_dashes.data(), ctx->style_dashes.size() * 8, 8}};
        const int rc = snapshot_replace(ctx, "style table", parts, 3);
        if (rc != OSMT_OK) return rc;
        ctx->d_n_styles = (uint32_t)n;
        ctx->styles_dirty = false;
    }
    snap->styles = ctx->d_styles;
    snap->rank = ctx->d_style_rank;
    snap->dashes = ctx->d_style_dashes;
    snap->n = ctx->d_n_styles;
    return OSMT_OK;
}

/* tile_base (optional): n_tiles + 1 entries, the areas of the tiles in front of each tile */
int validate_styled_batch(const osmt_styled_batch* b, osmt_ctx* ctx, std::vector<uint32_t>* tile_base) {
    if (!b) return fail(OSMT_INVALID_ARG, "styled batch is NULL");
    if (b->scale < 1 || b->scale > OSMT_MAX_SCALE) return fail(OSMT_INVALID_ARG, "scale %u not in 1..%u", b->scale, OSMT_MAX_SCALE);
    if ((b->n_tiles && !b->tiles) || (b->n_areas && !b->areas)) return fail(OSMT_INVALID_ARG, "NULL array with non-zero count");
    if (b->n_tiles >= 0x7FFFFFFFull / 64) return fail(OSMT_INVALID_ARG, "styled batch too large for 32-bit indices (tiles)");
    struct range {
        uint64_t lo, hi;
        uint32_t tile;
    };
    std::vector<range> rr;
    rr.reserve(b->n_tiles);
    unsigned long long total = 0;
    if (tile_base) tile_base->assign(b->n_tiles + 1, 0u);
    for (size_t t = 0; t < b->n_tiles; ++t) {
        const osmt_styled_tile& tl = b->tiles[t];
        if (tl.zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u > MAX_ZOOM (src/tile.rs:5)", t, tl.zoom);
        if ((size_t)tl.area_off + tl.n_areas > b->n_areas) return fail(OSMT_INVALID_ARG, "tile %zu: area range out of bounds", t);
        if (tl.n_areas > OSMT_STYLED_MAX_TILE_AREAS)
            return fail(OSMT_UNSUPPORTED, "tile %zu: %u areas (> OSMT_STYLED_MAX_TILE_AREAS = %u)", t, tl.n_areas, OSMT_STYLED_MAX_TILE_AREAS);
        if (tl.n_areas) rr.push_back({tl.area_off, (uint64_t)tl.area_off + tl.n_areas, (uint32_t)t});
        if (tile_base) (*tile_base)[t] = (uint32_t)total;
        total += tl.n_areas;
        if (3ull * total >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "styled batch too large for 32-bit indices (%llu areas x 3 passes)", total);
    }
    if (tile_base) (*tile_base)[b->n_tiles] = (uint32_t)total;
    std::sort(rr.begin(), rr.end(), [](const range& x, const range& y) { return x.lo < y.lo; });
    for (size_t i = 1; i < rr.size(); ++i)
        if (rr[i].lo < rr[i - 1].hi)
            return fail(OSMT_INVALID_ARG, "tile %u: area %llu also belongs to tile %u (area ranges must not overlap)", rr[i].tile, (unsigned long long)rr[i].lo,
                        rr[i - 1].tile);
    /* what the context has registered (a NULL context has nothing) */
    size_t n_ways = 0, n_mps = 0, n_styles = 0;
    if (!ctx) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (no context)", b->geodata_id);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (b->geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
        n_ways = ctx->geodata[b->geodata_id].n_ways;
        n_mps = ctx->geodata[b->geodata_id].n_mps;
        n_styles = ctx->styles.size();
    }
    /* only areas a tile names are read by the kernels, and only they are checked */
    for (const range& r : rr)
        for (uint64_t i = r.lo; i < r.hi; ++i) {
            const osmt_styled_area& a = b->areas[i];
            const uint32_t id = a.entity & ~OSMT_STYLED_MULTIPOLYGON;
            if (a.entity & OSMT_STYLED_MULTIPOLYGON) {
                if (id >= n_mps) return fail(OSMT_INVALID_ARG, "area %llu: multipolygon %u out of range (%zu multipolygons)", (unsigned long long)i, id, n_mps);
            } else if (id >= n_ways) {
                return fail(OSMT_INVALID_ARG, "area %llu: way %u out of range (%zu ways)", (unsigned long long)i, id, n_ways);
            }
            if (a.style >= n_styles) return fail(OSMT_INVALID_ARG, "area %llu: style %u is not registered (%zu styles)", (unsigned long long)i, a.style, n_styles);
        }
    return OSMT_OK;
}

int register_geodata_body(osmt_ctx* ctx, const osmt_geodata_desc* g, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = validate_geodata(g);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    /* per multipolygon: its rings of >= 2 nodes and their nodes (point_pairs.rs:36-40 drops the others) */
    std::vector<uint2> mp_sum(g->n_multipolygons);
    for (size_t m = 0; m < g->n_multipolygons; ++m) {
        unsigned long long rings = 0, refs = 0;
        for (uint32_t k = g->multipolygon_polygon_off[m]; k < g->multipolygon_polygon_off[m + 1]; ++k) {
            const uint32_t p = g->multipolygon_polygons[k];
            const uint32_t nn = g->polygon_node_off[p + 1] - g->polygon_node_off[p];
            if (nn >= 2) ++rings, refs += nn;
        }
        if (refs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "geodata: multipolygon %zu has %llu nodes (> 2^32)", m, refs);
        mp_sum[m] = make_uint2((uint32_t)rings, (uint32_t)refs);
    }
    std::vector<uint32_t> poly_off(g->n_polygons + 1);
    for (size_t p = 0; p <= g->n_polygons; ++p) poly_off[p] = g->polygon_node_off[p] + (uint32_t)g->n_way_nodes;
    pool_layout pl;
    const size_t o_nodes = pl.add(g->n_nodes * 16), o_wgid = pl.add(g->n_ways * 8), o_mgid = pl.add(g->n_multipolygons * 8);
    const size_t o_woff = pl.add((g->n_ways + 1) * 4), o_poff = pl.add((g->n_polygons + 1) * 4), o_moff = pl.add((g->n_multipolygons + 1) * 4);
    const size_t o_mpol = pl.add(g->n_multipolygon_polygons * 4), o_idx = pl.add((g->n_way_nodes + g->n_polygon_nodes) * 4);
    const size_t o_sum = pl.add(g->n_multipolygons * 8);
    table_upload up("geodata", pl);
    char* pool = up.pool;
    up.put(o_nodes, g->nodes, g->n_nodes * 16);
    up.put(o_wgid, g->way_ids, g->n_ways * 8);
    up.put(o_mgid, g->multipolygon_ids, g->n_multipolygons * 8);
    up.put(o_woff, g->way_node_off, (g->n_ways + 1) * 4);
    up.put(o_poff, poly_off.data(), (g->n_polygons + 1) * 4);
    up.put(o_moff, g->multipolygon_polygon_off, (g->n_multipolygons + 1) * 4);
    up.put(o_mpol, g->multipolygon_polygons, g->n_multipolygon_polygons * 4);
    up.put(o_idx, g->way_nodes, g->n_way_nodes * 4);
    up.put(o_idx + g->n_way_nodes * 4, g->polygon_nodes, g->n_polygon_nodes * 4);
    up.put(o_sum, mp_sum.data(), g->n_multipolygons * 8);
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::geodata_host h;
    h.n_nodes = g->n_nodes, h.n_ways = g->n_ways, h.n_mps = g->n_multipolygons;
    h.n_polys = g->n_polygons, h.n_way_nodes = g->n_way_nodes, h.n_poly_nodes = g->n_polygon_nodes, h.n_mp_polys = g->n_multipolygon_polygons;
    h.d_pool = pool;
    h.dev.nodes = (const double*)(pool + o_nodes);
    h.dev.way_gid = (const uint64_t*)(pool + o_wgid);
    h.dev.mp_gid = (const uint64_t*)(pool + o_mgid);
    h.dev.way_off = (const uint32_t*)(pool + o_woff);
    h.dev.poly_off = (const uint32_t*)(pool + o_poff);
    h.dev.mp_off = (const uint32_t*)(pool + o_moff);
    h.dev.mp_polys = (const uint32_t*)(pool + o_mpol);
    h.dev.idx = (const uint32_t*)(pool + o_idx);
    h.dev.mp_sum = (const uint2*)(pool + o_sum);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->geodata.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "geodata table too large");
    *out_id = (uint32_t)ctx->geodata.size();
    ctx->geodata.push_back(h);
    up.release();
    return OSMT_OK;
}

}  // namespace

namespace osmt_host {

int register_styles_body(osmt_ctx* ctx, const osmt_style_rec* st, size_t n, const double* dashes, size_t n_dashes, uint32_t* out_first) {
    if (!ctx || !out_first) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = validate_styles(st, n, dashes, n_dashes, ctx_image_count(ctx));
    if (rc != OSMT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->styles.size() + n >= 0xFFFFFFFFull || ctx->style_dashes.size() + n_dashes >= 0xFFFFFFFFull)
        return fail(OSMT_INVALID_ARG, "style table too large");
    const uint32_t first = (uint32_t)ctx->styles.size(), dash_base = (uint32_t)ctx->style_dashes.size();
    ctx->styles.reserve(ctx->styles.size() + n);
    ctx->style_dashes.insert(ctx->style_dashes.end(), dashes, dashes + n_dashes);
    for (size_t i = 0; i < n; ++i) {
        osmt_style_rec s = st[i];
        s.dashes_off = s.has_dashes ? s.dashes_off + dash_base : 0u;
        s.casing_dashes_off = s.has_casing_dashes ? s.casing_dashes_off + dash_base : 0u;
        ctx->styles.push_back(s);
    }
    ctx->styles_dirty = true;
    *out_first = first;
    return OSMT_OK;
}

}  // namespace osmt_host

namespace {

/* a styled batch on the device: what both entries hand to the shared half of the build */
struct styled_src {
    const osmt_styled_tile* tiles;
    const uint32_t* tile_base; /* [n_tiles + 1] */
    const osmt_styled_area* areas; /* indexed with the tiles' area_off */
    size_t n_tiles, total;         /* total = tile_base[n_tiles] */
    uint32_t scale, use_caps;
};

/* The half of the build both entries share: everything from osmt_launch_styled_count on, over a styled batch that is on the
 * device already (uploaded by osmt_scene_build_styled, derived by osmt_scene_build_tiles), on the caller's stream. */
int styled_build_back(osmt_ctx* ctx, hipStream_t st, const osmt_ctx::geodata_host& geo, const styles_snapshot& ss, const styled_src& in,
                      osmt_scene** out_scene) {
    const size_t n_tiles = in.n_tiles, total = in.total, n_elems = 3 * total, n_blk = (n_elems + 255) / 256;
    /* everything that lives only during the build, given back at the end: work[0] one allocation, work[1] the rings' sources */
    call_work wg(ctx, "styled build", st);
    int rc = wg.begin(4);
    if (rc != OSMT_OK) return rc;
    const bool trace = wg.trace;
    pool_layout pl;
    const size_t o_keys = pl.add(total * 16), o_sorted = pl.add(total * 4), o_pre = pl.add((size_t)OSMT_SQ_N * (n_elems + 1) * 4);
    const size_t o_blk = pl.add((size_t)OSMT_SQ_N * std::max<size_t>(n_blk, 1) * 8), o_tot = pl.add(OSMT_STYLED_TOTALS * 8);
    rc = wg.alloc(0, pl);
    if (rc != OSMT_OK) return rc;
    char* w = wg.work[0];
    osmt_styled_pass P;
    memset(&P, 0, sizeof P);
    P.geo = geo.dev;
    P.styles = ss.styles;
    P.style_rank = ss.rank;
    P.style_dashes = ss.dashes;
    P.tiles = in.tiles;
    P.tile_base = in.tile_base;
    P.areas = in.areas;
    P.n_tiles = (uint32_t)n_tiles;
    P.n_elems = (uint32_t)n_elems;
    P.scale = in.scale;
    P.use_caps = in.use_caps;
    P.keys = (ulonglong2*)(w + o_keys);
    P.sorted = (uint32_t*)(w + o_sorted);
    P.pre = (uint32_t*)(w + o_pre);
    P.blk = (unsigned long long*)(w + o_blk);
    P.totals = (unsigned long long*)(w + o_tot);
    /* the trace: the device time of the two launch sequences */
    HIP_TRY(wg.mark(0));
    HIP_TRY(osmt_launch_styled_count(P, st));
    HIP_TRY(wg.mark(1));
    unsigned long long tot[OSMT_STYLED_TOTALS];
    HIP_TRY(hipMemcpyAsync(tot, P.totals, sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    static const char* const what[OSMT_SQ_N] = {"ops", "rings", "node references", "dashes", "stroke ops", "64-edge blocks", "virtual stroke segments"};
    for (int q = 0; q < OSMT_SQ_N; ++q)
        if (tot[q] >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "styled batch needs %llu %s (> 2^32): split the batch", tot[q], what[q]);
    const size_t n_ops = tot[OSMT_SQ_OPS], n_rings = tot[OSMT_SQ_RINGS], n_pts = tot[OSMT_SQ_REFS], n_dashes = tot[OSMT_SQ_DASHES];
    const size_t n_strokes = tot[OSMT_SQ_STROKES], n_blocks = tot[OSMT_SQ_BLOCKS], n_vsegs = tot[OSMT_SQ_VSEGS];

    osmt_scene* s = new (std::nothrow) osmt_scene();
    if (!s) return fail(OSMT_OOM, "out of host memory");
    s->own_stream = st; /* until the build is complete: everything about the scene happens on this stream */
    s->ctx = ctx;
    ctx->refs.fetch_add(1);
    s->h_err = err_slot_acquire(ctx);
    s->n_jobs = (uint32_t)n_tiles;
    s->max_job_ops = (uint32_t)tot[OSMT_SQ_N];
    s->n_ops = (uint32_t)n_ops;
    s->n_rings = (uint32_t)n_rings;
    s->n_pts = (uint32_t)n_pts;
    s->n_dashes = (uint32_t)n_dashes;
    s->n_strokes = (uint32_t)n_strokes;
    s->n_blk = (uint32_t)n_blocks;
    s->n_vsegs = (uint32_t)n_vsegs;
    s->scale = in.scale;
    s->coord_kind = OSMT_COORD_NODE_REF;
    /* the front arrays in the order of scene_upload_impl — without a node table: d_latlon is the registered one */
    pl = pool_layout();
    const size_t o_jobs = pl.add(n_tiles * sizeof(osmt_tile_job)), o_ops = pl.add(n_ops * sizeof(osmt_op)), o_rings = pl.add(n_rings * sizeof(osmt_ring));
    const size_t o_refs = pl.add(n_pts * 4), o_pts = pl.add(n_pts * 8), o_dashes = pl.add((n_dashes + 1) * 8), o_ptjob = pl.add(n_pts * 4);
    const size_t o_opaux = pl.add(n_ops * 4), o_opblk = pl.add(n_ops * 4), o_opvseg = pl.add(n_ops * 4), o_opjob = pl.add(n_ops * 4);
    const scene_back bk = scene_carve_back(pl, n_tiles, n_ops, n_strokes, n_blocks, n_vsegs, in.scale);
    s->bytes = pl.size() + 256;
    hipError_t e = dev_alloc(ctx, (void**)&s->d_base, s->bytes);
    if (e == hipSuccess) {
        e = dev_alloc(ctx, (void**)&wg.work[1], std::max<size_t>(n_rings, 1) * 4);
        if (e != hipSuccess) wg.work[1] = nullptr;
    } else {
        s->d_base = nullptr;
    }
    if (e != hipSuccess) {
        dev_free(ctx, s->d_base);
        scene_delete(s);
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) failed: %s", pl.size(), hipGetErrorString(e));
    }
    char* base = s->d_base;
    s->d_jobs = (osmt_tile_job*)(base + o_jobs);
    s->d_ops = (osmt_op*)(base + o_ops);
    s->d_rings = (osmt_ring*)(base + o_rings);
    s->d_latlon = const_cast<double*>(geo.dev.nodes); /* not the scene's: the geodata snapshot's, never freed under it */
    s->d_node_refs = (uint32_t*)(base + o_refs);
    s->d_pts = (int32_t*)(base + o_pts);
    s->d_dashes = (double*)(base + o_dashes);
    s->d_pt_job = (uint32_t*)(base + o_ptjob);
    s->d_op_aux = (uint32_t*)(base + o_opaux);
    s->d_op_blk = (uint32_t*)(base + o_opblk);
    s->d_op_vseg = (uint32_t*)(base + o_opvseg);
    s->d_op_job = (uint32_t*)(base + o_opjob);
    scene_point_back(s, base, bk);
    P.jobs = s->d_jobs;
    P.ops = s->d_ops;
    P.rings = s->d_rings;
    P.refs = s->d_node_refs;
    P.dashes = s->d_dashes;
    P.op_job = s->d_op_job;
    P.op_aux = s->d_op_aux;
    P.op_blk = s->d_op_blk;
    P.op_vseg = s->d_op_vseg;
    P.ring_src = (uint32_t*)wg.work[1];
    P.n_rings = (uint32_t)n_rings;
    P.n_refs = (uint32_t)n_pts;
    (void)wg.mark(2);
    e = osmt_launch_styled_emit(P, st);
    if (e == hipSuccess) e = osmt_launch_ptjob(s->d_jobs, s->n_jobs, s->d_pt_job, s->n_pts, st);
    (void)wg.mark(3);
    if (e != hipSuccess) {
        osmt_scene_free(s);
        return fail(OSMT_HIP_ERROR, "styled build failed: %s", hipGetErrorString(e));
    }
    rc = scene_size_arenas(ctx, s, n_ops - n_strokes, false);
    if (rc == OSMT_OK) {
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "styled build failed: %s", hipGetErrorString(e));
    }
    if (rc != OSMT_OK) {
        osmt_scene_free(s);
        return rc;
    }
    if (trace)
        fprintf(stderr, "osmt styled build: sort + count + scan kernels %.1f us, emit kernels %.1f us (%zu tiles, %zu areas, %zu ops)\n",
                wg.us(0, 1), wg.us(2, 3), n_tiles, total, n_ops);
    s->own_stream = nullptr; /* from here on a public scene: waits go through its last-use events */
    *out_scene = s;
    return OSMT_OK;
}

int scene_build_styled_body(osmt_ctx* ctx, const osmt_styled_batch* b, osmt_scene** out_scene) {
    if (!ctx || !out_scene) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_scene = nullptr;
    std::vector<uint32_t> tile_base;
    int rc = validate_styled_batch(b, ctx, &tile_base);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    styles_snapshot ss;
    rc = sync_styles(ctx, &ss);
    if (rc != OSMT_OK) return rc;
    osmt_ctx::geodata_host geo;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geo = ctx->geodata[b->geodata_id];
    }
    const size_t n_tiles = b->n_tiles;
    /* the span of `areas` the tiles name (their ranges may lie anywhere in the array; the device indexes it as the caller does) */
    size_t a_lo = b->n_areas, a_hi = 0;
    for (size_t t = 0; t < n_tiles; ++t)
        if (b->tiles[t].n_areas) {
            a_lo = std::min<size_t>(a_lo, b->tiles[t].area_off);
            a_hi = std::max<size_t>(a_hi, (size_t)b->tiles[t].area_off + b->tiles[t].n_areas);
        }
    if (a_hi < a_lo) a_lo = a_hi = 0;
    /* the caller's arrays on the device: given back when the build is over */
    call_work fg(ctx, "styled build");
    rc = fg.begin(0);
    if (rc != OSMT_OK) return rc;
    hipStream_t st = fg.st;
    pool_layout pl;
    const size_t o_tiles = pl.add(n_tiles * sizeof(osmt_styled_tile)), o_base = pl.add((n_tiles + 1) * 4), o_areas = pl.add((a_hi - a_lo) * sizeof(osmt_styled_area));
    rc = fg.alloc(0, pl);
    if (rc != OSMT_OK) return rc;
    char* w = fg.work[0];
    if (n_tiles) HIP_TRY(hipMemcpyAsync(w + o_tiles, b->tiles, n_tiles * sizeof(osmt_styled_tile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w + o_base, tile_base.data(), (n_tiles + 1) * 4, hipMemcpyHostToDevice, st));
    if (a_hi > a_lo) HIP_TRY(hipMemcpyAsync(w + o_areas, b->areas + a_lo, (a_hi - a_lo) * sizeof(osmt_styled_area), hipMemcpyHostToDevice, st));
    styled_src in;
    in.tiles = (const osmt_styled_tile*)(w + o_tiles);
    in.tile_base = (const uint32_t*)(w + o_base);
    in.areas = (const osmt_styled_area*)(w + o_areas) - a_lo; /* indexed with the caller's offsets, from a_lo on */
    in.n_tiles = n_tiles, in.total = tile_base[n_tiles];
    in.scale = b->scale, in.use_caps = b->use_caps_for_dashes ? 1u : 0u;
    return styled_build_back(ctx, st, geo, ss, in, out_scene);
}

/* ---- scenes built from tile coordinates (include/osmtile.h, csrc/osmt_tilequery.hip) ---------------------------------- */
int validate_tile_index(const osmt_tile_index_desc* x, size_t n_ways, size_t n_mps) {
    if (!x) return fail(OSMT_INVALID_ARG, "tile index is NULL");
    if ((x->n_tiles && !x->tile_xy) || !x->way_off || (x->n_way_refs && !x->ways) || !x->multipolygon_off || (x->n_multipolygon_refs && !x->multipolygons))
        return fail(OSMT_INVALID_ARG, "tile index: NULL array (every offset array has at least its first entry)");
    if (x->n_tiles >= 0xFFFFFFFFull || x->n_way_refs >= 0xFFFFFFFFull || x->n_multipolygon_refs >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "tile index: too large for 32-bit indices");
    int rc = check_offsets_of("tile index", "way_off", x->way_off, x->n_tiles, x->n_way_refs);
    if (rc == OSMT_OK) rc = check_offsets_of("tile index", "multipolygon_off", x->multipolygon_off, x->n_tiles, x->n_multipolygon_refs);
    if (rc != OSMT_OK) return rc;
    const uint32_t world = 1u << OSMT_MAX_ZOOM;
    for (size_t i = 0; i < x->n_tiles; ++i) {
        const uint32_t tx = x->tile_xy[2 * i], ty = x->tile_xy[2 * i + 1];
        if (tx >= world || ty >= world) return fail(OSMT_INVALID_ARG, "tile index: tile %zu = (%u, %u) outside the zoom-18 world (coordinates < %u)", i, tx, ty, world);
        if (i) {
            const uint32_t px = x->tile_xy[2 * i - 2], py = x->tile_xy[2 * i - 1];
            if (px > tx || (px == tx && py >= ty))
                return fail(OSMT_INVALID_ARG, "tile index: tile %zu = (%u, %u) does not come after tile %zu = (%u, %u) (strictly ascending by x, then y)", i, tx, ty,
                            i - 1, px, py);
        }
    }
    for (size_t i = 0; i < x->n_way_refs; ++i)
        if (x->ways[i] >= n_ways) return fail(OSMT_INVALID_ARG, "tile index: ways[%zu] = %u is not a way (%zu ways)", i, x->ways[i], n_ways);
    for (size_t i = 0; i < x->n_multipolygon_refs; ++i)
        if (x->multipolygons[i] >= n_mps)
            return fail(OSMT_INVALID_ARG, "tile index: multipolygons[%zu] = %u is not a multipolygon (%zu multipolygons)", i, x->multipolygons[i], n_mps);
    return OSMT_OK;
}

int register_tile_index_body(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tile_index_desc* x) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    size_t n_ways = 0, n_mps = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
        if (ctx->geodata[geodata_id].d_index) return fail(OSMT_INVALID_ARG, "geodata id %u has a tile index already (one per file)", geodata_id);
        n_ways = ctx->geodata[geodata_id].n_ways, n_mps = ctx->geodata[geodata_id].n_mps;
    }
    const int rc = validate_tile_index(x, n_ways, n_mps);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    /* the column directory: the distinct x and the first tile of each */
    const size_t n = x->n_tiles;
    std::vector<uint32_t> col_x, col_first, tile_y(n);
    for (size_t i = 0; i < n; ++i) {
        tile_y[i] = x->tile_xy[2 * i + 1];
        if (i == 0 || x->tile_xy[2 * i] != x->tile_xy[2 * i - 2]) {
            col_x.push_back(x->tile_xy[2 * i]);
            col_first.push_back((uint32_t)i);
        }
    }
    col_first.push_back((uint32_t)n);
    pool_layout pl;
    const size_t o_cx = pl.add(col_x.size() * 4), o_cf = pl.add(col_first.size() * 4), o_ty = pl.add(n * 4), o_wo = pl.add((n + 1) * 4);
    const size_t o_w = pl.add(x->n_way_refs * 4), o_mo = pl.add((n + 1) * 4), o_m = pl.add(x->n_multipolygon_refs * 4);
    table_upload up("tile index", pl);
    char* pool = up.pool;
    up.put(o_cx, col_x.data(), col_x.size() * 4);
    up.put(o_cf, col_first.data(), col_first.size() * 4);
    up.put(o_ty, tile_y.data(), n * 4);
    up.put(o_wo, x->way_off, (n + 1) * 4);
    up.put(o_w, x->ways, x->n_way_refs * 4);
    up.put(o_mo, x->multipolygon_off, (n + 1) * 4);
    up.put(o_m, x->multipolygons, x->n_multipolygon_refs * 4);
    if (up.done() != OSMT_OK) return up.done();
    osmt_tq_index_dev d{};
    d.col_x = (const uint32_t*)(pool + o_cx);
    d.col_first = (const uint32_t*)(pool + o_cf);
    d.tile_y = (const uint32_t*)(pool + o_ty);
    d.way_off = (const uint32_t*)(pool + o_wo);
    d.ways = (const uint32_t*)(pool + o_w);
    d.mp_off = (const uint32_t*)(pool + o_mo);
    d.mps = (const uint32_t*)(pool + o_m);
    d.n_cols = (uint32_t)col_x.size();
    d.n_tiles = (uint32_t)n;
    d.level = OSMT_MAX_ZOOM;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->geodata[geodata_id].d_index) return fail(OSMT_INVALID_ARG, "geodata id %u has a tile index already (one per file)", geodata_id); /* another thread was first */
    ctx->geodata[geodata_id].d_index = pool;
    ctx->geodata[geodata_id].ix = d;
    up.release();
    return OSMT_OK;
}

int validate_style_bindings(const osmt_style_bindings_desc* b, osmt_ctx* ctx) {
    if (!b) return fail(OSMT_INVALID_ARG, "style bindings are NULL");
    if (b->zoom_lo > b->zoom_hi || b->zoom_hi > OSMT_MAX_ZOOM)
        return fail(OSMT_INVALID_ARG, "style bindings: zoom range %u..%u (zoom_lo <= zoom_hi <= %u)", b->zoom_lo, b->zoom_hi, OSMT_MAX_ZOOM);
    if (!ctx) return fail(OSMT_INVALID_ARG, "style bindings: geodata id %u is not registered (no context)", b->geodata_id);
    size_t n_ways = 0, n_mps = 0, n_styles = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (b->geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "style bindings: geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
        n_ways = ctx->geodata[b->geodata_id].n_ways, n_mps = ctx->geodata[b->geodata_id].n_mps;
        n_styles = ctx->styles.size();
    }
    if (!b->way_style_off || (b->n_way_styles && !b->way_styles) || !b->multipolygon_style_off || (b->n_multipolygon_styles && !b->multipolygon_styles))
        return fail(OSMT_INVALID_ARG, "style bindings: NULL array (every offset array has at least its first entry)");
    if (b->n_way_styles >= 0xFFFFFFFFull || b->n_multipolygon_styles >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "style bindings: too large for 32-bit indices");
    int rc = check_offsets_of("style bindings", "way_style_off", b->way_style_off, n_ways, b->n_way_styles);
    if (rc == OSMT_OK) rc = check_offsets_of("style bindings", "multipolygon_style_off", b->multipolygon_style_off, n_mps, b->n_multipolygon_styles);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < b->n_way_styles; ++i)
        if (b->way_styles[i] >= n_styles)
            return fail(OSMT_INVALID_ARG, "style bindings: way_styles[%zu] = %u is not a registered style (%zu styles)", i, b->way_styles[i], n_styles);
    for (size_t i = 0; i < b->n_multipolygon_styles; ++i)
        if (b->multipolygon_styles[i] >= n_styles)
            return fail(OSMT_INVALID_ARG, "style bindings: multipolygon_styles[%zu] = %u is not a registered style (%zu styles)", i, b->multipolygon_styles[i],
                        n_styles);
    return OSMT_OK;
}

int register_style_bindings_body(osmt_ctx* ctx, const osmt_style_bindings_desc* b, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = validate_style_bindings(b, ctx);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    size_t n_ways = 0, n_mps = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        n_ways = ctx->geodata[b->geodata_id].n_ways, n_mps = ctx->geodata[b->geodata_id].n_mps;
    }
    pool_layout pl;
    const size_t o_wo = pl.add((n_ways + 1) * 4), o_w = pl.add(b->n_way_styles * 4), o_mo = pl.add((n_mps + 1) * 4), o_m = pl.add(b->n_multipolygon_styles * 4);
    table_upload up("style bindings", pl);
    char* pool = up.pool;
    up.put(o_wo, b->way_style_off, (n_ways + 1) * 4);
    up.put(o_w, b->way_styles, b->n_way_styles * 4);
    up.put(o_mo, b->multipolygon_style_off, (n_mps + 1) * 4);
    up.put(o_m, b->multipolygon_styles, b->n_multipolygon_styles * 4);
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::bindings_host h;
    h.geodata_id = b->geodata_id, h.zoom_lo = b->zoom_lo, h.zoom_hi = b->zoom_hi;
    h.d_pool = pool;
    h.dev.way_off = (const uint32_t*)(pool + o_wo);
    h.dev.way_styles = (const uint32_t*)(pool + o_w);
    h.dev.mp_off = (const uint32_t*)(pool + o_mo);
    h.dev.mp_styles = (const uint32_t*)(pool + o_m);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "bindings table too large");
    *out_id = (uint32_t)ctx->bindings.size();
    ctx->bindings.push_back(h);
    up.release();
    return OSMT_OK;
}

/* bind (optional): the device tables of the zooms the batch's tiles have */
int validate_tile_batch(const osmt_tile_batch* b, osmt_ctx* ctx, osmt_tq_bind_dev* bind) {
    if (!b) return fail(OSMT_INVALID_ARG, "tile batch is NULL");
    if (b->scale < 1 || b->scale > OSMT_MAX_SCALE) return fail(OSMT_INVALID_ARG, "scale %u not in 1..%u", b->scale, OSMT_MAX_SCALE);
    if (b->n_tiles && !b->tiles) return fail(OSMT_INVALID_ARG, "NULL array with non-zero count");
    if (b->n_tiles >= 0x7FFFFFFFull / 64) return fail(OSMT_INVALID_ARG, "tile batch too large for 32-bit indices (tiles)");
    bool zoom_used[OSMT_MAX_ZOOM + 1] = {};
    size_t first_of_zoom[OSMT_MAX_ZOOM + 1] = {};
    for (size_t t = 0; t < b->n_tiles; ++t) {
        const osmt_query_tile& q = b->tiles[t];
        if (q.zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u > MAX_ZOOM (src/tile.rs:5)", t, q.zoom);
        if (q.x >= (1u << q.zoom) || q.y >= (1u << q.zoom))
            return fail(OSMT_INVALID_ARG, "tile %zu: (x, y) = (%u, %u) outside the %u x %u tiles of zoom %u", t, q.x, q.y, 1u << q.zoom, 1u << q.zoom, q.zoom);
        if (!zoom_used[q.zoom]) zoom_used[q.zoom] = true, first_of_zoom[q.zoom] = t;
    }
    if (!ctx) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (no context)", b->geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (b->geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
    if (!ctx->geodata[b->geodata_id].d_index) return fail(OSMT_INVALID_ARG, "geodata id %u has no tile index (osmt_register_tile_index)", b->geodata_id);
    for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) {
        if (!zoom_used[z]) continue;
        const uint32_t id = b->bindings_of_zoom[z];
        if (id == OSMT_BINDINGS_NONE) return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no bindings (OSMT_BINDINGS_NONE)", first_of_zoom[z], z);
        if (id >= ctx->bindings.size())
            return fail(OSMT_INVALID_ARG, "tile %zu: bindings id %u of zoom %u is not registered (%zu tables)", first_of_zoom[z], id, z, ctx->bindings.size());
        const osmt_ctx::bindings_host& h = ctx->bindings[id];
        if (h.geodata_id != b->geodata_id)
            return fail(OSMT_INVALID_ARG, "tile %zu: bindings id %u of zoom %u belongs to geodata id %u, not %u", first_of_zoom[z], id, z, h.geodata_id, b->geodata_id);
        if (z < h.zoom_lo || z > h.zoom_hi)
            return fail(OSMT_INVALID_ARG, "tile %zu: bindings id %u covers zooms %u..%u, not zoom %u", first_of_zoom[z], id, h.zoom_lo, h.zoom_hi, z);
        if (bind) bind[z] = h.dev;
    }
    return OSMT_OK;
}

}  // namespace

namespace osmt_host {

int scene_build_tiles_body(osmt_ctx* ctx, const osmt_tile_batch* b, uint32_t filter_id, osmt_scene** out_scene) {
    if (!ctx || !out_scene) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_scene = nullptr;
    osmt_tq_bind_dev bind[OSMT_MAX_ZOOM + 1];
    memset(bind, 0, sizeof bind);
    int rc = validate_tile_batch(b, ctx, bind);
    if (rc != OSMT_OK) return rc;
    osmt_ctx::id_filter_host flt;
    if (filter_id != OSMT_ID_FILTER_NONE) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (filter_id >= ctx->id_filters.size()) return fail(OSMT_INVALID_ARG, "id filter %u is not registered (%zu filters)", filter_id, ctx->id_filters.size());
        flt = ctx->id_filters[filter_id];
        if (flt.geodata_id != b->geodata_id)
            return fail(OSMT_INVALID_ARG, "id filter %u belongs to geodata id %u, not %u", filter_id, flt.geodata_id, b->geodata_id);
        flt.on = true;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    styles_snapshot ss;
    rc = sync_styles(ctx, &ss);
    if (rc != OSMT_OK) return rc;
    osmt_ctx::geodata_host geo;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        geo = ctx->geodata[b->geodata_id];
    }
    const size_t n_tiles = b->n_tiles;
    /* work[0]: per tile, work[1]: per item, work[2]: per candidate — given back at the end */
    /* the trace: the device time of the stages */
    enum { EV_SPAN0, EV_SPAN1, EV_COL0, EV_COL1, EV_GATHER0, EV_SORT0, EV_MARK0, EV_MARK1, EV_EMIT0, EV_EMIT1, EV_N };
    call_work wg(ctx, "tile query");
    rc = wg.begin(EV_N);
    if (rc != OSMT_OK) return rc;
    hipStream_t st = wg.st;
    const bool trace = wg.trace;
    pool_layout pl;

    unsigned long long tot[OSMT_TQ_N] = {};
    osmt_tq_pass P;
    memset(&P, 0, sizeof P);
    pl = pool_layout();
    const size_t o_q = pl.add(n_tiles * sizeof(osmt_query_tile)), o_bind = pl.add(sizeof bind), o_c0 = pl.add(n_tiles * 4), o_ib = pl.add((n_tiles + 1) * 4);
    const size_t o_tw = pl.add((n_tiles + 1) * 4), o_tm = pl.add((n_tiles + 1) * 4), o_tot = pl.add(OSMT_TQ_N * 8), o_blk0 = pl.add((n_tiles / 256 + 1) * 8);
    rc = wg.alloc(0, pl, "tiles");
    if (rc != OSMT_OK) return rc;
    char* w0 = wg.work[0];
    size_t n_items = 0, n_way_cand = 0, n_mp_cand = 0, n_cand = 0, n_areas = 0;
    if (n_tiles) {
        HIP_TRY(hipMemcpyAsync(w0 + o_q, b->tiles, n_tiles * sizeof(osmt_query_tile), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w0 + o_bind, bind, sizeof bind, hipMemcpyHostToDevice, st));
        tq_bind_levels(geo, false, geo.ix, P);
        P.geo_mp_off = geo.dev.mp_off;
        if (flt.on) P.keep_way = flt.way, P.keep_mp = flt.mp;
        P.bind = (const osmt_tq_bind_dev*)(w0 + o_bind);
        P.q = (const osmt_query_tile*)(w0 + o_q);
        P.n_tiles = (uint32_t)n_tiles;
        P.span_c0 = (uint32_t*)(w0 + o_c0);
        P.item_base = (uint32_t*)(w0 + o_ib);
        P.t_wbase = (uint32_t*)(w0 + o_tw);
        P.t_mbase = (uint32_t*)(w0 + o_tm);
        P.tot = (unsigned long long*)(w0 + o_tot);
        P.blk = (unsigned long long*)(w0 + o_blk0);
        /* 1. span */
        HIP_TRY(wg.mark(EV_SPAN0));
        HIP_TRY(osmt_launch_tq_span(P, st));
        HIP_TRY(wg.mark(EV_SPAN1));
        HIP_TRY(hipMemcpyAsync(tot, P.tot, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tot[OSMT_TQ_ITEMS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile batch needs %llu (tile, column) items (> 2^32): split the batch", tot[OSMT_TQ_ITEMS]);
        n_items = (size_t)tot[OSMT_TQ_ITEMS];
        /* 2. columns */
        pl = pool_layout();
        const size_t o_it = pl.add(n_items * 4), o_ws = pl.add(n_items * 4), o_ms = pl.add(n_items * 4), o_wb = pl.add((n_items + 1) * 4);
        const size_t o_mb = pl.add((n_items + 1) * 4), o_blk1 = pl.add((n_items / 256 + 1) * 8);
        rc = wg.alloc(1, pl, "columns");
        if (rc != OSMT_OK) return rc;
        char* w1 = wg.work[1];
        P.n_items = (uint32_t)n_items;
        P.item_tile = (uint32_t*)(w1 + o_it);
        P.item_wsrc = (uint32_t*)(w1 + o_ws);
        P.item_msrc = (uint32_t*)(w1 + o_ms);
        P.wbase = (uint32_t*)(w1 + o_wb);
        P.mbase = (uint32_t*)(w1 + o_mb);
        P.blk = (unsigned long long*)(w1 + o_blk1);
        HIP_TRY(wg.mark(EV_COL0));
        HIP_TRY(osmt_launch_tq_columns(P, st));
        HIP_TRY(wg.mark(EV_COL1));
        /* first read-back: the candidate totals, the largest tile, the first tile over the limit — nothing is gathered before */
        HIP_TRY(hipMemcpyAsync(tot, P.tot, OSMT_TQ_OVER_CAND * 8 + 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tot[OSMT_TQ_OVER_CAND] != ~0ull) {
            const size_t t = (size_t)tot[OSMT_TQ_OVER_CAND];
            uint32_t base[4]; /* t_wbase[t], t_wbase[t + 1], t_mbase[t], t_mbase[t + 1] */
            HIP_TRY(hipMemcpyAsync(base, P.t_wbase + t, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(base + 2, P.t_mbase + t, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint32_t nw = base[1] - base[0], nm = base[3] - base[2];
            return fail(OSMT_UNSUPPORTED, "tile %zu gathers %u %s references (> OSMT_QUERY_MAX_TILE_CANDIDATES = %u)", t,
                        nw > OSMT_QUERY_MAX_TILE_CANDIDATES ? nw : nm, nw > OSMT_QUERY_MAX_TILE_CANDIDATES ? "way" : "multipolygon",
                        OSMT_QUERY_MAX_TILE_CANDIDATES);
        }
        if (tot[OSMT_TQ_WAYS] + tot[OSMT_TQ_MPS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile batch gathers %llu references (%llu way + %llu multipolygon, > 2^32): split the batch",
                        tot[OSMT_TQ_WAYS] + tot[OSMT_TQ_MPS], tot[OSMT_TQ_WAYS], tot[OSMT_TQ_MPS]);
        n_way_cand = (size_t)tot[OSMT_TQ_WAYS], n_mp_cand = (size_t)tot[OSMT_TQ_MPS], n_cand = n_way_cand + n_mp_cand;
        tq_stats_set(ctx, n_items, n_way_cand, n_mp_cand, 0);
        /* 3. gather, 4. sort, mark */
        pl = pool_layout();
        const size_t o_cand = pl.add(n_cand * 4), o_apos = pl.add((n_cand + 1) * 4), o_blk2 = pl.add((n_cand / 256 + 1) * 8);
        rc = wg.alloc(2, pl, "candidates");
        if (rc != OSMT_OK) return rc;
        char* w2 = wg.work[2];
        P.n_ways = (uint32_t)n_way_cand;
        P.n_mps = (uint32_t)n_mp_cand;
        P.cand = (uint32_t*)(w2 + o_cand);
        P.apos = (uint32_t*)(w2 + o_apos);
        P.blk = (unsigned long long*)(w2 + o_blk2);
    }
    /* the derived styled batch: the tiles' records and tile_base (written before the areas are counted), and the areas;
     * two allocations that go to the scene (osmt_scene_read_styled_areas) */
    struct keep_guard {
        osmt_ctx* ctx;
        hipStream_t st;
        char* head = nullptr;
        char* areas = nullptr;
        ~keep_guard() {
            if (!head && !areas) return;
            (void)hipStreamSynchronize(st);
            dev_free(ctx, head);
            dev_free(ctx, areas);
        }
    } kg{ctx, st};
    pl = pool_layout();
    const size_t o_tiles = pl.add(n_tiles * sizeof(osmt_styled_tile)), o_base = pl.add((n_tiles + 1) * 4);
    rc = wg.alloc(&kg.head, pl, "styled tiles");
    if (rc != OSMT_OK) return rc;
    P.tiles = (osmt_styled_tile*)(kg.head + o_tiles);
    P.tile_base = (uint32_t*)(kg.head + o_base);
    if (n_tiles) {
        HIP_TRY(wg.mark(EV_GATHER0));
        HIP_TRY(osmt_launch_tq_gather(P, st));
        HIP_TRY(wg.mark(EV_SORT0));
        HIP_TRY(osmt_launch_tq_sort(P, st));
        HIP_TRY(wg.mark(EV_MARK0));
        HIP_TRY(osmt_launch_tq_mark(P, st));
        HIP_TRY(wg.mark(EV_MARK1));
        /* second read-back: the area total, the most areas of a tile, the first tile over the limit */
        HIP_TRY(hipMemcpyAsync(tot + OSMT_TQ_AREAS, P.tot + OSMT_TQ_AREAS, 3 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (3ull * tot[OSMT_TQ_AREAS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile batch too large for 32-bit indices (%llu areas x 3 passes): split the batch", tot[OSMT_TQ_AREAS]);
        if (tot[OSMT_TQ_OVER_AREAS] != ~0ull) {
            const size_t t = (size_t)tot[OSMT_TQ_OVER_AREAS];
            osmt_styled_tile tl;
            HIP_TRY(hipMemcpyAsync(&tl, P.tiles + t, sizeof tl, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return fail(OSMT_UNSUPPORTED, "tile %zu: %u areas (> OSMT_STYLED_MAX_TILE_AREAS = %u)", t, tl.n_areas, OSMT_STYLED_MAX_TILE_AREAS);
        }
        n_areas = (size_t)tot[OSMT_TQ_AREAS];
    } else {
        HIP_TRY(hipMemsetAsync(P.tile_base, 0, 4, st));
    }
    /* 5. emit */
    pl = pool_layout();
    (void)pl.add(n_areas * sizeof(osmt_styled_area));
    rc = wg.alloc(&kg.areas, pl, "styled areas");
    if (rc != OSMT_OK) return rc;
    P.areas = (osmt_styled_area*)kg.areas;
    if (n_tiles) {
        HIP_TRY(wg.mark(EV_EMIT0));
        HIP_TRY(osmt_launch_tq_emit(P, st));
        HIP_TRY(wg.mark(EV_EMIT1));
    }
    styled_src in;
    in.tiles = P.tiles;
    in.tile_base = P.tile_base;
    in.areas = P.areas;
    in.n_tiles = n_tiles, in.total = n_areas;
    in.scale = b->scale, in.use_caps = b->use_caps_for_dashes ? 1u : 0u;
    rc = styled_build_back(ctx, st, geo, ss, in, out_scene);
    if (rc != OSMT_OK) return rc;
    osmt_scene* s = *out_scene;
    s->d_tq = kg.head;
    s->d_tq_areas_buf = kg.areas;
    s->d_tq_tiles = P.tiles;
    s->d_tq_areas = P.areas;
    s->n_tq_areas = n_areas;
    s->h_tq_tiles.assign(b->tiles, b->tiles + n_tiles);
    s->tq_geodata_id = b->geodata_id;
    s->tq_filter = flt;
    kg.head = kg.areas = nullptr;
    if (trace && n_tiles) {
        fprintf(stderr,
                "osmt tile query: span %.1f us, columns %.1f us, gather %.1f us, sort %.1f us, mark + scan %.1f us, emit %.1f us (%zu tiles, %zu items, "
                "%zu + %zu candidates, at most %llu of one kind in a tile, %zu areas, at most %llu in a tile, %zu bytes sent)\n",
                wg.us(EV_SPAN0, EV_SPAN1), wg.us(EV_COL0, EV_COL1), wg.us(EV_GATHER0, EV_SORT0), wg.us(EV_SORT0, EV_MARK0), wg.us(EV_MARK0, EV_MARK1),
                wg.us(EV_EMIT0, EV_EMIT1), n_tiles, n_items, n_way_cand, n_mp_cand, tot[OSMT_TQ_MAX_CAND], n_areas, tot[OSMT_TQ_MAX_AREAS],
                n_tiles * sizeof(osmt_query_tile) + sizeof bind);
    }
    return OSMT_OK;
}

}  // namespace osmt_host

namespace {

int scene_read_styled_areas_body(osmt_ctx* ctx, osmt_scene* sc, osmt_styled_tile* tiles, osmt_styled_area* areas, size_t areas_cap, size_t* n_areas) {
    if (!ctx || !sc || !n_areas) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (!sc->d_tq) return fail(OSMT_INVALID_ARG, "the scene was not built by osmt_scene_build_tiles: it has no derived styled batch");
    *n_areas = sc->n_tq_areas;
    if (areas && areas_cap < sc->n_tq_areas) return fail(OSMT_INVALID_ARG, "areas_cap %zu is less than the scene's %zu areas", areas_cap, sc->n_tq_areas);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    if (tiles && sc->n_jobs) HIP_TRY(copy_back(ctx, tiles, sc->d_tq_tiles, (size_t)sc->n_jobs * sizeof(osmt_styled_tile)));
    if (areas && sc->n_tq_areas) HIP_TRY(copy_back(ctx, areas, sc->d_tq_areas, sc->n_tq_areas * sizeof(osmt_styled_area)));
    return OSMT_OK;
}

int scene_read_display_list_body(osmt_ctx* ctx, osmt_scene* sc, osmt_tile_job* jobs, osmt_op* ops, osmt_ring* rings, uint32_t* refs, double* dashes,
                                 size_t counts[5]) {
    if (!ctx || !sc || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    const bool nr = sc->coord_kind == OSMT_COORD_NODE_REF;
    counts[0] = sc->n_jobs, counts[1] = sc->n_ops, counts[2] = sc->n_rings, counts[3] = nr ? sc->n_pts : 0, counts[4] = sc->n_dashes;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    if (jobs) HIP_TRY(copy_back(ctx, jobs, sc->d_jobs, (size_t)sc->n_jobs * sizeof(osmt_tile_job)));
    if (ops) HIP_TRY(copy_back(ctx, ops, sc->d_ops, (size_t)sc->n_ops * sizeof(osmt_op)));
    if (rings) HIP_TRY(copy_back(ctx, rings, sc->d_rings, (size_t)sc->n_rings * sizeof(osmt_ring)));
    if (refs && nr) HIP_TRY(copy_back(ctx, refs, sc->d_node_refs, (size_t)sc->n_pts * 4));
    if (dashes) HIP_TRY(copy_back(ctx, dashes, sc->d_dashes, (size_t)sc->n_dashes * 8));
    return OSMT_OK;
}

/* ---- the id filter: filter_entities_by_ids (reader.rs:254-262) as three bit-planes ---- */
/* geo (optional): the file's record at the time of the call */
int validate_id_filter(const uint64_t* ids, size_t n, uint32_t geodata_id, osmt_ctx* ctx, osmt_ctx::geodata_host* geo) {
    if (n >= 0x80000000ull) return fail(OSMT_INVALID_ARG, "id filter: %zu ids (at most 2^31 - 1)", n);
    if (n && !ids) return fail(OSMT_INVALID_ARG, "id filter: ids is NULL with n = %zu", n);
    if (!ctx) return fail(OSMT_INVALID_ARG, "id filter: geodata id %u is not registered (no context)", geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size()) return fail(OSMT_INVALID_ARG, "id filter: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    if (geo) *geo = ctx->geodata[geodata_id];
    return OSMT_OK;
}

int register_id_filter_body(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* ids, size_t n, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx::geodata_host geo;
    const int rc = validate_id_filter(ids, n, geodata_id, ctx, &geo);
    if (rc != OSMT_OK) return rc;
    /* once per filter and small: the host sorts and dedups, the device bisects */
    {
        std::lock_guard<std::mutex> lk(ctx->mu); /* judged before any device work; once more where the filter is appended */
        if (ctx->id_filters.size() + 1 >= 0xFFFFFFFFull)
            return fail(OSMT_INVALID_ARG, "id filter: the context holds %zu filters already (at most 2^32 - 2)", ctx->id_filters.size());
    }
    const std::vector<uint64_t> set = osmt::id_filter_set(ids, n);
    const bool nodes = geo.d_node_index != nullptr; /* the nodes' global ids come with the node index */
    const size_t count[3] = {geo.n_ways, geo.n_mps, nodes ? geo.n_nodes : 0};
    for (size_t c : count)
        if (c >= 0xFFFFFF00ull) return fail(OSMT_UNSUPPORTED, "id filter: %zu entities of one kind do not fit 32-bit indices", c);
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    const size_t o_ids = pl.add(set.size() * 8);
    size_t o_plane[3], words[3]; /* 32-bit words: whole 64-bit words of the kernel */
    for (int k = 0; k < 3; ++k) words[k] = (count[k] + 63) / 64 * 2, o_plane[k] = pl.add(words[k] * 4);
    table_upload up("id filter", pl);
    char* pool = up.pool;
    if (up.done() != OSMT_OK) return up.done();
    if (poison_alloc()) HIP_TRY(dev_poison(ctx, pool, pl.size())); /* the planes are written by k_idf_plane alone */
    up.put(o_ids, set.data(), set.size() * 8);
    if (up.done() != OSMT_OK) return up.done();
    {
        hipStream_t st = nullptr;
        HIP_TRY(stream_acquire(ctx, &st));
        const uint64_t* d_ids = (const uint64_t*)(pool + o_ids);
        hipEvent_t ev[2] = {nullptr, nullptr}; /* OSMT_TRACE_UPLOAD=1 (diagnostic): the device time of the three planes */
        const bool trace = trace_upload() && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
        if (trace) (void)hipEventRecord(ev[0], st);
        hipError_t e = osmt_launch_idf_plane(geo.dev.way_gid, (uint32_t)count[0], d_ids, (uint32_t)set.size(), (uint32_t*)(pool + o_plane[0]), st);
        if (e == hipSuccess) e = osmt_launch_idf_plane(geo.dev.mp_gid, (uint32_t)count[1], d_ids, (uint32_t)set.size(), (uint32_t*)(pool + o_plane[1]), st);
        if (e == hipSuccess && nodes) e = osmt_launch_idf_plane(geo.d_node_gid, (uint32_t)count[2], d_ids, (uint32_t)set.size(), (uint32_t*)(pool + o_plane[2]), st);
        if (trace) (void)hipEventRecord(ev[1], st);
        const hipError_t es = hipStreamSynchronize(st); /* the table is complete before anyone can name it */
        float ms = 0.f;
        if (trace && e == hipSuccess && es == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
            fprintf(stderr, "osmt id filter: planes %.1f us (%zu ways, %zu multipolygons, %zu nodes, %zu ids of %zu given)\n", ms * 1e3, count[0], count[1],
                    count[2], set.size(), n);
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
        stream_release(ctx, st);
        HIP_TRY(e);
        HIP_TRY(es);
    }
    osmt_ctx::id_filter_host h;
    h.geodata_id = geodata_id;
    h.d_pool = pool;
    h.way = (const uint32_t*)(pool + o_plane[0]);
    h.mp = (const uint32_t*)(pool + o_plane[1]);
    h.node = nodes ? (const uint32_t*)(pool + o_plane[2]) : nullptr;
    h.n_way_words = words[0], h.n_mp_words = words[1], h.n_node_words = words[2];
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->id_filters.size() + 1 >= 0xFFFFFFFFull) /* other threads filled the table meanwhile */
        return fail(OSMT_INVALID_ARG, "id filter: the context holds %zu filters already (at most 2^32 - 2)", ctx->id_filters.size());
    *out_id = (uint32_t)ctx->id_filters.size();
    ctx->id_filters.push_back(h);
    up.release();
    return OSMT_OK;
}

int read_id_filter_body(osmt_ctx* ctx, uint32_t filter_id, uint32_t* way_words, uint32_t* mp_words, uint32_t* node_words, const size_t* caps, size_t* counts) {
    if (!ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx::id_filter_host h;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (filter_id >= ctx->id_filters.size()) return fail(OSMT_INVALID_ARG, "id filter %u is not registered (%zu filters)", filter_id, ctx->id_filters.size());
        h = ctx->id_filters[filter_id];
    }
    counts[0] = h.n_way_words, counts[1] = h.n_mp_words, counts[2] = h.n_node_words;
    uint32_t* const out[3] = {way_words, mp_words, node_words};
    const uint32_t* const src[3] = {h.way, h.mp, h.node};
    if ((way_words || mp_words || node_words) && !caps) return fail(OSMT_INVALID_ARG, "caps is NULL");
    for (int k = 0; k < 3; ++k)
        if (out[k] && caps[k] < counts[k]) return fail(OSMT_INVALID_ARG, "caps[%d] = %zu is less than the plane's %zu words", k, caps[k], counts[k]);
    HIP_TRY(hipSetDevice(ctx->device));
    for (int k = 0; k < 3; ++k)
        if (out[k] && counts[k]) HIP_TRY(copy_back(ctx, out[k], src[k], counts[k] * 4));
    return OSMT_OK;
}

}  // namespace

int osmt_validate_id_filter(const uint64_t* ids, size_t n, uint32_t geodata_id, osmt_ctx* ctx) {
    return guarded([&] { return validate_id_filter(ids, n, geodata_id, ctx, nullptr); });
}
int osmt_register_id_filter(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* ids, size_t n, uint32_t* out_filter_id) {
    return guarded([&] { return register_id_filter_body(ctx, geodata_id, ids, n, out_filter_id); });
}
int osmt_read_id_filter(osmt_ctx* ctx, uint32_t filter_id, uint32_t* way_words, uint32_t* mp_words, uint32_t* node_words, const size_t caps[3],
                        size_t counts[3]) {
    return guarded([&] { return read_id_filter_body(ctx, filter_id, way_words, mp_words, node_words, caps, counts); });
}

int osmt_validate_geodata(const osmt_geodata_desc* geodata) {
    return guarded([&] { return validate_geodata(geodata); });
}
int osmt_register_geodata(osmt_ctx* ctx, const osmt_geodata_desc* geodata, uint32_t* out_geodata_id) {
    return guarded([&] { return register_geodata_body(ctx, geodata, out_geodata_id); });
}
int osmt_validate_styles(const osmt_style_rec* styles, size_t n, const double* dashes, size_t n_dashes, osmt_ctx* ctx) {
    return guarded([&] { return validate_styles(styles, n, dashes, n_dashes, ctx_image_count(ctx)); });
}
int osmt_register_styles(osmt_ctx* ctx, const osmt_style_rec* styles, size_t n, const double* dashes, size_t n_dashes, uint32_t* out_first_style_id) {
    return guarded([&] { return register_styles_body(ctx, styles, n, dashes, n_dashes, out_first_style_id); });
}
int osmt_validate_styled_batch(const osmt_styled_batch* batch, osmt_ctx* ctx) {
    return guarded([&] { return validate_styled_batch(batch, ctx, nullptr); });
}
int osmt_scene_build_styled(osmt_ctx* ctx, const osmt_styled_batch* batch, osmt_scene** out_scene) {
    return guarded([&] { return scene_build_styled_body(ctx, batch, out_scene); });
}
int osmt_validate_tile_index(const osmt_tile_index_desc* index, size_t n_ways, size_t n_multipolygons) {
    return guarded([&] { return validate_tile_index(index, n_ways, n_multipolygons); });
}
int osmt_register_tile_index(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tile_index_desc* index) {
    return guarded([&] { return register_tile_index_body(ctx, geodata_id, index); });
}
int osmt_validate_style_bindings(const osmt_style_bindings_desc* b, osmt_ctx* ctx) {
    return guarded([&] { return validate_style_bindings(b, ctx); });
}
int osmt_register_style_bindings(osmt_ctx* ctx, const osmt_style_bindings_desc* b, uint32_t* out_bindings_id) {
    return guarded([&] { return register_style_bindings_body(ctx, b, out_bindings_id); });
}
int osmt_validate_tile_batch(const osmt_tile_batch* batch, osmt_ctx* ctx) {
    return guarded([&] { return validate_tile_batch(batch, ctx, nullptr); });
}
int osmt_scene_build_tiles(osmt_ctx* ctx, const osmt_tile_batch* batch, osmt_scene** out_scene) {
    return guarded([&] { return scene_build_tiles_body(ctx, batch, OSMT_ID_FILTER_NONE, out_scene); });
}
int osmt_scene_build_tiles_filtered(osmt_ctx* ctx, const osmt_tile_batch* batch, uint32_t filter_id, osmt_scene** out_scene) {
    return guarded([&] { return scene_build_tiles_body(ctx, batch, filter_id, out_scene); });
}
int osmt_scene_read_styled_areas(osmt_ctx* ctx, osmt_scene* scene, osmt_styled_tile* tiles, osmt_styled_area* areas, size_t areas_cap,
                                 size_t* n_areas) {
    return guarded([&] { return scene_read_styled_areas_body(ctx, scene, tiles, areas, areas_cap, n_areas); });
}
int osmt_scene_read_display_list(osmt_ctx* ctx, osmt_scene* scene, osmt_tile_job* jobs, osmt_op* ops, osmt_ring* rings, uint32_t* node_refs,
                                 double* dashes, size_t counts[5]) {
    return guarded([&] { return scene_read_display_list_body(ctx, scene, jobs, ops, rings, node_refs, dashes, counts); });
}
int osmt_scene_max_tile_ops(osmt_ctx* ctx, osmt_scene* scene, uint32_t* out_max_ops) {
    return guarded([&] {
        if (!ctx || !scene || !out_max_ops) return fail(OSMT_INVALID_ARG, "NULL argument");
        *out_max_ops = scene->max_job_ops;
        return (int)OSMT_OK;
    });
}

/* Glyph-run labels, first half: validates the instances, builds the (label, instance) pairs in label order, runs the
 * count pass and reads back each label's window summary (osmt_label_extent, ~20 bytes per label) and the error word.
 * *gtmp: the device buffer the emit pass still needs (the caller frees it after synchronising `st`).
 * Exactly one of gb (instances from the host) and tb (text runs: k_text_place writes the instances into sc->d_text_inst,
 * in front of the count pass on the same stream; tb has passed osmt::validate_text_labels) is given.
 * String labels come as tb too — the runs the validation built, tb->glyphs NULL, tb->n_glyphs the number of chars — with
 * the code points (chars) and the font id of every label (label_font): k_text_shape writes the records k_text_place
 * reads into sc->d_text_glyphs, in front of it on the same stream. */
static int glyph_labels_count(osmt_ctx* ctx, osmt_scene* sc, const osmt_glyph_label_batch* gb, const osmt_text_label_batch* tb, hipStream_t st,
                              char** gtmp, osmt_glyph_pass* gp, std::vector<osmt_label_extent>& ext, const uint32_t* chars = nullptr,
                              const uint32_t* label_font = nullptr) {
    glyph_snapshot snap;
    {
        const int rc = sync_glyphs(ctx, &snap);
        if (rc != OSMT_OK) return rc;
    }
    font_snapshot fsnap;
    if (label_font) {
        const int rc = sync_fonts(ctx, &fsnap);
        if (rc != OSMT_OK) return rc;
    }
    const osmt_label* const labels = gb ? gb->labels : tb->labels;
    const size_t n_labels = gb ? gb->n_labels : tb->n_labels, n_glyphs = gb ? gb->n_glyphs : tb->n_glyphs;
    for (size_t i = 0; gb && i < n_glyphs; ++i) {
        const osmt_glyph_instance& g = gb->glyphs[i];
        if (g.glyph_id >= snap.n) return fail(OSMT_INVALID_ARG, "glyph instance %zu: glyph id %u is not in the glyph table (%u glyphs)", i, g.glyph_id, snap.n);
        if (g.form != OSMT_GLYPH_CENTER && g.form != OSMT_GLYPH_LINE) return fail(OSMT_INVALID_ARG, "glyph instance %zu: unknown form %u", i, g.form);
        const int n_p = g.form == OSMT_GLYPH_LINE ? 6 : 2;
        bool finite = std::isfinite(g.scale);
        for (int k = 0; k < n_p; ++k) finite = finite && std::isfinite(g.p[k]);
        if (!finite) return fail(OSMT_INVALID_ARG, "glyph instance %zu: scale or placement not finite", i);
    }
    std::vector<uint32_t> pair_inst, pair_label;
    for (size_t l = 0; l < n_labels; ++l) {
        const osmt_label& in = labels[l];
        if (!in.has_text || in.n_segs == 0) continue;
        if ((size_t)in.seg_off + in.n_segs > n_glyphs) return fail(OSMT_INVALID_ARG, "label %zu: glyph instance range out of bounds", l);
        if (pair_inst.size() + in.n_segs >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "too many glyph instances");
        for (uint32_t k = 0; k < in.n_segs; ++k) {
            if (tb && !label_font && tb->glyphs[(size_t)in.seg_off + k].glyph_id >= snap.n)
                return fail(OSMT_INVALID_ARG, "label %zu, glyph %u: glyph id %u is not in the glyph table (%u glyphs)", l, k,
                            tb->glyphs[(size_t)in.seg_off + k].glyph_id, snap.n);
            pair_inst.push_back(in.seg_off + k);
            pair_label.push_back((uint32_t)l);
        }
    }
    const size_t n_pairs = pair_inst.size();
    pool_layout pl;
    const size_t o_inst = pl.add(gb ? n_glyphs * sizeof(osmt_glyph_instance) : 0);
    /* text runs: what k_text_place reads */
    const size_t n_way = tb ? tb->n_way_pts : 0;
    const size_t o_tlab = pl.add(tb ? n_labels * sizeof(osmt_label) : 0), o_trun = pl.add(tb ? n_labels * sizeof(osmt_text_run) : 0);
    const size_t o_tgl = pl.add(tb && !label_font ? n_glyphs * sizeof(osmt_text_glyph) : 0), o_twp = pl.add(n_way * 8), o_tws = pl.add(n_way * 16);
    /* string labels: what k_text_shape reads */
    const size_t o_chr = pl.add(label_font ? n_glyphs * 4 : 0), o_lfn = pl.add(label_font ? n_labels * 4 : 0);
    const size_t o_pi = pl.add(n_pairs * 4), o_pl = pl.add(n_pairs * 4), o_pc = pl.add(n_pairs * 4), o_pb = pl.add(n_pairs * 4);
    const size_t o_blk = pl.add((n_pairs / 1024 + 1) * 4);
    const size_t o_sum = pl.add(n_labels * sizeof(osmt_label_extent) + 4); /* the error word right behind: one read-back */
    const size_t off = pl.size();
    HIP_TRY(dev_alloc(ctx, (void**)gtmp, off));
    char* base = *gtmp;
    gp->verts = snap.verts;
    gp->voff = snap.voff;
    if (tb) { /* the instances outlive this call (osmt_scene_read_glyph_instances) */
        HIP_TRY(dev_alloc(ctx, (void**)&sc->d_text_inst, std::max<size_t>(n_glyphs, 1) * sizeof(osmt_glyph_instance)));
        gp->inst = sc->d_text_inst;
    } else {
        gp->inst = (const osmt_glyph_instance*)(base + o_inst);
    }
    gp->pair_inst = (const uint32_t*)(base + o_pi);
    gp->pair_label = (const uint32_t*)(base + o_pl);
    gp->n_pairs = (uint32_t)n_pairs;
    gp->W = (int32_t)(OSMT_TILE_SIZE * sc->scale);
    gp->sum = (osmt_label_extent*)(base + o_sum);
    gp->err = (uint32_t*)(base + o_sum + n_labels * sizeof(osmt_label_extent));
    gp->pair_cnt = (uint32_t*)(base + o_pc);
    gp->pair_base = (uint32_t*)(base + o_pb);
    gp->blk = (uint32_t*)(base + o_blk);
    if (gb && n_glyphs) HIP_TRY(hipMemcpyAsync(base + o_inst, gb->glyphs, n_glyphs * sizeof(osmt_glyph_instance), hipMemcpyHostToDevice, st));
    if (n_pairs) {
        HIP_TRY(hipMemcpyAsync(base + o_pi, pair_inst.data(), n_pairs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + o_pl, pair_label.data(), n_pairs * 4, hipMemcpyHostToDevice, st));
    }
    if (tb) {
        osmt_text_pass tp{};
        tp.labels = (const osmt_label*)(base + o_tlab);
        tp.n_labels = (uint32_t)n_labels;
        tp.runs = (const osmt_text_run*)(base + o_trun);
        if (label_font) { /* the records outlive this call (osmt_scene_read_text_glyphs) */
            HIP_TRY(dev_alloc(ctx, (void**)&sc->d_text_glyphs, std::max<size_t>(n_glyphs, 1) * sizeof(osmt_text_glyph)));
            tp.glyphs = sc->d_text_glyphs;
        } else {
            tp.glyphs = (const osmt_text_glyph*)(base + o_tgl);
        }
        tp.way_pts = (const int32_t*)(base + o_twp);
        tp.way_sincos = (const double*)(base + o_tws);
        tp.inst = sc->d_text_inst;
        HIP_TRY(hipMemcpyAsync(base + o_tlab, tb->labels, n_labels * sizeof(osmt_label), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + o_trun, tb->runs, n_labels * sizeof(osmt_text_run), hipMemcpyHostToDevice, st));
        if (n_glyphs && !label_font) HIP_TRY(hipMemcpyAsync(base + o_tgl, tb->glyphs, n_glyphs * sizeof(osmt_text_glyph), hipMemcpyHostToDevice, st));
        if (label_font) {
            osmt_shape_pass sp{};
            sp.labels = tp.labels;
            sp.label_font = (const uint32_t*)(base + o_lfn);
            sp.pair_inst = gp->pair_inst;
            sp.pair_label = gp->pair_label;
            sp.n_pairs = gp->n_pairs;
            sp.chars = (const uint32_t*)(base + o_chr);
            sp.fonts = fsnap.fonts;
            sp.out = sc->d_text_glyphs;
            if (n_glyphs) HIP_TRY(hipMemcpyAsync(base + o_chr, chars, n_glyphs * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(base + o_lfn, label_font, n_labels * 4, hipMemcpyHostToDevice, st));
            /* slots no label with text names read as zero */
            HIP_TRY(hipMemsetAsync(sc->d_text_glyphs, 0, std::max<size_t>(n_glyphs, 1) * sizeof(osmt_text_glyph), st));
            HIP_TRY(osmt_launch_text_shape(sp, st));
        }
        if (n_way) {
            HIP_TRY(hipMemcpyAsync(base + o_twp, tb->way_pts, n_way * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(base + o_tws, tb->way_sincos, n_way * 16, hipMemcpyHostToDevice, st));
        }
        /* slots no label with text names read as zero */
        HIP_TRY(hipMemsetAsync(sc->d_text_inst, 0, std::max<size_t>(n_glyphs, 1) * sizeof(osmt_glyph_instance), st));
        HIP_TRY(osmt_launch_text_place(tp, st));
    }
    HIP_TRY(osmt_launch_glyph_count(*gp, (uint32_t)n_labels, st));
    std::vector<char> back(n_labels * sizeof(osmt_label_extent) + 4);
    HIP_TRY(hipMemcpyAsync(back.data(), gp->sum, back.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st)); /* also: pair_inst / pair_label may be read until here */
    uint32_t err = 0;
    memcpy(&err, back.data() + n_labels * sizeof(osmt_label_extent), 4);
    if (err & OSMT_GLYPH_ERR_COORD) return fail(OSMT_UNSUPPORTED, "glyph labels: a draw_line coordinate is not finite or |v| > 2^20");
    if (err & OSMT_GLYPH_ERR_DEPTH)
        return fail(OSMT_UNSUPPORTED, "glyph labels: a curve needs more than %d levels of subdivision", OSMT_QUAD_MAX_DEPTH);
    if (err) return fail(OSMT_HIP_ERROR, "glyph count pass: internal error %u", err);
    ext.resize(n_labels);
    memcpy(ext.data(), back.data(), n_labels * sizeof(osmt_label_extent));
    return OSMT_OK;
}

/* Drawer::draw_labels (drawer.rs:221-262) as data: validates, sizes each label's coverage window and
 * uploads.  Window of a label = stripes its draw_line calls can create inside labels_bb's rows
 * (tile_pixels.rs:67-72) x every column those stripes can hold a key in (+-2 cells of slack for the
 * rounding of eval_x_at_y, font/rasterizer.rs:37).  Exactly one of lb (draw_line calls from the host) and gb (glyph
 * runs, expanded on the device) is used; both feed the same per-label summaries (osmt_label_extent) to the window code. */
static int osmt_scene_set_labels_body(osmt_ctx* ctx, osmt_scene* sc, const osmt_label_batch* lb, const osmt_glyph_label_batch* gb = nullptr,
                                      const osmt_text_label_batch* tb = nullptr, const osmt_string_label_batch* sb = nullptr) {
    if (!ctx || !sc || sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "bad ctx/scene");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = sc->own_stream;
    hipStream_t pooled = nullptr; /* public scene: copies on a private stream, complete on return (never the NULL stream) */
    if (!st) {
        HIP_TRY(stream_acquire(ctx, &pooled));
        st = pooled;
    }
    struct release_pooled {
        osmt_ctx* c;
        hipStream_t s;
        ~release_pooled() {
            if (s) {
                (void)hipStreamSynchronize(s);
                stream_release(c, s);
            }
        }
    } pooled_guard{ctx, pooled};
    HIP_TRY(scene_wait_idle(sc)); /* the previous label pass of THIS scene may still be in flight; nobody else is waited for */
    dev_free(ctx, sc->d_lab_base);
    sc->d_lab_base = nullptr;
    sc->n_labels = sc->n_label_segs = 0;
    sc->lab_cover_valid = false;
    dev_free(ctx, sc->d_text_inst);
    sc->d_text_inst = nullptr;
    sc->n_text_inst = 0;
    dev_free(ctx, sc->d_text_glyphs);
    sc->d_text_glyphs = nullptr;
    sc->n_text_glyphs = 0;
    /* string labels: validated here, then carried as text runs whose glyph records the device writes itself */
    std::vector<osmt_text_run> s_runs;
    std::vector<uint32_t> s_font;
    osmt_text_label_batch s_tb{};
    if (sb) {
        if (sb->n_labels == 0) return OSMT_OK;
        std::vector<std::shared_ptr<osmt_ctx::font_host>> keep;
        const std::vector<const osmt_font_desc*> fonts = font_views(ctx, &keep);
        std::string why;
        const int rc = osmt::validate_string_labels(sb, sc->n_jobs, fonts.data(), fonts.size(), &why, &s_runs);
        if (rc != OSMT_OK) return fail(rc, "%s", why.c_str());
        s_font.assign(sb->n_labels, 0u);
        for (size_t l = 0; l < sb->n_labels; ++l)
            if (sb->labels[l].has_text) s_font[l] = sb->runs[l].font_id;
        s_tb.labels = sb->labels;
        s_tb.n_labels = sb->n_labels;
        s_tb.job_label_off = sb->job_label_off;
        s_tb.runs = s_runs.data();
        s_tb.n_glyphs = sb->n_chars;
        s_tb.way_pts = sb->way_pts;
        s_tb.way_sincos = sb->way_sincos;
        s_tb.n_way_pts = sb->n_way_pts;
        tb = &s_tb;
    }
    const osmt_label* const labels = lb ? lb->labels : gb ? gb->labels : tb ? tb->labels : nullptr;
    const size_t n_labels = lb ? lb->n_labels : gb ? gb->n_labels : tb ? tb->n_labels : 0;
    const uint32_t* const job_label_off = lb ? lb->job_label_off : gb ? gb->job_label_off : tb ? tb->job_label_off : nullptr;
    if (n_labels == 0) return OSMT_OK;
    if (tb && !sb) {
        std::string why;
        const int rc = osmt::validate_text_labels(tb, sc->n_jobs, &why);
        if (rc != OSMT_OK) return fail(rc, "%s", why.c_str());
    }
    if (!labels || !job_label_off || (lb && lb->n_segs && !lb->segs) || (gb && gb->n_glyphs && !gb->glyphs))
        return fail(OSMT_INVALID_ARG, "NULL label pool");
    if (n_labels >= 0xFFFFFFFFull || (lb ? lb->n_segs : gb ? gb->n_glyphs : tb->n_glyphs) >= 0xFFFFFFFFull)
        return fail(OSMT_INVALID_ARG, "label batch too large");
    if (job_label_off[0] != 0 || job_label_off[sc->n_jobs] != n_labels)
        return fail(OSMT_INVALID_ARG, "job_label_off must run from 0 to n_labels over n_jobs + 1 entries");
    for (uint32_t j = 0; j < sc->n_jobs; ++j)
        if (job_label_off[j] > job_label_off[j + 1]) return fail(OSMT_INVALID_ARG, "job_label_off is not monotonic");
    const double LIM = 1048576.0; /* 2^20 */
    if (lb)
        for (size_t i = 0; i < 4 * lb->n_segs; ++i)
            if (!(std::fabs(lb->segs[i]) <= LIM)) return fail(OSMT_UNSUPPORTED, "label segment %zu: coordinate not finite or |v| > 2^20", i / 4);
    /* glyph runs: the count pass on the device gives every label's summary; the emit pass (below, once the arena is
     * carved) writes the calls.  gtmp lives until the emit pass has run. */
    std::vector<osmt_label_extent> gext;
    std::vector<uint32_t> gseg_off;
    osmt_glyph_pass gp{};
    struct tmp_guard {
        osmt_ctx* c;
        hipStream_t s;
        char* p;
        ~tmp_guard() {
            if (p) {
                (void)hipStreamSynchronize(s);
                dev_free(c, p);
            }
        }
    } gtmp{ctx, st, nullptr};
    /* text runs: the instances stay with the scene only if the whole call succeeds */
    struct inst_guard {
        osmt_ctx* c;
        osmt_scene* s;
        hipStream_t st;
        bool keep;
        ~inst_guard() {
            if (!keep && (s->d_text_inst || s->d_text_glyphs)) {
                (void)hipStreamSynchronize(st);
                dev_free(c, s->d_text_inst);
                dev_free(c, s->d_text_glyphs);
                s->d_text_inst = nullptr;
                s->d_text_glyphs = nullptr;
            }
        }
    } text_inst{ctx, sc, st, false};
    size_t n_segs_total = lb ? lb->n_segs : 0;
    if (!lb) {
        const int rc = glyph_labels_count(ctx, sc, gb, tb, st, &gtmp.p, &gp, gext, sb ? sb->chars : nullptr, sb ? s_font.data() : nullptr);
        if (rc != OSMT_OK) return rc;
        gseg_off.resize(n_labels);
        for (size_t l = 0; l < n_labels; ++l) {
            gseg_off[l] = (uint32_t)n_segs_total;
            n_segs_total += gext[l].n_segs;
            if (n_segs_total >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "glyph labels expand to more than 2^32 draw_line calls");
        }
    }

    std::vector<osmt_image_desc> images;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        images = ctx->images;
    }
    const int32_t W = (int32_t)(OSMT_TILE_SIZE * sc->scale);
    std::vector<osmt_labelinfo>& info = sc->h_lab_info; /* kept alive: the upload may be stream-ordered */
    std::vector<uint32_t>& wide = sc->h_lab_wide;
    std::vector<osmt_label_band>& bands = sc->h_lab_bands;
    bands.clear();
    info.assign(n_labels, osmt_labelinfo{});
    wide.clear();
    size_t cells = 0, wide_cells = 0, bit_words = 0; /* bit_words < cells / 64 + bands <= 2^26 */
    for (uint32_t j = 0; j < sc->n_jobs; ++j) {
        for (uint32_t l = job_label_off[j]; l < job_label_off[j + 1]; ++l) {
            const osmt_label& in = labels[l];
            osmt_labelinfo& o = info[l];
            memset(&o, 0, sizeof o);
            o.ry0 = 1;
            o.ry1 = 0;
            if (in.has_icon && in.image_id < images.size()) { /* icon missing from the cache: Some(0), no blit (labeler.rs:64-66) */
                if (!(std::fabs(in.icon_center_x) <= LIM) || !(std::fabs(in.icon_center_y) <= LIM))
                    return fail(OSMT_UNSUPPORTED, "label %u: icon centre not finite or |v| > 2^20", l);
                const osmt_image_desc& im = images[in.image_id];
                o.icon_w = im.width;
                o.icon_h = im.height;
                o.icon_off = im.offset;
                o.icon_x = (int32_t)(in.icon_center_x - ((double)im.width / 2.0)); /* get_start_coord (labeler.rs:92-95) */
                o.icon_y = (int32_t)(in.icon_center_y - ((double)im.height / 2.0));
            }
            o.has_text = in.has_text ? 1 : 0;
            memcpy(o.color, in.text_color, 3);
            if (!in.has_text || in.n_segs == 0) continue;
            osmt_label_extent ext;
            if (lb) {
                if ((size_t)in.seg_off + in.n_segs > lb->n_segs) return fail(OSMT_INVALID_ARG, "label %u: segment range out of bounds", l);
                o.seg_off = in.seg_off;
                osmt_label_extent_init(&ext);
                for (uint32_t k = 0; k < in.n_segs; ++k) {
                    const double* q = lb->segs + 4 * ((size_t)in.seg_off + k);
                    osmt_label_extent_add(&ext, q[0], q[1], q[2], q[3], W);
                }
            } else {
                ext = gext[l];
                if (ext.n_segs == 0) continue; /* blanks only: a text that drew nothing */
                o.seg_off = gseg_off[l];
            }
            o.n_segs = ext.n_segs;
            const int32_t ry0 = ext.ry0, ry1 = ext.ry1, cx0 = ext.cx0, cx1 = ext.cx1;
            if (ry0 > ry1) continue;
            const size_t rows = (size_t)(ry1 - ry0 + 1), cols = (size_t)(cx1 - cx0 + 1);
            if (rows * cols > ((size_t)1 << 24))
                return fail(OSMT_UNSUPPORTED, "label %u: coverage window of %zu x %zu cells is too large", l, cols, rows);
            o.ry0 = ry0;
            o.ry1 = ry1;
            o.cx0 = cx0;
            o.cols = (uint32_t)cols;
            o.plane_off = cells;
            cells += rows * cols;
            if (cols > OSMT_LABEL_LDS_CELLS) {
                if (wide_cells + 64 * cols >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "too many wide label windows");
                o.wide_off = (uint32_t)wide_cells;
                wide_cells += 64 * cols;
                wide.push_back(l);
            } else {
                const uint32_t band_rows = osmt_label_band_rows((uint32_t)cols);
                o.wide_off = (uint32_t)bit_words;
                for (uint32_t rb = 0; rb < rows; rb += band_rows) {
                    bands.push_back(osmt_label_band{l, rb});
                    bit_words += osmt_label_band_words((uint32_t)cols);
                }
            }
        }
    }
    if (cells > ((size_t)1 << 31)) return fail(OSMT_UNSUPPORTED, "label coverage windows need %zu cells (> 2^31)", cells);
    /* every band scans all of its label's draw_line calls: longest first (ties keep draw order) */
    std::stable_sort(bands.begin(), bands.end(),
                     [&](const osmt_label_band& a, const osmt_label_band& b) { return info[a.label].n_segs > info[b.label].n_segs; });
    /* workgroup b runs on XCD b mod 8, each with an L2 of its own: the bands of one label (neighbours in the sorted
     * list, all reading the same draw_line calls) are dealt to ONE residue class, G at a time, so that the calls come
     * from HBM once and from that XCD's L2 for the other bands */
    {
        constexpr size_t G = 16, CH = 8 * G;
        std::vector<osmt_label_band> dealt(bands.size());
        const size_t full = bands.size() / CH * CH;
        for (size_t i = 0; i < full; ++i) {
            const size_t c = i / CH, j = i % CH;
            dealt[c * CH + (j % G) * 8 + j / G] = bands[i];
        }
        for (size_t i = full; i < bands.size(); ++i) dealt[i] = bands[i];
        bands.swap(dealt);
    }

    pool_layout pl;
    const size_t EW = 3 * (size_t)W;
    const size_t words = (EW * EW + 31) / 32;
    const size_t o_info = pl.add(n_labels * sizeof(osmt_labelinfo));
    const size_t o_off = pl.add(((size_t)sc->n_jobs + 1) * 4);
    const size_t o_segs = pl.add(n_segs_total * 32);
    const size_t o_a = pl.add((cells + 1) * 8);
    const size_t o_s = pl.add((wide_cells + 1) * 8);
    const size_t o_bits = pl.add((bit_words + 2) * 8); /* + the word a funnel read may touch behind the last stream */
    const size_t o_wide = pl.add((wide.size() + 1) * 4);
    const size_t o_bands = pl.add((bands.size() + 1) * sizeof(osmt_label_band));
    const size_t o_bm = pl.add(words * 4 <= 96 * 1024 ? 4 : (size_t)sc->n_jobs * words * 4); /* scale 1: the map lives in LDS */
    const size_t o_tl = pl.add(n_labels * sizeof(osmt_tile_label));
    const size_t o_tlc = pl.add((size_t)sc->n_jobs * 4);
    const size_t o_ok = pl.add(n_labels);
    const size_t o_err = pl.add(4);
    hipError_t e = dev_alloc(ctx, (void**)&sc->d_lab_base, pl.size() + 256);
    if (e != hipSuccess) {
        sc->d_lab_base = nullptr;
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) for labels failed: %s", pl.size(),
                    hipGetErrorString(e));
    }
    char* base = sc->d_lab_base;
    sc->d_lab = (osmt_labelinfo*)(base + o_info);
    sc->d_job_label_off = (uint32_t*)(base + o_off);
    sc->d_lab_segs = (double*)(base + o_segs);
    sc->d_lab_a = (double*)(base + o_a);
    sc->d_lab_s_wide = (double*)(base + o_s);
    sc->d_lab_bits = (unsigned long long*)(base + o_bits);
    sc->d_lab_wide = (uint32_t*)(base + o_wide);
    sc->n_lab_wide = (uint32_t)wide.size();
    sc->d_lab_bands = (osmt_label_band*)(base + o_bands);
    sc->n_lab_bands = (uint32_t)bands.size();
    sc->d_tile_labels = (osmt_tile_label*)(base + o_tl);
    sc->d_tile_label_cnt = (uint32_t*)(base + o_tlc);
    sc->d_lab_bitmap = (uint32_t*)(base + o_bm);
    sc->d_lab_ok = (uint8_t*)(base + o_ok);
    sc->d_lab_err = (uint32_t*)(base + o_err);
    auto up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (!bytes) return hipSuccess;
        return st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    e = up(sc->d_lab, info.data(), info.size() * sizeof(osmt_labelinfo));
    if (e == hipSuccess) e = up(sc->d_job_label_off, job_label_off, ((size_t)sc->n_jobs + 1) * 4);
    if (e == hipSuccess && lb) e = up(sc->d_lab_segs, lb->segs, lb->n_segs * 32);
    if (e == hipSuccess && !lb) { /* the glyph runs' calls, written straight into the arena */
        gp.segs = sc->d_lab_segs;
        gp.n_segs = (uint32_t)n_segs_total;
        e = osmt_launch_glyph_emit(gp, st);
    }
    if (e == hipSuccess) e = up(sc->d_lab_wide, wide.data(), wide.size() * 4);
    if (e == hipSuccess) e = up(sc->d_lab_bands, bands.data(), bands.size() * sizeof(osmt_label_band));
    /* The verdicts and the error word are cleared by the label stage itself, on the render stream (osmt_launch_labels).
     * Until the first render with these labels they read "no label has been placed, no error": a status read between
     * osmt_scene_set_labels and the next render used to return whatever the recycled buffer held (found by the poisoned
     * allocator in round 5: error word 0xA5A5A5A5). */
    if (e == hipSuccess)
        e = st ? hipMemsetAsync(base + o_ok, 0, o_err + 4 - o_ok, st) : hipMemset(base + o_ok, 0, o_err + 4 - o_ok);
    if (e != hipSuccess) {
        dev_free(ctx, sc->d_lab_base);
        sc->d_lab_base = nullptr;
        return fail(OSMT_HIP_ERROR, "label upload failed: %s", hipGetErrorString(e));
    }
    if (!lb) { /* the emit pass's own check (a call beyond the arena the count pass sized): a 4-byte read-back */
        uint32_t err = 0;
        e = hipMemcpyAsync(&err, gp.err, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess || err) {
            dev_free(ctx, sc->d_lab_base);
            sc->d_lab_base = nullptr;
            return e != hipSuccess ? fail(OSMT_HIP_ERROR, "glyph emit pass failed: %s", hipGetErrorString(e))
                                   : fail(OSMT_HIP_ERROR, "glyph emit pass: internal error %u", err);
        }
    }
    sc->n_labels = (uint32_t)n_labels;
    sc->n_label_segs = (uint32_t)n_segs_total;
    if (tb) {
        sc->n_text_inst = (uint32_t)tb->n_glyphs;
        if (sb) sc->n_text_glyphs = (uint32_t)sb->n_chars;
        text_inst.keep = true;
    }
    return OSMT_OK;
}

int osmt_scene_set_labels(osmt_ctx* ctx, osmt_scene* sc, const osmt_label_batch* lb) {
    return guarded([&] { return osmt_scene_set_labels_body(ctx, sc, lb); });
}

int osmt_scene_set_glyph_labels(osmt_ctx* ctx, osmt_scene* sc, const osmt_glyph_label_batch* gb) {
    return guarded([&] { return osmt_scene_set_labels_body(ctx, sc, nullptr, gb); });
}

int osmt_scene_set_text_labels(osmt_ctx* ctx, osmt_scene* sc, const osmt_text_label_batch* tb) {
    return guarded([&] { return osmt_scene_set_labels_body(ctx, sc, nullptr, nullptr, tb); });
}

int osmt_validate_text_labels(const osmt_text_label_batch* tb, size_t n_jobs) {
    return guarded([&] {
        std::string why;
        const int rc = osmt::validate_text_labels(tb, n_jobs, &why);
        return rc == OSMT_OK ? OSMT_OK : fail(rc, "%s", why.c_str());
    });
}

int osmt_scene_set_string_labels(osmt_ctx* ctx, osmt_scene* sc, const osmt_string_label_batch* sb) {
    if (!sb) return osmt_scene_set_text_labels(ctx, sc, nullptr);
    return guarded([&] { return osmt_scene_set_labels_body(ctx, sc, nullptr, nullptr, nullptr, sb); });
}

/* ---- node labels of tile-built scenes (include/osmtile.h, csrc/osmt_tilelabels.hip) ------------------------------------ */
static int validate_node_index(const osmt_node_index_desc* x, uint32_t geodata_id, osmt_ctx* ctx, size_t* out_tiles) {
    if (!x) return fail(OSMT_INVALID_ARG, "node index is NULL");
    if (!ctx) return fail(OSMT_INVALID_ARG, "node index: geodata id %u is not registered (no context)", geodata_id);
    size_t n_nodes = 0, n_tiles = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "node index: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
        const osmt_ctx::geodata_host& g = ctx->geodata[geodata_id];
        if (!g.d_index) return fail(OSMT_INVALID_ARG, "node index: geodata id %u has no tile index (osmt_register_tile_index)", geodata_id);
        if (g.d_node_index) return fail(OSMT_INVALID_ARG, "node index: geodata id %u has a node index already (one per file)", geodata_id);
        n_nodes = g.n_nodes, n_tiles = g.ix.n_tiles;
    }
    if (x->n_nodes != n_nodes) return fail(OSMT_INVALID_ARG, "node index: n_nodes = %zu, the geodata has %zu nodes", x->n_nodes, n_nodes);
    if ((x->n_nodes && !x->node_ids) || !x->node_off || (x->n_node_refs && !x->nodes))
        return fail(OSMT_INVALID_ARG, "node index: NULL array (every offset array has at least its first entry)");
    if (x->n_node_refs >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "node index: too large for 32-bit indices");
    const int rc = check_offsets_of("node index", "node_off", x->node_off, n_tiles, x->n_node_refs);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < x->n_node_refs; ++i)
        if (x->nodes[i] >= n_nodes) return fail(OSMT_INVALID_ARG, "node index: nodes[%zu] = %u is not a node (%zu nodes)", i, x->nodes[i], n_nodes);
    if (out_tiles) *out_tiles = n_tiles;
    return OSMT_OK;
}

static int register_node_index_body(osmt_ctx* ctx, uint32_t geodata_id, const osmt_node_index_desc* x) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    size_t n = 0;
    const int rc = validate_node_index(x, geodata_id, ctx, &n);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    const size_t o_gid = pl.add(x->n_nodes * 8), o_off = pl.add((n + 1) * 4), o_refs = pl.add(x->n_node_refs * 4), o_zero = pl.add((n + 1) * 4);
    table_upload up("node index", pl);
    char* pool = up.pool;
    const std::vector<uint32_t> zeros(n + 1, 0u); /* the offsets of the empty second kind */
    up.put(o_gid, x->node_ids, x->n_nodes * 8);
    up.put(o_off, x->node_off, (n + 1) * 4);
    up.put(o_refs, x->nodes, x->n_node_refs * 4);
    up.put(o_zero, zeros.data(), (n + 1) * 4);
    if (up.done() != OSMT_OK) return up.done();
    std::lock_guard<std::mutex> lk(ctx->mu);
    osmt_ctx::geodata_host& g = ctx->geodata[geodata_id];
    if (g.d_node_index) return fail(OSMT_INVALID_ARG, "node index: geodata id %u has a node index already (one per file)", geodata_id); /* another thread was first */
    g.d_node_index = pool;
    g.d_node_gid = (const uint64_t*)(pool + o_gid);
    g.d_node_off = (const uint32_t*)(pool + o_off);
    g.d_node_refs = (const uint32_t*)(pool + o_refs);
    g.d_zero_off = (const uint32_t*)(pool + o_zero);
    up.release();
    return OSMT_OK;
}

namespace osmt_host {

int validate_label_styles(const osmt_label_style_rec* st, size_t n, osmt_ctx* ctx) {
    if (n && !st) return fail(OSMT_INVALID_ARG, "label styles are NULL");
    size_t n_images = 0, n_fonts = 0;
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        n_images = ctx->images.size(), n_fonts = ctx->fonts.size();
    }
    for (size_t i = 0; i < n; ++i) {
        const osmt_label_style_rec& s = st[i];
        if (std::isnan(s.z_index)) return fail(OSMT_INVALID_ARG, "label style %zu: z_index is NaN", i);
        if (s.has_icon && s.icon_image >= n_images)
            return fail(OSMT_INVALID_ARG, "label style %zu: icon_image %u is not registered (%zu images)", i, s.icon_image, n_images);
        if (s.text_position > OSMT_LABEL_POSITION_LINE) return fail(OSMT_INVALID_ARG, "label style %zu: unknown text_position %u", i, s.text_position);
        if (s.has_text_style && s.has_font_size) {
            if (!std::isfinite(s.font_size) || !std::isfinite(s.font_size * (double)OSMT_MAX_SCALE))
                return fail(OSMT_INVALID_ARG, "label style %zu: font_size not finite (after multiplication by %u)", i, OSMT_MAX_SCALE);
            if (s.font_id >= n_fonts) return fail(OSMT_INVALID_ARG, "label style %zu: font_id %u is not registered (%zu fonts)", i, s.font_id, n_fonts);
        }
    }
    return OSMT_OK;
}

int register_label_styles_body(osmt_ctx* ctx, const osmt_label_style_rec* st, size_t n, uint32_t* out_first) {
    if (!ctx || !out_first) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = validate_label_styles(st, n, ctx);
    if (rc != OSMT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->label_styles.size() + n >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "label style table too large");
    *out_first = (uint32_t)ctx->label_styles.size();
    ctx->label_styles.insert(ctx->label_styles.end(), st, st + n);
    if (n) ctx->label_styles_dirty = true;
    return OSMT_OK;
}

}  // namespace osmt_host

/* compare_styled_entities with for_labels (styler.rs:246-272), the part that depends on the style alone */
static int label_style_key_cmp(const osmt_label_style_rec& a, const osmt_label_style_rec& b) {
    const int64_t la = a.has_layer ? a.layer : 0, lb = b.has_layer ? b.layer : 0;
    if (la != lb) return la < lb ? -1 : 1;
    if (a.z_index != b.z_index) return a.z_index < b.z_index ? -1 : 1; /* -0.0 == +0.0; never NaN */
    return 0;
}

/* brings the device copy of the label style table up to date; the pointers stay valid for the life of the context */
static int sync_label_styles(osmt_ctx* ctx, const osmt_label_style_rec** styles, const uint32_t** rank) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->label_styles_dirty || !ctx->d_label_styles) {
        const size_t n = ctx->label_styles.size();
        std::vector<uint32_t> order(n), rk(n);
        for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return label_style_key_cmp(ctx->label_styles[x], ctx->label_styles[y]) < 0; });
        uint32_t r = 0;
        for (size_t i = 0; i < n; ++i) {
            if (i && label_style_key_cmp(ctx->label_styles[order[i - 1]], ctx->label_styles[order[i]]) != 0) ++r;
            rk[order[i]] = r;
        }
        const snap_part parts[2] = {{(void**)&ctx->d_label_styles, ctx->label_styles.data(), n * sizeof(osmt_label_style_rec), sizeof(osmt_label_style_rec)},
                                    {(void**)&ctx->d_label_rank, rk.data(), n * 4, 4}};
        const int rc = snapshot_replace(ctx, "label style table", parts, 2);
        if (rc != OSMT_OK) return rc;
        ctx->d_n_label_styles = (uint32_t)n;
        ctx->label_styles_dirty = false;
    }
    *styles = ctx->d_label_styles;
    *rank = ctx->d_label_rank;
    return OSMT_OK;
}

static int validate_label_bindings(const osmt_label_bindings_desc* b, osmt_ctx* ctx, size_t* out_nodes) {
    if (!b) return fail(OSMT_INVALID_ARG, "label bindings are NULL");
    if (b->zoom_lo > b->zoom_hi || b->zoom_hi > OSMT_MAX_ZOOM)
        return fail(OSMT_INVALID_ARG, "label bindings: zoom range %u..%u (zoom_lo <= zoom_hi <= %u)", b->zoom_lo, b->zoom_hi, OSMT_MAX_ZOOM);
    if (!ctx) return fail(OSMT_INVALID_ARG, "label bindings: geodata id %u is not registered (no context)", b->geodata_id);
    size_t n_nodes = 0, n_styles = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (b->geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "label bindings: geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
        n_nodes = ctx->geodata[b->geodata_id].n_nodes;
        n_styles = ctx->label_styles.size();
    }
    if (!b->node_off || (b->n_bindings && !b->bindings) || !b->text_off || (b->n_chars && !b->chars))
        return fail(OSMT_INVALID_ARG, "label bindings: NULL array (every offset array has at least its first entry)");
    if (b->n_bindings >= 0xFFFFFFFFull || b->n_texts >= 0xFFFFFFFFull || b->n_chars >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "label bindings: too large for 32-bit indices");
    int rc = check_offsets_of("label bindings", "node_off", b->node_off, n_nodes, b->n_bindings);
    if (rc == OSMT_OK) rc = check_offsets_of("label bindings", "text_off", b->text_off, b->n_texts, b->n_chars);
    if (rc != OSMT_OK) return rc;
    for (size_t i = 0; i < b->n_bindings; ++i) {
        if (b->bindings[i].style >= n_styles)
            return fail(OSMT_INVALID_ARG, "label bindings: bindings[%zu].style = %u is not a registered label style (%zu styles)", i, b->bindings[i].style, n_styles);
        if (b->bindings[i].text != OSMT_TEXT_NONE && b->bindings[i].text >= b->n_texts)
            return fail(OSMT_INVALID_ARG, "label bindings: bindings[%zu].text = %u is not in the text pool (%zu texts) nor OSMT_TEXT_NONE", i, b->bindings[i].text,
                        b->n_texts);
    }
    for (size_t i = 0; i < b->n_chars; ++i)
        if (!osmt::textshaper_detail::is_char(b->chars[i])) return fail(OSMT_INVALID_ARG, "label bindings: chars[%zu] = U+%X is not a Unicode scalar value", i, b->chars[i]);
    if (out_nodes) *out_nodes = n_nodes;
    return OSMT_OK;
}

static int register_label_bindings_body(osmt_ctx* ctx, const osmt_label_bindings_desc* b, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    size_t n_nodes = 0;
    const int rc = validate_label_bindings(b, ctx, &n_nodes);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    const size_t o_no = pl.add((n_nodes + 1) * 4), o_b = pl.add(b->n_bindings * sizeof(osmt_label_binding)), o_to = pl.add((b->n_texts + 1) * 4);
    const size_t o_c = pl.add(b->n_chars * 4);
    table_upload up("label bindings", pl);
    char* pool = up.pool;
    up.put(o_no, b->node_off, (n_nodes + 1) * 4);
    up.put(o_b, b->bindings, b->n_bindings * sizeof(osmt_label_binding));
    up.put(o_to, b->text_off, (b->n_texts + 1) * 4);
    up.put(o_c, b->chars, b->n_chars * 4);
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::label_bindings_host h;
    h.geodata_id = b->geodata_id, h.zoom_lo = b->zoom_lo, h.zoom_hi = b->zoom_hi;
    h.d_pool = pool;
    h.dev.node_off = (const uint32_t*)(pool + o_no);
    h.dev.bindings = (const osmt_label_binding*)(pool + o_b);
    h.dev.text_off = (const uint32_t*)(pool + o_to);
    h.dev.chars = (const uint32_t*)(pool + o_c);
    h.n_nodes = n_nodes, h.n_bindings = b->n_bindings, h.n_texts = b->n_texts, h.n_chars = b->n_chars;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->label_bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "label bindings table too large");
    *out_id = (uint32_t)ctx->label_bindings.size();
    ctx->label_bindings.push_back(h);
    up.release();
    return OSMT_OK;
}

/* the node labels of a batch as the device built them, tile behind tile */
struct node_label_batch {
    std::vector<osmt_label> labels;
    std::vector<osmt_string_run> runs;
    std::vector<uint32_t> chars, job_off;
};

/* The first half of osmt_scene_build_tile_labels: validates (the bindings, then the shape of `area`), builds the node labels on
 * the device and reads them back into `nb`.  The scene is not touched. */
static int tile_node_labels_build(osmt_ctx* ctx, osmt_scene* sc, const uint32_t* bindings_of_zoom, const osmt_string_label_batch* area,
                                  node_label_batch* nb) {
    if (!ctx || !sc || sc->ctx != ctx || !bindings_of_zoom) return fail(OSMT_INVALID_ARG, "bad ctx/scene/bindings");
    if (!sc->d_tq) return fail(OSMT_INVALID_ARG, "the scene was not built by osmt_scene_build_tiles: it has no tiles to query");
    const size_t n_tiles = sc->n_jobs;
    const std::vector<osmt_query_tile>& q = sc->h_tq_tiles;
    osmt_tl_bind_dev bind[OSMT_MAX_ZOOM + 1];
    memset(bind, 0, sizeof bind);
    osmt_ctx::geodata_host geo;
    std::vector<uint32_t> icon_h;
    {
        bool zoom_used[OSMT_MAX_ZOOM + 1] = {};
        size_t first_of_zoom[OSMT_MAX_ZOOM + 1] = {};
        for (size_t t = 0; t < n_tiles; ++t)
            if (!zoom_used[q[t].zoom]) zoom_used[q[t].zoom] = true, first_of_zoom[q[t].zoom] = t;
        std::lock_guard<std::mutex> lk(ctx->mu);
        geo = ctx->geodata[sc->tq_geodata_id];
        if (!geo.d_node_index) return fail(OSMT_INVALID_ARG, "geodata id %u has no node index (osmt_register_node_index)", sc->tq_geodata_id);
        if (sc->tq_filter.on && !sc->tq_filter.node)
            return fail(OSMT_INVALID_ARG,
                        "the scene's id filter has no node plane: it was registered before the node index of geodata id %u; register the node index first "
                        "(osmt_register_node_index), then the filter, and build the scene again",
                        sc->tq_geodata_id);
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) {
            if (!zoom_used[z]) continue;
            const uint32_t id = bindings_of_zoom[z];
            if (id == OSMT_BINDINGS_NONE) return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no label bindings (OSMT_BINDINGS_NONE)", first_of_zoom[z], z);
            if (id >= ctx->label_bindings.size())
                return fail(OSMT_INVALID_ARG, "tile %zu: label bindings id %u of zoom %u is not registered (%zu tables)", first_of_zoom[z], id, z,
                            ctx->label_bindings.size());
            const osmt_ctx::label_bindings_host& h = ctx->label_bindings[id];
            if (h.geodata_id != sc->tq_geodata_id)
                return fail(OSMT_INVALID_ARG, "tile %zu: label bindings id %u of zoom %u belongs to geodata id %u, not %u", first_of_zoom[z], id, z, h.geodata_id,
                            sc->tq_geodata_id);
            if (z < h.zoom_lo || z > h.zoom_hi)
                return fail(OSMT_INVALID_ARG, "tile %zu: label bindings id %u covers zooms %u..%u, not zoom %u", first_of_zoom[z], id, h.zoom_lo, h.zoom_hi, z);
            bind[z] = h.dev;
        }
        icon_h.resize(ctx->images.size());
        for (size_t i = 0; i < icon_h.size(); ++i) icon_h[i] = ctx->images[i].height;
    }
    if (area) {
        if ((area->n_labels && (!area->labels || !area->runs)) || !area->job_label_off || (area->n_chars && !area->chars) ||
            (area->n_way_pts && (!area->way_pts || !area->way_sincos)))
            return fail(OSMT_INVALID_ARG, "area labels: NULL array with a non-zero count (job_label_off has at least its first entry)");
        if (area->job_label_off[0] != 0 || area->job_label_off[n_tiles] != area->n_labels)
            return fail(OSMT_INVALID_ARG, "area labels: job_label_off must run from 0 to n_labels over the scene's %zu tiles", n_tiles);
        for (size_t t = 0; t < n_tiles; ++t)
            if (area->job_label_off[t] > area->job_label_off[t + 1]) return fail(OSMT_INVALID_ARG, "area labels: job_label_off is not monotonic");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const osmt_label_style_rec* d_styles = nullptr;
    const uint32_t* d_rank = nullptr;
    int rc = sync_label_styles(ctx, &d_styles, &d_rank);
    if (rc != OSMT_OK) return rc;
    /* work[0]: per tile, [1]: per item, [2]: per candidate, [3]: per label, [4]: the chars — given back at the end */
    /* the trace: the device time of the stages */
    enum { EV_Q0, EV_Q1, EV_G0, EV_M0, EV_M1, EV_O0, EV_O1, EV_E0, EV_E1, EV_N };
    call_work wg(ctx, "tile labels");
    const int brc = wg.begin(EV_N);
    if (brc != OSMT_OK) return brc;
    hipStream_t st = wg.st;
    const bool trace = wg.trace;
    pool_layout pl;

    std::vector<osmt_label>& labels = nb->labels;
    std::vector<osmt_string_run>& runs = nb->runs;
    std::vector<uint32_t>&chars = nb->chars, &job_off = nb->job_off;
    labels.clear(), runs.clear(), chars.clear();
    job_off.assign(n_tiles + 1, 0u);
    size_t n_items = 0, n_cand = 0, n_labels = 0, n_chars = 0;
    unsigned long long max_labels = 0;
    if (n_tiles) {
        unsigned long long tq_tot[OSMT_TQ_N] = {}, tl_tot[OSMT_TL_N] = {};
        osmt_tq_pass Q;
        memset(&Q, 0, sizeof Q);
        osmt_tl_pass P;
        memset(&P, 0, sizeof P);
        pl = pool_layout();
        const size_t o_q = pl.add(n_tiles * sizeof(osmt_query_tile)), o_bind = pl.add(sizeof bind), o_c0 = pl.add(n_tiles * 4), o_ib = pl.add((n_tiles + 1) * 4);
        const size_t o_tw = pl.add((n_tiles + 1) * 4), o_tm = pl.add((n_tiles + 1) * 4), o_tot = pl.add((OSMT_TQ_N + OSMT_TL_N) * 8);
        const size_t o_blk0 = pl.add((n_tiles / 256 + 1) * 8), o_ih = pl.add(std::max<size_t>(icon_h.size(), 1) * 4), o_jo = pl.add((n_tiles + 1) * 4);
        rc = wg.alloc(0, pl, "tiles");
        if (rc != OSMT_OK) return rc;
        char* w0 = wg.work[0];
        HIP_TRY(hipMemcpyAsync(w0 + o_q, q.data(), n_tiles * sizeof(osmt_query_tile), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w0 + o_bind, bind, sizeof bind, hipMemcpyHostToDevice, st));
        if (!icon_h.empty()) HIP_TRY(hipMemcpyAsync(w0 + o_ih, icon_h.data(), icon_h.size() * 4, hipMemcpyHostToDevice, st));
        /* the query over the node pools: the node lists as the "ways", no second kind */
        osmt_tq_index_dev z18 = geo.ix;
        z18.way_off = geo.d_node_off, z18.ways = geo.d_node_refs;
        z18.mp_off = geo.d_zero_off, z18.mps = geo.d_node_refs;
        tq_bind_levels(geo, true, z18, Q);
        Q.q = (const osmt_query_tile*)(w0 + o_q);
        Q.n_tiles = (uint32_t)n_tiles;
        Q.span_c0 = (uint32_t*)(w0 + o_c0);
        Q.item_base = (uint32_t*)(w0 + o_ib);
        Q.t_wbase = (uint32_t*)(w0 + o_tw);
        Q.t_mbase = (uint32_t*)(w0 + o_tm);
        Q.tot = (unsigned long long*)(w0 + o_tot);
        Q.blk = (unsigned long long*)(w0 + o_blk0);
        HIP_TRY(wg.mark(EV_Q0));
        HIP_TRY(osmt_launch_tq_span(Q, st));
        HIP_TRY(hipMemcpyAsync(tq_tot, Q.tot, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tq_tot[OSMT_TQ_ITEMS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile labels: the batch needs %llu (tile, column) items (> 2^32): split the batch", tq_tot[OSMT_TQ_ITEMS]);
        n_items = (size_t)tq_tot[OSMT_TQ_ITEMS];
        pl = pool_layout();
        const size_t o_it = pl.add(n_items * 4), o_ws = pl.add(n_items * 4), o_ms = pl.add(n_items * 4), o_wb = pl.add((n_items + 1) * 4);
        const size_t o_mb = pl.add((n_items + 1) * 4), o_blk1 = pl.add((n_items / 256 + 1) * 8);
        rc = wg.alloc(1, pl, "columns");
        if (rc != OSMT_OK) return rc;
        char* w1 = wg.work[1];
        Q.n_items = (uint32_t)n_items;
        Q.item_tile = (uint32_t*)(w1 + o_it);
        Q.item_wsrc = (uint32_t*)(w1 + o_ws);
        Q.item_msrc = (uint32_t*)(w1 + o_ms);
        Q.wbase = (uint32_t*)(w1 + o_wb);
        Q.mbase = (uint32_t*)(w1 + o_mb);
        Q.blk = (unsigned long long*)(w1 + o_blk1);
        HIP_TRY(osmt_launch_tq_columns(Q, st));
        HIP_TRY(wg.mark(EV_Q1));
        /* first read-back: the candidate total, the first tile over the limit — nothing is gathered before */
        HIP_TRY(hipMemcpyAsync(tq_tot, Q.tot, OSMT_TQ_OVER_CAND * 8 + 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tq_tot[OSMT_TQ_OVER_CAND] != ~0ull) {
            const size_t t = (size_t)tq_tot[OSMT_TQ_OVER_CAND];
            uint32_t base[2];
            HIP_TRY(hipMemcpyAsync(base, Q.t_wbase + t, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return fail(OSMT_UNSUPPORTED, "tile %zu gathers %u node references (> OSMT_QUERY_MAX_TILE_CANDIDATES = %u)", t, base[1] - base[0],
                        OSMT_QUERY_MAX_TILE_CANDIDATES);
        }
        if (tq_tot[OSMT_TQ_WAYS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile labels: the batch gathers %llu node references (> 2^32): split the batch", tq_tot[OSMT_TQ_WAYS]);
        n_cand = (size_t)tq_tot[OSMT_TQ_WAYS];
        tq_stats_set(ctx, n_items, 0, 0, n_cand);
        pl = pool_layout();
        const size_t o_cand = pl.add(n_cand * 4), o_lpos = pl.add((n_cand + 1) * 4), o_blk2 = pl.add((n_cand / 256 + 1) * 8);
        rc = wg.alloc(2, pl, "candidates");
        if (rc != OSMT_OK) return rc;
        char* w2 = wg.work[2];
        Q.n_ways = (uint32_t)n_cand;
        Q.n_mps = 0u;
        Q.cand = (uint32_t*)(w2 + o_cand);
        HIP_TRY(wg.mark(EV_G0));
        HIP_TRY(osmt_launch_tq_gather(Q, st));
        HIP_TRY(osmt_launch_tq_sort(Q, st));
        /* expand */
        P.q = Q.q;
        P.bind = (const osmt_tl_bind_dev*)(w0 + o_bind);
        P.nodes = geo.dev.nodes;
        P.node_gid = geo.d_node_gid;
        P.styles = d_styles;
        P.style_rank = d_rank;
        P.icon_h = (const uint32_t*)(w0 + o_ih);
        P.n_tiles = (uint32_t)n_tiles;
        P.n_cand = (uint32_t)n_cand;
        P.scale = sc->scale;
        P.t_base = Q.t_wbase;
        P.cand = Q.cand;
        if (sc->tq_filter.on) P.keep_node = sc->tq_filter.node;
        P.lpos = (uint32_t*)(w2 + o_lpos);
        P.job_label_off = (uint32_t*)(w0 + o_jo);
        P.blk = (unsigned long long*)(w2 + o_blk2);
        P.tot = Q.tot + OSMT_TQ_N;
        HIP_TRY(wg.mark(EV_M0));
        HIP_TRY(osmt_launch_tl_mark(P, st));
        HIP_TRY(wg.mark(EV_M1));
        /* second read-back: the label total, the most labels of a tile, the first tile over the limit */
        HIP_TRY(hipMemcpyAsync(tl_tot, P.tot, 3 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tl_tot[OSMT_TL_OVER] != ~0ull) {
            const size_t t = (size_t)tl_tot[OSMT_TL_OVER];
            uint32_t base[2];
            HIP_TRY(hipMemcpyAsync(base, P.job_label_off + t, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return fail(OSMT_UNSUPPORTED, "tile %zu: %u node labels (> OSMT_TILE_LABELS_MAX = %u)", t, base[1] - base[0], OSMT_TILE_LABELS_MAX);
        }
        if (tl_tot[OSMT_TL_LABELS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile labels: the batch has %llu node labels (> 2^32): split the batch", tl_tot[OSMT_TL_LABELS]);
        n_labels = (size_t)tl_tot[OSMT_TL_LABELS];
        max_labels = tl_tot[OSMT_TL_MAX_LABELS];
        pl = pool_layout();
        const size_t o_keys = pl.add(n_labels * 16), o_eb = pl.add(n_labels * 4), o_en = pl.add(n_labels * 4), o_cp = pl.add((n_labels + 1) * 4);
        const size_t o_cs = pl.add(n_labels * 4), o_blk3 = pl.add((n_labels / 256 + 1) * 8), o_lab = pl.add(n_labels * sizeof(osmt_label));
        const size_t o_run = pl.add(n_labels * sizeof(osmt_string_run));
        rc = wg.alloc(3, pl, "labels");
        if (rc != OSMT_OK) return rc;
        char* w3 = wg.work[3];
        P.n_labels = (uint32_t)n_labels;
        P.keys = (ulonglong2*)(w3 + o_keys);
        P.el_bind = (uint32_t*)(w3 + o_eb);
        P.el_node = (uint32_t*)(w3 + o_en);
        P.chpos = (uint32_t*)(w3 + o_cp);
        P.ch_src = (uint32_t*)(w3 + o_cs);
        P.blk = (unsigned long long*)(w3 + o_blk3);
        P.labels = (osmt_label*)(w3 + o_lab);
        P.runs = (osmt_string_run*)(w3 + o_run);
        HIP_TRY(wg.mark(EV_O0));
        HIP_TRY(osmt_launch_tl_order(P, st));
        HIP_TRY(wg.mark(EV_O1));
        /* third read-back: the char total */
        HIP_TRY(hipMemcpyAsync(tl_tot + OSMT_TL_CHARS, P.tot + OSMT_TL_CHARS, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tl_tot[OSMT_TL_CHARS] >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile labels: the batch has %llu chars of label text (> 2^32): split the batch", tl_tot[OSMT_TL_CHARS]);
        n_chars = (size_t)tl_tot[OSMT_TL_CHARS];
        pl = pool_layout();
        (void)pl.add(n_chars * 4);
        rc = wg.alloc(4, pl, "chars");
        if (rc != OSMT_OK) return rc;
        P.n_chars = (uint32_t)n_chars;
        P.chars = (uint32_t*)wg.work[4];
        HIP_TRY(wg.mark(EV_E0));
        HIP_TRY(osmt_launch_tl_emit(P, st));
        HIP_TRY(wg.mark(EV_E1));
        /* the batch comes back: a few KB per tile */
        labels.resize(n_labels), runs.resize(n_labels), chars.resize(n_chars);
        if (n_labels) HIP_TRY(hipMemcpyAsync(labels.data(), P.labels, n_labels * sizeof(osmt_label), hipMemcpyDeviceToHost, st));
        if (n_labels) HIP_TRY(hipMemcpyAsync(runs.data(), P.runs, n_labels * sizeof(osmt_string_run), hipMemcpyDeviceToHost, st));
        if (n_chars) HIP_TRY(hipMemcpyAsync(chars.data(), P.chars, n_chars * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(job_off.data(), P.job_label_off, (n_tiles + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (trace) {
            fprintf(stderr,
                    "osmt tile labels: span + columns %.1f us, gather + sort %.1f us, mark + scan %.1f us, expand + sort + count %.1f us, emit %.1f us "
                    "(%zu tiles, %zu items, %zu candidates, %zu labels, at most %llu in a tile, %zu chars, %zu bytes read back)\n",
                    wg.us(EV_Q0, EV_Q1), wg.us(EV_G0, EV_M0), wg.us(EV_M0, EV_M1), wg.us(EV_O0, EV_O1), wg.us(EV_E0, EV_E1), n_tiles, n_items, n_cand, n_labels, max_labels,
                    n_chars, n_labels * (sizeof(osmt_label) + sizeof(osmt_string_run)) + n_chars * 4 + (n_tiles + 1) * 4);
        }
    }
    return OSMT_OK;
}

/* The second half: each tile's area labels (may be NULL) in front of its node labels (drawer.rs:229-261), seg_off re-based,
 * attached as one string batch; on success the scene keeps the node batch for osmt_scene_read_tile_labels. */
static int tile_labels_attach(osmt_ctx* ctx, osmt_scene* sc, const osmt_string_label_batch* area, node_label_batch* nb) {
    std::vector<osmt_label>& labels = nb->labels;
    std::vector<osmt_string_run>& runs = nb->runs;
    std::vector<uint32_t>&chars = nb->chars, &job_off = nb->job_off;
    const size_t n_tiles = sc->n_jobs, n_labels = labels.size(), n_chars = chars.size();
    int rc = OSMT_OK;
    osmt_string_label_batch sb{};
    std::vector<osmt_label> m_labels;
    std::vector<osmt_string_run> m_runs;
    std::vector<uint32_t> m_chars, m_off;
    if (area && area->n_labels) {
        if ((unsigned long long)area->n_labels + n_labels >= 0xFFFFFFFFull || (unsigned long long)area->n_chars + n_chars >= 0xFFFFFFFFull)
            return fail(OSMT_UNSUPPORTED, "tile labels: area and node labels together do not fit 32-bit indices");
        m_labels.reserve(area->n_labels + n_labels), m_runs.reserve(area->n_labels + n_labels);
        m_off.assign(n_tiles + 1, 0u);
        m_chars.assign(area->chars, area->chars + area->n_chars);
        m_chars.insert(m_chars.end(), chars.begin(), chars.end());
        for (size_t t = 0; t < n_tiles; ++t) {
            m_off[t] = (uint32_t)m_labels.size();
            m_labels.insert(m_labels.end(), area->labels + area->job_label_off[t], area->labels + area->job_label_off[t + 1]);
            m_runs.insert(m_runs.end(), area->runs + area->job_label_off[t], area->runs + area->job_label_off[t + 1]);
            for (uint32_t l = job_off[t]; l < job_off[t + 1]; ++l) {
                osmt_label x = labels[l];
                x.seg_off += (uint32_t)area->n_chars; /* the node chars sit behind the areas'; a node label has no way points */
                m_labels.push_back(x);
                m_runs.push_back(runs[l]);
            }
        }
        m_off[n_tiles] = (uint32_t)m_labels.size();
        sb.labels = m_labels.data(), sb.n_labels = m_labels.size(), sb.job_label_off = m_off.data(), sb.runs = m_runs.data();
        sb.chars = m_chars.data(), sb.n_chars = m_chars.size();
        sb.way_pts = area->way_pts, sb.way_sincos = area->way_sincos, sb.n_way_pts = area->n_way_pts;
    } else {
        sb.labels = labels.data(), sb.n_labels = labels.size(), sb.job_label_off = job_off.data(), sb.runs = runs.data();
        sb.chars = chars.data(), sb.n_chars = chars.size();
    }
    rc = osmt_scene_set_labels_body(ctx, sc, nullptr, nullptr, nullptr, &sb);
    if (rc != OSMT_OK) return rc;
    sc->h_tl_labels.swap(labels);
    sc->h_tl_runs.swap(runs);
    sc->h_tl_chars.swap(chars);
    sc->h_tl_off.swap(job_off);
    return OSMT_OK;
}

static int scene_build_tile_labels_body(osmt_ctx* ctx, osmt_scene* sc, const uint32_t* bindings_of_zoom, const osmt_string_label_batch* area) {
    node_label_batch nb;
    const int rc = tile_node_labels_build(ctx, sc, bindings_of_zoom, area, &nb);
    return rc != OSMT_OK ? rc : tile_labels_attach(ctx, sc, area, &nb);
}

static int scene_read_tile_labels_body(osmt_ctx* ctx, osmt_scene* sc, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, uint32_t* job_label_off,
                                       const size_t* caps, size_t* counts) {
    if (!ctx || !sc || sc->ctx != ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (sc->h_tl_off.empty()) return fail(OSMT_INVALID_ARG, "the scene has no device-built node labels (osmt_scene_build_tile_labels)");
    counts[0] = sc->h_tl_labels.size(), counts[1] = sc->h_tl_chars.size();
    if ((labels || runs || chars) && !caps) return fail(OSMT_INVALID_ARG, "caps is NULL");
    if ((labels || runs) && caps[0] < counts[0]) return fail(OSMT_INVALID_ARG, "caps[0] = %zu is less than the scene's %zu node labels", caps[0], counts[0]);
    if (chars && caps[1] < counts[1]) return fail(OSMT_INVALID_ARG, "caps[1] = %zu is less than the scene's %zu chars", caps[1], counts[1]);
    if (labels && counts[0]) memcpy(labels, sc->h_tl_labels.data(), counts[0] * sizeof(osmt_label));
    if (runs && counts[0]) memcpy(runs, sc->h_tl_runs.data(), counts[0] * sizeof(osmt_string_run));
    if (chars && counts[1]) memcpy(chars, sc->h_tl_chars.data(), counts[1] * 4);
    if (job_label_off) memcpy(job_label_off, sc->h_tl_off.data(), sc->h_tl_off.size() * 4);
    return OSMT_OK;
}

int osmt_validate_node_index(const osmt_node_index_desc* index, uint32_t geodata_id, osmt_ctx* ctx) {
    return guarded([&] { return validate_node_index(index, geodata_id, ctx, nullptr); });
}
int osmt_register_node_index(osmt_ctx* ctx, uint32_t geodata_id, const osmt_node_index_desc* index) {
    return guarded([&] { return register_node_index_body(ctx, geodata_id, index); });
}
int osmt_validate_label_styles(const osmt_label_style_rec* styles, size_t n, osmt_ctx* ctx) {
    return guarded([&] { return validate_label_styles(styles, n, ctx); });
}
int osmt_register_label_styles(osmt_ctx* ctx, const osmt_label_style_rec* styles, size_t n, uint32_t* out_first_style_id) {
    return guarded([&] { return register_label_styles_body(ctx, styles, n, out_first_style_id); });
}
int osmt_validate_label_bindings(const osmt_label_bindings_desc* b, osmt_ctx* ctx) {
    return guarded([&] { return validate_label_bindings(b, ctx, nullptr); });
}
int osmt_register_label_bindings(osmt_ctx* ctx, const osmt_label_bindings_desc* b, uint32_t* out_bindings_id) {
    return guarded([&] { return register_label_bindings_body(ctx, b, out_bindings_id); });
}
int osmt_scene_build_tile_labels(osmt_ctx* ctx, osmt_scene* scene, const uint32_t label_bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                                 const osmt_string_label_batch* area_labels) {
    return guarded([&] { return scene_build_tile_labels_body(ctx, scene, label_bindings_of_zoom, area_labels); });
}
int osmt_scene_read_tile_labels(osmt_ctx* ctx, osmt_scene* scene, osmt_label* labels, osmt_string_run* runs, uint32_t* chars,
                                uint32_t* job_label_off, const size_t caps[2], size_t counts[2]) {
    return guarded([&] { return scene_read_tile_labels_body(ctx, scene, labels, runs, chars, job_label_off, caps, counts); });
}

int osmt_validate_string_labels(const osmt_string_label_batch* sb, size_t n_jobs, osmt_ctx* ctx) {
    return guarded([&] {
        if (!ctx) return fail(OSMT_INVALID_ARG, "NULL context");
        std::vector<std::shared_ptr<osmt_ctx::font_host>> keep;
        const std::vector<const osmt_font_desc*> fonts = font_views(ctx, &keep);
        std::string why;
        const int rc = osmt::validate_string_labels(sb, n_jobs, fonts.data(), fonts.size(), &why);
        return rc == OSMT_OK ? OSMT_OK : fail(rc, "%s", why.c_str());
    });
}

static int osmt_scene_read_text_glyphs_body(osmt_ctx* ctx, osmt_scene* sc, osmt_text_glyph* out, size_t cap, size_t* n) {
    if (!ctx || !sc || sc->ctx != ctx || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    *n = sc->n_labels && sc->d_text_glyphs ? sc->n_text_glyphs : 0;
    if (!out) return OSMT_OK;
    if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu text glyphs, the scene has %zu", cap, *n);
    if (*n) HIP_TRY(copy_back(ctx, out, sc->d_text_glyphs, *n * sizeof(osmt_text_glyph)));
    return OSMT_OK;
}

int osmt_scene_read_text_glyphs(osmt_ctx* ctx, osmt_scene* sc, osmt_text_glyph* out, size_t cap, size_t* n) {
    return guarded([&] { return osmt_scene_read_text_glyphs_body(ctx, sc, out, cap, n); });
}

static int osmt_scene_read_glyph_instances_body(osmt_ctx* ctx, osmt_scene* sc, osmt_glyph_instance* out, size_t cap, size_t* n) {
    if (!ctx || !sc || sc->ctx != ctx || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    *n = sc->n_labels && sc->d_text_inst ? sc->n_text_inst : 0;
    if (!out) return OSMT_OK;
    if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu glyph instances, the scene has %zu", cap, *n);
    if (*n) HIP_TRY(copy_back(ctx, out, sc->d_text_inst, *n * sizeof(osmt_glyph_instance)));
    return OSMT_OK;
}

int osmt_scene_read_glyph_instances(osmt_ctx* ctx, osmt_scene* sc, osmt_glyph_instance* out, size_t cap, size_t* n) {
    return guarded([&] { return osmt_scene_read_glyph_instances_body(ctx, sc, out, cap, n); });
}

static int osmt_scene_read_label_segs_body(osmt_ctx* ctx, osmt_scene* sc, double* out, size_t cap, size_t* n) {
    if (!ctx || !sc || sc->ctx != ctx || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    *n = sc->n_labels ? sc->n_label_segs : 0;
    if (!out) return OSMT_OK;
    if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu draw_line calls, the arena has %zu", cap, *n);
    if (*n) HIP_TRY(copy_back(ctx, out, sc->d_lab_segs, *n * 32));
    return OSMT_OK;
}

int osmt_scene_read_label_segs(osmt_ctx* ctx, osmt_scene* sc, double* out, size_t cap, size_t* n) {
    return guarded([&] { return osmt_scene_read_label_segs_body(ctx, sc, out, cap, n); });
}

static int osmt_scene_read_label_cover_body(osmt_ctx* ctx, osmt_scene* sc, uint32_t label, int32_t window[4], double* out, size_t cap,
                                            size_t* n) {
    if (!ctx || !sc || sc->ctx != ctx || !window || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
    *n = 0;
    window[0] = 1, window[1] = 0, window[2] = 0, window[3] = 0;
    if (label >= sc->n_labels) return fail(OSMT_INVALID_ARG, "label %u: the scene has %u labels attached", label, sc->n_labels);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    /* The planes are written by the label stage of a render, not at upload: before the first one the pool holds
     * whatever the recycled buffer held (the lesson of osmt_scene_read_label_status). */
    if (!sc->lab_cover_valid) return fail(OSMT_INVALID_ARG, "no render has written the coverage planes of these labels yet");
    const osmt_labelinfo& li = sc->h_lab_info[label];
    if (!li.has_text || li.n_segs == 0 || li.ry0 > li.ry1) return OSMT_OK; /* no window: zero rows */
    window[0] = li.ry0, window[1] = li.ry1, window[2] = li.cx0, window[3] = (int32_t)li.cols;
    *n = (size_t)(li.ry1 - li.ry0 + 1) * li.cols;
    if (!out) return OSMT_OK;
    if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu cells, the window of label %u has %zu", cap, label, *n);
    uint32_t err = 0;
    HIP_TRY(copy_back(ctx, &err, sc->d_lab_err, 4));
    if (err) return fail(OSMT_HIP_ERROR, "label coverage window overflow (internal error %u)", err);
    HIP_TRY(copy_back(ctx, out, sc->d_lab_a + li.plane_off, *n * 8));
    return OSMT_OK;
}

int osmt_scene_read_label_cover(osmt_ctx* ctx, osmt_scene* sc, uint32_t label, int32_t window[4], double* out, size_t cap, size_t* n) {
    return guarded([&] { return osmt_scene_read_label_cover_body(ctx, sc, label, window, out, cap, n); });
}

static int osmt_debug_hypot_body(osmt_ctx* ctx, const double* xy, size_t n, double* out) {
    if (!ctx || (n && (!xy || !out))) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (n >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "too many pairs");
    if (!n) return OSMT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = nullptr;
    HIP_TRY(stream_acquire(ctx, &st));
    char* d = nullptr;
    hipError_t e = dev_alloc(ctx, (void**)&d, n * 24);
    if (e == hipSuccess) e = hipMemcpyAsync(d, xy, n * 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = osmt_launch_hypot((const double*)d, (uint32_t)n, (double*)(d + n * 16), st);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + n * 16, n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d) dev_free(ctx, d);
    stream_release(ctx, st);
    if (e != hipSuccess) return fail(OSMT_HIP_ERROR, "device hypot failed: %s", hipGetErrorString(e));
    return OSMT_OK;
}

int osmt_debug_hypot(osmt_ctx* ctx, const double* xy, size_t n, double* out) {
    return guarded([&] { return osmt_debug_hypot_body(ctx, xy, n, out); });
}

/* ---- label anchors (osmt_label_positions) ---------------------------------------------------------------------- */
struct osmt_label_job {
    osmt_ctx* ctx = nullptr;
    hipStream_t st = nullptr;
    char* d_base = nullptr;
    char* d_front = nullptr; /* tile requests: what was allocated before the totals were known */
    char* stage = nullptr; /* pinned: the request records going up, then the positions and the counters coming back */
    size_t n = 0, back_off = 0;
};

static void label_job_free(osmt_label_job* j) {
    if (!j) return;
    if (j->ctx) {
        if (j->d_base) dev_free(j->ctx, j->d_base);
        if (j->d_front) dev_free(j->ctx, j->d_front);
        if (j->stage) stage_release(j->ctx, j->stage);
        if (j->st) stream_release(j->ctx, j->st);
    }
    delete j;
}

static int label_positions_validate(const osmt_label_request_batch* b, size_t* keep_words) {
    if (b->n_requests >= 0xFFFFFFFFull || b->n_rings >= 0xFFFFFFFFull || b->n_pts >= 0xFFFFFFFFull)
        return fail(OSMT_INVALID_ARG, "label request batch too large for 32-bit indices");
    if (!b->requests || (b->n_rings && !b->rings) || (b->n_pts && !b->points)) return fail(OSMT_INVALID_ARG, "NULL pool with non-zero count");
    size_t words = 0;
    for (size_t i = 0; i < b->n_requests; ++i) {
        const osmt_label_request& rq = b->requests[i];
        if ((size_t)rq.ring_off + rq.n_rings > b->n_rings) return fail(OSMT_INVALID_ARG, "label request %zu: ring range out of bounds", i);
        if (!std::isfinite(rq.scale)) return fail(OSMT_INVALID_ARG, "label request %zu: scale not finite", i);
        for (uint32_t k = 0; k < rq.n_rings; ++k) {
            const osmt_ring& r = b->rings[rq.ring_off + k];
            if ((size_t)r.first_pt + r.n_pts > b->n_pts) return fail(OSMT_INVALID_ARG, "label request %zu ring %u: point range out of bounds", i, k);
        }
        words += rq.n_rings;
    }
    if (words >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "label request batch too large for 32-bit indices");
    /* the whole pool is uploaded, so the whole pool is checked: under 2^28 no intermediate of the search overflows */
    const double LIM = 268435456.0;
    for (size_t i = 0; i < 2 * b->n_pts; ++i)
        if (!(std::fabs(b->points[i]) <= LIM)) return fail(OSMT_UNSUPPORTED, "label point %zu: coordinate not finite or |v| > 2^28", i / 2);
    *keep_words = words;
    return OSMT_OK;
}

static int osmt_label_positions_begin_body(osmt_ctx* ctx, const osmt_label_request_batch* b, osmt_label_job** out_job) {
    if (!ctx || !b || !out_job) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_job = nullptr;
    osmt_label_job* j = new osmt_label_job();
    j->ctx = ctx;
    j->n = b->n_requests;
    if (!j->n) { /* no device is touched */
        *out_job = j;
        return OSMT_OK;
    }
    struct guard {
        osmt_label_job* j;
        ~guard() { label_job_free(j); }
    } gd{j};
    size_t keep_words = 0;
    const int rc = label_positions_validate(b, &keep_words);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(stream_acquire(ctx, &j->st));
    const size_t n = j->n;
    const uint32_t n_slots = (uint32_t)std::min<size_t>(n, OSMT_PL_MAX_SLOTS);
    pool_layout pl;
    const size_t o_req = pl.add(n * sizeof(osmt_pl_req)), o_rings = pl.add(b->n_rings * sizeof(osmt_ring)), o_pts = pl.add(b->n_pts * 16),
                 o_keep = pl.add(keep_words * 4), o_over = pl.add(n * 4), o_back = pl.add(n * sizeof(osmt_label_position) + 16),
                 o_ws = pl.add((size_t)n_slots * OSMT_PL_CELL_DOUBLES * OSMT_PL_GLOBAL_CELLS * sizeof(double));
    const size_t back_bytes = n * sizeof(osmt_label_position) + 16;
    j->back_off = align_up(n * sizeof(osmt_pl_req), 64);
    j->stage = (char*)stage_acquire(ctx, j->back_off + back_bytes);
    if (!j->stage) return fail(OSMT_OOM, "pinned staging for %zu label requests could not be allocated", n);
    osmt_pl_req* rq = (osmt_pl_req*)j->stage;
    uint32_t words = 0;
    for (size_t i = 0; i < n; ++i) {
        rq[i] = {b->requests[i].ring_off, b->requests[i].n_rings, words, 0u, b->requests[i].scale};
        words += b->requests[i].n_rings;
    }
    const size_t off = pl.size();
    HIP_TRY(dev_alloc(ctx, (void**)&j->d_base, off));
    char* d = j->d_base;
    HIP_TRY(hipMemcpyAsync(d + o_req, rq, n * sizeof(osmt_pl_req), hipMemcpyHostToDevice, j->st));
    if (b->n_rings) HIP_TRY(hipMemcpyAsync(d + o_rings, b->rings, b->n_rings * sizeof(osmt_ring), hipMemcpyHostToDevice, j->st));
    if (b->n_pts) HIP_TRY(hipMemcpyAsync(d + o_pts, b->points, b->n_pts * 16, hipMemcpyHostToDevice, j->st));
    osmt_polylabel_args a{};
    a.req = (const osmt_pl_req*)(d + o_req);
    a.n_req = (uint32_t)n;
    a.rings = (const osmt_ring*)(d + o_rings);
    a.n_rings = (uint32_t)b->n_rings;
    a.pts = (const double2*)(d + o_pts);
    a.keep = (uint32_t*)(d + o_keep);
    a.over = (uint32_t*)(d + o_over);
    a.out = (osmt_label_position*)(d + o_back);
    a.cnt = (uint32_t*)(d + o_back + n * sizeof(osmt_label_position));
    a.ws = (double*)(d + o_ws);
    a.n_slots = n_slots;
    HIP_TRY(osmt_launch_polylabel(a, j->st));
    HIP_TRY(hipMemcpyAsync(j->stage + j->back_off, d + o_back, back_bytes, hipMemcpyDeviceToHost, j->st));
    gd.j = nullptr;
    *out_job = j;
    return OSMT_OK;
}

static int osmt_label_positions_end_body(osmt_label_job* j, osmt_label_position* out) {
    if (!j) return fail(OSMT_INVALID_ARG, "NULL job");
    struct guard {
        osmt_label_job* j;
        ~guard() { label_job_free(j); }
    } gd{j};
    if (!j->n) return OSMT_OK;
    HIP_TRY(hipSetDevice(j->ctx->device));
    HIP_TRY(hipStreamSynchronize(j->st));
    if (!out) return fail(OSMT_INVALID_ARG, "out is NULL");
    const char* back = j->stage + j->back_off;
    uint32_t cnt[4];
    memcpy(cnt, back + j->n * sizeof(osmt_label_position), sizeof cnt);
    if (cnt[3]) return fail(OSMT_HIP_ERROR, "label positions: internal error %u (a bounded loop of the kernel passed its bound)", cnt[3]);
    memcpy(out, back, j->n * sizeof(osmt_label_position));
    std::lock_guard<std::mutex> lk(j->ctx->cache_mu);
    j->ctx->pl_stats[0] = j->n;
    j->ctx->pl_stats[1] = cnt[0];
    j->ctx->pl_stats[2] = cnt[2];
    return OSMT_OK;
}

int osmt_label_positions_begin(osmt_ctx* ctx, const osmt_label_request_batch* b, osmt_label_job** out_job) {
    return guarded([&] { return osmt_label_positions_begin_body(ctx, b, out_job); });
}

int osmt_label_positions_end(osmt_label_job* j, osmt_label_position* out) {
    return guarded([&] { return osmt_label_positions_end_body(j, out); });
}

int osmt_label_positions(osmt_ctx* ctx, const osmt_label_request_batch* b, osmt_label_position* out) {
    return guarded([&] {
        if (b && b->n_requests && !out) return fail(OSMT_INVALID_ARG, "out is NULL");
        osmt_label_job* j = nullptr;
        const int rc = osmt_label_positions_begin_body(ctx, b, &j);
        return rc != OSMT_OK ? rc : osmt_label_positions_end_body(j, out);
    });
}

int osmt_label_positions_stats(osmt_ctx* ctx, uint64_t stats[3]) {
    return guarded([&] {
        if (!ctx || !stats) return fail(OSMT_INVALID_ARG, "NULL argument");
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        for (int i = 0; i < 3; ++i) stats[i] = ctx->pl_stats[i];
        return (int)OSMT_OK;
    });
}

/* ---- label anchors from tile coordinates (include/osmtile.h, csrc/osmt_anchors.hip) ------------------------------------ */
static int validate_node_mercator(const double* f, size_t n, uint32_t geodata_id, osmt_ctx* ctx) {
    if (n && !f) return fail(OSMT_INVALID_ARG, "node mercator: factors are NULL with n_nodes = %zu", n);
    for (size_t i = 0; i < 2 * n; ++i)
        if (!(f[i] >= 0.0) || !(f[i] <= 1.0)) /* a NaN fails both */
            return fail(OSMT_INVALID_ARG, "node mercator: node %zu: %s factor %g is not finite or outside [0, 1]", i / 2, i % 2 ? "y" : "x", f[i]);
    if (!ctx) return fail(OSMT_INVALID_ARG, "node mercator: geodata id %u is not registered (no context)", geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (geodata_id >= ctx->geodata.size())
        return fail(OSMT_INVALID_ARG, "node mercator: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
    const osmt_ctx::geodata_host& g = ctx->geodata[geodata_id];
    if (n != g.n_nodes) return fail(OSMT_INVALID_ARG, "node mercator: n_nodes = %zu, the geodata has %zu nodes", n, g.n_nodes);
    if (g.d_factors) return fail(OSMT_INVALID_ARG, "node mercator: geodata id %u has its factors already (one table per file)", geodata_id);
    return OSMT_OK;
}

static int register_node_mercator_body(osmt_ctx* ctx, uint32_t geodata_id, const double* f) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "node mercator: geodata id %u is not registered (%zu files)", geodata_id, ctx->geodata.size());
        n = ctx->geodata[geodata_id].n_nodes; /* the table's length is the file's: there is no count to get wrong */
    }
    const int rc = validate_node_mercator(f, n, geodata_id, ctx);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    (void)pl.add(n * 16);
    table_upload up("node mercator", pl);
    up.put(0, f, n * 16);
    if (up.done() != OSMT_OK) return up.done();
    std::lock_guard<std::mutex> lk(ctx->mu);
    osmt_ctx::geodata_host& g = ctx->geodata[geodata_id];
    if (g.d_factors) return fail(OSMT_INVALID_ARG, "node mercator: geodata id %u has its factors already (one table per file)", geodata_id); /* another thread was first */
    g.d_factors = (const double2*)up.pool;
    up.release();
    return OSMT_OK;
}

/* geo (optional): the registered file's tables as they are at the time of the call */
static int validate_label_tile_batch(const osmt_label_tile_batch* b, osmt_ctx* ctx, osmt_ctx::geodata_host* geo) {
    if (!b) return fail(OSMT_INVALID_ARG, "label tile batch is NULL");
    if ((b->n_requests && !b->requests) || (b->n_tiles && !b->tiles)) return fail(OSMT_INVALID_ARG, "label tile batch: NULL pool with non-zero count");
    if (b->n_requests >= 0xFFFFFFFFull || b->n_tiles >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "label tile batch too large for 32-bit indices");
    if (b->scale < 1u || b->scale > OSMT_MAX_SCALE) return fail(OSMT_INVALID_ARG, "label tile batch: scale %u outside 1..%u", b->scale, OSMT_MAX_SCALE);
    for (size_t t = 0; t < b->n_tiles; ++t) {
        const osmt_query_tile& q = b->tiles[t];
        if (q.zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "label tile batch: tile %zu: zoom %u > %u", t, q.zoom, OSMT_MAX_ZOOM);
        if (q.x >= (1u << q.zoom) || q.y >= (1u << q.zoom))
            return fail(OSMT_INVALID_ARG, "label tile batch: tile %zu: (x, y) = (%u, %u) outside zoom %u", t, q.x, q.y, q.zoom);
    }
    for (size_t i = 0; i < b->n_requests; ++i)
        if (b->requests[i].tile >= b->n_tiles)
            return fail(OSMT_INVALID_ARG, "label tile request %zu: tile %u is not a tile of the batch (%zu tiles)", i, b->requests[i].tile, b->n_tiles);
    if (!ctx) return fail(OSMT_INVALID_ARG, "label tile batch: geodata id %u is not registered (no context)", b->geodata_id);
    osmt_ctx::geodata_host g;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (b->geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "label tile batch: geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
        g = ctx->geodata[b->geodata_id];
    }
    if (!g.d_factors)
        return fail(OSMT_INVALID_ARG, "label tile batch: geodata id %u has no Mercator factors (osmt_register_node_mercator)", b->geodata_id);
    for (size_t i = 0; i < b->n_requests; ++i) {
        const uint32_t e = b->requests[i].entity, id = e & ~OSMT_STYLED_MULTIPOLYGON;
        if (e & OSMT_STYLED_MULTIPOLYGON) {
            if (id >= g.n_mps) return fail(OSMT_INVALID_ARG, "label tile request %zu: multipolygon %u out of range (%zu multipolygons)", i, id, g.n_mps);
        } else if (id >= g.n_ways) {
            return fail(OSMT_INVALID_ARG, "label tile request %zu: way %u out of range (%zu ways)", i, id, g.n_ways);
        }
    }
    if (geo) *geo = g;
    return OSMT_OK;
}

/* The projection of a validated batch with requests, on j->st: count and scans, the wait for the totals (they decide the
 * refusals and size everything else), then rings, records and points.  The second allocation gets extra_of(rings) bytes
 * behind the arrays of the projection — the caller's arrays, starting at j->d_base + *extra_off.  sizes_only: the totals
 * and nothing after them. */
static int label_tiles_expand(osmt_ctx* ctx, const osmt_label_tile_batch* b, const osmt_ctx::geodata_host& geo, osmt_label_job* j, bool sizes_only,
                              const std::function<size_t(size_t)>& extra_of, size_t* extra_off, osmt_an_pass* out_pass,
                              const osmt_label_tile_request* d_req = nullptr, const osmt_query_tile* d_tiles = nullptr) {
    const size_t n = b->n_requests;
    pool_layout pl;
    const size_t o_req = pl.add(d_req ? 0 : n * sizeof(osmt_label_tile_request)), o_tiles = pl.add(d_req ? 0 : b->n_tiles * sizeof(osmt_query_tile)),
                 o_rpos = pl.add((n + 1) * 4),
                 o_ppos = pl.add((n + 1) * 4), o_blk = pl.add(((n + 255) / 256 + 1) * 8), o_tot = pl.add(OSMT_AN_N * 8);
    size_t off = pl.size();
    HIP_TRY(dev_alloc(ctx, (void**)&j->d_front, off));
    char* d = j->d_front;
    if (!d_req) { /* d_req, d_tiles: the requests and tiles are on the device already (b->requests and b->tiles are not read) */
        HIP_TRY(hipMemcpyAsync(d + o_req, b->requests, n * sizeof(osmt_label_tile_request), hipMemcpyHostToDevice, j->st));
        HIP_TRY(hipMemcpyAsync(d + o_tiles, b->tiles, b->n_tiles * sizeof(osmt_query_tile), hipMemcpyHostToDevice, j->st));
    }
    osmt_an_pass a{};
    a.geo = geo.dev;
    a.factors = geo.d_factors;
    a.req = d_req ? d_req : (const osmt_label_tile_request*)(d + o_req);
    a.tiles = d_req ? d_tiles : (const osmt_query_tile*)(d + o_tiles);
    a.n_req = (uint32_t)n;
    a.scale = b->scale;
    a.rpos = (uint32_t*)(d + o_rpos);
    a.ppos = (uint32_t*)(d + o_ppos);
    a.blk = (unsigned long long*)(d + o_blk);
    a.tot = (unsigned long long*)(d + o_tot);
    HIP_TRY(osmt_launch_an_count(a, j->st));
    HIP_TRY(hipMemcpyAsync(j->stage, a.tot, 3 * 8, hipMemcpyDeviceToHost, j->st)); /* the front of the job's pinned buffer */
    HIP_TRY(hipStreamSynchronize(j->st));
    unsigned long long tot[3];
    memcpy(tot, j->stage, sizeof tot);
    const unsigned long long n_rings = tot[OSMT_AN_RINGS], n_pts = tot[OSMT_AN_POINTS] + tot[OSMT_AN_HIGH];
    if (n_rings >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "label tile batch: %llu rings do not fit 32-bit indices", n_rings);
    if (n_pts >= 0xFFFFFFFFull) return fail(OSMT_UNSUPPORTED, "label tile batch: %llu points do not fit 32-bit indices", n_pts);
    a.n_rings = (uint32_t)n_rings;
    a.n_pts = (uint32_t)n_pts;
    *out_pass = a;
    if (sizes_only) return OSMT_OK;
    pl = pool_layout();
    const size_t o_base = pl.add((n_rings + 1) * 4), o_src = pl.add(n_rings * 4), o_rreq = pl.add(n_rings * 4), o_blk2 = pl.add(((n_rings + 255) / 256 + 1) * 8),
                 o_pl = pl.add(n * sizeof(osmt_pl_req)), o_rings = pl.add(n_rings * sizeof(osmt_ring)), o_pts = pl.add(n_pts * 16);
    *extra_off = off = pl.size();
    HIP_TRY(dev_alloc(ctx, (void**)&j->d_base, off + extra_of((size_t)n_rings)));
    d = j->d_base;
    a.ring_base = (uint32_t*)(d + o_base);
    a.ring_src = (uint32_t*)(d + o_src);
    a.ring_req = (uint32_t*)(d + o_rreq);
    a.blk = (unsigned long long*)(d + o_blk2);
    a.pl_req = (osmt_pl_req*)(d + o_pl);
    a.rings = (osmt_ring*)(d + o_rings);
    a.pts = (double2*)(d + o_pts);
    HIP_TRY(osmt_launch_an_expand(a, j->st));
    *out_pass = a;
    return OSMT_OK;
}

static int osmt_label_positions_tiles_begin_body(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_label_job** out_job) {
    if (!ctx || !b || !out_job) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_job = nullptr;
    osmt_ctx::geodata_host geo;
    const int rc = validate_label_tile_batch(b, ctx, &geo);
    if (rc != OSMT_OK) return rc;
    osmt_label_job* j = new osmt_label_job();
    j->ctx = ctx;
    j->n = b->n_requests;
    if (!j->n) { /* no device is touched */
        *out_job = j;
        return OSMT_OK;
    }
    struct guard {
        osmt_label_job* j;
        ~guard() { label_job_free(j); }
    } gd{j};
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(stream_acquire(ctx, &j->st));
    const size_t n = j->n;
    const size_t back_bytes = n * sizeof(osmt_label_position) + 16;
    j->back_off = 64; /* the totals come back in front of the positions */
    j->stage = (char*)stage_acquire(ctx, j->back_off + back_bytes);
    if (!j->stage) return fail(OSMT_OOM, "pinned staging for %zu label requests could not be allocated", n);
    const uint32_t n_slots = (uint32_t)std::min<size_t>(n, OSMT_PL_MAX_SLOTS);
    /* the work areas of the search, behind the arrays of the projection */
    size_t o_keep = 0, o_over = 0, o_back = 0, o_ws = 0;
    auto search_bytes = [&](size_t n_rings) {
        pool_layout pl;
        o_keep = pl.add(n_rings * 4), o_over = pl.add(n * 4), o_back = pl.add(back_bytes);
        o_ws = pl.add((size_t)n_slots * OSMT_PL_CELL_DOUBLES * OSMT_PL_GLOBAL_CELLS * sizeof(double));
        return pl.size();
    };
    osmt_an_pass p{};
    size_t x0 = 0;
    const int erc = label_tiles_expand(ctx, b, geo, j, false, search_bytes, &x0, &p);
    if (erc != OSMT_OK) return erc;
    char* d = j->d_base + x0;
    osmt_polylabel_args a{};
    a.req = p.pl_req;
    a.n_req = (uint32_t)n;
    a.rings = p.rings;
    a.n_rings = p.n_rings;
    a.pts = p.pts;
    a.keep = (uint32_t*)(d + o_keep);
    a.over = (uint32_t*)(d + o_over);
    a.out = (osmt_label_position*)(d + o_back);
    a.cnt = (uint32_t*)(d + o_back + n * sizeof(osmt_label_position));
    a.ws = (double*)(d + o_ws);
    a.n_slots = n_slots;
    HIP_TRY(osmt_launch_polylabel(a, j->st));
    HIP_TRY(hipMemcpyAsync(j->stage + j->back_off, d + o_back, back_bytes, hipMemcpyDeviceToHost, j->st));
    gd.j = nullptr;
    *out_job = j;
    return OSMT_OK;
}

static int osmt_label_tile_batch_expand_body(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_ring* rings, double* points, size_t rings_cap,
                                             size_t points_cap, size_t counts[2]) {
    if (!ctx || !b || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx::geodata_host geo;
    const int rc = validate_label_tile_batch(b, ctx, &geo);
    if (rc != OSMT_OK) return rc;
    counts[0] = counts[1] = 0;
    if (!b->n_requests) return OSMT_OK;
    osmt_label_job* j = new osmt_label_job();
    j->ctx = ctx;
    j->n = b->n_requests;
    struct guard {
        osmt_label_job* j;
        ~guard() { label_job_free(j); }
    } gd{j};
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(stream_acquire(ctx, &j->st));
    j->stage = (char*)stage_acquire(ctx, 64);
    if (!j->stage) return fail(OSMT_OOM, "pinned staging for the totals could not be allocated");
    const bool sizes_only = !rings && !points;
    osmt_an_pass p{};
    size_t x0 = 0;
    const int erc = label_tiles_expand(ctx, b, geo, j, sizes_only, [](size_t) { return (size_t)0; }, &x0, &p);
    if (erc != OSMT_OK) return erc;
    counts[0] = p.n_rings, counts[1] = p.n_pts;
    if (sizes_only) return OSMT_OK;
    int out_rc = OSMT_OK;
    if ((rings && rings_cap < p.n_rings) || (points && points_cap < p.n_pts))
        out_rc = fail(OSMT_INVALID_ARG, "label tile batch: %u rings and %u points, the capacities are %zu and %zu", p.n_rings, p.n_pts, rings_cap, points_cap);
    if (out_rc == OSMT_OK && rings && p.n_rings) HIP_TRY(hipMemcpyAsync(rings, p.rings, (size_t)p.n_rings * sizeof(osmt_ring), hipMemcpyDeviceToHost, j->st));
    if (out_rc == OSMT_OK && points && p.n_pts) HIP_TRY(hipMemcpyAsync(points, p.pts, (size_t)p.n_pts * 16, hipMemcpyDeviceToHost, j->st));
    HIP_TRY(hipStreamSynchronize(j->st)); /* also on a refusal: the job's buffers go back to the pool behind the kernels */
    return out_rc;
}

/* ---- area labels of tile-built scenes (include/osmtile.h, csrc/osmt_arealabels.hip) ------------------------------------ */
static int validate_area_label_bindings(const osmt_area_label_bindings_desc* b, osmt_ctx* ctx, size_t* out_ways, size_t* out_mps) {
    if (!b) return fail(OSMT_INVALID_ARG, "area label bindings are NULL");
    if (b->zoom_lo > b->zoom_hi || b->zoom_hi > OSMT_MAX_ZOOM)
        return fail(OSMT_INVALID_ARG, "area label bindings: zoom range %u..%u (zoom_lo <= zoom_hi <= %u)", b->zoom_lo, b->zoom_hi, OSMT_MAX_ZOOM);
    if (!ctx) return fail(OSMT_INVALID_ARG, "area label bindings: geodata id %u is not registered (no context)", b->geodata_id);
    size_t n_ways = 0, n_mps = 0, n_styles = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (b->geodata_id >= ctx->geodata.size())
            return fail(OSMT_INVALID_ARG, "area label bindings: geodata id %u is not registered (%zu files)", b->geodata_id, ctx->geodata.size());
        const osmt_ctx::geodata_host& g = ctx->geodata[b->geodata_id];
        if (!g.d_index) return fail(OSMT_INVALID_ARG, "area label bindings: geodata id %u has no tile index (osmt_register_tile_index)", b->geodata_id);
        if (!g.d_factors)
            return fail(OSMT_INVALID_ARG, "area label bindings: geodata id %u has no Mercator factors (osmt_register_node_mercator)", b->geodata_id);
        n_ways = g.n_ways, n_mps = g.n_mps;
        n_styles = ctx->label_styles.size();
    }
    if (!b->way_off || !b->multipolygon_off || (b->n_way_bindings && !b->way_bindings) || (b->n_multipolygon_bindings && !b->multipolygon_bindings) ||
        !b->text_off || (b->n_chars && !b->chars))
        return fail(OSMT_INVALID_ARG, "area label bindings: NULL array (every offset array has at least its first entry)");
    if (b->n_way_bindings >= 0xFFFFFFFFull || b->n_multipolygon_bindings >= 0xFFFFFFFFull || b->n_texts >= 0xFFFFFFFFull || b->n_chars >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area label bindings: too large for 32-bit indices");
    int rc = check_offsets_of("area label bindings", "way_off", b->way_off, n_ways, b->n_way_bindings);
    if (rc == OSMT_OK) rc = check_offsets_of("area label bindings", "multipolygon_off", b->multipolygon_off, n_mps, b->n_multipolygon_bindings);
    if (rc == OSMT_OK) rc = check_offsets_of("area label bindings", "text_off", b->text_off, b->n_texts, b->n_chars);
    if (rc != OSMT_OK) return rc;
    for (int kind = 0; kind < 2; ++kind) {
        const osmt_label_binding* v = kind ? b->multipolygon_bindings : b->way_bindings;
        const size_t n = kind ? b->n_multipolygon_bindings : b->n_way_bindings;
        const char* name = kind ? "multipolygon_bindings" : "way_bindings";
        for (size_t i = 0; i < n; ++i) {
            if (v[i].style >= n_styles)
                return fail(OSMT_INVALID_ARG, "area label bindings: %s[%zu].style = %u is not a registered label style (%zu styles)", name, i, v[i].style, n_styles);
            if (v[i].text != OSMT_TEXT_NONE && v[i].text >= b->n_texts)
                return fail(OSMT_INVALID_ARG, "area label bindings: %s[%zu].text = %u is not in the text pool (%zu texts) nor OSMT_TEXT_NONE", name, i, v[i].text,
                            b->n_texts);
        }
    }
    for (size_t i = 0; i < b->n_chars; ++i)
        if (!osmt::textshaper_detail::is_char(b->chars[i]))
            return fail(OSMT_INVALID_ARG, "area label bindings: chars[%zu] = U+%X is not a Unicode scalar value", i, b->chars[i]);
    if (out_ways) *out_ways = n_ways;
    if (out_mps) *out_mps = n_mps;
    return OSMT_OK;
}

static int register_area_label_bindings_body(osmt_ctx* ctx, const osmt_area_label_bindings_desc* b, uint32_t* out_id) {
    if (!ctx || !out_id) return fail(OSMT_INVALID_ARG, "NULL argument");
    size_t n_ways = 0, n_mps = 0;
    const int rc = validate_area_label_bindings(b, ctx, &n_ways, &n_mps);
    if (rc != OSMT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    pool_layout pl;
    const size_t o_wo = pl.add((n_ways + 1) * 4), o_mo = pl.add((n_mps + 1) * 4), o_wb = pl.add(b->n_way_bindings * sizeof(osmt_label_binding));
    const size_t o_mb = pl.add(b->n_multipolygon_bindings * sizeof(osmt_label_binding)), o_to = pl.add((b->n_texts + 1) * 4), o_c = pl.add(b->n_chars * 4);
    table_upload up("area label bindings", pl);
    char* pool = up.pool;
    up.put(o_wo, b->way_off, (n_ways + 1) * 4);
    up.put(o_mo, b->multipolygon_off, (n_mps + 1) * 4);
    up.put(o_wb, b->way_bindings, b->n_way_bindings * sizeof(osmt_label_binding));
    up.put(o_mb, b->multipolygon_bindings, b->n_multipolygon_bindings * sizeof(osmt_label_binding));
    up.put(o_to, b->text_off, (b->n_texts + 1) * 4);
    up.put(o_c, b->chars, b->n_chars * 4);
    if (up.done() != OSMT_OK) return up.done();
    osmt_ctx::area_label_bindings_host h;
    h.geodata_id = b->geodata_id, h.zoom_lo = b->zoom_lo, h.zoom_hi = b->zoom_hi;
    h.d_pool = pool;
    h.dev.way_off = (const uint32_t*)(pool + o_wo);
    h.dev.mp_off = (const uint32_t*)(pool + o_mo);
    h.dev.way_bind = (const osmt_label_binding*)(pool + o_wb);
    h.dev.mp_bind = (const osmt_label_binding*)(pool + o_mb);
    h.dev.text_off = (const uint32_t*)(pool + o_to);
    h.dev.chars = (const uint32_t*)(pool + o_c);
    h.n_ways = n_ways, h.n_mps = n_mps, h.n_way_bindings = b->n_way_bindings, h.n_mp_bindings = b->n_multipolygon_bindings;
    h.n_texts = b->n_texts, h.n_chars = b->n_chars;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->area_label_bindings.size() + 1 >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "area label bindings table too large");
    *out_id = (uint32_t)ctx->area_label_bindings.size();
    ctx->area_label_bindings.push_back(h);
    up.release();
    return OSMT_OK;
}

/* the area labels of a batch as the device built them, tile behind tile, with the angles of the host */
struct area_label_batch {
    std::vector<osmt_label> labels;
    std::vector<osmt_string_run> runs;
    std::vector<uint32_t> chars, job_off;
    std::vector<int32_t> pts;   /* [n][2] */
    std::vector<double> sincos; /* [n][2] */
};

static_assert(OSMT_STYLED_MAX_TILE_AREAS == OSMT_TILE_LABELS_MAX, "k_tq_tiles reports the first tile over OSMT_STYLED_MAX_TILE_AREAS: the two limits are one");

/* way_sincos of the runs of a batch (text_placer.rs:87-101, 256-262): (-atan2(dy, dx)).sin_cos() of the integer differences
 * of every edge, with the libm of the process — the one the caller's own code would have called; the last entry of a run is 0 */
static void area_label_angles(const std::vector<osmt_label>& labels, const std::vector<osmt_string_run>& runs, const std::vector<int32_t>& pts,
                              std::vector<double>* sincos) {
    sincos->assign(pts.size(), 0.0);
    for (size_t l = 0; l < labels.size(); ++l) {
        const osmt_string_run& r = runs[l];
        if (!labels[l].has_text || r.position != OSMT_TEXT_LINE) continue;
        for (uint32_t e = 0; e + 1 < r.n_pts; ++e) {
            const int32_t* p = pts.data() + 2 * ((size_t)r.pt_off + e);
            const double dx = (double)((int64_t)p[2] - (int64_t)p[0]), dy = (double)((int64_t)p[3] - (int64_t)p[1]);
            const double a = std::atan2(dy, dx);
            double* o = sincos->data() + 2 * ((size_t)r.pt_off + e);
            o[0] = std::sin(-a);
            o[1] = std::cos(-a);
        }
    }
}

/* Builds the area labels of every tile of `sc` on the device and reads them back into `out`.  The scene's labels are not
 * touched; sc->h_al_declined is what the anchor search declined in THIS call. */
static int tile_area_labels_build(osmt_ctx* ctx, osmt_scene* sc, const uint32_t* bindings_of_zoom, const osmt_area_anchor* anchors, size_t n_anchors,
                                  area_label_batch* out) {
    const size_t n_tiles = sc->n_jobs;
    const std::vector<osmt_query_tile>& q = sc->h_tq_tiles;
    osmt_al_bind_dev bind[OSMT_MAX_ZOOM + 1];
    osmt_tq_bind_dev tq_bind[OSMT_MAX_ZOOM + 1];
    memset(bind, 0, sizeof bind);
    memset(tq_bind, 0, sizeof tq_bind);
    osmt_ctx::geodata_host geo;
    std::vector<uint32_t> icon_h;
    {
        bool zoom_used[OSMT_MAX_ZOOM + 1] = {};
        size_t first_of_zoom[OSMT_MAX_ZOOM + 1] = {};
        for (size_t t = 0; t < n_tiles; ++t)
            if (!zoom_used[q[t].zoom]) zoom_used[q[t].zoom] = true, first_of_zoom[q[t].zoom] = t;
        std::lock_guard<std::mutex> lk(ctx->mu);
        geo = ctx->geodata[sc->tq_geodata_id];
        if (!geo.d_factors) return fail(OSMT_INVALID_ARG, "geodata id %u has no Mercator factors (osmt_register_node_mercator)", sc->tq_geodata_id);
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) {
            if (!zoom_used[z]) continue;
            const uint32_t id = bindings_of_zoom[z];
            if (id == OSMT_BINDINGS_NONE)
                return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no area label bindings (OSMT_BINDINGS_NONE)", first_of_zoom[z], z);
            if (id >= ctx->area_label_bindings.size())
                return fail(OSMT_INVALID_ARG, "tile %zu: area label bindings id %u of zoom %u is not registered (%zu tables)", first_of_zoom[z], id, z,
                            ctx->area_label_bindings.size());
            const osmt_ctx::area_label_bindings_host& h = ctx->area_label_bindings[id];
            if (h.geodata_id != sc->tq_geodata_id)
                return fail(OSMT_INVALID_ARG, "tile %zu: area label bindings id %u of zoom %u belongs to geodata id %u, not %u", first_of_zoom[z], id, z,
                            h.geodata_id, sc->tq_geodata_id);
            if (z < h.zoom_lo || z > h.zoom_hi)
                return fail(OSMT_INVALID_ARG, "tile %zu: area label bindings id %u covers zooms %u..%u, not zoom %u", first_of_zoom[z], id, h.zoom_lo,
                            h.zoom_hi, z);
            bind[z] = h.dev;
            tq_bind[z].way_off = h.dev.way_off, tq_bind[z].mp_off = h.dev.mp_off; /* k_tq_mark and k_tq_tiles read no style */
        }
        icon_h.resize(ctx->images.size());
        for (size_t i = 0; i < icon_h.size(); ++i) icon_h[i] = ctx->images[i].height;
    }
    if (n_anchors && !anchors) return fail(OSMT_INVALID_ARG, "anchors are NULL with n_anchors = %zu", n_anchors);
    if (n_anchors >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "too many anchors for 32-bit indices");
    for (size_t i = 0; i < n_anchors; ++i) {
        const osmt_area_anchor& a = anchors[i];
        const uint32_t id = a.entity & ~OSMT_STYLED_MULTIPOLYGON;
        if (a.tile >= n_tiles) return fail(OSMT_INVALID_ARG, "anchor %zu: tile %u is not a tile of the scene (%zu tiles)", i, a.tile, n_tiles);
        if (id >= ((a.entity & OSMT_STYLED_MULTIPOLYGON) ? geo.n_mps : geo.n_ways))
            return fail(OSMT_INVALID_ARG, "anchor %zu: %s %u out of range", i, (a.entity & OSMT_STYLED_MULTIPOLYGON) ? "multipolygon" : "way", id);
        if (a.status != OSMT_LABEL_OK && a.status != OSMT_LABEL_NONE)
            return fail(OSMT_INVALID_ARG, "anchor %zu: status %u (a handed-in anchor is OSMT_LABEL_OK or OSMT_LABEL_NONE)", i, a.status);
        if (!(std::fabs(a.x) <= 268435456.0) || !(std::fabs(a.y) <= 268435456.0))
            return fail(OSMT_INVALID_ARG, "anchor %zu: (x, y) not finite or |v| > 2^28", i);
        if (i && !(anchors[i - 1].tile < a.tile || (anchors[i - 1].tile == a.tile && anchors[i - 1].entity < a.entity)))
            return fail(OSMT_INVALID_ARG, "anchor %zu: the anchors must be strictly ascending by (tile, entity)", i);
    }
    out->labels.clear(), out->runs.clear(), out->chars.clear(), out->pts.clear(), out->sincos.clear();
    out->job_off.assign(n_tiles + 1, 0u);
    if (!n_tiles) return OSMT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const osmt_label_style_rec* d_styles = nullptr;
    const uint32_t* d_rank = nullptr;
    int rc = sync_label_styles(ctx, &d_styles, &d_rank);
    if (rc != OSMT_OK) return rc;
    /* the job carries the stream, the pinned words of the totals and the two allocations of the anchors' projection;
     * work[0]: per tile, [1]: per item, [2]: per candidate, [3]: per label, [4]: requests, [5]: chars and way points */
    struct job_guard {
        osmt_label_job* j;
        ~job_guard() { label_job_free(j); }
    } jg{new osmt_label_job()};
    osmt_label_job* j = jg.j;
    j->ctx = ctx;
    HIP_TRY(stream_acquire(ctx, &j->st));
    hipStream_t st = j->st;
    /* the trace: the device time of the stages */
    enum { EV_Q0, EV_Q1, EV_X0, EV_X1, EV_A0, EV_A1, EV_C0, EV_C1, EV_E0, EV_E1, EV_N };
    call_work wg(ctx, "area labels", st); /* behind the job's guard: it waits for the job's stream before the job gives it back */
    rc = wg.begin(EV_N);
    if (rc != OSMT_OK) return rc;
    const bool trace = wg.trace;
    j->stage = (char*)stage_acquire(ctx, 256);
    if (!j->stage) return fail(OSMT_OOM, "pinned staging for the totals could not be allocated");
    pool_layout pl;

    unsigned long long tq_tot[OSMT_TQ_N] = {}, al_tot[OSMT_AL_N] = {};
    osmt_tq_pass Q;
    memset(&Q, 0, sizeof Q);
    osmt_al_pass P;
    memset(&P, 0, sizeof P);
    pl = pool_layout();
    const size_t o_q = pl.add(n_tiles * sizeof(osmt_query_tile)), o_bind = pl.add(sizeof bind), o_tqb = pl.add(sizeof tq_bind), o_c0 = pl.add(n_tiles * 4);
    const size_t o_ib = pl.add((n_tiles + 1) * 4), o_tw = pl.add((n_tiles + 1) * 4), o_tm = pl.add((n_tiles + 1) * 4), o_tot = pl.add((OSMT_TQ_N + OSMT_AL_N) * 8);
    const size_t o_blk0 = pl.add((n_tiles / 256 + 1) * 8), o_ih = pl.add(std::max<size_t>(icon_h.size(), 1) * 4), o_jo = pl.add((n_tiles + 1) * 4);
    const size_t o_st = pl.add(n_tiles * sizeof(osmt_styled_tile)), o_an = pl.add(std::max<size_t>(n_anchors, 1) * sizeof(osmt_area_anchor));
    rc = wg.alloc(0, pl, "tiles");
    if (rc != OSMT_OK) return rc;
    char* w0 = wg.work[0];
    HIP_TRY(hipMemcpyAsync(w0 + o_q, q.data(), n_tiles * sizeof(osmt_query_tile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w0 + o_bind, bind, sizeof bind, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w0 + o_tqb, tq_bind, sizeof tq_bind, hipMemcpyHostToDevice, st));
    if (!icon_h.empty()) HIP_TRY(hipMemcpyAsync(w0 + o_ih, icon_h.data(), icon_h.size() * 4, hipMemcpyHostToDevice, st));
    if (n_anchors) HIP_TRY(hipMemcpyAsync(w0 + o_an, anchors, n_anchors * sizeof(osmt_area_anchor), hipMemcpyHostToDevice, st));
    /* 1. the query over the way and multipolygon pools, as osmt_scene_build_tiles runs it */
    tq_bind_levels(geo, false, geo.ix, Q);
    Q.geo_mp_off = geo.dev.mp_off;
    if (sc->tq_filter.on) Q.keep_way = sc->tq_filter.way, Q.keep_mp = sc->tq_filter.mp; /* the scene's filter: one per request (reader.rs:60) */
    Q.bind = (const osmt_tq_bind_dev*)(w0 + o_tqb);
    Q.q = (const osmt_query_tile*)(w0 + o_q);
    Q.n_tiles = (uint32_t)n_tiles;
    Q.span_c0 = (uint32_t*)(w0 + o_c0);
    Q.item_base = (uint32_t*)(w0 + o_ib);
    Q.t_wbase = (uint32_t*)(w0 + o_tw);
    Q.t_mbase = (uint32_t*)(w0 + o_tm);
    Q.tot = (unsigned long long*)(w0 + o_tot);
    Q.blk = (unsigned long long*)(w0 + o_blk0);
    Q.tiles = (osmt_styled_tile*)(w0 + o_st);
    Q.tile_base = (uint32_t*)(w0 + o_jo);
    HIP_TRY(wg.mark(EV_Q0));
    HIP_TRY(osmt_launch_tq_span(Q, st));
    HIP_TRY(hipMemcpyAsync(tq_tot, Q.tot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tq_tot[OSMT_TQ_ITEMS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area labels: the batch needs %llu (tile, column) items (> 2^32): split the batch", tq_tot[OSMT_TQ_ITEMS]);
    const size_t n_items = (size_t)tq_tot[OSMT_TQ_ITEMS];
    pl = pool_layout();
    const size_t o_it = pl.add(n_items * 4), o_ws = pl.add(n_items * 4), o_ms = pl.add(n_items * 4), o_wb = pl.add((n_items + 1) * 4);
    const size_t o_mb = pl.add((n_items + 1) * 4), o_blk1 = pl.add((n_items / 256 + 1) * 8);
    rc = wg.alloc(1, pl, "columns");
    if (rc != OSMT_OK) return rc;
    char* w1 = wg.work[1];
    Q.n_items = (uint32_t)n_items;
    Q.item_tile = (uint32_t*)(w1 + o_it);
    Q.item_wsrc = (uint32_t*)(w1 + o_ws);
    Q.item_msrc = (uint32_t*)(w1 + o_ms);
    Q.wbase = (uint32_t*)(w1 + o_wb);
    Q.mbase = (uint32_t*)(w1 + o_mb);
    Q.blk = (unsigned long long*)(w1 + o_blk1);
    HIP_TRY(osmt_launch_tq_columns(Q, st));
    HIP_TRY(hipMemcpyAsync(tq_tot, Q.tot, OSMT_TQ_OVER_CAND * 8 + 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tq_tot[OSMT_TQ_OVER_CAND] != ~0ull) {
        const size_t t = (size_t)tq_tot[OSMT_TQ_OVER_CAND];
        uint32_t base[4];
        HIP_TRY(hipMemcpyAsync(base, Q.t_wbase + t, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(base + 2, Q.t_mbase + t, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t nw = base[1] - base[0], nm = base[3] - base[2];
        return fail(OSMT_UNSUPPORTED, "tile %zu gathers %u %s references (> OSMT_QUERY_MAX_TILE_CANDIDATES = %u)", t,
                    nw > OSMT_QUERY_MAX_TILE_CANDIDATES ? nw : nm, nw > OSMT_QUERY_MAX_TILE_CANDIDATES ? "way" : "multipolygon",
                    OSMT_QUERY_MAX_TILE_CANDIDATES);
    }
    if (tq_tot[OSMT_TQ_WAYS] + tq_tot[OSMT_TQ_MPS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area labels: the batch gathers %llu references (> 2^32): split the batch", tq_tot[OSMT_TQ_WAYS] + tq_tot[OSMT_TQ_MPS]);
    const size_t n_cand = (size_t)(tq_tot[OSMT_TQ_WAYS] + tq_tot[OSMT_TQ_MPS]);
    tq_stats_set(ctx, n_items, tq_tot[OSMT_TQ_WAYS], tq_tot[OSMT_TQ_MPS], 0);
    pl = pool_layout();
    const size_t o_cand = pl.add(n_cand * 4), o_apos = pl.add((n_cand + 1) * 4), o_need = pl.add((n_cand + 1) * 4), o_ov = pl.add(n_cand * 4);
    const size_t o_blk2 = pl.add((n_cand / 256 + 1) * 8);
    rc = wg.alloc(2, pl, "candidates");
    if (rc != OSMT_OK) return rc;
    char* w2 = wg.work[2];
    Q.n_ways = (uint32_t)tq_tot[OSMT_TQ_WAYS];
    Q.n_mps = (uint32_t)tq_tot[OSMT_TQ_MPS];
    Q.cand = (uint32_t*)(w2 + o_cand);
    Q.apos = (uint32_t*)(w2 + o_apos);
    Q.blk = (unsigned long long*)(w2 + o_blk2);
    HIP_TRY(osmt_launch_tq_gather(Q, st));
    HIP_TRY(osmt_launch_tq_sort(Q, st));
    HIP_TRY(osmt_launch_tq_mark(Q, st)); /* with the label bindings' offsets: apos counts labels, tile_base is job_label_off */
    HIP_TRY(wg.mark(EV_Q1));
    HIP_TRY(hipMemcpyAsync(tq_tot + OSMT_TQ_AREAS, Q.tot + OSMT_TQ_AREAS, 3 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tq_tot[OSMT_TQ_OVER_AREAS] != ~0ull) {
        const size_t t = (size_t)tq_tot[OSMT_TQ_OVER_AREAS];
        osmt_styled_tile tl;
        HIP_TRY(hipMemcpyAsync(&tl, Q.tiles + t, sizeof tl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return fail(OSMT_UNSUPPORTED, "tile %zu: %u area labels (> OSMT_TILE_LABELS_MAX = %u)", t, tl.n_areas, OSMT_TILE_LABELS_MAX);
    }
    if (tq_tot[OSMT_TQ_AREAS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area labels: the batch has %llu area labels (> 2^32): split the batch", tq_tot[OSMT_TQ_AREAS]);
    const size_t n_labels = (size_t)tq_tot[OSMT_TQ_AREAS];
    /* 2. expand: keys, element tables, the pairs that are searched */
    pl = pool_layout();
    const size_t o_keys = pl.add(n_labels * 16), o_eb = pl.add(n_labels * 4), o_es = pl.add(n_labels * 4), o_cp = pl.add((n_labels + 1) * 4);
    const size_t o_cs = pl.add(n_labels * 4), o_pp = pl.add((n_labels + 1) * 4), o_ps = pl.add(n_labels * 4), o_blk3 = pl.add((n_labels / 256 + 1) * 8);
    const size_t o_lab = pl.add(n_labels * sizeof(osmt_label)), o_run = pl.add(n_labels * sizeof(osmt_string_run));
    rc = wg.alloc(3, pl, "labels");
    if (rc != OSMT_OK) return rc;
    char* w3 = wg.work[3];
    P.geo = geo.dev;
    P.q = Q.q;
    P.bind = (const osmt_al_bind_dev*)(w0 + o_bind);
    P.styles = d_styles;
    P.style_rank = d_rank;
    P.icon_h = (const uint32_t*)(w0 + o_ih);
    P.anchors = (const osmt_area_anchor*)(w0 + o_an);
    P.n_tiles = (uint32_t)n_tiles;
    P.n_cand = (uint32_t)n_cand;
    P.n_labels = (uint32_t)n_labels;
    P.n_anchors = (uint32_t)n_anchors;
    P.scale = sc->scale;
    P.t_wbase = Q.t_wbase, P.t_mbase = Q.t_mbase;
    P.cand = Q.cand;
    P.apos = Q.apos;
    P.job_label_off = Q.tile_base;
    P.need = (uint32_t*)(w2 + o_need);
    P.ov = (uint32_t*)(w2 + o_ov);
    P.keys = (ulonglong2*)(w3 + o_keys);
    P.el_bind = (uint32_t*)(w3 + o_eb);
    P.el_slot = (uint32_t*)(w3 + o_es);
    P.chpos = (uint32_t*)(w3 + o_cp);
    P.ch_src = (uint32_t*)(w3 + o_cs);
    P.ptpos = (uint32_t*)(w3 + o_pp);
    P.pt_src = (uint32_t*)(w3 + o_ps);
    P.labels = (osmt_label*)(w3 + o_lab);
    P.runs = (osmt_string_run*)(w3 + o_run);
    P.tot = Q.tot + OSMT_TQ_N;
    P.blk = (unsigned long long*)(w2 + o_blk2);
    HIP_TRY(wg.mark(EV_X0));
    HIP_TRY(osmt_launch_al_expand(P, st));
    {
        osmt_tl_pass S;
        memset(&S, 0, sizeof S);
        S.keys = P.keys, S.job_label_off = Q.tile_base, S.n_tiles = (uint32_t)n_tiles;
        if (n_labels) HIP_TRY(osmt_launch_tl_sort(S, st));
    }
    HIP_TRY(wg.mark(EV_X1));
    HIP_TRY(hipMemcpyAsync(j->stage, P.tot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(al_tot, j->stage, 8);
    const size_t n_req = (size_t)al_tot[OSMT_AL_REQS]; /* at most one per candidate: fits */
    /* 3. anchors: the requests stay on the device; only the totals that size the pools come back */
    uint32_t pl_cnt[4] = {0, 0, 0, 0};
    const uint32_t* d_cnt = nullptr;
    HIP_TRY(wg.mark(EV_A0));
    if (n_req) {
        pl = pool_layout();
        (void)pl.add(n_req * sizeof(osmt_label_tile_request));
        rc = wg.alloc(4, pl, "anchor requests");
        if (rc != OSMT_OK) return rc;
        P.n_req = (uint32_t)n_req;
        P.req = (osmt_label_tile_request*)wg.work[4];
        HIP_TRY(osmt_launch_al_requests(P, st));
        j->n = n_req;
        osmt_label_tile_batch lb{};
        lb.n_requests = n_req, lb.n_tiles = n_tiles, lb.geodata_id = sc->tq_geodata_id, lb.scale = sc->scale;
        const size_t back_bytes = n_req * sizeof(osmt_label_position) + 16;
        const uint32_t n_slots = (uint32_t)std::min<size_t>(n_req, OSMT_PL_MAX_SLOTS);
        size_t o_keep = 0, o_over = 0, o_back = 0, o_wsp = 0;
        auto search_bytes = [&](size_t n_rings) {
            pool_layout pl;
            o_keep = pl.add(n_rings * 4), o_over = pl.add(n_req * 4), o_back = pl.add(back_bytes);
            o_wsp = pl.add((size_t)n_slots * OSMT_PL_CELL_DOUBLES * OSMT_PL_GLOBAL_CELLS * sizeof(double));
            return pl.size();
        };
        osmt_an_pass ap{};
        size_t x0 = 0;
        rc = label_tiles_expand(ctx, &lb, geo, j, false, search_bytes, &x0, &ap, P.req, Q.q);
        if (rc != OSMT_OK) return rc;
        char* d = j->d_base + x0;
        osmt_polylabel_args a{};
        a.req = ap.pl_req;
        a.n_req = (uint32_t)n_req;
        a.rings = ap.rings;
        a.n_rings = ap.n_rings;
        a.pts = ap.pts;
        a.keep = (uint32_t*)(d + o_keep);
        a.over = (uint32_t*)(d + o_over);
        a.out = (osmt_label_position*)(d + o_back);
        a.cnt = (uint32_t*)(d + o_back + n_req * sizeof(osmt_label_position));
        a.ws = (double*)(d + o_wsp);
        a.n_slots = n_slots;
        HIP_TRY(osmt_launch_polylabel(a, st));
        P.pos = a.out;
        d_cnt = a.cnt;
    }
    HIP_TRY(wg.mark(EV_A1));
    /* 4. what every sorted label holds: chars and way points */
    P.blk = (unsigned long long*)(w3 + o_blk3);
    HIP_TRY(wg.mark(EV_C0));
    HIP_TRY(osmt_launch_al_count(P, st));
    HIP_TRY(wg.mark(EV_C1));
    HIP_TRY(hipMemcpyAsync(j->stage, P.tot, OSMT_AL_N * 8, hipMemcpyDeviceToHost, st));
    if (d_cnt) HIP_TRY(hipMemcpyAsync(j->stage + 64, d_cnt, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(al_tot, j->stage, sizeof al_tot);
    if (d_cnt) memcpy(pl_cnt, j->stage + 64, sizeof pl_cnt);
    if (pl_cnt[3]) return fail(OSMT_HIP_ERROR, "area labels: internal error %u of the anchor search (a bounded loop of the kernel passed its bound)", pl_cnt[3]);
    {
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        ctx->pl_stats[0] = n_req, ctx->pl_stats[1] = pl_cnt[0], ctx->pl_stats[2] = pl_cnt[2];
    }
    if (al_tot[OSMT_AL_DECLINED]) {
        std::vector<osmt_label_tile_request> rq(n_req);
        std::vector<osmt_label_position> ps(n_req);
        HIP_TRY(hipMemcpyAsync(rq.data(), P.req, n_req * sizeof(osmt_label_tile_request), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ps.data(), P.pos, n_req * sizeof(osmt_label_position), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < n_req; ++i) /* requests are in (tile, way before multipolygon, id) order: ascending by (tile, entity) */
            if (ps[i].status == OSMT_LABEL_TOO_LARGE) sc->h_al_declined.push_back(osmt_area_anchor{rq[i].tile, rq[i].entity, 0.0, 0.0, OSMT_LABEL_TOO_LARGE, 0u});
        const osmt_area_anchor& f = sc->h_al_declined.front();
        return fail(OSMT_UNSUPPORTED,
                    "area labels: the anchor search declined %zu (tile, entity) pairs as too large (OSMT_LABEL_MAX_CELLS = %u), the first is tile %u, %s %u: "
                    "read them with osmt_scene_read_declined_anchors, compute them on the host and hand them in as anchors",
                    sc->h_al_declined.size(), OSMT_LABEL_MAX_CELLS, f.tile, (f.entity & OSMT_STYLED_MULTIPOLYGON) ? "multipolygon" : "way",
                    f.entity & ~OSMT_STYLED_MULTIPOLYGON);
    }
    if (al_tot[OSMT_AL_CHARS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area labels: the batch has %llu chars of label text (> 2^32): split the batch", al_tot[OSMT_AL_CHARS]);
    if (al_tot[OSMT_AL_PTS] >= 0xFFFFFFFFull)
        return fail(OSMT_UNSUPPORTED, "area labels: the batch has %llu way points of text along ways (> 2^32): split the batch", al_tot[OSMT_AL_PTS]);
    const size_t n_chars = (size_t)al_tot[OSMT_AL_CHARS], n_pts = (size_t)al_tot[OSMT_AL_PTS];
    /* 5. way points, records, chars */
    pl = pool_layout();
    const size_t o_ch = pl.add(n_chars * 4), o_pf = pl.add(n_pts * 8), o_pt = pl.add(n_pts * 8);
    rc = wg.alloc(5, pl, "chars and way points");
    if (rc != OSMT_OK) return rc;
    char* w5 = wg.work[5];
    P.n_chars = (uint32_t)n_chars;
    P.n_pts = (uint32_t)n_pts;
    P.chars = (uint32_t*)(w5 + o_ch);
    P.pts_fwd = (int2*)(w5 + o_pf);
    P.pts = (int2*)(w5 + o_pt);
    HIP_TRY(wg.mark(EV_E0));
    HIP_TRY(osmt_launch_al_emit(P, st));
    HIP_TRY(wg.mark(EV_E1));
    out->labels.resize(n_labels), out->runs.resize(n_labels), out->chars.resize(n_chars), out->pts.resize(2 * n_pts);
    if (n_labels) HIP_TRY(hipMemcpyAsync(out->labels.data(), P.labels, n_labels * sizeof(osmt_label), hipMemcpyDeviceToHost, st));
    if (n_labels) HIP_TRY(hipMemcpyAsync(out->runs.data(), P.runs, n_labels * sizeof(osmt_string_run), hipMemcpyDeviceToHost, st));
    if (n_chars) HIP_TRY(hipMemcpyAsync(out->chars.data(), P.chars, n_chars * 4, hipMemcpyDeviceToHost, st));
    if (n_pts) HIP_TRY(hipMemcpyAsync(out->pts.data(), P.pts, n_pts * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->job_off.data(), P.job_label_off, (n_tiles + 1) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    /* 6. the angles: libm, on the host */
    const auto t0 = std::chrono::steady_clock::now();
    area_label_angles(out->labels, out->runs, out->pts, &out->sincos);
    if (trace) {
        const double angle_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr,
                "osmt area labels: query %.1f us, expand + sort %.1f us, anchors %.1f us, count + scans %.1f us, emit %.1f us, host angles %.1f us "
                "(%zu tiles, %zu candidates, %zu labels, %zu anchor requests, %zu chars, %zu way points, %zu bytes read back)\n",
                wg.us(EV_Q0, EV_Q1), wg.us(EV_X0, EV_X1), wg.us(EV_A0, EV_A1), wg.us(EV_C0, EV_C1), wg.us(EV_E0, EV_E1), angle_us, n_tiles, n_cand, n_labels, n_req, n_chars,
                n_pts, n_labels * (sizeof(osmt_label) + sizeof(osmt_string_run)) + n_chars * 4 + n_pts * 8 + (n_tiles + 1) * 4);
    }
    return OSMT_OK;
}

namespace osmt_host {

int scene_build_tile_labels_all_body(osmt_ctx* ctx, osmt_scene* sc, const uint32_t* area_of_zoom, const uint32_t* node_of_zoom,
                                            const osmt_area_anchor* anchors, size_t n_anchors) {
    if (!ctx || !sc || sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "bad ctx/scene");
    if (!sc->d_tq) return fail(OSMT_INVALID_ARG, "the scene was not built by osmt_scene_build_tiles: it has no tiles to query");
    sc->h_al_declined.clear();
    const size_t n_tiles = sc->n_jobs;
    area_label_batch ab;
    ab.job_off.assign(n_tiles + 1, 0u);
    if (area_of_zoom) {
        const int rc = tile_area_labels_build(ctx, sc, area_of_zoom, anchors, n_anchors, &ab);
        if (rc != OSMT_OK) return rc;
    }
    osmt_string_label_batch area{};
    area.labels = ab.labels.data(), area.n_labels = ab.labels.size(), area.job_label_off = ab.job_off.data(), area.runs = ab.runs.data();
    area.chars = ab.chars.data(), area.n_chars = ab.chars.size();
    area.way_pts = ab.pts.data(), area.way_sincos = ab.sincos.data(), area.n_way_pts = ab.pts.size() / 2;
    node_label_batch nb;
    nb.job_off.assign(n_tiles + 1, 0u);
    if (node_of_zoom) {
        const int rc = tile_node_labels_build(ctx, sc, node_of_zoom, &area, &nb);
        if (rc != OSMT_OK) return rc;
    }
    const int rc = tile_labels_attach(ctx, sc, &area, &nb);
    if (rc != OSMT_OK) return rc;
    sc->h_al_labels.swap(ab.labels);
    sc->h_al_runs.swap(ab.runs);
    sc->h_al_chars.swap(ab.chars);
    sc->h_al_off.swap(ab.job_off);
    sc->h_al_pts.swap(ab.pts);
    sc->h_al_sincos.swap(ab.sincos);
    return OSMT_OK;
}

}  // namespace osmt_host

static int scene_read_declined_anchors_body(osmt_ctx* ctx, osmt_scene* sc, osmt_area_anchor* out, size_t cap, size_t* n) {
    if (!ctx || !sc || sc->ctx != ctx || !n) return fail(OSMT_INVALID_ARG, "NULL argument");
    *n = sc->h_al_declined.size();
    if (!out) return OSMT_OK;
    if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu anchors, the last build declined %zu", cap, *n);
    if (*n) memcpy(out, sc->h_al_declined.data(), *n * sizeof(osmt_area_anchor));
    return OSMT_OK;
}

static int scene_read_tile_area_labels_body(osmt_ctx* ctx, osmt_scene* sc, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, int32_t* way_pts,
                                            double* way_sincos, uint32_t* job_label_off, const size_t* caps, size_t* counts) {
    if (!ctx || !sc || sc->ctx != ctx || !counts) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (sc->h_al_off.empty()) return fail(OSMT_INVALID_ARG, "the scene has no device-built area labels (osmt_scene_build_tile_labels_all)");
    counts[0] = sc->h_al_labels.size(), counts[1] = sc->h_al_chars.size(), counts[2] = sc->h_al_pts.size() / 2;
    if ((labels || runs || chars || way_pts || way_sincos) && !caps) return fail(OSMT_INVALID_ARG, "caps is NULL");
    if ((labels || runs) && caps[0] < counts[0]) return fail(OSMT_INVALID_ARG, "caps[0] = %zu is less than the scene's %zu area labels", caps[0], counts[0]);
    if (chars && caps[1] < counts[1]) return fail(OSMT_INVALID_ARG, "caps[1] = %zu is less than the scene's %zu chars", caps[1], counts[1]);
    if ((way_pts || way_sincos) && caps[2] < counts[2]) return fail(OSMT_INVALID_ARG, "caps[2] = %zu is less than the scene's %zu way points", caps[2], counts[2]);
    if (labels && counts[0]) memcpy(labels, sc->h_al_labels.data(), counts[0] * sizeof(osmt_label));
    if (runs && counts[0]) memcpy(runs, sc->h_al_runs.data(), counts[0] * sizeof(osmt_string_run));
    if (chars && counts[1]) memcpy(chars, sc->h_al_chars.data(), counts[1] * 4);
    if (way_pts && counts[2]) memcpy(way_pts, sc->h_al_pts.data(), counts[2] * 8);
    if (way_sincos && counts[2]) memcpy(way_sincos, sc->h_al_sincos.data(), counts[2] * 16);
    if (job_label_off) memcpy(job_label_off, sc->h_al_off.data(), sc->h_al_off.size() * 4);
    return OSMT_OK;
}

int osmt_validate_area_label_bindings(const osmt_area_label_bindings_desc* b, osmt_ctx* ctx) {
    return guarded([&] { return validate_area_label_bindings(b, ctx, nullptr, nullptr); });
}
int osmt_register_area_label_bindings(osmt_ctx* ctx, const osmt_area_label_bindings_desc* b, uint32_t* out_bindings_id) {
    return guarded([&] { return register_area_label_bindings_body(ctx, b, out_bindings_id); });
}
int osmt_scene_build_tile_labels_all(osmt_ctx* ctx, osmt_scene* scene, const uint32_t area_bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                                     const uint32_t node_bindings_of_zoom[OSMT_MAX_ZOOM + 1], const osmt_area_anchor* anchors, size_t n_anchors) {
    return guarded([&] { return scene_build_tile_labels_all_body(ctx, scene, area_bindings_of_zoom, node_bindings_of_zoom, anchors, n_anchors); });
}
int osmt_scene_read_declined_anchors(osmt_ctx* ctx, osmt_scene* scene, osmt_area_anchor* out, size_t cap, size_t* n) {
    return guarded([&] { return scene_read_declined_anchors_body(ctx, scene, out, cap, n); });
}
int osmt_scene_read_tile_area_labels(osmt_ctx* ctx, osmt_scene* scene, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, int32_t* way_pts,
                                     double* way_sincos, uint32_t* job_label_off, const size_t caps[3], size_t counts[3]) {
    return guarded([&] { return scene_read_tile_area_labels_body(ctx, scene, labels, runs, chars, way_pts, way_sincos, job_label_off, caps, counts); });
}

int osmt_validate_node_mercator(const double* factors, size_t n_nodes, uint32_t geodata_id, osmt_ctx* ctx) {
    return guarded([&] { return validate_node_mercator(factors, n_nodes, geodata_id, ctx); });
}

int osmt_register_node_mercator(osmt_ctx* ctx, uint32_t geodata_id, const double* factors) {
    return guarded([&] { return register_node_mercator_body(ctx, geodata_id, factors); });
}

int osmt_validate_label_tile_batch(const osmt_label_tile_batch* b, osmt_ctx* ctx) {
    return guarded([&] { return validate_label_tile_batch(b, ctx, nullptr); });
}

int osmt_label_positions_tiles_begin(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_label_job** out_job) {
    return guarded([&] { return osmt_label_positions_tiles_begin_body(ctx, b, out_job); });
}

int osmt_label_positions_tiles(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_label_position* out) {
    return guarded([&] {
        if (b && b->n_requests && !out) return fail(OSMT_INVALID_ARG, "out is NULL");
        osmt_label_job* j = nullptr;
        const int rc = osmt_label_positions_tiles_begin_body(ctx, b, &j);
        return rc != OSMT_OK ? rc : osmt_label_positions_end_body(j, out);
    });
}

int osmt_label_tile_batch_expand(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_ring* rings, double* points, size_t rings_cap, size_t points_cap,
                                 size_t counts[2]) {
    return guarded([&] { return osmt_label_tile_batch_expand_body(ctx, b, rings, points, rings_cap, points_cap, counts); });
}

static int osmt_scene_read_label_status_body(osmt_ctx* ctx, osmt_scene* sc, uint8_t* ok) {
    if (!ctx || !sc || sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "bad ctx/scene");
    if (sc->n_labels == 0) return OSMT_OK;
    if (!ok) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    uint32_t err = 0;
    HIP_TRY(copy_back(ctx, &err, sc->d_lab_err, 4));
    if (err) return fail(OSMT_HIP_ERROR, "label coverage window overflow (internal error %u)", err);
    HIP_TRY(copy_back(ctx, ok, sc->d_lab_ok, sc->n_labels));
    return OSMT_OK;
}

int osmt_scene_read_label_status(osmt_ctx* ctx, osmt_scene* sc, uint8_t* ok) {
    return guarded([&] { return osmt_scene_read_label_status_body(ctx, sc, ok); });
}

static int osmt_render_scene_body(osmt_ctx* ctx, osmt_scene* scene, void* d_out_rgba, size_t stride, void* stream) {
    return render_impl(ctx, scene, 7u, d_out_rgba, stride, false, stream);
}

int osmt_render_scene(osmt_ctx* ctx, osmt_scene* scene, void* d_out_rgba, size_t stride, void* stream) {
    return guarded([&] { return osmt_render_scene_body(ctx, scene, d_out_rgba, stride, stream); });
}

static int osmt_render_scene_f64_body(osmt_ctx* ctx, osmt_scene* scene, void* d_out_f64, void* stream) {
    return render_impl(ctx, scene, 7u, d_out_f64, 0, true, stream);
}

int osmt_render_scene_f64(osmt_ctx* ctx, osmt_scene* scene, void* d_out_f64, void* stream) {
    return guarded([&] { return osmt_render_scene_f64_body(ctx, scene, d_out_f64, stream); });
}

static int osmt_render_scene_stages_body(osmt_ctx* ctx, osmt_scene* scene, uint32_t stage_mask, void* d_out_rgba, size_t stride,
                             void* stream) {
    return render_impl(ctx, scene, stage_mask & 7u, d_out_rgba, stride, false, stream);
}

int osmt_render_scene_stages(osmt_ctx* ctx, osmt_scene* scene, uint32_t stage_mask, void* d_out_rgba, size_t stride,
                             void* stream) {
    return guarded([&] { return osmt_render_scene_stages_body(ctx, scene, stage_mask, d_out_rgba, stride, stream); });
}

static int osmt_scene_check_body(osmt_ctx* ctx, osmt_scene* sc) {
    if (!ctx || !sc || sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "bad ctx/scene");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    return prepass_error_check(sc);
}

int osmt_scene_check(osmt_ctx* ctx, osmt_scene* scene) {
    return guarded([&] { return osmt_scene_check_body(ctx, scene); });
}

static int osmt_scene_read_points_body(osmt_ctx* ctx, osmt_scene* sc, int32_t* xy) {
    if (!ctx || !sc || !xy) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(scene_wait_idle(sc));
    if (sc->n_pts) HIP_TRY(copy_back(ctx, xy, sc->d_pts, (size_t)sc->n_pts * 8));
    return OSMT_OK;
}

int osmt_scene_read_points(osmt_ctx* ctx, osmt_scene* sc, int32_t* xy) {
    return guarded([&] { return osmt_scene_read_points_body(ctx, sc, xy); });
}

int osmt_render_batch(osmt_ctx* ctx, const osmt_batch* batch, uint8_t* out_rgba, size_t stride) {
    return osmt_render_batch_labels(ctx, batch, nullptr, out_rgba, stride);
}

static int osmt_render_batch_labels_once(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba, size_t stride,
                                         bool rgb, bool trusted, bool allow_guess, const osmt_glyph_label_batch* glabels,
                                         const osmt_text_label_batch* tlabels, const osmt_string_label_batch* slabels);

namespace osmt_host {

/* the host-buffer render: arenas guessed from the recent densities first; a miss renders again with exact sizing */
int osmt_render_batch_labels_body(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba,
                                         size_t stride, bool rgb, bool trusted, const osmt_glyph_label_batch* glabels,
                                         const osmt_text_label_batch* tlabels, const osmt_string_label_batch* slabels) {
    g_arena_guess_missed = false;
    int rc = osmt_render_batch_labels_once(ctx, batch, labels, out_rgba, stride, rgb, trusted, true, glabels, tlabels, slabels);
    if (rc != OSMT_OK && g_arena_guess_missed) {
        g_arena_guess_missed = false;
        rc = osmt_render_batch_labels_once(ctx, batch, labels, out_rgba, stride, rgb, true, false, glabels, tlabels, slabels); /* validated the first time */
    }
    return rc;
}

}  // namespace osmt_host

/* The back half of every host-buffer render, where the scene exists: shared by the batch forms (a per-call scene that lives
 * on `st`) and osmt_render_scene_host (a public scene, borrowed).  Takes one of three routes — zero-copy, the two-stream
 * chunked read-back, one plain copy — and returns with the pixels in out_rgba and both streams idle.  The caller owns the
 * scene and `st`. */
static int scene_render_host_back(osmt_ctx* ctx, osmt_scene* sc, hipStream_t st, uint8_t* out_rgba, size_t stride, bool rgb) {
    const uint32_t n_jobs = sc->n_jobs, scale = sc->scale;
    const size_t W = (size_t)OSMT_TILE_SIZE * scale;
    const size_t tile_bytes = W * W * 4;                   /* what k_raster writes */
    const size_t host_bytes = rgb ? W * W * 3 : tile_bytes; /* what crosses PCIe */
    int rc = OSMT_OK;
    if (stride < host_bytes) return fail(OSMT_INVALID_ARG, rgb ? "out_tile_stride_bytes < W*H*3" : "out_tile_stride_bytes < W*H*4");
    /* Output in pinned host memory (osmt_host_alloc / hipHostMalloc / a registered range) and a batch worth
     * splitting: kernels of chunk k overlap the D2H copy of chunk k-1 on a second stream. */
    bool pinned = false;
    if (n_jobs >= 2u * std::max<uint32_t>(1u, 128u / (scale * scale))) { /* the query is not free: only where it can pay */
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, out_rgba) == hipSuccess)
            pinned = at.type == hipMemoryTypeHost;
        else
            (void)hipGetLastError();
    }
    const uint32_t chunk = std::max<uint32_t>(1u, 128u / (scale * scale));
    if (pinned && n_jobs >= 2u * chunk) {
        hipStream_t s_k = st, s_c = nullptr; /* kernels stay on the call's stream (the scene was uploaded there) */
        hipEvent_t done[2] = {nullptr, nullptr}, freed[2] = {nullptr, nullptr};
        char* d_out = nullptr;
        hipError_t e = stream_acquire(ctx, &s_c);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&freed[k], hipEventDisableTiming);
        }
        char* d_rgb = nullptr;
        /* RGB8: k_raster packs the triples itself (no RGBA8 framebuffer, no packing kernel) */
        if (e == hipSuccess && !rgb) e = dev_alloc(ctx, (void**)&d_out, 2 * (size_t)chunk * tile_bytes);
        if (e == hipSuccess && rgb) e = dev_alloc(ctx, (void**)&d_rgb, 2 * (size_t)chunk * host_bytes);
        if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "pipeline setup failed: %s", hipGetErrorString(e));
        if (rc == OSMT_OK) rc = render_impl(ctx, sc, 1u | 2u | 8u, nullptr, tile_bytes, false, s_k);
        uint32_t c = 0;
        for (uint32_t first = 0; rc == OSMT_OK && first < n_jobs; first += chunk, ++c) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(chunk, n_jobs - first);
            const int k = (int)(c & 1u);
            char* dst = rgb ? d_rgb + (size_t)k * chunk * host_bytes : d_out + (size_t)k * chunk * tile_bytes;
            if (c >= 2) e = hipStreamWaitEvent(s_k, freed[k], 0);
            if (e == hipSuccess) rc = render_impl(ctx, sc, 4u | 16u | (rgb ? 32u : 0u), dst, host_bytes, false, s_k, first, cnt);
            if (rc != OSMT_OK) break;
            const char* src = dst;
            if (e == hipSuccess) e = hipEventRecord(done[k], s_k);
            if (e == hipSuccess) e = hipStreamWaitEvent(s_c, done[k], 0);
            if (e == hipSuccess) {
                if (stride == host_bytes) /* tightly packed tiles: one linear copy (2D copies are slower) */
                    e = hipMemcpyAsync(out_rgba + (size_t)first * stride, src, (size_t)cnt * host_bytes, hipMemcpyDeviceToHost, s_c);
                else
                    e = hipMemcpy2DAsync(out_rgba + (size_t)first * stride, stride, src, host_bytes, host_bytes, cnt,
                                         hipMemcpyDeviceToHost, s_c);
            }
            if (e == hipSuccess) e = hipEventRecord(freed[k], s_c);
            if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "pipelined readback failed: %s", hipGetErrorString(e));
        }
        if (s_k) (void)hipStreamSynchronize(s_k);
        if (rc == OSMT_OK) rc = label_error_check(sc, s_k);
        if (s_c) {
            e = hipStreamSynchronize(s_c);
            if (e != hipSuccess && rc == OSMT_OK) rc = fail(OSMT_HIP_ERROR, "pipelined readback failed: %s", hipGetErrorString(e));
        }
        for (int k = 0; k < 2; ++k) {
            if (done[k]) (void)hipEventDestroy(done[k]);
            if (freed[k]) (void)hipEventDestroy(freed[k]);
        }
        dev_free(ctx, d_out);
        dev_free(ctx, d_rgb);
        stream_release(ctx, s_c);
        return rc;
    }
    void* d_out = nullptr;
    /* A FEW tiles into PINNED caller memory (osmt_host_alloc / hipHostMalloc: mapped into the device's address space): k_raster
     * writes the pixels straight there — no device framebuffer, no copy.  Round 5 measured why it matters: asynchronous
     * device-to-host copies into pinned buffers from several threads at once queue up behind each other in the runtime (one-tile
     * requests, 4 threads: 10.9 k tiles/s with pinned caller buffers against 35.5 k with pageable ones, which the runtime
     * copies synchronously on the calling thread; profiles/r05_f_worker_pinned.txt).  The worker entry's gathered groups land
     * in the library's own pinned staging, so they take this path too: 16 tiles = the groups that 32 request threads form
     * (98 k tiles/s against 73 k with 8 tiles, the same with 32; profiles/r05_h_zero_copy_threshold.txt).
     * OSMT_ZERO_COPY_TILES: most tiles of such a call (0: never). */
    bool zero_copy = false;
    static const uint32_t zc_max = [] {
        const char* v = getenv("OSMT_ZERO_COPY_TILES");
        return (uint32_t)(v ? std::min(std::max(atoi(v), 0), 64) : 16);
    }();
    if (n_jobs && n_jobs <= zc_max && ((uintptr_t)out_rgba & 3u) == 0u && (stride & 3u) == 0u) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, out_rgba) == hipSuccess) {
            if (at.type == hipMemoryTypeHost && at.devicePointer) {
                d_out = at.devicePointer;
                zero_copy = true;
            }
        } else {
            (void)hipGetLastError(); /* pageable memory: not an error */
        }
    }
    if (n_jobs && !zero_copy) {
        hipError_t e = dev_alloc(ctx, &d_out, n_jobs * host_bytes); /* RGB8: written by k_raster as packed triples */
        if (e != hipSuccess) return fail(OSMT_OOM, "hipMalloc(output) failed: %s", hipGetErrorString(e));
    }
    rc = render_impl(ctx, sc, 7u | (rgb ? 32u : 0u), d_out ? d_out : (void*)4, zero_copy ? stride : host_bytes, false, st);
    if (rc == OSMT_OK && n_jobs) {
        hipError_t e = hipSuccess;
        const void* src = d_out;
        if (rc == OSMT_OK && e == hipSuccess && !zero_copy) {
            if (stride == host_bytes)
                e = hipMemcpyAsync(out_rgba, src, n_jobs * host_bytes, hipMemcpyDeviceToHost, st);
            else
                e = hipMemcpy2DAsync(out_rgba, stride, src, host_bytes, host_bytes, n_jobs, hipMemcpyDeviceToHost, st);
        }
        if (rc == OSMT_OK && e == hipSuccess) e = n_jobs <= 64 ? stream_sync_small(st) : hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "readback failed: %s", hipGetErrorString(e));
    }
    if (rc == OSMT_OK) rc = label_error_check(sc, st);
    if (rc != OSMT_OK) { /* whatever was queued may still write d_out; keep the reason across the wait */
        const std::string msg = osmt_last_error();
        (void)hipStreamSynchronize(st);
        rc = fail(rc, "%s", msg.c_str());
    }
    if (!zero_copy) dev_free(ctx, d_out);
    return rc;
}

static int osmt_render_batch_labels_once(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba, size_t stride,
                                         bool rgb, bool trusted, bool allow_guess, const osmt_glyph_label_batch* glabels,
                                         const osmt_text_label_batch* tlabels, const osmt_string_label_batch* slabels) {
    if (!ctx || !out_rgba) return fail(OSMT_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = nullptr; /* the whole call lives on its own stream: concurrent callers overlap on the GPU */
    HIP_TRY(stream_acquire(ctx, &st));
    osmt_scene* sc = nullptr;
    int rc = scene_upload_impl(ctx, batch, &sc, st, trusted, allow_guess);
    if (rc != OSMT_OK) {
        stream_release(ctx, st);
        return rc;
    }
    if (labels || glabels || tlabels || slabels) {
        rc = labels ? osmt_scene_set_labels(ctx, sc, labels)
                    : glabels ? osmt_scene_set_glyph_labels(ctx, sc, glabels)
                              : tlabels ? osmt_scene_set_text_labels(ctx, sc, tlabels) : osmt_scene_set_string_labels(ctx, sc, slabels);
        if (rc != OSMT_OK) {
            osmt_scene_free(sc);
            stream_release(ctx, st);
            return rc;
        }
    }
    rc = scene_render_host_back(ctx, sc, st, out_rgba, stride, rgb);
    const std::string msg = rc != OSMT_OK ? std::string(osmt_last_error()) : std::string();
    const bool missed = g_arena_guess_missed; /* set by the back half's error check; osmt_scene_free does not touch it */
    osmt_scene_free(sc); /* waits for the call's stream */
    stream_release(ctx, st);
    g_arena_guess_missed = missed;
    return rc != OSMT_OK ? fail(rc, "%s", msg.c_str()) : OSMT_OK;
}

/* osmt_render_scene_host: the same back half on a borrowed public scene. */
static int osmt_render_scene_host_body(osmt_ctx* ctx, osmt_scene* sc, uint32_t format, uint8_t* out, size_t stride) {
    if (!ctx || !sc || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "the scene belongs to another context");
    if (format != OSMT_PIXELS_RGBA8 && format != OSMT_PIXELS_RGB8) return fail(OSMT_INVALID_ARG, "unknown pixel format %u", format);
    const bool rgb = format == OSMT_PIXELS_RGB8;
    const size_t W = (size_t)OSMT_TILE_SIZE * sc->scale;
    if (stride < W * W * (rgb ? 3u : 4u)) return fail(OSMT_INVALID_ARG, rgb ? "out_tile_stride_bytes < W*H*3" : "out_tile_stride_bytes < W*H*4");
    if (rgb && ((stride & 3u) || ((uintptr_t)out & 3u))) return fail(OSMT_INVALID_ARG, "RGB8 output: pointer or tile stride not a multiple of 4");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = nullptr;
    HIP_TRY(stream_acquire(ctx, &st));
    int rc = OSMT_OK;
    const hipError_t e = scene_wait_idle(sc); /* the pre-pass rewrites the scene's lists: its earlier launches first */
    if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "scene: %s", hipGetErrorString(e));
    if (rc == OSMT_OK) rc = scene_render_host_back(ctx, sc, st, out, stride, rgb);
    stream_release(ctx, st);
    return rc;
}

int osmt_render_scene_host(osmt_ctx* ctx, osmt_scene* scene, uint32_t format, uint8_t* out, size_t out_tile_stride_bytes) {
    return guarded([&] { return osmt_render_scene_host_body(ctx, scene, format, out, out_tile_stride_bytes); });
}

int osmt_render_batch_rgb(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgb, size_t stride) {
    return guarded([&] { return osmt_render_batch_labels_body(ctx, batch, labels, out_rgb, stride, true); });
}

int osmt_render_batch_rgb_glyphs(osmt_ctx* ctx, const osmt_batch* batch, const osmt_glyph_label_batch* labels, uint8_t* out_rgb, size_t stride) {
    return guarded([&] { return osmt_render_batch_labels_body(ctx, batch, nullptr, out_rgb, stride, true, false, labels); });
}

int osmt_render_batch_rgb_text(osmt_ctx* ctx, const osmt_batch* batch, const osmt_text_label_batch* labels, uint8_t* out_rgb, size_t stride) {
    return guarded([&] { return osmt_render_batch_labels_body(ctx, batch, nullptr, out_rgb, stride, true, false, nullptr, labels); });
}

int osmt_render_batch_rgb_strings(osmt_ctx* ctx, const osmt_batch* batch, const osmt_string_label_batch* labels, uint8_t* out_rgb, size_t stride) {
    return guarded([&] { return osmt_render_batch_labels_body(ctx, batch, nullptr, out_rgb, stride, true, false, nullptr, nullptr, labels); });
}

int osmt_render_batch_labels(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba,
                             size_t stride) {
    return guarded([&] { return osmt_render_batch_labels_body(ctx, batch, labels, out_rgba, stride); });
}

/* ---- PNG files straight from the GPU -------------------------------------- */
static uint32_t ihdr_crc(uint32_t W, uint32_t H) {
    /* CRC-32 of "IHDR" + width, height, 8, 2, 0, 0, 0 (bitwise; once per call) */
    uint8_t b[17] = {'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                     (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, 2, 0, 0, 0};
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t v : b) {
        c ^= v;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

size_t osmt_png_device_bound(uint32_t W, uint32_t H) {
    /* 43 header bytes + one deflate block (its constant header, then at most PNG_LMAX bits per filtered byte, EOB) +
     * Adler, CRC, IEND */
    const size_t bits = PNG_BLOCK_HDR_BITS + (size_t)H * (3 * (size_t)W + 1) * PNG_LMAX + PNG_LMAX;
    /* + slack: the fast kernel stages its eight row bands in the slot behind the header words, each rounded up to words (3 words per band) */
    return align_up(43 + (bits + 7) / 8 + 4 + 4 + 12 + 8 + 4 * PNG_HEAD_WORDS + 128, 256);
}

static int osmt_encode_png_device_body(osmt_ctx* ctx, const void* d_rgba, size_t tile_stride, uint32_t n, uint32_t W, uint32_t H, void* d_png,
                           size_t png_stride, uint32_t* d_len, void* stream) {
    if (!ctx) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (n == 0) return OSMT_OK;
    if (!d_rgba || !d_png || !d_len) return fail(OSMT_INVALID_ARG, "NULL device pointer");
    if (W == 0 || H == 0 || W > 1024 || (W % 4) != 0) return fail(OSMT_UNSUPPORTED, "PNG width %u not supported (multiple of 4, <= 1024)", W);
    /* k_png_encode keeps one LDS word per row (position, Adler sums): PNG_MAX_W of them */
    if (H > 1024) return fail(OSMT_UNSUPPORTED, "PNG height %u not supported (<= 1024)", H);
    if (tile_stride < (size_t)W * H * 4 || (tile_stride % 4) != 0) return fail(OSMT_INVALID_ARG, "tile stride too small / not a multiple of 4");
    if (png_stride < osmt_png_device_bound(W, H) || (png_stride % 4) != 0) return fail(OSMT_INVALID_ARG, "png_stride < osmt_png_device_bound()");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(osmt_launch_png(d_rgba, tile_stride, n, W, H, ihdr_crc(W, H), d_png, png_stride, d_len, (hipStream_t)stream));
    return OSMT_OK;
}

int osmt_encode_png_device(osmt_ctx* ctx, const void* d_rgba, size_t tile_stride, uint32_t n, uint32_t W, uint32_t H, void* d_png,
                           size_t png_stride, uint32_t* d_len, void* stream) {
    return guarded([&] { return osmt_encode_png_device_body(ctx, d_rgba, tile_stride, n, W, H, d_png, png_stride, d_len, stream); });
}

/* One call, its own pipeline.  The pre-pass runs once for the whole batch; then the tiles go through raster -> PNG
 * encode -> file lengths in CHUNKS on the call's stream, all enqueued up front.  The host walks the chunks behind the
 * GPU: as soon as a chunk's lengths are back it sums the file offsets and queues that chunk's compaction and read-back
 * on a second stream — the PCIe transfer of chunk c runs under the kernels of chunk c + 1. */
/* One batch on its way through the PNG pipeline: everything osmt_render_batch_png_begin queued and what
 * osmt_render_batch_png_end needs to finish it. */
struct osmt_png_job {
    osmt_ctx* ctx = nullptr;
    hipStream_t st = nullptr, s_c = nullptr; /* the job's own stream; the compaction / read-back stream (more than one chunk) */
    osmt_scene* sc = nullptr;
    bool owns_scene = true;    /* false: begun from the caller's scene (osmt_render_scene_png_begin), which outlives the job */
    char* d = nullptr;         /* framebuffers of two chunks, PNG slots, lengths, offsets */
    char* d_blob = nullptr;    /* compacted files, ONLY when a chunk's dead framebuffers cannot take them (see png_end_body) */
    uint32_t* h_len = nullptr; /* pinned: lengths come back asynchronously, offsets go out */
    std::vector<hipEvent_t> ev;
    uint32_t n = 0, W = 0, chunk = 0, n_chunks = 0;
    size_t slot = 0, tile_bytes = 0, o_rgba = 0, o_png = 0, o_len = 0, o_off = 0;
    int rc = OSMT_OK; /* a failure of the first half, reported by the second */
    std::string err;
    const osmt_batch* batch = nullptr; /* the caller's arrays (valid until _end returns): a missed arena guess renders them again */
    const osmt_label_batch* labels = nullptr;
};

static void png_job_release(osmt_png_job* j) {
    if (!j) return;
    osmt_ctx* ctx = j->ctx;
    for (hipEvent_t v : j->ev)
        if (v) (void)hipEventDestroy(v);
    if (j->sc && j->owns_scene) {
        osmt_scene_free(j->sc); /* waits for the job's stream */
    } else { /* a borrowed scene stays; the job's buffers and streams go back only once nothing queued can touch them */
        if (j->s_c) (void)hipStreamSynchronize(j->s_c);
        if (j->st) (void)hipStreamSynchronize(j->st);
    }
    dev_free(ctx, j->d);
    dev_free(ctx, j->d_blob);
    if (j->h_len) stage_release(ctx, j->h_len);
    if (j->s_c) stream_release(ctx, j->s_c);
    if (j->st) stream_release(ctx, j->st);
    delete j;
    /* the job's own reference (png_begin_body), dropped LAST: a job that outlives osmt_destroy — ended or dropped after the
     * caller closed the context — would otherwise free its scene, with it the last reference, and then hand buffers and streams
     * back to a context that ctx_teardown has deleted */
    ctx_release(ctx);
}

/* A job with its context reference and its own stream, nothing else yet. */
static int png_job_new(osmt_ctx* ctx, osmt_png_job** out) {
    osmt_png_job* j = new (std::nothrow) osmt_png_job();
    if (!j) return fail(OSMT_OOM, "out of host memory");
    j->ctx = ctx;
    ctx->refs.fetch_add(1); /* like a scene: the context outlives its jobs (released at the end of png_job_release) */
    hipError_t e = stream_acquire(ctx, &j->st); /* the whole job lives on its own stream */
    if (e != hipSuccess) {
        delete j;
        ctx_release(ctx);
        return fail(OSMT_HIP_ERROR, "stream: %s", hipGetErrorString(e));
    }
    *out = j;
    return OSMT_OK;
}

/* The back half of both _begin forms, where the scene exists (j->sc: the batch form's own, or the caller's): the pre-pass
 * once, then the tiles through raster -> PNG encode -> file lengths in CHUNKS on the job's stream, all enqueued here;
 * nothing is waited for. */
static int png_begin_back(osmt_ctx* ctx, osmt_png_job* j) {
    int rc = OSMT_OK;
    hipError_t e = hipSuccess;
    const uint32_t n = j->n = j->sc->n_jobs, scale = j->sc->scale;
    if (n) {
        const uint32_t W = j->W = OSMT_TILE_SIZE * scale;
        const size_t tile_bytes = (size_t)W * W * 4, slot = j->slot = osmt_png_device_bound(W, W);
        /* the encoder is one workgroup per tile: below ~2 workgroups per CU it is latency-bound and a chunk costs more than
         * its overlap brings (measured on 1024 tiles: 1 chunk 4.21 ms, 2 chunks 4.10, 4 chunks 4.82, 8 chunks 7.07) */
        const uint32_t min_chunk = std::max<uint32_t>(1u, 512u / (scale * scale));
        uint32_t chunk = n;
        if (n >= 2u * min_chunk) chunk = std::max<uint32_t>(min_chunk, (n + 1u) / 2u);
        /* OSMT_PNG_CHUNKS (diagnostic: force the number of chunks): read ONCE — getenv on every call from worker threads is
         * not safe against a host that calls setenv — and clamped, so that a large value cannot turn one call into n events,
         * n tiny encode launches and n copies */
        static const int forced_chunks = [] {
            const char* v = getenv("OSMT_PNG_CHUNKS");
            return v ? std::min(std::max(atoi(v), 1), 16) : 0;
        }();
        if (forced_chunks) chunk = std::max<uint32_t>(1u, (n + (uint32_t)forced_chunks - 1u) / (uint32_t)forced_chunks);
        j->chunk = chunk;
        const uint32_t n_chunks = j->n_chunks = (n + chunk - 1u) / chunk;
        pool_layout pl;
        const size_t o_rgba = j->o_rgba = pl.add((size_t)std::min<uint32_t>(2u, n_chunks) * chunk * tile_bytes); /* two chunks of framebuffers, alternating */
        j->tile_bytes = tile_bytes;
        j->o_png = pl.add((size_t)n * slot);
        j->o_len = pl.add((size_t)n * 4);
        j->o_off = pl.add((size_t)n * 8);
        e = dev_alloc(ctx, (void**)&j->d, pl.size());
        if (e != hipSuccess) rc = fail(OSMT_OOM, "hipMalloc(%zu) failed: %s", pl.size(), hipGetErrorString(e));
        if (rc == OSMT_OK) {
            j->h_len = (uint32_t*)stage_acquire(ctx, (size_t)n * 12 + 16);
            if (!j->h_len) rc = fail(OSMT_OOM, "pinned staging for %u file lengths", n);
        }
        if (rc == OSMT_OK && n_chunks > 1u) {
            e = stream_acquire(ctx, &j->s_c);
            if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "stream: %s", hipGetErrorString(e));
        }
        j->ev.assign(n_chunks, nullptr);
        for (uint32_t c = 0; rc == OSMT_OK && c < n_chunks; ++c) {
            e = hipEventCreateWithFlags(&j->ev[c], hipEventDisableTiming);
            if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "event: %s", hipGetErrorString(e));
        }
        /* ---- everything the GPU has to do, queued at once ---- */
        if (rc == OSMT_OK) rc = render_impl(ctx, j->sc, 1u | 2u | 8u, nullptr, tile_bytes, false, j->st);
        for (uint32_t c = 0; rc == OSMT_OK && c < n_chunks; ++c) {
            const uint32_t first = c * chunk, cnt = std::min(chunk, n - first);
            char* rgba = j->d + o_rgba + (size_t)(c & 1u) * chunk * tile_bytes;
            rc = render_impl(ctx, j->sc, 4u | 16u, rgba, tile_bytes, false, j->st, first, cnt);
            if (rc == OSMT_OK)
                rc = osmt_encode_png_device(ctx, rgba, tile_bytes, cnt, W, W, j->d + j->o_png + (size_t)first * slot, slot,
                                            (uint32_t*)(j->d + j->o_len) + first, j->st);
            if (rc == OSMT_OK) {
                e = hipMemcpyAsync(j->h_len + first, j->d + j->o_len + (size_t)first * 4, (size_t)cnt * 4, hipMemcpyDeviceToHost, j->st);
                if (e == hipSuccess) e = hipEventRecord(j->ev[c], j->st);
                if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "PNG pipeline: %s", hipGetErrorString(e));
            }
        }
    }
    return rc;
}

/* First half of the batch form: validate, upload, attach the labels, then the shared back half. */
static int png_begin_body(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, osmt_png_job** out_job, bool allow_guess = true) {
    if (!ctx || !out_job) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_job = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    osmt_png_job* j = nullptr;
    int rc = png_job_new(ctx, &j);
    if (rc != OSMT_OK) return rc;
    j->batch = batch;
    j->labels = labels;
    rc = scene_upload_impl(ctx, batch, &j->sc, j->st, false, allow_guess);
    if (rc == OSMT_OK && labels) rc = osmt_scene_set_labels(ctx, j->sc, labels);
    if (rc == OSMT_OK) rc = png_begin_back(ctx, j);
    if (rc != OSMT_OK) {
        const std::string msg = osmt_last_error();
        png_job_release(j);
        return fail(rc, "%s", msg.c_str());
    }
    *out_job = j;
    return OSMT_OK;
}

/* First half of the scene form.  The scene is borrowed: the job waits for the scene's earlier launches (the pre-pass rewrites
 * its lists — a second job on the same scene is therefore serialised behind the first one's raster), marks its own (render_impl)
 * and never frees it. */
static int scene_png_begin_body(osmt_ctx* ctx, osmt_scene* sc, osmt_png_job** out_job) {
    if (out_job) *out_job = nullptr;
    if (!ctx || !sc || !out_job) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "the scene belongs to another context");
    HIP_TRY(hipSetDevice(ctx->device));
    osmt_png_job* j = nullptr;
    int rc = png_job_new(ctx, &j);
    if (rc != OSMT_OK) return rc;
    j->sc = sc;
    j->owns_scene = false;
    const hipError_t e = scene_wait_idle(sc);
    if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "scene: %s", hipGetErrorString(e));
    if (rc == OSMT_OK) rc = png_begin_back(ctx, j);
    if (rc != OSMT_OK) {
        const std::string msg = osmt_last_error();
        png_job_release(j);
        return fail(rc, "%s", msg.c_str());
    }
    *out_job = j;
    return OSMT_OK;
}

/* Second half.  The host walks the chunks behind the GPU: as soon as a chunk's lengths are back it sums the file
 * offsets and queues that chunk's compaction and read-back on a second stream — the PCIe transfer of chunk c runs under
 * the kernels of chunk c + 1 (and under the kernels of the NEXT job, when the caller has already begun one).  Releases
 * the job whatever happens. */
static int png_end_body(osmt_png_job* j, uint8_t* out_png, size_t out_capacity, uint64_t* out_off) {
    if (!j) return fail(OSMT_INVALID_ARG, "NULL job");
    if (!out_off || (!out_png && out_capacity)) {
        png_job_release(j);
        return fail(OSMT_INVALID_ARG, "NULL argument");
    }
    osmt_ctx* ctx = j->ctx;
    int rc = OSMT_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "hipSetDevice: %s", hipGetErrorString(e));
    const uint32_t n = j->n, chunk = j->chunk;
    std::vector<unsigned long long> offs((size_t)n + 1, 0ull);
    if (rc == OSMT_OK && n) {
        unsigned long long* const h_off = reinterpret_cast<unsigned long long*>(j->h_len + ((n + 1u) & ~1u)); /* chunk-relative offsets */
        hipStream_t s_copy = j->s_c ? j->s_c : j->st;
        char* const d = j->d;
        const size_t slot = j->slot;
        bool fits = true;
        for (uint32_t c = 0; rc == OSMT_OK && c < j->n_chunks; ++c) {
            const uint32_t first = c * chunk, cnt = std::min(chunk, n - first);
            e = hipEventSynchronize(j->ev[c]);
            if (e != hipSuccess) {
                rc = fail(OSMT_HIP_ERROR, "PNG pipeline: %s", hipGetErrorString(e));
                break;
            }
            for (uint32_t i = 0; i < cnt; ++i) {
                h_off[first + i] = offs[first + i] - offs[first];
                offs[first + i + 1] = offs[first + i] + j->h_len[first + i];
            }
            const size_t c_bytes = (size_t)(offs[first + cnt] - offs[first]);
            if (offs[first + cnt] > out_capacity) fits = false; /* keep summing: the caller learns the size it needs */
            if (!fits || c_bytes == 0) continue;
            /* The compacted files of a chunk go where its framebuffers were: they are dead once the chunk is encoded (the
             * event above), each chunk has its own as long as there are at most two, and map tiles compress to a fifth of
             * them.  Only files that would not fit (noise: the slot bound is 12 bits per byte) or a forced chunk count above
             * two (framebuffers re-used by chunk c + 2) get a buffer of their own. */
            char* blob = d + j->o_rgba + (size_t)(c & 1u) * chunk * j->tile_bytes;
            static const bool own_blob = [] { /* diagnostic: OSMT_PNG_OWN_BLOB=1 always compacts into a buffer of its own */
                const char* v = getenv("OSMT_PNG_OWN_BLOB");
                return v && atoi(v) != 0;
            }();
            if (own_blob || j->n_chunks > 2u || c_bytes > (size_t)cnt * j->tile_bytes) {
                if (!j->d_blob) {
                    e = dev_alloc(ctx, (void**)&j->d_blob, (size_t)n * slot);
                    if (e != hipSuccess) {
                        rc = fail(OSMT_OOM, "hipMalloc(%zu) failed: %s", (size_t)n * slot, hipGetErrorString(e));
                        break;
                    }
                }
                blob = j->d_blob + (size_t)first * slot;
            }
            e = hipMemcpyAsync(d + j->o_off + (size_t)first * 8, h_off + first, (size_t)cnt * 8, hipMemcpyHostToDevice, s_copy);
            if (e == hipSuccess)
                e = osmt_launch_png_compact(d + j->o_png + (size_t)first * slot, slot, (const uint32_t*)(d + j->o_len) + first,
                                            (const unsigned long long*)(d + j->o_off) + first, cnt, blob, s_copy);
            if (e == hipSuccess) e = hipMemcpyAsync(out_png + offs[first], blob, c_bytes, hipMemcpyDeviceToHost, s_copy);
            if (e != hipSuccess) rc = fail(OSMT_HIP_ERROR, "PNG readback failed: %s", hipGetErrorString(e));
        }
        if (j->s_c) {
            e = hipStreamSynchronize(j->s_c);
            if (e != hipSuccess && rc == OSMT_OK) rc = fail(OSMT_HIP_ERROR, "PNG readback failed: %s", hipGetErrorString(e));
        }
        e = hipStreamSynchronize(j->st);
        if (e != hipSuccess && rc == OSMT_OK) rc = fail(OSMT_HIP_ERROR, "PNG pipeline: %s", hipGetErrorString(e));
        if (rc == OSMT_OK && !fits) rc = fail(OSMT_INVALID_ARG, "out_capacity %zu < %llu bytes of PNG data", out_capacity, offs[n]);
    }
    for (uint32_t i = 0; i <= n; ++i) out_off[i] = offs[i];
    g_arena_guess_missed = false;
    if (rc == OSMT_OK) rc = label_error_check(j->sc, j->st);
    const std::string msg = rc != OSMT_OK ? std::string(osmt_last_error()) : std::string();
    const bool missed = rc != OSMT_OK && g_arena_guess_missed && j->owns_scene; /* public scenes are sized exactly: no retry */
    const osmt_batch* batch = j->batch;
    const osmt_label_batch* labels = j->labels;
    png_job_release(j);
    if (missed) { /* the guessed arenas were too small for this batch: the whole job again with exact sizing */
        g_arena_guess_missed = false;
        osmt_png_job* again = nullptr;
        rc = png_begin_body(ctx, batch, labels, &again, false);
        if (rc != OSMT_OK) return rc;
        return png_end_body(again, out_png, out_capacity, out_off);
    }
    return rc != OSMT_OK ? fail(rc, "%s", msg.c_str()) : OSMT_OK;
}

int osmt_render_batch_png_begin(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, osmt_png_job** out_job) {
    return guarded([&] { return png_begin_body(ctx, batch, labels, out_job); });
}

int osmt_render_batch_png_end(osmt_png_job* job, uint8_t* out_png, size_t out_capacity, uint64_t* out_off) {
    return guarded([&] { return png_end_body(job, out_png, out_capacity, out_off); });
}

/* One call = its own pipeline: begin + end. */
int osmt_render_batch_png(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_png, size_t out_capacity,
                          uint64_t* out_off) {
    return guarded([&] {
        if (!ctx || !out_off || (!out_png && out_capacity)) return fail(OSMT_INVALID_ARG, "NULL argument");
        osmt_png_job* j = nullptr;
        const int rc = png_begin_body(ctx, batch, labels, &j);
        if (rc != OSMT_OK) return rc;
        return png_end_body(j, out_png, out_capacity, out_off);
    });
}

int osmt_render_scene_png_begin(osmt_ctx* ctx, osmt_scene* scene, osmt_png_job** out_job) {
    return guarded([&] { return scene_png_begin_body(ctx, scene, out_job); });
}

/* One call = begin + end, as the batch form. */
int osmt_render_scene_png(osmt_ctx* ctx, osmt_scene* scene, uint8_t* out_png, size_t out_capacity, uint64_t* out_off) {
    return guarded([&] {
        if (!ctx || !scene || !out_off || (!out_png && out_capacity)) return fail(OSMT_INVALID_ARG, "NULL argument");
        osmt_png_job* j = nullptr;
        const int rc = scene_png_begin_body(ctx, scene, &j);
        if (rc != OSMT_OK) return rc;
        return png_end_body(j, out_png, out_capacity, out_off);
    });
}

/* ---- the device form: everything on the caller's stream ---- */
namespace {
struct scene_png_work {
    size_t o_rgba = 0, o_png = 0, o_len = 0, bytes = 0, tile_bytes = 0, slot = 0;
};
void scene_png_work_layout(const osmt_scene* sc, scene_png_work& w) {
    const size_t W = (size_t)OSMT_TILE_SIZE * sc->scale, n = sc->n_jobs;
    w.tile_bytes = W * W * 4;
    w.slot = osmt_png_device_bound((uint32_t)W, (uint32_t)W);
    w.o_rgba = 0;
    w.o_png = align_up(n * w.tile_bytes, 256);
    w.o_len = w.o_png + align_up(n * w.slot, 256);
    w.bytes = w.o_len + align_up(n * 4, 256);
}
}  // namespace

size_t osmt_scene_png_work_bytes(osmt_ctx* ctx, osmt_scene* scene) {
    if (!ctx || !scene || scene->ctx != ctx) return 0;
    scene_png_work w;
    scene_png_work_layout(scene, w);
    return w.bytes;
}

static int scene_png_device_body(osmt_ctx* ctx, osmt_scene* sc, void* d_work, size_t work_bytes, void* d_png, size_t png_capacity,
                                 uint64_t* d_off, uint32_t* d_status, void* stream) {
    if (!ctx || !sc || !d_off || !d_status) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (sc->ctx != ctx) return fail(OSMT_INVALID_ARG, "the scene belongs to another context");
    scene_png_work w;
    scene_png_work_layout(sc, w);
    const uint32_t n = sc->n_jobs;
    if (n && !d_work) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (!d_png && png_capacity) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (work_bytes < w.bytes) return fail(OSMT_INVALID_ARG, "work_bytes %zu < osmt_scene_png_work_bytes() = %zu", work_bytes, w.bytes);
    if (((uintptr_t)d_work & 255u) || ((uintptr_t)d_off & 7u) || ((uintptr_t)d_status & 3u))
        return fail(OSMT_INVALID_ARG, "d_work must be aligned to 256 bytes, d_off to 8, d_status to 4");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    char* const d = (char*)d_work;
    uint32_t* const d_len = (uint32_t*)(d + w.o_len);
    if (n) {
        const uint32_t W = OSMT_TILE_SIZE * sc->scale;
        int rc = render_impl(ctx, sc, 7u, d + w.o_rgba, w.tile_bytes, false, stream);
        if (rc == OSMT_OK) rc = osmt_encode_png_device(ctx, d + w.o_rgba, w.tile_bytes, n, W, W, d + w.o_png, w.slot, d_len, stream);
        if (rc != OSMT_OK) return rc;
    }
    HIP_TRY(osmt_launch_png_offsets(d_len, n, png_capacity, (unsigned long long*)d_off, d_status, st));
    HIP_TRY(osmt_launch_png_compact(d + w.o_png, w.slot, d_len, (const unsigned long long*)d_off, n, d_png, st, d_status));
    return OSMT_OK;
}

int osmt_render_scene_png_device(osmt_ctx* ctx, osmt_scene* scene, void* d_work, size_t work_bytes, void* d_png, size_t png_capacity,
                                 uint64_t* d_off, uint32_t* d_status, void* stream) {
    return guarded([&] { return scene_png_device_body(ctx, scene, d_work, work_bytes, d_png, png_capacity, d_off, d_status, stream); });
}

static int debug_png_offsets_body(osmt_ctx* ctx, const uint32_t* d_len, uint32_t n, uint64_t capacity, uint64_t* d_off, uint32_t* d_status,
                                  void* stream) {
    if (!ctx || !d_off || !d_status || (n && !d_len)) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (n > 0x80000000u) return fail(OSMT_INVALID_ARG, "more than 2^31 lengths");
    if (((uintptr_t)d_len & 3u) || ((uintptr_t)d_off & 7u) || ((uintptr_t)d_status & 3u)) return fail(OSMT_INVALID_ARG, "misaligned device pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(osmt_launch_png_offsets(d_len, n, capacity, (unsigned long long*)d_off, d_status, (hipStream_t)stream));
    return OSMT_OK;
}

int osmt_debug_png_offsets(osmt_ctx* ctx, const uint32_t* d_len, uint32_t n, uint64_t capacity, uint64_t* d_off, uint32_t* d_status,
                           void* stream) {
    return guarded([&] { return debug_png_offsets_body(ctx, d_len, n, capacity, d_off, d_status, stream); });
}

static int osmt_host_alloc_body(osmt_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return OSMT_OK;
}

int osmt_host_alloc(osmt_ctx* ctx, size_t bytes, void** out) {
    return guarded([&] { return osmt_host_alloc_body(ctx, bytes, out); });
}

void osmt_host_free(osmt_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    (void)hipSetDevice(ctx->device);
    (void)hipHostFree(p);
}

static int osmt_project_body(osmt_ctx* ctx, const double* latlon, size_t n, uint8_t zoom, uint32_t tx, uint32_t ty, double scale,
                 int32_t* xy) {
    if (!ctx || (n && (!latlon || !xy))) return fail(OSMT_INVALID_ARG, "NULL argument");
    /* 1u << zoom is undefined from 32 and 256 * 2^zoom wraps to 0 at 24: refused as every other entry refuses it */
    if (zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "zoom %u > MAX_ZOOM (src/tile.rs:5)", zoom);
    if (n >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "too many points");
    if (n == 0) return OSMT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    /* device buffers from the per-context cache, the whole call on a pooled private stream: concurrent worker threads
     * neither pay hipMalloc/hipFree per call nor wait for each other's work */
    char* d = nullptr;
    hipStream_t st = nullptr;
    HIP_TRY(stream_acquire(ctx, &st));
    const size_t in_bytes = align_up(n * 16, 256);
    hipError_t e = dev_alloc(ctx, (void**)&d, in_bytes + n * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(d, latlon, n * 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = osmt_launch_project_single((const double*)d, (uint32_t)n, zoom, tx, ty, scale, (int32_t*)(d + in_bytes), st);
    if (e == hipSuccess) e = hipMemcpyAsync(xy, d + in_bytes, n * 8, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st); /* also on the error path: the buffer goes back to the cache */
    if (e == hipSuccess) e = es;
    dev_free(ctx, d);
    stream_release(ctx, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "osmt_project: %s", hipGetErrorString(e));
    return OSMT_OK;
}

int osmt_project(osmt_ctx* ctx, const double* latlon, size_t n, uint8_t zoom, uint32_t tx, uint32_t ty, double scale,
                 int32_t* xy) {
    return guarded([&] { return osmt_project_body(ctx, latlon, n, zoom, tx, ty, scale, xy); });
}

static int osmt_composite_device_body(osmt_ctx* ctx, const void* d_planes, const double canvas[4], uint32_t n, uint32_t L,
                          uint32_t W, uint32_t H, void* d_out, void* stream) {
    if (!ctx || !canvas) return fail(OSMT_INVALID_ARG, "NULL argument");
    if ((uint64_t)W * H >= 0xFFFFFFFFull) return fail(OSMT_INVALID_ARG, "tile too large");
    if (((uint64_t)W * H) % 64u) return fail(OSMT_INVALID_ARG, "W*H must be a multiple of 64 (tiles are (256*scale)^2)");
    if ((size_t)n * W * H && (!d_planes || !d_out)) return fail(OSMT_INVALID_ARG, "NULL device pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(osmt_launch_composite(d_planes, canvas, n, L, W * H, d_out, (hipStream_t)stream));
    return OSMT_OK;
}

int osmt_composite_device(osmt_ctx* ctx, const void* d_planes, const double canvas[4], uint32_t n, uint32_t L,
                          uint32_t W, uint32_t H, void* d_out, void* stream) {
    return guarded([&] { return osmt_composite_device_body(ctx, d_planes, canvas, n, L, W, H, d_out, stream); });
}

static int osmt_composite_body(osmt_ctx* ctx, const double* planes, const double canvas[4], uint32_t n, uint32_t L, uint32_t W,
                   uint32_t H, uint8_t* out_rgba) {
    if (!ctx || !canvas) return fail(OSMT_INVALID_ARG, "NULL argument");
    const size_t npx = (size_t)n * W * H;
    if (npx == 0) return OSMT_OK;
    if (!planes || !out_rgba) return fail(OSMT_INVALID_ARG, "NULL buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    char* d = nullptr;
    hipStream_t st = nullptr;
    HIP_TRY(stream_acquire(ctx, &st));
    const size_t in_bytes = align_up(npx * L * 32, 256);
    hipError_t e = dev_alloc(ctx, (void**)&d, in_bytes + npx * 4);
    if (e == hipSuccess && L) e = hipMemcpyAsync(d, planes, npx * L * 32, hipMemcpyHostToDevice, st);
    int rc = OSMT_OK;
    if (e == hipSuccess) rc = osmt_composite_device(ctx, d, canvas, n, L, W, H, d + in_bytes, st);
    if (e == hipSuccess && rc == OSMT_OK) e = hipMemcpyAsync(out_rgba, d + in_bytes, npx * 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    dev_free(ctx, d);
    stream_release(ctx, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "osmt_composite: %s", hipGetErrorString(e));
    return rc;
}

int osmt_composite(osmt_ctx* ctx, const double* planes, const double canvas[4], uint32_t n, uint32_t L, uint32_t W,
                   uint32_t H, uint8_t* out_rgba) {
    return guarded([&] { return osmt_composite_body(ctx, planes, canvas, n, L, W, H, out_rgba); });
}

static int hbm_copy_probe_body(osmt_ctx* ctx, size_t bytes, uint32_t iters, double* out_copy, double* out_read) {
    if (!ctx || !out_copy) return fail(OSMT_INVALID_ARG, "NULL argument");
    if (bytes < 16 || iters == 0) return fail(OSMT_INVALID_ARG, "nothing to copy");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n16 = bytes / 16;
    char* d = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    HIP_TRY(stream_acquire(ctx, &st));
    hipError_t e = dev_alloc(ctx, (void**)&d, 2 * n16 * 16);
    if (e == hipSuccess) e = hipMemsetAsync(d, 0x5A, 2 * n16 * 16, st);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = osmt_launch_copy16(d, d + n16 * 16, n16, false, st); /* warm-up */
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    for (uint32_t i = 0; i < iters && e == hipSuccess; ++i) e = osmt_launch_copy16(d, d + n16 * 16, n16, false, st);
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    for (uint32_t i = 0; i < iters && e == hipSuccess; ++i) e = osmt_launch_copy16(d, d + n16 * 16, n16, true, st);
    if (e == hipSuccess) e = hipEventRecord(ev[2], st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    float ms_copy = 0.f, ms_read = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_copy, ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_read, ev[1], ev[2]);
    for (int k = 0; k < 3; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    dev_free(ctx, d);
    stream_release(ctx, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "osmt_hbm_copy_probe: %s", hipGetErrorString(e));
    *out_copy = 2.0 * (double)(n16 * 16) * iters / ((double)ms_copy * 1e-3) / 1e9;
    if (out_read) *out_read = (double)(n16 * 16) * iters / ((double)ms_read * 1e-3) / 1e9;
    return OSMT_OK;
}

int osmt_debug_poison_enabled(void) { return poison_alloc() ? 1 : 0; }

int osmt_hbm_copy_probe(osmt_ctx* ctx, size_t bytes, uint32_t iters, double* out_copy, double* out_read) {
    return guarded([&] { return hbm_copy_probe_body(ctx, bytes, iters, out_copy, out_read); });
}
