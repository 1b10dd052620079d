/*
 * osmt_host_worker.cpp — host side of libosmtile.so: the per-request entries.  The coalescing worker (osmt_worker_render), the tile
 * server, and osmt_worker_render_tile_png; both entries gather concurrent requests through ONE group-commit gate (group_commit).
 * Shares osmt_host.h with osmt_api.cpp.
 */
#include "osmt_host.h"

using namespace osmt_host;

namespace {

/* ---- the per-request entry: worker handles that gather concurrent one-tile requests -------------------------------
 * The reference's server hands ONE tile per request to each of available_parallelism() worker threads, every one with
 * its own TilePixels (src/http_server.rs:50-83,105-108,134-181).  Sixteen threads that each run the whole chain — five
 * pre-pass launches, a raster launch for 128 waves, a copy, a synchronisation — for one tile queue up behind each other
 * on the device (round 3: 17 k tiles/s, p99 9.6 ms from 16 workers).  The GPU renders 16 tiles in the time of one, so
 * the requests are gathered ("group commit"): a request that finds fewer than OSMT_WORKER_INFLIGHT groups on the
 * device becomes a leader at once and takes EVERY request that is waiting (up to 64 tiles) with it; requests that
 * arrive while the device is busy wait for the next leader.  No timer: a lone request never waits for company, and
 * the group size follows the load.  The leader merges the display lists (a valid batch: op ranges partition the merged
 * pool, every request was validated by its own thread), renders them with ONE launch sequence into pinned staging and
 * every requester copies its own tiles out in parallel.  A group of one skips all of that and is osmt_render_batch_rgb. */
struct staged_group {
    osmt_ctx* ctx = nullptr;
    void* stage = nullptr;
    std::atomic<int> pending{0}; /* requesters that still have to copy their tiles (their file) out of `stage` */
};

/* a requester has copied its share out: the last one gives the staging back */
void staged_group_release(staged_group* g) {
    if (g->pending.fetch_sub(1) == 1) {
        stage_release(g->ctx, g->stage);
        delete g;
    }
}

}  // namespace

namespace osmt_host {

struct coalesce_req {
    const osmt_batch* b = nullptr;
    const osmt_label_batch* lb = nullptr;
    uint8_t* out = nullptr;
    size_t stride = 0;
    bool taken = false, done = false, ran = false; /* ran: rendered on its own (rc is its verdict) */
    int rc = OSMT_OK;
    std::string err;
    staged_group* grp = nullptr; /* where the pixels are (NULL: already in `out`, or failed) */
    const uint8_t* src = nullptr;
};

}  // namespace osmt_host

struct osmt_worker {
    osmt_ctx* ctx = nullptr;
};

namespace {

constexpr size_t CO_MAX_TILES = 64;

int co_max_in_flight() {
    static const int v = [] {
        const char* e = getenv("OSMT_WORKER_INFLIGHT");
        /* 16 / 32 native threads, one-tile requests: 48 / 64 k tiles/s with 1, 45 / 72 k with 2, 35 / 53 k with 3, 28 / 49 k with 4,
         * 20 / 37 k with 6 (profiles/r04_j_worker_inflight.txt): every group in flight is a host thread in the runtime, and
         * they queue up behind each other's calls */
        return e ? std::min(std::max(atoi(e), 1), 16) : 2;
    }();
    return v;
}

/* ---- the group-commit gate of both per-request entries ----
 * Queues `me` and returns when it is done.  lk holds ctx->co_mu, on entry and on return.  While fewer than co_max_in_flight()
 * groups are on the device — ONE count for both entries — a request that nobody has taken leads: it takes the waiters at the
 * head of its queue in arrival order for as long as admit(r, n_taken) says yes (n_taken == 0: r opens a new group and is
 * always admitted), reports taken(n) under the lock, and runs the group unlocked.  group: empty, with room for the largest
 * group, so that taking a waiter cannot throw. */
template <class Req, class Admit, class Run, class Taken>
void group_commit(osmt_ctx* ctx, std::unique_lock<std::mutex>& lk, std::deque<Req*>& queue, Req* me, std::vector<Req*>& group, Admit admit, Run run,
                  Taken taken) {
    queue.push_back(me);
    for (;;) {
        if (me->done) break;
        if (!me->taken && ctx->co_in_flight < co_max_in_flight()) {
            /* leader: everything that waits and is admitted, in arrival order, up to the first request that is not — that one
             * is the next leader's.  The leader's own request is in there, or sits behind such a request. */
            while (!queue.empty()) {
                Req* r = queue.front();
                if (!admit(r, group.size())) break;
                r->taken = true;
                group.push_back(r);
                queue.pop_front();
            }
            ++ctx->co_in_flight;
            taken(group.size());
            lk.unlock();
            /* whatever happens in there, the group's members are marked done and the slot is given back: followers
             * wait on co_cv with no timeout */
            try {
                run(group);
            } catch (...) {
                for (Req* r : group)
                    if (!r->grp && !r->ran) r->rc = OSMT_OOM; /* (err stays empty: assigning a string could throw again) */
            }
            lk.lock();
            --ctx->co_in_flight;
            for (Req* r : group) r->done = true;
            group.clear();
            ctx->co_cv.notify_all();
            continue; /* its own request may have been behind an incompatible one: look again */
        }
        ctx->co_cv.wait(lk);
    }
}

/* the display lists (and label lists) of several requests as ONE batch, in request order */
struct merged_batch {
    std::vector<osmt_tile_job> jobs;
    std::vector<osmt_op> ops;
    std::vector<osmt_ring> rings;
    std::vector<double> latlon; /* per point, or the concatenated node tables */
    std::vector<int32_t> points;
    std::vector<uint32_t> node_refs;
    std::vector<double> dashes;
    std::vector<osmt_label> labels;
    std::vector<uint32_t> job_label_off;
    std::vector<double> segs;
    osmt_batch b;
    osmt_label_batch lb;
    bool has_labels = false;
};

void merge_requests(const std::vector<coalesce_req*>& reqs, merged_batch* m) {
    const osmt_batch* b0 = reqs[0]->b;
    const bool ll = b0->coord_kind == OSMT_COORD_LATLON_F64, nr = b0->coord_kind == OSMT_COORD_NODE_REF;
    for (const coalesce_req* r : reqs)
        if (r->lb && r->lb->n_labels) m->has_labels = true;
    if (m->has_labels) m->job_label_off.push_back(0u);
    for (const coalesce_req* r : reqs) {
        const osmt_batch* b = r->b;
        const uint32_t op0 = (uint32_t)m->ops.size(), ring0 = (uint32_t)m->rings.size(), dash0 = (uint32_t)m->dashes.size();
        const uint32_t pt0 = (uint32_t)(ll ? m->latlon.size() / 2 : nr ? m->node_refs.size() : m->points.size() / 2);
        const uint32_t node0 = nr ? (uint32_t)(m->latlon.size() / 2) : 0u;
        for (size_t j = 0; j < b->n_jobs; ++j) {
            osmt_tile_job job = b->jobs[j];
            job.op_off += op0;
            job.pt_off += pt0;
            m->jobs.push_back(job);
        }
        for (size_t o = 0; o < b->n_ops; ++o) {
            osmt_op op = b->ops[o];
            if (op.kind != OSMT_OP_NONE) {
                op.ring_off += ring0;
                if (op.kind == OSMT_OP_STROKE && op.has_dashes) op.dashes_off += dash0;
            }
            m->ops.push_back(op);
        }
        for (size_t k = 0; k < b->n_rings; ++k) {
            osmt_ring ring = b->rings[k];
            ring.first_pt += pt0;
            m->rings.push_back(ring);
        }
        if (ll) {
            m->latlon.insert(m->latlon.end(), b->latlon, b->latlon + 2 * b->n_pts);
        } else if (nr) {
            m->latlon.insert(m->latlon.end(), b->nodes, b->nodes + 2 * b->n_nodes);
            for (size_t i = 0; i < b->n_pts; ++i) m->node_refs.push_back(b->node_refs[i] + node0);
        } else {
            m->points.insert(m->points.end(), b->points, b->points + 2 * b->n_pts);
        }
        if (b->n_dashes) m->dashes.insert(m->dashes.end(), b->dashes, b->dashes + b->n_dashes);
        if (m->has_labels) {
            const osmt_label_batch* lb = r->lb;
            const uint32_t lab0 = (uint32_t)m->labels.size(), seg0 = (uint32_t)(m->segs.size() / 4);
            if (lb && lb->n_labels) {
                for (size_t i = 0; i < lb->n_labels; ++i) {
                    osmt_label l = lb->labels[i];
                    l.seg_off += seg0;
                    m->labels.push_back(l);
                }
                m->segs.insert(m->segs.end(), lb->segs, lb->segs + 4 * lb->n_segs);
                for (size_t j = 0; j < b->n_jobs; ++j) m->job_label_off.push_back(lab0 + lb->job_label_off[j + 1]);
            } else {
                for (size_t j = 0; j < b->n_jobs; ++j) m->job_label_off.push_back(lab0);
            }
        }
    }
    memset(&m->b, 0, sizeof m->b);
    m->b.jobs = m->jobs.data();
    m->b.n_jobs = m->jobs.size();
    m->b.ops = m->ops.data();
    m->b.n_ops = m->ops.size();
    m->b.rings = m->rings.data();
    m->b.n_rings = m->rings.size();
    m->b.coord_kind = b0->coord_kind;
    m->b.scale = b0->scale;
    m->b.n_pts = ll ? m->latlon.size() / 2 : nr ? m->node_refs.size() : m->points.size() / 2;
    m->b.latlon = ll ? m->latlon.data() : nullptr;
    m->b.points = (!ll && !nr) ? m->points.data() : nullptr;
    m->b.nodes = nr ? m->latlon.data() : nullptr;
    m->b.n_nodes = nr ? m->latlon.size() / 2 : 0;
    m->b.node_refs = nr ? m->node_refs.data() : nullptr;
    m->b.dashes = m->dashes.data();
    m->b.n_dashes = m->dashes.size();
    memset(&m->lb, 0, sizeof m->lb);
    m->lb.labels = m->labels.data();
    m->lb.n_labels = m->labels.size();
    m->lb.job_label_off = m->job_label_off.data();
    m->lb.segs = m->segs.data();
    m->lb.n_segs = m->segs.size() / 4;
}

/* label batches are validated where they are attached (osmt_scene_set_labels); here only what merging itself reads */
int label_batch_shape_ok(const osmt_batch* b, const osmt_label_batch* lb) {
    if (!lb || !lb->n_labels) return OSMT_OK;
    if (!lb->labels || !lb->job_label_off || (lb->n_segs && !lb->segs)) return fail(OSMT_INVALID_ARG, "label batch: NULL pool");
    if (lb->n_labels >= 0x7FFFFFFFull || lb->n_segs >= 0x7FFFFFFFull) return fail(OSMT_INVALID_ARG, "label batch too large");
    if (lb->job_label_off[0] != 0u) return fail(OSMT_INVALID_ARG, "job_label_off[0] must be 0");
    for (size_t j = 0; j < b->n_jobs; ++j)
        if (lb->job_label_off[j + 1] < lb->job_label_off[j] || lb->job_label_off[j + 1] > lb->n_labels)
            return fail(OSMT_INVALID_ARG, "job_label_off not monotonic / out of range at tile %zu", j);
    if (lb->job_label_off[b->n_jobs] != lb->n_labels) return fail(OSMT_INVALID_ARG, "job_label_off[n_jobs] != n_labels");
    /* a label's draw_line calls must lie in ITS request's pool: re-based into the merged pool an out-of-range seg_off would
     * land in another request's calls and pass the merged check instead of failing alone */
    for (size_t i = 0; i < lb->n_labels; ++i)
        if ((unsigned long long)lb->labels[i].seg_off + lb->labels[i].n_segs > lb->n_segs)
            return fail(OSMT_INVALID_ARG, "label %zu: seg_off + n_segs beyond the batch's draw_line calls", i);
    return OSMT_OK;
}

/* renders the requests of one group; fills rc / err / grp / src of every request (the caller marks them done) */
void coalesce_run_group(osmt_ctx* ctx, const std::vector<coalesce_req*>& reqs) {
    auto run_alone = [&](coalesce_req* r) {
        /* its requester has validated it: trusted, like the merged batch (no second pass over the ops and points) */
        r->rc = guarded([&] {
            return osmt_render_batch_labels_body(ctx, r->b, (r->lb && r->lb->n_labels) ? r->lb : nullptr, r->out, r->stride, true, true);
        });
        r->ran = true;
        if (r->rc != OSMT_OK) r->err = osmt_last_error();
    };
    if (reqs.size() == 1) {
        run_alone(reqs[0]);
        return;
    }
    const size_t W = (size_t)OSMT_TILE_SIZE * reqs[0]->b->scale, tile_rgb = W * W * 3;
    size_t n_tiles = 0;
    for (const coalesce_req* r : reqs) n_tiles += r->b->n_jobs;
    int rc = OSMT_OK;
    void* stage = nullptr;
    /* OSMT_TRACE_WORKER=1 (diagnostic): one stderr line per gathered group — requests, tiles, merge and render time */
    static const bool trace_worker = getenv("OSMT_TRACE_WORKER") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto t1 = t0;
    try {
        merged_batch m;
        merge_requests(reqs, &m);
        stage = stage_acquire(ctx, n_tiles * tile_rgb);
        t1 = std::chrono::steady_clock::now();
        if (!stage) {
            rc = OSMT_OOM;
        } else {
            rc = osmt_render_batch_labels_body(ctx, &m.b, m.has_labels ? &m.lb : nullptr, (uint8_t*)stage, tile_rgb, true, true);
        }
    } catch (...) {
        rc = OSMT_OOM;
    }
    if (trace_worker) {
        const auto t2 = std::chrono::steady_clock::now();
        fprintf(stderr, "osmt worker group: %zu requests, %zu tiles, merge+staging %.0f us, render %.0f us, rc %d\n", reqs.size(), n_tiles,
                std::chrono::duration<double, std::micro>(t1 - t0).count(), std::chrono::duration<double, std::micro>(t2 - t1).count(), rc);
    }
    if (rc != OSMT_OK) {
        /* whatever went wrong (one request's labels refused, no pinned memory): every request on its own, so that a bad
         * one fails alone */
        if (stage) stage_release(ctx, stage);
        for (coalesce_req* r : reqs) run_alone(r);
        return;
    }
    staged_group* g = new (std::nothrow) staged_group();
    if (!g) {
        stage_release(ctx, stage);
        for (coalesce_req* r : reqs) run_alone(r);
        return;
    }
    g->ctx = ctx;
    g->stage = stage;
    g->pending.store((int)reqs.size());
    size_t first = 0;
    for (coalesce_req* r : reqs) {
        r->grp = g;
        r->src = (const uint8_t*)stage + first * tile_rgb;
        r->rc = OSMT_OK;
        first += r->b->n_jobs;
    }
}

int worker_render_body(osmt_worker* w, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgb, size_t stride) {
    if (!w || !w->ctx || !out_rgb) return fail(OSMT_INVALID_ARG, "NULL argument");
    osmt_ctx* ctx = w->ctx;
    int rc = validate_batch(batch); /* by the requesting thread: the merged batch is trusted */
    if (rc != OSMT_OK) return rc;
    rc = label_batch_shape_ok(batch, labels);
    if (rc != OSMT_OK) return rc;
    const size_t W = (size_t)OSMT_TILE_SIZE * batch->scale, tile_rgb = W * W * 3;
    if (stride < tile_rgb) return fail(OSMT_INVALID_ARG, "out_tile_stride_bytes < W*H*3");
    if (batch->n_jobs == 0) return OSMT_OK;
    if (batch->n_jobs > CO_MAX_TILES) return osmt_render_batch_rgb(ctx, batch, labels, out_rgb, stride); /* a batch of its own anyway */

    coalesce_req me;
    me.b = batch;
    me.lb = labels;
    me.out = out_rgb;
    me.stride = stride;
    std::vector<coalesce_req*> group;
    group.reserve(CO_MAX_TILES); /* every request has at least one tile: push_back in group_commit cannot throw */
    /* admitted: the same scale and coordinate kind as the group's first request, at most 64 tiles together, and — the merged
     * pools are indexed with 32 bits and rendered without a second validation — no pool past 2^31 entries: a request that
     * would take one there waits for the next leader (alone it is what its own validation saw) */
    size_t tiles = 0;
    unsigned long long pool[7] = {0, 0, 0, 0, 0, 0, 0};
    const osmt_batch* b0 = nullptr;
    auto admit = [&](const coalesce_req* r, size_t n_taken) {
        if (!n_taken) {
            tiles = 0;
            for (int k = 0; k < 7; ++k) pool[k] = 0;
            b0 = r->b;
        }
        if (r->b->scale != b0->scale || r->b->coord_kind != b0->coord_kind) return false; /* the next leader's */
        if (n_taken && tiles + r->b->n_jobs > CO_MAX_TILES) return false;
        const unsigned long long add[7] = {r->b->n_ops, r->b->n_rings, r->b->n_pts, r->b->n_nodes, r->b->n_dashes,
                                           r->lb ? r->lb->n_labels : 0ull, r->lb ? r->lb->n_segs : 0ull};
        bool fits32 = true;
        for (int k = 0; k < 7; ++k) fits32 = fits32 && pool[k] + add[k] < 0x7FFFFFFFull;
        if (n_taken && !fits32) return false;
        for (int k = 0; k < 7; ++k) pool[k] += add[k];
        tiles += r->b->n_jobs;
        return true;
    };
    {
        std::unique_lock<std::mutex> lk(ctx->co_mu);
        group_commit(ctx, lk, ctx->co_queue, &me, group, admit, [&](const std::vector<coalesce_req*>& g) { coalesce_run_group(ctx, g); }, [](size_t) {});
    }
    if (me.rc != OSMT_OK) return fail(me.rc, "%s", me.err.c_str());
    if (me.grp) {
        /* the requester's own share of the read-back: pinned staging -> its buffer, all requesters in parallel */
        for (size_t j = 0; j < batch->n_jobs; ++j) memcpy(out_rgb + j * stride, me.src + j * tile_rgb, tile_rgb);
        staged_group_release(me.grp);
    }
    return OSMT_OK;
}

}  // namespace

int osmt_worker_create(osmt_ctx* ctx, osmt_worker** out_worker) {
    return guarded([&] {
        if (!ctx || !out_worker) return fail(OSMT_INVALID_ARG, "NULL argument");
        osmt_worker* w = new (std::nothrow) osmt_worker();
        if (!w) return fail(OSMT_OOM, "out of host memory");
        w->ctx = ctx;
        ctx->refs.fetch_add(1); /* like a scene: the context outlives its workers */
        *out_worker = w;
        return (int)OSMT_OK;
    });
}

void osmt_worker_destroy(osmt_worker* w) {
    if (!w) return;
    osmt_ctx* ctx = w->ctx;
    delete w;
    if (ctx) ctx_release(ctx);
}

int osmt_worker_render(osmt_worker* w, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgb, size_t out_tile_stride_bytes) {
    return guarded([&] { return worker_render_body(w, batch, labels, out_rgb, out_tile_stride_bytes); });
}

/* ---- tile requests: (z, x, y, scale) in, PNG out ---------------------------------------------------------------------
 * try_handle_connection (src/http_server.rs:134-181) per request: get_entities_in_tile_with_neighbors(tile, osm_ids) ->
 * draw_tile -> PNG bytes.  A tile server states once what every request is rendered with — geodata, bindings per zoom,
 * canvas, filter; osmt_tile_server_render_png is build (filtered or not) -> label -> osmt_render_scene_png -> free for a
 * list of tiles, and osmt_worker_render_tile_png gathers the one-tile requests of concurrent threads into such lists by the
 * group commit of osmt_worker_render above, sharing its cap on groups in flight. */
struct osmt_tile_server {
    osmt_ctx* ctx = nullptr;
    osmt_tile_server_desc d{};
    bool area_labels = false, node_labels = false; /* the label array is not all OSMT_BINDINGS_NONE */
};

namespace {

/* the pairs the last tile-server call of this thread declined (osmt_last_declined_anchors) */
thread_local std::vector<osmt_area_anchor> tl_declined;

bool any_bound(const uint32_t* of_zoom) {
    for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z)
        if (of_zoom[z] != OSMT_BINDINGS_NONE) return true;
    return false;
}

int validate_tile_server(const osmt_tile_server_desc* d, osmt_ctx* ctx) {
    if (!d) return fail(OSMT_INVALID_ARG, "tile server: the description is NULL");
    if (!ctx) return fail(OSMT_INVALID_ARG, "tile server: geodata id %u is not registered (no context)", d->geodata_id);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (d->geodata_id >= ctx->geodata.size())
        return fail(OSMT_INVALID_ARG, "tile server: geodata id %u is not registered (%zu files)", d->geodata_id, ctx->geodata.size());
    if (!ctx->geodata[d->geodata_id].d_index)
        return fail(OSMT_INVALID_ARG, "tile server: geodata id %u has no tile index (osmt_register_tile_index)", d->geodata_id);
    /* one table of one kind under one zoom: known, of this file, covering that zoom */
    auto table_ok = [&](const char* kind, uint32_t id, uint32_t z, size_t n, uint32_t geodata_id, uint32_t lo, uint32_t hi) {
        if (id >= n) return fail(OSMT_INVALID_ARG, "tile server: %s id %u of zoom %u is not registered (%zu tables)", kind, id, z, n);
        if (geodata_id != d->geodata_id)
            return fail(OSMT_INVALID_ARG, "tile server: %s id %u of zoom %u belongs to geodata id %u, not %u", kind, id, z, geodata_id, d->geodata_id);
        if (z < lo || z > hi) return fail(OSMT_INVALID_ARG, "tile server: %s id %u covers zooms %u..%u, not zoom %u", kind, id, lo, hi, z);
        return (int)OSMT_OK;
    };
    for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) {
        int rc = OSMT_OK;
        uint32_t id = d->bindings_of_zoom[z];
        if (id != OSMT_BINDINGS_NONE) {
            const bool known = id < ctx->bindings.size();
            rc = table_ok("bindings", id, z, ctx->bindings.size(), known ? ctx->bindings[id].geodata_id : 0u, known ? ctx->bindings[id].zoom_lo : 0u,
                          known ? ctx->bindings[id].zoom_hi : 0u);
            if (rc != OSMT_OK) return rc;
        }
        id = d->area_label_bindings_of_zoom[z];
        if (id != OSMT_BINDINGS_NONE) {
            const bool known = id < ctx->area_label_bindings.size();
            rc = table_ok("area label bindings", id, z, ctx->area_label_bindings.size(), known ? ctx->area_label_bindings[id].geodata_id : 0u,
                          known ? ctx->area_label_bindings[id].zoom_lo : 0u, known ? ctx->area_label_bindings[id].zoom_hi : 0u);
            if (rc != OSMT_OK) return rc;
        }
        id = d->node_label_bindings_of_zoom[z];
        if (id != OSMT_BINDINGS_NONE) {
            const bool known = id < ctx->label_bindings.size();
            rc = table_ok("node label bindings", id, z, ctx->label_bindings.size(), known ? ctx->label_bindings[id].geodata_id : 0u,
                          known ? ctx->label_bindings[id].zoom_lo : 0u, known ? ctx->label_bindings[id].zoom_hi : 0u);
            if (rc != OSMT_OK) return rc;
        }
    }
    if (any_bound(d->node_label_bindings_of_zoom) && !ctx->geodata[d->geodata_id].d_node_index)
        return fail(OSMT_INVALID_ARG, "tile server: node label bindings, but geodata id %u has no node index (osmt_register_node_index)", d->geodata_id);
    if (d->id_filter != OSMT_ID_FILTER_NONE) {
        if (d->id_filter >= ctx->id_filters.size())
            return fail(OSMT_INVALID_ARG, "tile server: id filter %u is not registered (%zu filters)", d->id_filter, ctx->id_filters.size());
        const osmt_ctx::id_filter_host& f = ctx->id_filters[d->id_filter];
        if (f.geodata_id != d->geodata_id)
            return fail(OSMT_INVALID_ARG, "tile server: id filter %u belongs to geodata id %u, not %u", d->id_filter, f.geodata_id, d->geodata_id);
        if (any_bound(d->node_label_bindings_of_zoom) && !f.node)
            return fail(OSMT_INVALID_ARG,
                        "tile server: node label bindings, but id filter %u has no node plane: register the node index first (osmt_register_node_index), "
                        "then the filter",
                        d->id_filter);
    }
    return OSMT_OK;
}

/* what a requesting thread judges of its own tiles before anything is queued or built: the rules of osmt_validate_tile_batch and
 * of osmt_scene_build_tile_labels_all for the zooms these tiles have */
int tile_request_ok(const osmt_tile_server* s, const osmt_tile_coord* tiles, size_t n, uint32_t scale) {
    if (scale < 1 || scale > OSMT_MAX_SCALE) return fail(OSMT_INVALID_ARG, "scale %u not in 1..%u", scale, OSMT_MAX_SCALE);
    for (size_t t = 0; t < n; ++t) {
        const osmt_tile_coord& q = tiles[t];
        if (q.zoom > OSMT_MAX_ZOOM) return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u > MAX_ZOOM (src/tile.rs:5)", t, q.zoom);
        if (q.x >= (1u << q.zoom) || q.y >= (1u << q.zoom))
            return fail(OSMT_INVALID_ARG, "tile %zu: (x, y) = (%u, %u) outside the %u x %u tiles of zoom %u", t, q.x, q.y, 1u << q.zoom, 1u << q.zoom, q.zoom);
        if (s->d.bindings_of_zoom[q.zoom] == OSMT_BINDINGS_NONE)
            return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no bindings (OSMT_BINDINGS_NONE)", t, q.zoom);
        if (s->area_labels && s->d.area_label_bindings_of_zoom[q.zoom] == OSMT_BINDINGS_NONE)
            return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no area label bindings (OSMT_BINDINGS_NONE)", t, q.zoom);
        if (s->node_labels && s->d.node_label_bindings_of_zoom[q.zoom] == OSMT_BINDINGS_NONE)
            return fail(OSMT_INVALID_ARG, "tile %zu: zoom %u has no label bindings (OSMT_BINDINGS_NONE)", t, q.zoom);
    }
    return OSMT_OK;
}

/* build (filtered or not) -> label -> PNG -> free, on the library's own streams.  tiles have passed tile_request_ok.  declined (may be
 * NULL): gets the pairs the anchor search declined when that is why the call fails. */
int tile_server_run(osmt_tile_server* s, const osmt_tile_coord* tiles, size_t n, uint32_t scale, const osmt_area_anchor* anchors, size_t n_anchors,
                    uint8_t* out_png, size_t out_capacity, uint64_t* out_off, std::vector<osmt_area_anchor>* declined) {
    osmt_ctx* ctx = s->ctx;
    std::vector<osmt_query_tile> q(n);
    for (size_t t = 0; t < n; ++t) {
        osmt_query_tile& o = q[t];
        memset(&o, 0, sizeof o);
        o.x = tiles[t].x, o.y = tiles[t].y, o.zoom = (uint8_t)tiles[t].zoom;
        o.has_canvas = s->d.has_canvas ? 1 : 0;
        if (o.has_canvas) memcpy(o.canvas_rgb, s->d.canvas_rgb, 3);
    }
    osmt_tile_batch b;
    memset(&b, 0, sizeof b);
    b.tiles = q.data(), b.n_tiles = n;
    b.geodata_id = s->d.geodata_id, b.scale = scale, b.use_caps_for_dashes = s->d.use_caps_for_dashes;
    memcpy(b.bindings_of_zoom, s->d.bindings_of_zoom, sizeof b.bindings_of_zoom);
    osmt_scene* sc = nullptr;
    int rc = scene_build_tiles_body(ctx, &b, s->d.id_filter, &sc);
    if (rc != OSMT_OK) return rc;
    if (s->area_labels || s->node_labels)
        rc = scene_build_tile_labels_all_body(ctx, sc, s->area_labels ? s->d.area_label_bindings_of_zoom : nullptr,
                                              s->node_labels ? s->d.node_label_bindings_of_zoom : nullptr, anchors, n_anchors);
    if (rc == OSMT_OK) rc = osmt_render_scene_png(ctx, sc, out_png, out_capacity, out_off);
    if (rc == OSMT_OK) {
        osmt_scene_free(sc);
        return OSMT_OK;
    }
    const std::string why = osmt_last_error(); /* freeing a scene may report nothing, but it must not lose this */
    if (declined && rc == OSMT_UNSUPPORTED) *declined = sc->h_al_declined;
    osmt_scene_free(sc);
    return fail(rc, "%s", why.c_str());
}

int tile_server_render_png_body(osmt_tile_server* s, const osmt_tile_coord* tiles, size_t n, uint32_t scale, const osmt_area_anchor* anchors,
                                size_t n_anchors, uint8_t* out_png, size_t out_capacity, uint64_t* out_off) {
    tl_declined.clear();
    if (!s || !out_off || (n && !tiles) || (!out_png && out_capacity) || (n_anchors && !anchors)) return fail(OSMT_INVALID_ARG, "NULL argument");
    const int rc = tile_request_ok(s, tiles, n, scale);
    if (rc != OSMT_OK) return rc;
    if (n == 0) {
        out_off[0] = 0; /* no tiles, no files: no device is touched */
        return OSMT_OK;
    }
    return tile_server_run(s, tiles, n, scale, anchors, n_anchors, out_png, out_capacity, out_off, &tl_declined);
}

}  // namespace

namespace osmt_host {

/* ---- the per-request entry for tile coordinates ---- */
struct tile_req {
    osmt_tile_server* s = nullptr;
    osmt_tile_coord tile{};
    uint32_t scale = 1;
    const osmt_area_anchor* anchors = nullptr;
    size_t n_anchors = 0;
    uint8_t* out = nullptr;
    size_t cap = 0;
    bool taken = false, done = false, ran = false; /* ran: rendered on its own (rc, len and declined are its verdict) */
    int rc = OSMT_OK;
    std::string err;
    std::vector<osmt_area_anchor> declined; /* tile 0 in each: what its own run declined */
    staged_group* grp = nullptr;            /* where the file is (NULL: already in `out`, or failed) */
    const uint8_t* src = nullptr;
    size_t len = 0; /* the file's size, also when it did not fit */
};

}  // namespace osmt_host

namespace {

void tile_run_group(osmt_ctx* ctx, const std::vector<tile_req*>& reqs) {
    auto run_alone = [&](tile_req* r) {
        uint64_t off[2] = {0, 0};
        r->rc = guarded([&] { return tile_server_run(r->s, &r->tile, 1, r->scale, r->anchors, r->n_anchors, r->out, r->cap, off, &r->declined); });
        r->ran = true;
        r->len = (size_t)off[1];
        if (r->rc != OSMT_OK) r->err = osmt_last_error();
    };
    if (reqs.size() == 1) {
        run_alone(reqs[0]);
        return;
    }
    const size_t n = reqs.size(), W = (size_t)OSMT_TILE_SIZE * reqs[0]->scale, slot = osmt_png_device_bound((uint32_t)W, (uint32_t)W);
    int rc = OSMT_OK;
    void* stage = nullptr;
    std::vector<uint64_t> off;
    try {
        /* the tiles concatenated; every requester's anchors re-based from tile 0 to its index: ascending by (tile, entity) already */
        std::vector<osmt_tile_coord> tiles(n);
        std::vector<osmt_area_anchor> anchors;
        off.assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            tiles[i] = reqs[i]->tile;
            for (size_t k = 0; k < reqs[i]->n_anchors; ++k) {
                osmt_area_anchor a = reqs[i]->anchors[k];
                a.tile = (uint32_t)i;
                anchors.push_back(a);
            }
        }
        stage = stage_acquire(ctx, n * slot);
        if (!stage)
            rc = OSMT_OOM;
        else
            rc = guarded([&] {
                return tile_server_run(reqs[0]->s, tiles.data(), n, reqs[0]->scale, anchors.data(), anchors.size(), (uint8_t*)stage, n * slot, off.data(), nullptr);
            });
    } catch (...) {
        rc = OSMT_OOM;
    }
    staged_group* g = rc == OSMT_OK ? new (std::nothrow) staged_group() : nullptr;
    if (!g) {
        /* whatever went wrong (a member's anchors refused, a declined pair, no pinned memory): every member on its own, so that a
         * bad request or a declined anchor fails alone and the others get their files */
        if (stage) stage_release(ctx, stage);
        for (tile_req* r : reqs) run_alone(r);
        return;
    }
    g->ctx = ctx;
    g->stage = stage;
    g->pending.store((int)n);
    for (size_t i = 0; i < n; ++i) {
        reqs[i]->grp = g;
        reqs[i]->src = (const uint8_t*)stage + off[i];
        reqs[i]->len = (size_t)(off[i + 1] - off[i]);
        reqs[i]->rc = OSMT_OK;
    }
}

int worker_render_tile_png_body(osmt_worker* w, osmt_tile_server* s, const osmt_tile_coord* tile, uint32_t scale, const osmt_area_anchor* anchors,
                                size_t n_anchors, uint8_t* out_png, size_t out_capacity, size_t* out_len) {
    tl_declined.clear();
    if (!w || !w->ctx || !s || !tile || !out_len || (!out_png && out_capacity) || (n_anchors && !anchors)) return fail(OSMT_INVALID_ARG, "NULL argument");
    *out_len = 0;
    if (s->ctx != w->ctx) return fail(OSMT_INVALID_ARG, "the tile server belongs to another context than the worker");
    osmt_ctx* ctx = w->ctx;
    int rc = tile_request_ok(s, tile, 1, scale); /* by the requesting thread: a bad request never joins a group */
    if (rc != OSMT_OK) return rc;
    for (size_t k = 0; k < n_anchors; ++k)
        if (anchors[k].tile != 0u) return fail(OSMT_INVALID_ARG, "anchor %zu: tile %u (a request is one tile: tile 0)", k, anchors[k].tile);

    tile_req me;
    me.s = s, me.tile = *tile, me.scale = scale;
    me.anchors = anchors, me.n_anchors = n_anchors;
    me.out = out_png, me.cap = out_capacity;
    std::vector<tile_req*> group;
    group.reserve(CO_MAX_TILES);
    /* admitted: the requests of the server and scale of the group's first, at most 64 — the first request of another server or
     * scale is the next leader's, as in osmt_worker_render.  Running other threads' requests (the group, or its members alone)
     * overwrites THIS thread's osmt_last_error and declined list in between; both are set again from its own request on the
     * way out (fail() and the swap below). */
    const tile_req* r0 = nullptr;
    auto admit = [&](const tile_req* r, size_t n_taken) {
        if (!n_taken) r0 = r;
        return n_taken < CO_MAX_TILES && r->s == r0->s && r->scale == r0->scale;
    };
    auto taken = [&](size_t n) {
        ++ctx->co_tile_stats[1];
        if (n > ctx->co_tile_stats[2]) ctx->co_tile_stats[2] = n;
    };
    {
        std::unique_lock<std::mutex> lk(ctx->co_mu);
        ++ctx->co_tile_stats[0];
        group_commit(ctx, lk, ctx->co_tile_queue, &me, group, admit, [&](const std::vector<tile_req*>& g) { tile_run_group(ctx, g); }, taken);
    }
    tl_declined.swap(me.declined); /* left for ITS thread, whoever led the group */
    *out_len = me.len;
    if (me.rc != OSMT_OK) return fail(me.rc, "%s", me.err.c_str());
    if (me.grp) {
        const bool fits = me.len <= out_capacity;
        if (fits) memcpy(out_png, me.src, me.len);
        staged_group_release(me.grp);
        if (!fits) return fail(OSMT_INVALID_ARG, "out_capacity %zu < %zu bytes of PNG data", out_capacity, me.len);
    }
    return OSMT_OK;
}

}  // namespace

int osmt_validate_tile_server(const osmt_tile_server_desc* d, osmt_ctx* ctx) {
    return guarded([&] { return validate_tile_server(d, ctx); });
}

int osmt_tile_server_create(osmt_ctx* ctx, const osmt_tile_server_desc* d, osmt_tile_server** out) {
    return guarded([&] {
        if (!ctx || !out) return fail(OSMT_INVALID_ARG, "NULL argument");
        *out = nullptr;
        const int rc = validate_tile_server(d, ctx);
        if (rc != OSMT_OK) return rc;
        osmt_tile_server* s = new osmt_tile_server();
        s->ctx = ctx;
        s->d = *d;
        s->area_labels = any_bound(d->area_label_bindings_of_zoom);
        s->node_labels = any_bound(d->node_label_bindings_of_zoom);
        ctx->refs.fetch_add(1); /* like a scene or a worker: the context outlives its servers */
        *out = s;
        return (int)OSMT_OK;
    });
}

void osmt_tile_server_free(osmt_tile_server* s) {
    if (!s) return;
    osmt_ctx* ctx = s->ctx;
    delete s;
    if (ctx) ctx_release(ctx);
}

int osmt_tile_server_render_png(osmt_tile_server* s, const osmt_tile_coord* tiles, size_t n, uint32_t scale, const osmt_area_anchor* anchors,
                                size_t n_anchors, uint8_t* out_png, size_t out_capacity, uint64_t* out_off) {
    return guarded([&] { return tile_server_render_png_body(s, tiles, n, scale, anchors, n_anchors, out_png, out_capacity, out_off); });
}

int osmt_last_declined_anchors(osmt_area_anchor* out, size_t cap, size_t* n) {
    return guarded([&] {
        if (!n) return fail(OSMT_INVALID_ARG, "NULL argument");
        *n = tl_declined.size();
        if (!out) return (int)OSMT_OK;
        if (cap < *n) return fail(OSMT_INVALID_ARG, "out holds %zu anchors, the last call declined %zu", cap, *n);
        if (*n) memcpy(out, tl_declined.data(), *n * sizeof(osmt_area_anchor));
        return (int)OSMT_OK;
    });
}

int osmt_worker_render_tile_png(osmt_worker* w, osmt_tile_server* s, const osmt_tile_coord* tile, uint32_t scale, const osmt_area_anchor* anchors,
                                size_t n_anchors, uint8_t* out_png, size_t out_capacity, size_t* out_len) {
    return guarded([&] { return worker_render_tile_png_body(w, s, tile, scale, anchors, n_anchors, out_png, out_capacity, out_len); });
}

int osmt_worker_tile_stats(osmt_ctx* ctx, uint64_t stats[3]) {
    return guarded([&] {
        if (!ctx || !stats) return fail(OSMT_INVALID_ARG, "NULL argument");
        std::lock_guard<std::mutex> lk(ctx->co_mu);
        for (int k = 0; k < 3; ++k) stats[k] = ctx->co_tile_stats[k];
        return (int)OSMT_OK;
    });
}
