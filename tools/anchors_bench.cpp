// The two ways to the label anchors of a batch of (tile, area) pairs, timed natively on one host thread (tools/bench_anchors.py):
//   ab_host:   what a caller does without registered factors — project every node of every pair with libm (tile.rs:88-106,
//              labelable.rs:61-68: tan and log per node AND per pair), assemble rings and points, osmt_label_positions
//   ab_device: osmt_label_positions_tiles over the registered factors (8 bytes per pair)
// Both return the positions; ms[] gets the wall time of the stages, bytes the upload of the call.
#include <chrono>
#include <cmath>
#include <vector>

#include "../include/osmtile.h"

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

extern "C" {

int ab_host(osmt_ctx* ctx, const osmt_geodata_desc* g, const osmt_query_tile* tiles, const osmt_label_tile_request* rq, size_t n, uint32_t scale,
            osmt_label_position* out, double ms[2], uint64_t* bytes) {
    const double PI = 3.14159265358979323846264338327950288;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<osmt_label_request> reqs(n);
    std::vector<osmt_ring> rings;
    std::vector<double> pts;
    auto ring = [&](const uint32_t* nodes, uint32_t cnt, const osmt_query_tile& t) {
        rings.push_back({(uint32_t)(pts.size() / 2), cnt});
        const double dim = (double)(OSMT_TILE_SIZE * (1u << t.zoom));
        for (uint32_t i = 0; i < cnt; ++i) {
            const double lat_rad = g->nodes[2 * (size_t)nodes[i]] * (PI / 180.0), lon_rad = g->nodes[2 * (size_t)nodes[i] + 1] * (PI / 180.0);
            const double x = lon_rad + PI;
            const double y = PI - std::log(std::tan((PI / 4.0) + (lat_rad / 2.0)));
            const double px = (x / (2.0 * PI)) * dim - (double)(uint32_t)(t.x * OSMT_TILE_SIZE);
            const double py = (y / (2.0 * PI)) * dim - (double)(uint32_t)(t.y * OSMT_TILE_SIZE);
            pts.push_back(px * (double)scale);
            pts.push_back(py * (double)scale);
        }
    };
    for (size_t i = 0; i < n; ++i) {
        const uint32_t e = rq[i].entity, id = e & ~OSMT_STYLED_MULTIPOLYGON;
        const osmt_query_tile& t = tiles[rq[i].tile];
        reqs[i].ring_off = (uint32_t)rings.size();
        reqs[i].scale = (double)scale;
        if (e & OSMT_STYLED_MULTIPOLYGON) {
            for (uint32_t k = g->multipolygon_polygon_off[id]; k < g->multipolygon_polygon_off[id + 1]; ++k) {
                const uint32_t p = g->multipolygon_polygons[k];
                ring(g->polygon_nodes + g->polygon_node_off[p], g->polygon_node_off[p + 1] - g->polygon_node_off[p], t);
            }
        } else {
            ring(g->way_nodes + g->way_node_off[id], g->way_node_off[id + 1] - g->way_node_off[id], t);
        }
        reqs[i].n_rings = (uint32_t)rings.size() - reqs[i].ring_off;
    }
    ms[0] = ms_since(t0);
    osmt_label_request_batch b{};
    b.requests = reqs.data(), b.n_requests = n;
    b.rings = rings.data(), b.n_rings = rings.size();
    b.points = pts.data(), b.n_pts = pts.size() / 2;
    *bytes = n * 24 + rings.size() * sizeof(osmt_ring) + pts.size() * 8; /* request records as uploaded, rings, points */
    const auto t1 = std::chrono::steady_clock::now();
    const int rc = osmt_label_positions(ctx, &b, out);
    ms[1] = ms_since(t1);
    return rc;
}

int ab_device(osmt_ctx* ctx, const osmt_label_tile_batch* b, osmt_label_position* out, double* ms, uint64_t* bytes) {
    *bytes = b->n_requests * sizeof(osmt_label_tile_request) + b->n_tiles * sizeof(osmt_query_tile);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = osmt_label_positions_tiles(ctx, b, out);
    *ms = ms_since(t0);
    return rc;
}
}
