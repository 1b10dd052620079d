// The reference's server shape with native threads, for tile coordinates: T threads x R one-tile requests through the
// per-request entry osmt_worker_render_tile_png and through the same threads each running the three-call chain it replaces —
// osmt_scene_build_tiles, osmt_render_scene_png, osmt_scene_free.  The native twin of the `requests` section of
// tools/bench_tile_requests.py, which writes the world and starts this program (tools/worker_bench.cpp is the same for the
// batch entry):
//   tile_requests_bench <geodata file> <tiles file: "zoom x y" per line> <runs> <warmup> <requests per thread> <threads>...
// One style (a fill and a stroke) is bound to every way, no labels.  Both forms alternate, the order flips from run to run; a
// run is timed from the moment every thread has passed a barrier to the last join.  Before anything is timed the two forms'
// files of 16 tiles are compared byte for byte.  Per thread count one JSON line: per form the tiles/s, p50 and p99 of every
// timed run, and for the entry the requests and groups osmt_worker_tile_stats counted over this thread count's runs.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"
#include "../osm_renderer_amd/host/osmt_draw.hpp"

using namespace osmt;
using clk = std::chrono::steady_clock;

struct Barrier { /* std::barrier is C++20 */
    std::mutex mu;
    std::condition_variable cv;
    size_t waiting = 0, n, phase = 0;
    explicit Barrier(size_t n_) : n(n_) {}
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        const size_t p = phase;
        if (++waiting == n) {
            waiting = 0, ++phase;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return phase != p; });
        }
    }
};

static double pct(std::vector<double> v, double q) {
    std::sort(v.begin(), v.end());
    return v[std::min(v.size() - 1, (size_t)(q * (double)v.size()))];
}
static void print_list(const char* name, const std::vector<double>& v, bool last = false) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%.4f", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    try {
        GeodataReader r(argv[1]);
        std::vector<osmt_tile_coord> tiles;
        {
            FILE* f = fopen(argv[2], "r");
            if (!f) return 2;
            unsigned z, x, y;
            while (fscanf(f, "%u %u %u", &z, &x, &y) == 3) tiles.push_back(osmt_tile_coord{x, y, z});
            fclose(f);
        }
        const int runs = atoi(argv[3]), warmup = atoi(argv[4]);
        const size_t n_req = (size_t)atoi(argv[5]);
        if (tiles.empty() || runs < 1 || n_req < 1) return 2;
        Context ctx(0);
        GeodataDesc geo(r);
        const uint32_t gid = ctx.register_geodata(geo.desc);
        TileIndexDesc tix(r);
        ctx.register_tile_index(gid, tix.desc);
        osmt_style_rec st{};
        st.has_fill_color = 1, st.fill_color[0] = 170, st.fill_color[1] = 200, st.fill_color[2] = 150, st.is_foreground_fill = 1;
        st.has_color = 1, st.color[0] = 70, st.color[1] = 70, st.color[2] = 90, st.has_width = 1, st.width = 1.5;
        const uint32_t style = ctx.register_styles({st}, {});
        StyleBindings sb(gid, 0, 18, r.way_count(), r.multipolygon_count());
        for (size_t i = 0; i < r.way_count(); ++i) sb.bind_way(i, {style});
        const uint32_t bid = ctx.register_style_bindings(sb.desc());
        osmt_tile_server_desc d = TileServer::describe(gid, Color{241, 238, 232});
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) d.bindings_of_zoom[z] = bid;
        TileServer server(ctx, d);
        const size_t bound = osmt_png_device_bound(TILE_SIZE, TILE_SIZE);

        /* the chain for one tile into `out`; returns the file's length */
        auto chain = [&](const osmt_tile_coord& t, uint8_t* out) {
            osmt_query_tile q{};
            q.x = t.x, q.y = t.y, q.zoom = (uint8_t)t.zoom, q.has_canvas = 1, q.canvas_rgb[0] = 241, q.canvas_rgb[1] = 238, q.canvas_rgb[2] = 232;
            osmt_tile_batch b{};
            b.tiles = &q, b.n_tiles = 1, b.geodata_id = gid, b.scale = 1, b.use_caps_for_dashes = 1;
            for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) b.bindings_of_zoom[z] = bid;
            osmt_scene* sc = nullptr;
            check(osmt_scene_build_tiles(ctx.raw(), &b, &sc));
            uint64_t off[2] = {0, 0};
            const int rc = osmt_render_scene_png(ctx.raw(), sc, out, bound, off);
            osmt_scene_free(sc);
            check(rc);
            return (size_t)off[1];
        };
        {
            Worker w(ctx);
            std::vector<uint8_t> a(bound), b(bound);
            for (size_t i = 0; i < 16; ++i) {
                const osmt_tile_coord& t = tiles[(i * 61) % tiles.size()];
                size_t la = 0;
                check(osmt_worker_render_tile_png(w.raw(), server.raw(), &t, 1, nullptr, 0, a.data(), bound, &la));
                const size_t lb = chain(t, b.data());
                if (la != lb || memcmp(a.data(), b.data(), la) != 0) {
                    fprintf(stderr, "the two forms' files of tile %zu differ\n", i);
                    return 1;
                }
            }
        }
        for (int a = 6; a < argc; ++a) {
            const size_t T = (size_t)atoi(argv[a]);
            if (T < 1) return 2;
            std::vector<std::vector<uint8_t>> out(T, std::vector<uint8_t>(bound));
            std::vector<std::unique_ptr<Worker>> workers;
            for (size_t t = 0; t < T; ++t) workers.emplace_back(new Worker(ctx));
            std::vector<double> res[2][3]; /* [form][tiles/s, p50 ms, p99 ms] */
            uint64_t before[3], after[3], entry_requests = 0, entry_groups = 0;
            for (int rep = 0; rep < warmup + runs; ++rep)
                for (int k = 0; k < 2; ++k) {
                    const int form = rep % 2 == 0 ? k : 1 - k; /* 0: the entry, 1: the chain */
                    std::vector<std::vector<double>> lat(T);
                    std::atomic<int> failed{0};
                    Barrier start(T + 1);
                    check(osmt_worker_tile_stats(ctx.raw(), before));
                    std::vector<std::thread> th;
                    for (size_t t = 0; t < T; ++t)
                        th.emplace_back([&, t] {
                            lat[t].reserve(n_req);
                            start.wait();
                            for (size_t c = 0; c < n_req; ++c) {
                                const osmt_tile_coord& tile = tiles[(t * 131 + c * 17) % tiles.size()];
                                const auto t0 = clk::now();
                                try {
                                    if (form == 0) {
                                        size_t len = 0;
                                        check(osmt_worker_render_tile_png(workers[t]->raw(), server.raw(), &tile, 1, nullptr, 0, out[t].data(), bound, &len));
                                    } else {
                                        chain(tile, out[t].data());
                                    }
                                } catch (const std::exception& e) {
                                    if (failed.fetch_add(1) == 0) fprintf(stderr, "request failed: %s\n", e.what());
                                    return;
                                }
                                lat[t].push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
                            }
                        });
                    start.wait();
                    const auto t0 = clk::now();
                    for (std::thread& x : th) x.join();
                    const double wall = std::chrono::duration<double>(clk::now() - t0).count();
                    if (failed.load()) return 1;
                    check(osmt_worker_tile_stats(ctx.raw(), after));
                    if (form == 0) entry_requests += after[0] - before[0], entry_groups += after[1] - before[1];
                    if (rep < warmup) continue;
                    std::vector<double> all;
                    for (const auto& v : lat) all.insert(all.end(), v.begin(), v.end());
                    res[form][0].push_back((double)all.size() / wall);
                    res[form][1].push_back(pct(all, 0.50));
                    res[form][2].push_back(pct(all, 0.99));
                }
            printf("{\"threads\": %zu, \"requests_per_thread\": %zu, ", T, n_req);
            for (int form = 0; form < 2; ++form) {
                printf("\"%s\": {", form ? "three_call_chain" : "worker_entry");
                print_list("tiles_per_s", res[form][0]);
                print_list("p50_ms", res[form][1]);
                print_list("p99_ms", res[form][2], true);
                printf("}, ");
            }
            printf("\"entry_requests\": %llu, \"entry_groups\": %llu}\n", (unsigned long long)entry_requests, (unsigned long long)entry_groups);
            fflush(stdout);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
