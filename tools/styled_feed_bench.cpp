// Native half of tools/bench_styled_feed.py: the two feeds of one batch of tiles, each timed from the caller's arrays to a
// scene that is complete on the device (both library calls synchronise their stream before they return).
//   (a) osmt::SceneBuilder::add_tile for every tile on this thread, then osmt_scene_upload       — the host feed
//   (b) osmt_scene_build_styled over the registered geodata and styles                            — the device feed
// Style records arrive in the layout of tests/styled_shim.cpp, whose conversion to osmt::Style is reused.
#include <chrono>

#include "../tests/styled_shim.cpp"

namespace {
struct BenchTile {
    Tile tile;
    std::vector<uint32_t> way_ids, way_style;
};
struct Bench {
    GeodataReader reader;
    std::vector<Style> styles;
    std::vector<BenchTile> tiles;
    Bench(const char* path, const ShimStyle* st, size_t n, const double* pool) : reader(path), styles(styles_of(st, n, pool)) {}
};
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

extern "C" {
void* sfb_new(const char* path, const ShimStyle* st, size_t n, const double* pool) {
    try {
        return new Bench(path, st, n, pool);
    } catch (...) {
        return nullptr;
    }
}
void sfb_free(void* h) { delete (Bench*)h; }
void sfb_add_tile(void* h, uint8_t zoom, uint32_t x, uint32_t y, const uint32_t* way_ids, const uint32_t* way_style, size_t n) {
    BenchTile t{Tile{zoom, x, y}, std::vector<uint32_t>(way_ids, way_ids + n), std::vector<uint32_t>(way_style, way_style + n)};
    ((Bench*)h)->tiles.push_back(std::move(t));
}
// (a): returns the seconds, *out_scene the uploaded scene (the caller frees it), counts = ops, rings, refs, dashes, nodes
int sfb_run_host_feed(void* h, osmt_ctx* ctx, uint32_t scale, const uint8_t canvas[3], osmt_scene** out_scene, double* seconds, uint64_t counts[5]) {
    Bench& b = *(Bench*)h;
    SceneBuilder sb(b.reader, scale); /* copies the file's node table: once per file in a server, so outside the timed part */
    const auto t0 = std::chrono::steady_clock::now();
    const std::optional<Color> cv = Color{canvas[0], canvas[1], canvas[2]};
    for (const BenchTile& t : b.tiles) sb.add_tile(t.tile, entities_of(t.way_ids.data(), t.way_style.data(), t.way_ids.size(), b.styles), {}, cv, true);
    const osmt_batch batch = sb.batch();
    const int rc = osmt_scene_upload(ctx, &batch, out_scene);
    *seconds = seconds_since(t0);
    counts[0] = batch.n_ops, counts[1] = batch.n_rings, counts[2] = batch.n_pts, counts[3] = batch.n_dashes, counts[4] = batch.n_nodes;
    return rc;
}
// (b)
int sfb_run_device_feed(osmt_ctx* ctx, const osmt_styled_batch* batch, osmt_scene** out_scene, double* seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = osmt_scene_build_styled(ctx, batch, out_scene);
    *seconds = seconds_since(t0);
    return rc;
}
}
