// Tile requests through the C++ binding (host/osmt_draw.hpp: Context::register_id_filter, TileServer::render_png,
// Worker::render_tile_png and their retry loop over osmt_last_declined_anchors), linked to the C ABI — what a server thread does
// per request:
//   tile_server_host_demo <geodata file> <scale> <out dir> <n filter ids, or -1> <id>... {<zoom> <x> <y>}...
// Registers the file as tests/scene_png_host_demo.cpp does — one draw style (a foreground fill) bound to every way and
// multipolygon, one label style (an icon of 3 x 7 pixels with the bytes (37 k + 11) mod 256, every alpha 255) bound to every odd
// way and every multipolygon — and, with ids, an id filter; states it all once in a TileServer; then
//   * TileServer::render_png: every tile in one call; anchors the device declines are computed on this thread and the call is
//     repeated;
//   * Worker::render_tile_png: tile by tile, which must give the same files.
// Writes <out dir>/tile_<i>.png; prints "OK <tiles> <png bytes> <anchors computed on the host>".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"
#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

static bool write_file(const std::string& path, const uint8_t* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    try {
        GeodataReader r(argv[1]);
        const uint32_t scale = (uint32_t)atoi(argv[2]);
        const std::string dir = argv[3];
        const long n_ids = atol(argv[4]);
        int a = 5;
        std::vector<uint64_t> ids;
        for (long i = 0; i < n_ids && a < argc; ++i, ++a) ids.push_back(strtoull(argv[a], nullptr, 10));
        if ((n_ids >= 0 && (long)ids.size() != n_ids) || (argc - a) % 3 || a == argc) return 2;
        Context ctx(0);
        GeodataDesc geo(r);
        const uint32_t gid = ctx.register_geodata(geo.desc);
        TileIndexDesc tix(r);
        ctx.register_tile_index(gid, tix.desc);
        const std::vector<double> factors = mercator_factors(geo.nodes.data(), geo.nodes.size() / 2);
        check(osmt_register_node_mercator(ctx.raw(), gid, factors.data()));
        osmt_style_rec fill{};
        fill.has_fill_color = 1, fill.fill_color[0] = 170, fill.fill_color[1] = 200, fill.fill_color[2] = 150, fill.is_foreground_fill = 1;
        const uint32_t draw = ctx.register_styles({fill}, {});
        StyleBindings sb(gid, 0, 18, r.way_count(), r.multipolygon_count());
        for (size_t i = 0; i < r.way_count(); ++i) sb.bind_way(i, {draw});
        for (size_t i = 0; i < r.multipolygon_count(); ++i) sb.bind_multipolygon(i, {draw});
        const uint32_t draw_bind = ctx.register_style_bindings(sb.desc());
        uint8_t rgba[7 * 3 * 4];
        for (size_t k = 0; k < sizeof rgba; ++k) rgba[k] = (k & 3) == 3 ? 255 : (uint8_t)(37 * k + 11);
        const uint32_t icon = ctx.register_image(rgba, 3, 7);
        LabelStyle ls;
        ls.rec.has_icon = 1, ls.rec.icon_image = icon, ls.icon_height = 7;
        const uint32_t first = ctx.register_label_styles({ls.rec});
        AreaLabelBindings lb(gid, 0, 18, r.way_count(), r.multipolygon_count());
        for (size_t i = 1; i < r.way_count(); i += 2) lb.bind_way(i, {osmt_label_binding{first, OSMT_TEXT_NONE}});
        for (size_t i = 0; i < r.multipolygon_count(); ++i) lb.bind_multipolygon(i, {osmt_label_binding{first, OSMT_TEXT_NONE}});
        const uint32_t lbid = ctx.register_area_label_bindings(lb.desc());

        osmt_tile_server_desc d = TileServer::describe(gid, Color{241, 238, 232});
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) d.bindings_of_zoom[z] = draw_bind, d.area_label_bindings_of_zoom[z] = lbid;
        if (n_ids >= 0) d.id_filter = ctx.register_id_filter(gid, ids);
        TileServer server(ctx, d);

        std::vector<osmt_tile_coord> tiles;
        std::vector<osmt_query_tile> qt; /* what osmt::HostAnchors reads: the same tiles */
        for (; a + 2 < argc; a += 3) {
            osmt_tile_coord t{(uint32_t)strtoul(argv[a + 1], nullptr, 10), (uint32_t)strtoul(argv[a + 2], nullptr, 10), (uint32_t)atoi(argv[a])};
            tiles.push_back(t);
            osmt_query_tile q{};
            q.x = t.x, q.y = t.y, q.zoom = (uint8_t)t.zoom;
            qt.push_back(q);
        }
        size_t on_host = 0;
        const std::vector<std::vector<uint8_t>> files = server.render_png(tiles, scale, HostAnchors{&geo.desc, factors.data(), qt.data(), scale}, &on_host);
        Worker worker(ctx);
        size_t bytes = 0;
        for (size_t i = 0; i < tiles.size(); ++i) {
            size_t mine = 0;
            const std::vector<uint8_t> one = worker.render_tile_png(server, tiles[i], scale, HostAnchors{&geo.desc, factors.data(), &qt[i], scale}, &mine);
            if (one != files[i]) {
                printf("DIFFERENT file %zu\n", i);
                return 1;
            }
            on_host += mine;
            if (!write_file(dir + "/tile_" + std::to_string(i) + ".png", files[i].data(), files[i].size())) return 4;
            bytes += files[i].size();
        }
        printf("OK %zu %zu %zu\n", files.size(), bytes, on_host);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
