// Tile coordinates in, PNG files out, through the C++ binding (host/osmt_draw.hpp: Context::render_tiles_png, TileScene::render_png /
// render_host), linked to the C ABI — what a server thread without a HIP runtime of its own does per batch of requests:
//   scene_png_host_demo <geodata file> <scale> <out dir> <zoom> <x> <y> [<zoom> <x> <y> ...]
// Registers the file with one draw style (a foreground fill) bound to every way and multipolygon and one label style (an icon
// of 3 x 7 pixels with the bytes (37 k + 11) mod 256, every alpha 255) bound to every odd way and every multipolygon, then
//   * Context::render_tiles_png: build, label (anchors the device declines are computed on this thread), render, files;
//   * the same by hand — TileScene, build_all_labels, render_png — which must give the same files, twice (the scene is borrowed);
//   * TileScene::render_host, RGB8 and RGBA8, which must agree pixel for pixel.
// Writes <out dir>/tile_<i>.png and <out dir>/tiles.rgb (the RGB8 tiles back to back); prints "OK <tiles> <png bytes>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 7 || (argc - 4) % 3 != 0) return 2;
    try {
        GeodataReader r(argv[1]);
        const uint32_t scale = (uint32_t)atoi(argv[2]);
        const std::string dir = argv[3];
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
        std::vector<osmt_query_tile> tiles;
        for (int a = 4; a + 2 < argc; a += 3) {
            osmt_query_tile q{};
            q.zoom = (uint8_t)atoi(argv[a]), q.x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), q.y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
            q.has_canvas = 1, q.canvas_rgb[0] = 241, q.canvas_rgb[1] = 238, q.canvas_rgb[2] = 232;
            tiles.push_back(q);
        }
        osmt_tile_batch tb{};
        tb.tiles = tiles.data(), tb.n_tiles = tiles.size(), tb.geodata_id = gid, tb.scale = scale, tb.use_caps_for_dashes = 1;
        uint32_t of_zoom[OSMT_MAX_ZOOM + 1];
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) tb.bindings_of_zoom[z] = draw_bind, of_zoom[z] = lbid;
        const HostAnchors host{&geo.desc, factors.data(), tiles.data(), scale};

        const std::vector<std::vector<uint8_t>> files = ctx.render_tiles_png(tb, of_zoom, nullptr, host);

        TileScene scene(ctx, tb);
        scene.build_all_labels(of_zoom, nullptr, host);
        if (scene.render_png() != files || scene.render_png() != files) {
            printf("DIFFERENT files\n");
            return 1;
        }
        const std::vector<uint8_t> rgb = scene.render_host(true), px = scene.render_host(false);
        const size_t n_px = tiles.size() * (size_t)TILE_SIZE * scale * TILE_SIZE * scale;
        if (rgb.size() != 3 * n_px || px.size() != 4 * n_px) return 1;
        for (size_t i = 0; i < n_px; ++i)
            if (memcmp(&rgb[3 * i], &px[4 * i], 3) != 0) {
                printf("DIFFERENT pixel %zu\n", i);
                return 1;
            }
        size_t bytes = 0;
        for (size_t i = 0; i < files.size(); ++i) {
            if (!write_file(dir + "/tile_" + std::to_string(i) + ".png", files[i].data(), files[i].size())) return 4;
            bytes += files[i].size();
        }
        if (!write_file(dir + "/tiles.rgb", rgb.data(), rgb.size())) return 4;
        printf("OK %zu %zu\n", files.size(), bytes);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
