// The C++ binding of the area labels of tile-built scenes (host/osmt_draw.hpp: Context::register_area_label_bindings,
// TileScene::build_all_labels / read_tile_area_labels; host/osmt_arealabels.hpp: AreaLabelBindings, HostAnchors), linked to the
// C ABI:
//   arealabels_host_demo <geodata file> <scale> <zoom> <x> <y> [<zoom> <x> <y> ...]
// Registers the file with text-free styles (an icon, nothing, a text style without a font size: no font is needed) under the
// binding rule "entity i of a kind gets i % 4 bindings, binding k names style (i + k) % 3", builds the tiles' scene and all its
// labels on the GPU — computing on this thread the anchors the device declines — and compares the area batch, byte for byte,
// with osmt::area_labels_of_tile fed with osmt_project's points and the anchors of osmt::TileLabelPositions.
// Prints "OK <labels> <anchors computed on the host>"; exit status 1 on a difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"
#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 3) % 3 != 0) return 2;
    try {
        GeodataReader r(argv[1]);
        const uint32_t scale = (uint32_t)atoi(argv[2]);
        Context ctx(0);
        GeodataDesc geo(r);
        const uint32_t gid = ctx.register_geodata(geo.desc);
        TileIndexDesc tix(r);
        ctx.register_tile_index(gid, tix.desc);
        const std::vector<double> factors = mercator_factors(geo.nodes.data(), geo.nodes.size() / 2);
        check(osmt_register_node_mercator(ctx.raw(), gid, factors.data()));
        StyleBindings sb(gid, 0, 18, r.way_count(), r.multipolygon_count());
        const uint32_t draw_bind = ctx.register_style_bindings(sb.desc());
        const uint8_t rgba[7 * 3 * 4] = {};
        const uint32_t icon = ctx.register_image(rgba, 3, 7); /* 7 high: y_offset 3 */
        std::vector<LabelStyle> st(3);
        st[0].rec.z_index = 1.0, st[0].rec.has_icon = 1, st[0].rec.icon_image = icon, st[0].icon_height = 7;
        st[1].rec.has_layer = 1, st[1].rec.layer = 0, st[1].rec.z_index = -0.0;
        st[2].rec.has_layer = 1, st[2].rec.layer = -1, st[2].rec.has_text_style = 1;
        std::vector<osmt_label_style_rec> recs;
        for (const LabelStyle& s : st) recs.push_back(s.rec);
        const uint32_t first = ctx.register_label_styles(recs);
        std::vector<LabelStyle> all(first);
        all.insert(all.end(), st.begin(), st.end());
        AreaLabelBindings lb(gid, 0, 18, r.way_count(), r.multipolygon_count());
        lb.add_text({0x41, 0x42, 0x43});
        for (int kind = 0; kind < 2; ++kind)
            for (size_t i = 0; i < (kind ? r.multipolygon_count() : r.way_count()); ++i) {
                std::vector<osmt_label_binding> b;
                for (uint32_t k = 0; k < i % 4; ++k) b.push_back(osmt_label_binding{first + (uint32_t)((i + k) % 3), k % 2 ? OSMT_TEXT_NONE : 0u});
                if (b.empty()) continue;
                if (kind)
                    lb.bind_multipolygon(i, b);
                else
                    lb.bind_way(i, b);
            }
        const uint32_t lbid = ctx.register_area_label_bindings(lb.desc());
        std::vector<osmt_query_tile> tiles;
        for (int a = 3; a + 2 < argc; a += 3) {
            osmt_query_tile q{};
            q.zoom = (uint8_t)atoi(argv[a]), q.x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), q.y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
            tiles.push_back(q);
        }
        osmt_tile_batch tb{};
        tb.tiles = tiles.data(), tb.n_tiles = tiles.size(), tb.geodata_id = gid, tb.scale = scale;
        uint32_t of_zoom[OSMT_MAX_ZOOM + 1];
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z) tb.bindings_of_zoom[z] = draw_bind, of_zoom[z] = lbid;
        TileScene scene(ctx, tb);
        const size_t on_host = scene.build_all_labels(of_zoom, nullptr, HostAnchors{&geo.desc, factors.data(), tiles.data(), scale});
        const TileAreaLabels got = scene.read_tile_area_labels();
        /* the yardstick: every entity's anchor under every tile through the batched call with its host fallback */
        TileLabelPositions tp(geo.desc, factors.data(), gid, scale);
        for (const osmt_query_tile& q : tiles) {
            const uint32_t t = tp.add_tile(q.zoom, q.x, q.y);
            for (size_t i = 0; i < r.way_count(); ++i) tp.add_way((uint32_t)i, t);
            for (size_t i = 0; i < r.multipolygon_count(); ++i) tp.add_multipolygon((uint32_t)i, t);
        }
        const std::vector<osmt_label_position> pos = tp.run(ctx.raw());
        const size_t per_tile = r.way_count() + r.multipolygon_count();
        AreaLabels want;
        std::vector<uint32_t> off{0u};
        const std::vector<double> ll = r.node_table();
        std::vector<int32_t> pts(ll.size());
        for (size_t t = 0; t < tiles.size(); ++t) {
            const osmt_query_tile& q = tiles[t];
            if (!ll.empty()) check(osmt_project(ctx.raw(), ll.data(), ll.size() / 2, q.zoom, q.x, q.y, (double)scale, pts.data()));
            area_labels_of_tile(
                r, q.zoom, q.x, q.y, scale, all, lb, [&](uint32_t n, double, double) { return std::pair<int32_t, int32_t>(pts[2 * n], pts[2 * n + 1]); },
                [&](uint32_t e) {
                    const size_t i = (e & OSMT_STYLED_MULTIPOLYGON) ? r.way_count() + (e & ~OSMT_STYLED_MULTIPOLYGON) : e;
                    return pos[t * per_tile + i];
                },
                want);
            off.push_back((uint32_t)want.labels.size());
        }
        const bool same = got.job_label_off == off && got.chars == want.chars && got.way_pts == want.way_pts && got.way_sincos == want.way_sincos &&
                          got.labels.size() == want.labels.size() &&
                          (want.labels.empty() || (memcmp(got.labels.data(), want.labels.data(), want.labels.size() * sizeof(osmt_label)) == 0 &&
                                                   memcmp(got.runs.data(), want.runs.data(), want.runs.size() * sizeof(osmt_string_run)) == 0));
        if (!same) {
            printf("DIFFERENT %zu %zu\n", got.labels.size(), want.labels.size());
            return 1;
        }
        printf("OK %zu %zu\n", want.labels.size(), on_host);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
