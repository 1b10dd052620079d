/*
 * osmt_host.h — what the host files of libosmtile.so (osmt_api.cpp, osmt_host_worker.cpp, osmt_host_multi.cpp,
 * osmt_host_tagstyle.cpp, osmt_host_pyramid.cpp, osmt_host_polygons.cpp, osmt_host_resolve.cpp) share: the context and scene objects, guarded(), HIP_TRY, the two per-call
 * holders table_upload and call_work, and the declarations of what one file takes from another.  Internal: nothing declared here leaves the library
 * (hidden visibility).  Nothing here is a variable, a static function or an anonymous namespace: every function has ONE
 * definition, in the .cpp named above its declaration, and is documented there (inline here: guarded, align_up and the members
 * of the two holders); every thread-local and every cached setting stays private to its file.
 */
#ifndef OSMT_HOST_H
#define OSMT_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <dlfcn.h>

#include <memory>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_cascade_tables.h" /* the tables of a rule set: osmt_cs_resolve */
#include "osmt_geom.h"
#include "osmt_internal.h"
#include "osmt_pool_layout.h"
#include "osmt_numparse.h" /* osmt_bytes_cmp: the key order of osmt_validate_tags */
#include "osmt_utf8.h"     /* the byte a refused tag value stops the decoder at */
#include "osmt_png_table.h" /* PNG_LMAX, PNG_BLOCK_HDR_BITS: the slot bound */
#include "../host/osmt_idfilter.hpp"   /* osmt::id_filter_set: the sort and dedup of a registered id filter */
#include "../host/osmt_textplacer.hpp" /* osmt::validate_text_labels */
#include "../host/osmt_textshaper.hpp" /* osmt::validate_font, osmt::validate_string_labels */

#pragma GCC visibility push(hidden)

namespace osmt_host {

/* the two request types osmt_ctx queues; defined in osmt_host_worker.cpp */
struct coalesce_req; /* osmt_worker_render */
struct tile_req;     /* osmt_worker_render_tile_png */

/* osmt_api.cpp: the message osmt_last_error() returns, per thread */
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(_e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "%s failed: %s", #expr, \
                        hipGetErrorString(_e));                                                  \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* No C++ exception may cross the C boundary (a std::bad_alloc from a host-side table, say): every entry point
 * runs its body through this. */
template <class F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(OSMT_OOM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(OSMT_HIP_ERROR, "internal error: %s", e.what());
    } catch (...) {
        return fail(OSMT_HIP_ERROR, "internal error");
    }
}

}  // namespace osmt_host

struct osmt_ctx {
    int device = 0;
    std::mutex mu; /* guards the image registry */
    /* Device buffers of finished calls, kept for the next one: a per-request server loop uploads, renders and frees
     * a scene per call, and hipMalloc / hipFree of a few hundred MB cost more than the kernels. */
    struct cached_buf {
        void* p;
        size_t bytes;
        bool used;
        uint64_t tick; /* when it was last handed out: the idle buffers given back to the driver are the least recently used */
    };
    std::mutex cache_mu;
    std::vector<cached_buf> cache;
    uint64_t cache_tick = 0;
    /* idle non-blocking streams: every host-buffer call runs on its own stream, so calls from the reference's N
     * worker threads (http_server.rs:50-83) overlap on the GPU instead of queueing behind the NULL stream */
    std::vector<hipStream_t> idle_streams;
    hipStream_t poison_stream = nullptr; /* OSMT_POISON_ALLOC: the fills run on a stream of the highest priority (dev_poison) */
    std::vector<cached_buf> host_cache; /* pinned staging buffers (one packed H2D copy per small call) */
    std::vector<osmt_image_desc> images;
    std::vector<double> image_pool_host; /* premultiplied f64 RGBA */
    /* Device copy of the registry.  A registration followed by a render makes a NEW pair of buffers; the old pair
     * moves to `image_graveyard` and lives until the context goes, so a kernel launched by another worker thread
     * with the previous snapshot never reads freed memory (registrations are rare: once per icon at start-up). */
    osmt_image_desc* d_images = nullptr;
    double4* d_image_pool = nullptr;
    uint32_t d_n_images = 0;
    std::vector<void*> image_graveyard;
    bool images_dirty = false;
    /* the glyph table of osmt_register_glyphs (outlines of glyph-run labels), same snapshot rules as the icons: a
     * registration followed by a use makes a new device pair, the old one joins image_graveyard */
    std::vector<osmt_glyph_vertex> glyph_verts;
    std::vector<uint32_t> glyph_voff{0u};
    osmt_glyph_vertex* d_glyph_verts = nullptr;
    uint32_t* d_glyph_voff = nullptr;
    uint32_t d_n_glyphs = 0;
    bool glyphs_dirty = false;
    /* the fonts of osmt_register_font (string labels).  The host copies serve the validation (metrics, table sizes) and
     * the upload; a font's tables get ONE device allocation at their first use and never move, so only the array of
     * osmt_font_dev records is replaced when a font is appended — the old array joins image_graveyard, and a launch
     * that holds it keeps reading valid records of valid tables */
    struct font_host {
        std::vector<osmt_cmap_entry> cmap;
        std::vector<int32_t> advance;
        std::vector<uint32_t> outline;
        std::vector<osmt_kern_pair> kern;
        osmt_font_desc view{}; /* over the vectors above */
        void* d_pool = nullptr;
        osmt_font_dev dev{};
    };
    std::vector<std::shared_ptr<font_host>> fonts;
    osmt_font_dev* d_fonts = nullptr;
    uint32_t d_n_fonts = 0;
    bool fonts_dirty = false;
    /* the geodata files of osmt_register_geodata (scenes built on the device): one device allocation per file, made at
     * registration, that never moves and lives as long as the context — a built scene's node table points into it */
    struct geodata_host {
        size_t n_nodes = 0, n_ways = 0, n_mps = 0;
        size_t n_polys = 0, n_way_nodes = 0, n_poly_nodes = 0, n_mp_polys = 0; /* the other lengths of dev's arrays (osmt_build_tile_index) */
        void* d_pool = nullptr;
        osmt_geo_dev dev{};
        /* its z18 tile index (osmt_register_tile_index): at most one, an allocation of its own under the same rules */
        void* d_index = nullptr;
        osmt_tq_index_dev ix{};
        /* the node lists of that index and the nodes' global ids (osmt_register_node_index): at most one, same rules */
        void* d_node_index = nullptr;
        const uint32_t *d_node_off = nullptr, *d_node_refs = nullptr, *d_zero_off = nullptr; /* [ix.n_tiles + 1], pool, [ix.n_tiles + 1] zeros */
        const uint64_t* d_node_gid = nullptr;
        /* an index built on the device (osmt_build_tile_index, osmt_host_pyramid.cpp): d_index, and d_node_index where the build
         * registered the node index too, then name ONE dev_alloc buffer that is never given back and goes with the context's
         * buffers — the teardown frees only what a registration allocated itself.  The build always makes the node lists:
         * built_node_off / built_nodes ([ix.n_tiles + 1], pool) serve osmt_read_tile_index where no node index is registered */
        bool index_built = false, node_index_built = false;
        bool index_building = false; /* a build is under way: a second one is refused */
        const uint32_t *built_node_off = nullptr, *built_nodes = nullptr;
        /* its tile index pyramid (osmt_register_tile_pyramid, osmt_host_pyramid.cpp): at most one.  A level is a dev_alloc
         * buffer that is never given back: it never moves and goes with the context's buffers */
        struct pyramid_level {
            osmt_tq_index_dev ix{};          /* as the tile query reads it */
            const uint32_t* tile_x = nullptr; /* [ix.n_tiles], for osmt_read_tile_pyramid */
            const uint32_t *node_off = nullptr, *nodes = nullptr, *zero_off = nullptr; /* node lists (or NULL), [ix.n_tiles + 1] zeros */
            size_t n_way_refs = 0, n_mp_refs = 0, n_node_refs = 0;
        };
        struct pyramid_host {
            uint32_t mask = 0, node_mask = 0;
            pyramid_level level[OSMT_MAX_ZOOM + 1];
            /* [OSMT_MAX_ZOOM + 1] each, device memory, written once at registration: the index a tile of each zoom reads — the
             * smallest level >= the zoom, the z18 index where there is none; node_table (NULL without node lists): the same
             * over the node lists */
            const osmt_tq_index_dev *area_table = nullptr, *node_table = nullptr;
        };
        std::shared_ptr<const pyramid_host> pyramid;
        bool pyramid_building = false; /* a registration is under way: a second one is refused */
        /* the Mercator factors of its nodes (osmt_register_node_mercator): at most one table, same rules */
        const double2* d_factors = nullptr; /* [n_nodes] */
        /* its tags (osmt_register_tags): at most one table, same rules */
        void* d_tags = nullptr;
        osmt_sm_tags_dev tags{};
        size_t tags_string_bytes = 0, n_node_tags = 0, n_way_tags = 0;
    };
    std::vector<geodata_host> geodata;
    /* the selector sets of osmt_register_selectors: append-only, one device allocation each that never moves */
    struct selectors_host {
        void* d_pool = nullptr;
        osmt_sm_sels_dev dev{};
        std::shared_ptr<const std::vector<uint8_t>> zooms; /* [n_sels][2] the zooms a selector admits, inclusive: for the rule sets */
    };
    std::vector<selectors_host> selectors;
    /* the rule sets of osmt_register_rules, under the same rules */
    struct rules_host {
        void* d_pool = nullptr;
        osmt_cs_rules_dev dev{};
        uint32_t selectors_id = 0;
        std::shared_ptr<const std::vector<uint32_t>> key_off; /* the pooled `text` strings */
        std::shared_ptr<const std::vector<uint8_t>> key_bytes;
    };
    std::vector<rules_host> rules;
    uint32_t match_hash_bits = 32; /* osmt_debug_match_hash_bits */
    uint32_t vertex_hash_bits = 32; /* osmt_debug_vertex_hash_bits (osmt_host_polygons.cpp) */
    uint32_t resolve_short_way_max = OSMT_RES_SHORT_WAY_DEFAULT; /* osmt_debug_resolve_short_way_max (osmt_host_resolve.cpp) */
    /* the tables of osmt_register_style_bindings: append-only, one device allocation each that never moves, so a build
     * that holds a table's pointers is not disturbed by a later registration */
    struct bindings_host {
        uint32_t geodata_id = 0;
        uint8_t zoom_lo = 0, zoom_hi = 0;
        void* d_pool = nullptr;
        osmt_tq_bind_dev dev{};
    };
    std::vector<bindings_host> bindings;
    /* the tables of osmt_register_label_bindings, under the same rules */
    struct label_bindings_host {
        uint32_t geodata_id = 0;
        uint8_t zoom_lo = 0, zoom_hi = 0;
        void* d_pool = nullptr;
        osmt_tl_bind_dev dev{};
        size_t n_nodes = 0, n_bindings = 0, n_texts = 0, n_chars = 0; /* osmt_read_label_bindings */
    };
    std::vector<label_bindings_host> label_bindings;
    /* the tables of osmt_register_area_label_bindings, under the same rules */
    struct area_label_bindings_host {
        uint32_t geodata_id = 0;
        uint8_t zoom_lo = 0, zoom_hi = 0;
        void* d_pool = nullptr;
        osmt_al_bind_dev dev{};
        size_t n_ways = 0, n_mps = 0, n_way_bindings = 0, n_mp_bindings = 0, n_texts = 0, n_chars = 0; /* osmt_read_area_label_bindings */
    };
    std::vector<area_label_bindings_host> area_label_bindings;
    /* the id filters of osmt_register_id_filter, under the same rules: the sorted set and the three planes in one allocation */
    struct id_filter_host {
        uint32_t geodata_id = 0;
        bool on = false; /* in a scene: it was built with this filter */
        void* d_pool = nullptr;
        const uint32_t *way = nullptr, *mp = nullptr, *node = nullptr; /* node: NULL without a node plane */
        size_t n_way_words = 0, n_mp_words = 0, n_node_words = 0;      /* 32-bit words */
    };
    std::vector<id_filter_host> id_filters;
    /* the label styles of osmt_register_label_styles: records and ranks, replaced like the style table when it has grown */
    std::vector<osmt_label_style_rec> label_styles;
    osmt_label_style_rec* d_label_styles = nullptr;
    uint32_t* d_label_rank = nullptr;
    uint32_t d_n_label_styles = 0;
    bool label_styles_dirty = false;
    /* the styles of osmt_register_styles, same snapshot rules as the glyph table: a registration followed by a build makes
     * a new device triple (records, ranks, dash pool), the old one joins image_graveyard */
    std::vector<osmt_style_rec> styles;
    std::vector<double> style_dashes;
    osmt_style_rec* d_styles = nullptr;
    uint32_t* d_style_rank = nullptr;
    double* d_style_dashes = nullptr;
    uint32_t d_n_styles = 0;
    bool styles_dirty = false;
    /* one reference for the handle returned by osmt_create + one per live scene: osmt_destroy on a context that still
     * has scenes only drops the handle's reference, the last osmt_scene_free tears the context down */
    std::atomic<int> refs{1};
    /* RCCL communicator of the tile-count reduction (osmt_comm_init_*): ncclComm_t, rank and size */
    void* comm = nullptr;
    uint32_t comm_rank = 0, comm_size = 0;
    unsigned long long* d_count = nullptr; /* device words of the reductions: [0], [1] blocking call, [2], [3] enqueued one */
    /* One pinned, device-visible word per live scene: a pre-pass kernel whose arena reservation does not fit stores a code
     * there (osmt_prepass_args.err) and the host reads it behind the synchronisation it does anyway — an internal error
     * surfaces as OSMT_HIP_ERROR instead of blank tiles, and costs no copy and no extra wait. */
    uint32_t* err_page = nullptr;
    std::vector<uint16_t> err_free;
    /* What the pre-pass arenas of recent big uploads needed per fill op / per virtual stroke segment, by scale: the next
     * big upload of a host-buffer call takes its arenas from these densities (+ 25 %) instead of asking the device with a
     * counting run of the pre-pass and a round trip; see scene_size_arenas (guarded by cache_mu). */
    struct arena_density {
        double groups_per_fill = 0.0, recs_per_vseg = 0.0;
        uint32_t uploads = 0;
    } density[OSMT_MAX_SCALE + 1];
    /* The gathering point of the per-request entry (osmt_worker_render): requests of concurrent worker threads wait here
     * and are rendered together, see osmt_host_worker.cpp. */
    std::mutex co_mu;
    std::condition_variable co_cv;
    std::deque<osmt_host::coalesce_req*> co_queue;
    int co_in_flight = 0;
    /* the same for osmt_worker_render_tile_png: its own queue, the SAME count of groups in flight, and osmt_worker_tile_stats */
    std::deque<osmt_host::tile_req*> co_tile_queue;
    uint64_t co_tile_stats[3] = {0, 0, 0}; /* requests, groups run, tiles of the largest group */
    /* osmt_label_positions_stats: requests / left the LDS tier / answered TOO_LARGE of the last completed call (cache_mu) */
    uint64_t pl_stats[3] = {0, 0, 0};
    /* osmt_tile_query_stats: (tile, column) items and way / multipolygon / node candidates the last completed tile query
     * gathered, before dedup (cache_mu) */
    uint64_t tq_stats[4] = {0, 0, 0, 0};
};

struct osmt_scene {
    osmt_ctx* ctx = nullptr;
    uint32_t n_jobs = 0, n_ops = 0, n_rings = 0, n_pts = 0, n_dashes = 0, n_strokes = 0;
    uint32_t scale = 1, coord_kind = 0, n_blk = 0;
    char* d_base = nullptr; /* one allocation, carved below */
    char* d_front = nullptr; /* big uploads: the arrays the host provides, in an allocation of their own (copied by a helper thread while the tables are built) */
    size_t bytes = 0;
    osmt_tile_job* d_jobs = nullptr;
    osmt_op* d_ops = nullptr;
    osmt_ring* d_rings = nullptr;
    double* d_latlon = nullptr;     /* per point, or the node table (OSMT_COORD_NODE_REF) */
    uint32_t* d_node_refs = nullptr;
    int32_t* d_pts = nullptr;
    double* d_dashes = nullptr;
    uint32_t* d_pt_job = nullptr;
    uint32_t* d_op_aux = nullptr;
    osmt_opinfo* d_info = nullptr;
    osmt_stroke_aux* d_aux = nullptr;
    osmt_dash_seg* d_dseg = nullptr;
    uint32_t* d_submask = nullptr;
    uint32_t* d_op_blk = nullptr;
    uint32_t* d_op_vseg = nullptr; /* op -> its first virtual segment (stroke ops with segments) */
    osmt_blk_bbox* d_blk = nullptr;
    uint32_t* d_op_job = nullptr;
    osmt_vseg* d_vseg = nullptr; /* per virtual segment: end points, traveled, length, slot offset, op (k_opinfo -> k_prebin) */
    unsigned long long* d_cursors = nullptr; /* 4 words; the per-sub-tile list counts follow (one memset) */
    uint32_t* d_cnt = nullptr;
    uint2* d_hdr = nullptr;
    osmt_ent* d_ent = nullptr;
    unsigned long long ent_cap = 0;
    uint32_t n_fill_ops = 0;
    uint32_t n_vsegs = 0;
    /* the two arenas of the pre-pass (fill coverage words, stroke records + keys): one allocation, sized at upload */
    char* d_arena = nullptr;
    uint32_t* d_fmask = nullptr;
    osmt_srec* d_srec = nullptr;
    uint2* d_skey = nullptr;
    unsigned long long fmask_cap = 0, srec_cap = 0; /* 64-byte groups / records */
    /* the fill slots of k_prebin (osmt_fill_slots.h), in the same allocation */
    osmt_fill_slot* d_slots = nullptr;
    unsigned long long slot_cap = 0;
    uint32_t n_fill_pass = 0; /* passes of four slots, where the sizing run counted them; 0: not known (worst-case or guessed sizes) */
    /* host-side tables whose upload may still be in flight on the call's stream */
    std::vector<uint32_t> h_pt_job, h_op_aux, h_op_blk, h_op_vseg, h_op_job, h_lab_wide;
    std::vector<osmt_label_band> h_lab_bands;
    std::vector<osmt_labelinfo> h_lab_info;
    hipStream_t own_stream = nullptr; /* internal per-call scene: everything about it happens on this stream */
    /* public scenes: one event per stream the scene was rendered on, recorded behind the last launch that reads it.
     * osmt_scene_free / set_labels / read_* wait for THESE events only — never for the device — so worker threads
     * with their own scenes and streams do not stall each other (http_server.rs:50-83: independent workers). */
    std::mutex use_mu;
    std::vector<std::pair<hipStream_t, hipEvent_t>> last_use;
    void* h_stage = nullptr;          /* pinned staging of a packed upload, returned to the pool when the scene goes */
    uint32_t* h_err = nullptr;        /* the scene's word of osmt_ctx::err_page (NULL: none left, errors stay unreported) */
    uint32_t max_job_ops = 0;         /* most ops of any of the scene's tiles: at most OSMT_FOLD_MAX_OPS = no list kernel */
    bool arena_guess = false;         /* the arenas were sized from osmt_ctx::density, not by the device: an overflow is a miss, not a bug */
    /* label pass (osmt_scene_set_labels): its own allocation */
    uint32_t n_labels = 0, n_label_segs = 0;
    char* d_lab_base = nullptr;
    osmt_labelinfo* d_lab = nullptr;
    uint32_t* d_job_label_off = nullptr;
    double* d_lab_segs = nullptr;
    double* d_lab_a = nullptr;
    double* d_lab_s_wide = nullptr;
    uint32_t* d_lab_wide = nullptr;
    osmt_label_band* d_lab_bands = nullptr;
    unsigned long long* d_lab_bits = nullptr;
    uint32_t n_lab_bands = 0;
    uint32_t n_lab_wide = 0;
    bool lab_cover_valid = false; /* a render has written the coverage planes of the attached labels (osmt_scene_read_label_cover) */
    uint32_t* d_lab_bitmap = nullptr;
    uint8_t* d_lab_ok = nullptr;
    uint32_t* d_lab_err = nullptr;
    osmt_tile_label* d_tile_labels = nullptr;
    uint32_t* d_tile_label_cnt = nullptr;
    /* text-run labels (osmt_scene_set_text_labels): the glyph instances k_text_place wrote, kept for
     * osmt_scene_read_glyph_instances; an allocation of its own, gone with the next set call */
    osmt_glyph_instance* d_text_inst = nullptr;
    uint32_t n_text_inst = 0;
    /* string labels (osmt_scene_set_string_labels): the records k_text_shape wrote and k_text_place read, kept for
     * osmt_scene_read_text_glyphs under the same rules */
    osmt_text_glyph* d_text_glyphs = nullptr;
    uint32_t n_text_glyphs = 0;
    /* a scene of osmt_scene_build_tiles: the styled batch the device derived, kept for osmt_scene_read_styled_areas */
    char* d_tq = nullptr;           /* tiles + tile_base */
    char* d_tq_areas_buf = nullptr; /* the areas */
    const osmt_styled_tile* d_tq_tiles = nullptr;
    const osmt_styled_area* d_tq_areas = nullptr;
    size_t n_tq_areas = 0;
    std::vector<osmt_query_tile> h_tq_tiles; /* the tiles it was built from, for osmt_scene_build_tile_labels */
    uint32_t tq_geodata_id = 0;
    osmt_ctx::id_filter_host tq_filter; /* the snapshot of the filter it was built with (osmt_scene_build_tiles_filtered); `on` false: none */
    /* the node batch the last osmt_scene_build_tile_labels read back (osmt_scene_read_tile_labels) */
    std::vector<osmt_label> h_tl_labels;
    std::vector<osmt_string_run> h_tl_runs;
    std::vector<uint32_t> h_tl_chars, h_tl_off;
    /* the area batch the last osmt_scene_build_tile_labels_all read back (osmt_scene_read_tile_area_labels), and the pairs
     * its anchor search declined (osmt_scene_read_declined_anchors) */
    std::vector<osmt_label> h_al_labels;
    std::vector<osmt_string_run> h_al_runs;
    std::vector<uint32_t> h_al_chars, h_al_off;
    std::vector<int32_t> h_al_pts;
    std::vector<double> h_al_sincos;
    std::vector<osmt_area_anchor> h_al_declined;
};

namespace osmt_host {

/* ---- osmt_api.cpp ---- */
bool poison_alloc();
hipError_t dev_alloc(osmt_ctx* ctx, void** out, size_t bytes);
hipError_t stream_acquire(osmt_ctx* ctx, hipStream_t* out);
void stream_release(osmt_ctx* ctx, hipStream_t st);
void* stage_acquire(osmt_ctx* ctx, size_t bytes);
void stage_release(osmt_ctx* ctx, void* p);
void dev_free(osmt_ctx* ctx, void* p);
bool trace_upload();
void ctx_release(osmt_ctx* ctx);
hipError_t copy_back(osmt_ctx* ctx, void* dst, const void* src, size_t bytes);
int validate_batch_global(const osmt_batch* b);
int validate_job(const osmt_batch* b, size_t j, bool with_coords = true);
int validate_nodes(const osmt_batch* b, size_t lo, size_t hi);
int validate_batch(const osmt_batch* b, bool with_coords = true);
int check_offsets_of(const char* who, const char* what, const uint32_t* offs, size_t count, size_t total);
int validate_styles(const osmt_style_rec* st, size_t n, const double* dashes, size_t n_dashes, size_t n_images);
size_t ctx_image_count(osmt_ctx* ctx);
int register_styles_body(osmt_ctx* ctx, const osmt_style_rec* st, size_t n, const double* dashes, size_t n_dashes, uint32_t* out_first);
int validate_label_styles(const osmt_label_style_rec* st, size_t n, osmt_ctx* ctx);
int register_label_styles_body(osmt_ctx* ctx, const osmt_label_style_rec* st, size_t n, uint32_t* out_first);
int scene_build_tiles_body(osmt_ctx* ctx, const osmt_tile_batch* b, uint32_t filter_id, osmt_scene** out_scene);
int scene_build_tile_labels_all_body(osmt_ctx* ctx, osmt_scene* sc, const uint32_t* area_of_zoom, const uint32_t* node_of_zoom,
                                     const osmt_area_anchor* anchors, size_t n_anchors);
int osmt_render_batch_labels_body(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba,
                                  size_t stride, bool rgb = false, bool trusted = false, const osmt_glyph_label_batch* glabels = nullptr,
                                  const osmt_text_label_batch* tlabels = nullptr, const osmt_string_label_batch* slabels = nullptr);

/* ---- osmt_host_pyramid.cpp ---- */
/* The index a tile query reads per zoom: P.ix = z18 (the registered index in the form the query reads), and P.ixz = the
 * resident table of the file's pyramid for the kind (nodes: the node query of the tile labels, which reads node lists as its
 * "ways"), NULL where the file has no pyramid that serves the kind.  Nothing is uploaded. */
void tq_bind_levels(const osmt_ctx::geodata_host& geo, bool nodes, const osmt_tq_index_dev& z18, osmt_tq_pass& P);
/* what osmt_tile_query_stats reports from now on */
void tq_stats_set(osmt_ctx* ctx, uint64_t items, uint64_t ways, uint64_t mps, uint64_t nodes);

/* ---- osmt_host_multi.cpp ---- */
void comm_destroy(osmt_ctx* ctx); /* ctx_teardown: the communicator and the words of the reductions go with the context */

/* ---- a registered table on its way to the device ---- */
struct table_upload {
    char* pool = nullptr;
    /* one device allocation that never moves once it is registered; a failure is remembered and skips the copies */
    table_upload(const char* name, const pool_layout& pl) : name_(name) {
        const hipError_t e = hipMalloc((void**)&pool, pl.size());
        if (e == hipSuccess) return;
        pool = nullptr;
        rc_ = fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) for the %s failed: %s", pl.size(), name, hipGetErrorString(e));
    }
    table_upload(const table_upload&) = delete;
    table_upload& operator=(const table_upload&) = delete;
    ~table_upload() {
        if (pool) (void)hipFree(pool);
    }
    /* blocking copies; after the first error the others are skipped */
    void put(size_t o, const void* src, size_t bytes) {
        if (rc_ != OSMT_OK || !bytes) return;
        const hipError_t e = hipMemcpy(pool + o, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc_ = fail(OSMT_HIP_ERROR, "%s upload failed: %s", name_, hipGetErrorString(e)); /* every table says so, OOM or not */
    }
    /* OSMT_OK, or what the first failure reported */
    int done() const { return rc_; }
    /* registered: the context owns the allocation from here on */
    void release() { pool = nullptr; }

   private:
    const char* name_;
    int rc_ = OSMT_OK;
};

/* ---- what a per-call GPU pipeline holds while it runs ---- */
struct call_work {
    enum { MAX_WORK = 8, MAX_EV = 12 };
    osmt_ctx* ctx;
    hipStream_t st = nullptr;
    char* work[MAX_WORK] = {}; /* dev_alloc buffers, given back at the end */
    char* pool = nullptr;      /* a hipMalloc'ed table, until it is registered */
    const bool trace = trace_upload(); /* OSMT_TRACE_UPLOAD=1 (diagnostic): the device time of the stages, one line on stderr */
    hipEvent_t ev[MAX_EV] = {};

    /* who: "tile query" in "hipMalloc(%zu) for the tile query (%s) failed"; borrowed: the caller's stream, or NULL — begin() takes a pooled one */
    call_work(osmt_ctx* ctx_, const char* who, hipStream_t borrowed = nullptr) : ctx(ctx_), st(borrowed), who_(who), own_stream_(!borrowed) {}
    call_work(const call_work&) = delete;
    call_work& operator=(const call_work&) = delete;
    ~call_work() {
        if (st) (void)hipStreamSynchronize(st); /* nothing may still read the buffers or the caller's arrays */
        for (char* p : work) dev_free(ctx, p);
        if (pool) (void)hipFree(pool);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (own_stream_) stream_release(ctx, st);
    }
    int begin(int n_ev) {
        if (n_ev > MAX_EV) return fail(OSMT_HIP_ERROR, "internal error: the %s marks %d trace events (at most %d)", who_, n_ev, (int)MAX_EV);
        if (own_stream_) HIP_TRY(stream_acquire(ctx, &st));
        if (trace)
            for (; n_ev_ < n_ev; ++n_ev_) HIP_TRY(hipEventCreate(&ev[n_ev_]));
        return OSMT_OK;
    }
    /* a work buffer of the layout's size (+ 256: the kernels' reads past a last element stay inside) */
    int alloc(char** out, const pool_layout& pl, const char* what = nullptr) const {
        const hipError_t e = dev_alloc(ctx, (void**)out, pl.size() + 256);
        if (e == hipSuccess) return OSMT_OK;
        *out = nullptr;
        const int code = e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR;
        if (!what) return fail(code, "hipMalloc(%zu) for the %s failed: %s", pl.size(), who_, hipGetErrorString(e));
        return fail(code, "hipMalloc(%zu) for the %s (%s) failed: %s", pl.size(), who_, what, hipGetErrorString(e));
    }
    int alloc(int slot, const pool_layout& pl, const char* what = nullptr) {
        if (slot < 0 || slot >= MAX_WORK) return fail(OSMT_HIP_ERROR, "internal error: the %s asks for work buffer %d (at most %d)", who_, slot, (int)MAX_WORK);
        return alloc(&work[slot], pl, what);
    }
    int alloc_pool(const pool_layout& pl) {
        const hipError_t e = hipMalloc((void**)&pool, pl.size());
        if (e == hipSuccess) return OSMT_OK;
        pool = nullptr;
        return fail(e == hipErrorOutOfMemory ? OSMT_OOM : OSMT_HIP_ERROR, "hipMalloc(%zu) for the %s (table) failed: %s", pl.size(), who_, hipGetErrorString(e));
    }
    /* i, a, b: below the n_ev of begin(); without the trace there are no events and nothing is recorded */
    hipError_t mark(int i) const { return i < n_ev_ ? hipEventRecord(ev[i], st) : trace ? hipErrorInvalidValue : hipSuccess; }
    double us(int a, int b) const {
        float ms = 0.f;
        if (a < n_ev_ && b < n_ev_) (void)hipEventElapsedTime(&ms, ev[a], ev[b]);
        return ms * 1e3;
    }

   private:
    const char* who_;
    bool own_stream_;
    int n_ev_ = 0; /* events created */
};

}  // namespace osmt_host

#pragma GCC visibility pop

#endif /* OSMT_HOST_H */
