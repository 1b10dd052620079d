/*
 * osmtile.h — C ABI of the MI355X tile rasterizer (libosmtile.so).
 *
 * Drop-in boundary for ONE hot path of dfyz/osm-renderer: the per-tile
 * project -> fill -> stroke -> blend -> RGB(A) pipeline.  The reference has no
 * FFI of its own (pure Rust crate); every entry point below cites the
 * reference interface (path:line under /root/reference) it stands in for.
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; all structs are POD with fixed layout;
 *   - the caller owns every input/output buffer for the duration of a call
 *     (borrowed, never retained — the Rust `&` / `&mut` of the reference);
 *   - every function returns an osmt_status (0 = OK, negative = error) unless
 *     stated; the message of the last error on the calling thread is
 *     available from osmt_last_error(); no exception crosses this boundary;
 *   - geometry outside the tile is not an error: pixels outside the drawable
 *     box are silently dropped (src/draw/tile_pixels.rs:107-111,191-195);
 *   - pixel coordinates are tile-relative, already multiplied by `scale`,
 *     y down; W = H = 256*scale (src/tile.rs:6, src/draw/tile_pixels.rs:57-66).
 */
#ifndef OSMTILE_H
#define OSMTILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSMT_TILE_SIZE 256u /* src/tile.rs:6  TILE_SIZE */
#define OSMT_MAX_ZOOM 18u   /* src/tile.rs:5  MAX_ZOOM  */
#define OSMT_MAX_SCALE 4u
#define OSMT_MAX_DASHES 16u /* dash-pattern entries per op (stylesheets use <= 6) */
/* Fill groups of ONE scene: a group is the 16 coverage words (64 bytes) of one (fill op, 32x16-pixel sub-tile of the op's
 * window).  A list entry holds a group's place in the fill arena as a 32-bit word index, so a scene whose fills need 2^28
 * groups or more (a 16 GiB fill arena) is refused with OSMT_UNSUPPORTED by every upload, build and host-buffer call, with
 * the exact figure in osmt_last_error(): split the batch.  A tile-covering fill is 128 * scale^2 groups: 2048 at scale 4,
 * where 131 072 such ops in one batch reach the limit. */
#define OSMT_MAX_FILL_GROUPS (1ull << 28)

typedef enum osmt_status {
    OSMT_OK = 0,
    OSMT_INVALID_ARG = -1,
    OSMT_OOM = -2,
    OSMT_HIP_ERROR = -3,
    OSMT_UNSUPPORTED = -4,
    OSMT_NO_DEVICE = -5,
    OSMT_RCCL_ERROR = -6 /* the RCCL library could not be loaded, or a collective failed */
} osmt_status;

/* One draw_one_area() call of the reference == one op == one "generation"
 * (src/draw/drawer.rs:156-219, bump_generation at :218).  Casing is a STROKE
 * op with opacity 1.0 emitted at the casing-pass position (drawer.rs:186-201). */
typedef enum osmt_op_kind {
    OSMT_OP_NONE = 0,       /* draws nothing (generation bump only)            */
    OSMT_OP_FILL_COLOR = 1, /* fill_contour(.., Filler::Color, opacity)  fill.rs:16 */
    OSMT_OP_FILL_IMAGE = 2, /* fill_contour(.., Filler::Image, _)        fill.rs:36-40 */
    OSMT_OP_STROKE = 3      /* draw_lines(..)                            line.rs:9-61 */
} osmt_op_kind;

/* Option<LineCap>  (src/mapcss/styler.rs:11-16) */
typedef enum osmt_line_cap {
    OSMT_CAP_NONE = 0,
    OSMT_CAP_BUTT = 1,
    OSMT_CAP_ROUND = 2,
    OSMT_CAP_SQUARE = 3
} osmt_line_cap;

typedef enum osmt_coord_kind {
    OSMT_COORD_LATLON_F64 = 0, /* (lat, lon) degrees; projected on the GPU (tile.rs:88-106, point.rs:11-19) */
    OSMT_COORD_POINT_I32 = 1,  /* already-projected draw::point::Point {x, y} (point.rs:5-8) */
    OSMT_COORD_NODE_REF = 2    /* indices into a shared node table of (lat, lon) — the layout of the reference's
                                * geodata file, where ways hold node REFERENCES and neighbouring tiles share nodes
                                * (reader.rs:291-336, saver.rs:54-109); SURVEY.md 8(f) N2: removes the 16 B/point stream */
} osmt_coord_kind;

/* 64-byte op header. */
typedef struct osmt_op {
    uint8_t kind;                /* osmt_op_kind                                              */
    uint8_t cap;                 /* osmt_line_cap (STROKE)                       line.rs:15   */
    uint8_t use_caps_for_dashes; /* Styler::use_caps_for_dashes (STROKE)         line.rs:16   */
    uint8_t has_dashes;          /* 1 = Some(dashes), 0 = None (STROKE)          line.rs:14   */
    uint8_t color[3];            /* mapcss::color::Color {r,g,b}                 color.rs:2-6 */
    uint8_t _pad0;
    double opacity;              /* fill_opacity / opacity (1.0 when the style has none; drawer.rs:169) */
    double width;                /* STROKE: line width, already * scale          drawer.rs:191,206 */
    uint32_t n_dashes;           /* entries in the dash pattern (<= OSMT_MAX_DASHES)          */
    uint32_t dashes_off;         /* first entry in osmt_batch.dashes (already * scale; drawer.rs:171-172) */
    uint32_t n_rings;            /* Way: 1; Multipolygon: polygon_count()        point_pairs.rs:36-40 */
    uint32_t ring_off;           /* first entry in osmt_batch.rings                           */
    uint32_t image_id;           /* FILL_IMAGE: id from osmt_register_image                   */
    uint32_t _reserved[5];
} osmt_op;

/* One ring = consecutive nodes of a Way / Polygon; edges are (P[i-1], P[i]),
 * i = 1..n_pts-1 (point_pairs.rs:11-22).  A multipolygon's rings share ONE
 * running edge index (fill.rs:19). */
typedef struct osmt_ring {
    uint32_t first_pt; /* index into osmt_batch.latlon / .points */
    uint32_t n_pts;
} osmt_ring;

/* One tile == one Drawer::draw_to_pixels() call (drawer.rs:60-131), minus labels. */
typedef struct osmt_tile_job {
    uint32_t x, y;         /* tile::Tile {x, y}        tile.rs:9-13 */
    uint8_t zoom;          /* tile::Tile {zoom}                      */
    uint8_t has_canvas;    /* 0: canvas = opaque black (tile_pixels.rs:231-236) */
    uint8_t canvas_rgb[3]; /* Styler::canvas_fill_color (tile_pixels.rs:89-93)  */
    uint8_t _pad[3];
    uint32_t n_ops;  /* ops of this tile, in draw (= generation) order  */
    uint32_t op_off; /* first op in osmt_batch.ops                      */
    uint32_t n_pts;  /* the tile's points are one contiguous pool range */
    uint32_t pt_off;
} osmt_tile_job;

/* A batch of tiles sharing flat pools (display list).  All indices absolute. */
typedef struct osmt_batch {
    const osmt_tile_job* jobs;
    size_t n_jobs;
    const osmt_op* ops;
    size_t n_ops;
    const osmt_ring* rings;
    size_t n_rings;
    uint32_t coord_kind;  /* osmt_coord_kind: which of the two pools below is used */
    uint32_t scale;       /* integer scale: 1 or 2 (.. OSMT_MAX_SCALE); http_server.rs:250-258 */
    const double* latlon; /* [n_pts][2] = (lat, lon) degrees   (coords.rs:1-14) */
    const int32_t* points; /* [n_pts][2] = (x, y)               (point.rs:5-8)   */
    size_t n_pts;
    const double* dashes; /* dash pool, already * scale */
    size_t n_dashes;
    /* OSMT_COORD_NODE_REF only: point i of the pools above is nodes[node_refs[i]] */
    const double* nodes;       /* [n_nodes][2] = (lat, lon) degrees, uploaded once per scene */
    size_t n_nodes;
    const uint32_t* node_refs; /* [n_pts] */
} osmt_batch;

/* ---- label pass ---------------------------------------- */
/* One Labeler::label_entity call (labeler.rs:16-38): an optional icon blit
 * (labeler.rs:91-106) followed by an optional text (TextPlacer::place,
 * font/text_placer.rs:24-160).  The text arrives as the Rasterizer::draw_line
 * calls the reference's glyph walk makes (font/rasterizer.rs:27-88; draw_quad,
 * :90-113, flattens curves into draw_line calls on the host, so libm's hypot
 * stays where the reference calls it), in call order: the GPU replays them
 * into the exact-area accumulators and runs save_to_figure (:115-147),
 * set_label_pixel / bump_label_generation (tile_pixels.rs:131-162) and the
 * final blend_unfinished_pixels(true) (:154-158, 205-223).  40 bytes. */
typedef struct osmt_label {
    uint8_t has_icon;      /* style.icon_image found in the IconCache AND get_label_position is Some (labeler.rs:48-66) */
    uint8_t has_text;      /* place() reached save_to_figure (text_placer.rs:159); 0 = place() returned true early / no text_style */
    uint8_t text_color[3]; /* Rasterizer::color (text_placer.rs:50-54) */
    uint8_t _pad[3];
    uint32_t image_id;     /* has_icon: id from osmt_register_image */
    uint32_t seg_off;      /* first draw_line call in osmt_label_batch.segs (osmt_glyph_label_batch: first glyph instance) */
    uint32_t n_segs;       /* draw_line calls (osmt_glyph_label_batch: glyph instances) */
    uint32_t _reserved;
    double icon_center_x, icon_center_y; /* get_label_position (labeler.rs:57-60), already scaled */
} osmt_label;

/* Labels of a whole batch; tile i owns labels [job_label_off[i], job_label_off[i+1]) in
 * draw order (drawer.rs:221-262: areas first, then nodes). */
typedef struct osmt_label_batch {
    const osmt_label* labels;
    size_t n_labels;
    const uint32_t* job_label_off; /* [n_jobs + 1] */
    const double* segs;            /* [n_segs][4] = (x0, y0, x1, y1) exactly as passed to Rasterizer::draw_line */
    size_t n_segs;
} osmt_label_batch;

/* ---- label text as glyph runs ------------------------------------------------ */
/* The second, optional form of label text: instead of the draw_line calls of the glyph walk, the caller registers the
 * font's outlines once per context and names, per label, the glyph instances TextPlacer::place would rasterize
 * (font/text_placer.rs:24-160) with the transform it would pass to Glyph::rasterize (:232-259).  The GPU walks the
 * outlines — including Rasterizer::draw_quad's subdivision (font/rasterizer.rs:90-113) with a device hypot equal to the
 * host libm's — and writes exactly the draw_line sequence the host would have produced, in the same order, into the
 * segment arena the label kernels read.  64 bytes per glyph instead of ~32 bytes x hundreds of calls. */

/* stb_truetype's Vertex (10 bytes): one outline command in font units; type 1 = MoveTo, 2 = LineTo, 3 = CurveTo
 * (text_placer.rs:241-256).  (cx, cy) is the control point of a CurveTo. */
typedef struct osmt_glyph_vertex {
    int16_t x, y, cx, cy;
    uint8_t type;
    uint8_t _pad;
} osmt_glyph_vertex;

#define OSMT_GLYPH_MOVE_TO 1u
#define OSMT_GLYPH_LINE_TO 2u
#define OSMT_GLYPH_CURVE_TO 3u

/* osmt_glyph_instance.form: which of TextPlacer::place's two `tr` closures maps outline points to pixels */
#define OSMT_GLYPH_CENTER 0u /* p = {x_offset, baseline}: tr(x, y) = (x_offset + x, baseline - y)   (text_placer.rs:150-153) */
#define OSMT_GLYPH_LINE 1u   /* p = {glyph_center_x, glyph_center_y, angle_sin, angle_cos, way_x, way_y}, with
                              * (angle_sin, angle_cos) = (-way_pos.angle).sin_cos() computed by the caller's libm:
                              * tr = translate by -glyph_center, rotate, back-translate to way_pos  (text_placer.rs:87-101) */

/* One Glyph::rasterize call (64 bytes).  `scale` is f64::from(font.scale_for_pixel_height(size as f32)); the GPU applies
 * `convert` (f64::from(v) * scale) itself.  Unused entries of p are ignored (CENTER reads p[0], p[1]). */
typedef struct osmt_glyph_instance {
    uint32_t glyph_id; /* id from osmt_register_glyphs */
    uint32_t form;     /* OSMT_GLYPH_CENTER / OSMT_GLYPH_LINE */
    double scale;
    double p[6];
} osmt_glyph_instance;

/* Labels of a batch with glyph-run text.  The osmt_label records are the same as in osmt_label_batch — icons, has_text
 * and colours mean what they mean there — except that seg_off / n_segs name a range of GLYPH INSTANCES of `glyphs`
 * (in rasterize order), not of draw_line calls. */
typedef struct osmt_glyph_label_batch {
    const osmt_label* labels;
    size_t n_labels;
    const uint32_t* job_label_off; /* [n_jobs + 1] */
    const osmt_glyph_instance* glyphs;
    size_t n_glyphs;
} osmt_glyph_label_batch;

/* ---- label text as text runs ---------------------------------------------------- */
/* The third, optional form of label text: the caller says WHAT the text is (glyph ids and the font's metrics) and WHERE
 * it goes (an anchor, or the way's points); the GPU runs TextPlacer::place (font/text_placer.rs:24-168) — the width
 * sums, the row breaking of centred text, the walk along a way — and feeds the glyph instances it produces, without
 * leaving the device, to the expansion of osmt_scene_set_glyph_labels.  What stays with the caller is the font lookup
 * (cmap, hmtx, kern) and libm: atan2 and sin_cos are not reproducible bit for bit on the device, so the caller hands in
 * (-get_angle(points, e)).sin_cos() per edge, as OSMT_GLYPH_LINE already requires per glyph.  16 bytes per glyph + 64 per
 * label + 24 per way point instead of 64 bytes per glyph. */

/* one char of text_to_glyphs (text_placer.rs:170-197); 16 bytes */
typedef struct osmt_text_glyph {
    uint32_t glyph_id; /* id from osmt_register_glyphs */
    int32_t advance;   /* get_glyph_h_metrics(g).advance_width, font units */
    int32_t kern;      /* get_glyph_kern_advance(prev, g); ignored for the first glyph of a text */
    uint32_t flags;    /* bit 0: ch.is_whitespace() */
} osmt_text_glyph;

#define OSMT_TEXT_CENTER 0u /* TextPosition::Center: rows around (center_x, center_y)  (text_placer.rs:112-163) */
#define OSMT_TEXT_LINE 1u   /* TextPosition::Line: along way_pts[pt_off .. pt_off + n_pts)  (text_placer.rs:60-111) */

/* One TextPlacer::place call; 64 bytes, one per label, read only when the label has_text.
 * LINE: way_pts holds get_waypoints ALREADY in walking order — the caller applies the reversal of text_placer.rs:65-67
 * (points[0].x > last.x) before it fills way_pts and way_sincos, because the angles depend on it.  A LINE run with
 * n_pts < 2 and a text wider than its way are legal and place nothing (place() returns early). */
typedef struct osmt_text_run {
    uint32_t position; /* OSMT_TEXT_CENTER / OSMT_TEXT_LINE */
    uint32_t y_offset; /* CENTER: what label_with_icon returned (icon.height / 2, or 0) */
    uint32_t pt_off, n_pts; /* LINE: range in way_pts / way_sincos */
    double scale;      /* f64::from(font.scale_for_pixel_height(font_size as f32)) */
    int32_t ascent, descent, line_gap, _pad; /* font.get_v_metrics(), font units */
    double center_x, center_y; /* CENTER: get_label_position */
    double _reserved;
} osmt_text_run;

/* Labels of a batch with text-run text.  The osmt_label records are the same as in osmt_label_batch, except that
 * seg_off / n_segs name a range of `glyphs` (the chars of the text, in order). */
typedef struct osmt_text_label_batch {
    const osmt_label* labels;
    size_t n_labels;
    const uint32_t* job_label_off; /* [n_jobs + 1] */
    const osmt_text_run* runs;     /* [n_labels] */
    const osmt_text_glyph* glyphs;
    size_t n_glyphs;
    const int32_t* way_pts;   /* [n_way_pts][2]: Point (x, y) of get_waypoints, in walking order */
    const double* way_sincos; /* [n_way_pts][2]: entry pt_off + e = (-get_angle(points, e)).sin_cos() of edge e -> e + 1;
                               * the last entry of a label's range is unused */
    size_t n_way_pts;
} osmt_text_label_batch;

/* osmt_glyph_instance.form of a glyph whose text place() returned from before rasterizing (wider than its way, fewer
 * than two way points): expands to no draw_line call.  Only ever seen through osmt_scene_read_glyph_instances; not a
 * form osmt_scene_set_glyph_labels accepts. */
#define OSMT_GLYPH_NONE 2u

/* ---- label text as strings ------------------------------------------------------ */
/* The fourth, optional form of label text: the caller registers a font's lookup tables once per context
 * (osmt_register_font) and gives a label as its code points and a font size; the GPU runs TextPlacer::text_to_glyphs
 * (font/text_placer.rs:170-197) — find_glyph_index, get_glyph_h_metrics, get_glyph_kern_advance, the "no kern for the
 * first glyph" rule, ch.is_whitespace() — and writes the osmt_text_glyph records the text-run form uploads (k_text_shape),
 * in front of k_text_place on the same stream.  What stays with the caller is parsing the TrueType file, once per font,
 * and libm (way_sincos), as in the text-run form.  4 bytes per char + 64 per label + 24 per way point.
 * Only the scene entries below and osmt_render_batch_rgb_strings take string labels; the PNG, worker and multi-GPU
 * entries take osmt_label_batch only, as they do for glyph and text runs. */

/* The flat tables of one font, read out of the file once by the caller (stb_truetype names in INTEGRATION.md 2b).
 * Borrowed for the call; the library keeps copies. */
typedef struct osmt_cmap_entry {
    uint32_t code_point, glyph;
} osmt_cmap_entry;

typedef struct osmt_kern_pair {
    uint32_t left, right; /* glyph indices */
    int32_t value;        /* get_glyph_kern_advance(left, right), font units */
} osmt_kern_pair;

typedef struct osmt_font_desc {
    const osmt_cmap_entry* cmap; /* [n_cmap], strictly increasing in code point, glyph < n_glyphs; a code point that is
                                  * not listed is glyph 0 (find_glyph_index) */
    size_t n_cmap;
    const int32_t* advance;      /* [n_glyphs]: get_glyph_h_metrics(g).advance_width, |v| <= 65535 */
    const uint32_t* outline_id;  /* [n_glyphs]: id from osmt_register_glyphs of glyph g's outline (no shape: an empty outline) */
    size_t n_glyphs;             /* >= 1: glyph 0 is what a missing code point shapes to */
    const osmt_kern_pair* kern;  /* [n_kern], strictly increasing in (left, right), left and right < n_glyphs, |value| <=
                                  * 65535; a pair that is not listed is 0 (get_glyph_kern_advance) */
    size_t n_kern;               /* 0 is legal (kern may be NULL then) */
    int32_t ascent, descent, line_gap; /* get_v_metrics(), font units; ascent - descent != 0 */
    int32_t _pad;
} osmt_font_desc;

/* One TextPlacer::place call of a string label; 64 bytes, one per label, read only when the label has_text: osmt_text_run
 * without what the font knows.  The library computes scale = (double)((float)font_size / (float)(ascent - descent)) =
 * f64::from(font.scale_for_pixel_height(font_size as f32)). */
typedef struct osmt_string_run {
    uint32_t position; /* OSMT_TEXT_CENTER / OSMT_TEXT_LINE */
    uint32_t y_offset; /* CENTER: what label_with_icon returned (icon.height / 2, or 0) */
    uint32_t pt_off, n_pts; /* LINE: range in way_pts / way_sincos */
    uint32_t font_id;  /* id from osmt_register_font */
    uint32_t _pad;
    double font_size;  /* text_style.font_size * global_scale: the value place() casts to f32 */
    double center_x, center_y; /* CENTER: get_label_position */
    double _reserved[2];
} osmt_string_run;

/* Labels of a batch with string text.  The osmt_label records are the same as in osmt_label_batch, except that seg_off /
 * n_segs name a range of `chars` (the code points of the text, in text order). */
typedef struct osmt_string_label_batch {
    const osmt_label* labels;
    size_t n_labels;
    const uint32_t* job_label_off; /* [n_jobs + 1] */
    const osmt_string_run* runs;   /* [n_labels] */
    const uint32_t* chars;         /* Unicode scalar values (Rust `char`): <= 0x10FFFF and no surrogate */
    size_t n_chars;
    const int32_t* way_pts;   /* as in osmt_text_label_batch */
    const double* way_sincos; /* as in osmt_text_label_batch */
    size_t n_way_pts;
} osmt_string_label_batch;

typedef struct osmt_config {
    int32_t device; /* HIP device ordinal */
    uint32_t flags; /* reserved, 0 */
} osmt_config;

typedef struct osmt_ctx osmt_ctx;     /* one per GPU; analogue of Drawer + worker pool state */
typedef struct osmt_scene osmt_scene; /* a batch resident in HBM + its workspace              */

/* ---- lifecycle --------------------------------------------------------- */
/* Drawer::new (drawer.rs:33-38) + per-worker TilePixels::new (tile_pixels.rs:57-87). */
int osmt_create(const osmt_config* cfg, osmt_ctx** out_ctx);
/* Scenes hold a reference on their context: destroying a context that still has scenes only drops the handle; its
 * device buffers, streams and icon registry go with the last osmt_scene_free (no use-after-free in either order). */
void osmt_destroy(osmt_ctx* ctx);
/* anyhow::Error text (http_server.rs:127-132 prints it); thread-local, never NULL. */
const char* osmt_last_error(void);
/* Library / ABI version: (major << 16) | minor. */
uint32_t osmt_version(void);

/* ---- icons for Filler::Image ------------------------------------------- */
/* Icon::load result (icon.rs:14-58): straight-alpha RGBA8 pixels, row-major;
 * stored premultiplied exactly as RgbaColor::from_components (tile_pixels.rs:21-23). */
int osmt_register_image(osmt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t* out_image_id);

/* ---- display-list validation (host only, no device needed) ----------------- */
/* The checks every upload runs first; what the reference's type system and borrow checker guarantee for
 * Drawer::draw_to_pixels' arguments (drawer.rs:60-67) has to be verified at a C boundary.  OSMT_OK, or
 * OSMT_INVALID_ARG / OSMT_UNSUPPORTED with the reason in osmt_last_error():
 *   - indices in range; the jobs' op ranges PARTITION the op pool (every op belongs to exactly one job — the per-op
 *     pre-pass runs over the whole pool) and their point ranges do not overlap (a point is projected against the
 *     tile of the job that owns it);
 *   - zoom <= OSMT_MAX_ZOOM, scale in 1..OSMT_MAX_SCALE, opacity in [0, 2^52], finite widths, known caps, dash lists
 *     non-empty (Some([]) panics in the reference, opacity_calculator.rs:109) and <= OSMT_MAX_DASHES;
 *   - coordinates the integer walks can hold: |x|, |y| <= 2^28 for OSMT_COORD_POINT_I32; finite (lat, lon) inside the
 *     Web-Mercator square (|lat| <= 85.06, |lon| <= 180) otherwise — beyond it Point::from_node saturates
 *     (point.rs:11-19) and the reference itself draws garbage. */
int osmt_validate_batch(const osmt_batch* batch);

/* ---- whole path, host buffers (Drawer::draw_to_pixels, drawer.rs:60-131) -- */
/* out_rgba: n_jobs tiles of (256*scale)^2 RGBA8 pixels (A = 255), tile i at
 * out_rgba + i*out_tile_stride_bytes, rows tightly packed
 * (TileRenderedPixels, drawer.rs:27-30; to_rgb_triples, tile_pixels.rs:164-181). */
int osmt_render_batch(osmt_ctx* ctx, const osmt_batch* batch, uint8_t* out_rgba, size_t out_tile_stride_bytes);

/* The same with the reference's own output format: packed RGB8, 3 bytes per pixel, tile i at out_rgb +
 * i*out_tile_stride_bytes (>= W*H*3) — byte for byte the memory of TileRenderedPixels.triples: Vec<(u8, u8, u8)>
 * (drawer.rs:27-30, tile_pixels.rs:46,164-181), so a Rust caller takes the buffer as it is.  The alpha byte is dropped on
 * the device: a quarter less PCIe traffic than osmt_render_batch.  `labels` may be NULL. */
int osmt_render_batch_rgb(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgb,
                          size_t out_tile_stride_bytes);

/* The same followed by the label pass (drawer.rs:107-125) when `labels` is not NULL. */
int osmt_render_batch_labels(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_rgba,
                             size_t out_tile_stride_bytes);

/* Pinned host memory for out_rgba: with it (or any hipHostMalloc'ed / hipHostRegister'ed buffer) and a batch of
 * >= 256 tiles, osmt_render_batch[_labels] overlaps the kernels of one 128-tile chunk with the device-to-host
 * copy of the previous one on a second stream (the per-GPU pipeline of SURVEY.md 8(e)); pageable buffers
 * take one blocking copy at the end.  Analogue of the reference's per-worker output Vec (drawer.rs:27-30). */
int osmt_host_alloc(osmt_ctx* ctx, size_t bytes, void** out_ptr);
void osmt_host_free(osmt_ctx* ctx, void* ptr);

/* ---- whole path, HBM-resident (the fast path) --------------------------- */
int osmt_scene_upload(osmt_ctx* ctx, const osmt_batch* batch, osmt_scene** out_scene);
void osmt_scene_free(osmt_scene* scene);
/* d_out_rgba: DEVICE pointer, same layout as osmt_render_batch's out_rgba.
 * stream: hipStream_t (NULL = default stream).  Asynchronous w.r.t. the host. */
int osmt_render_scene(osmt_ctx* ctx, osmt_scene* scene, void* d_out_rgba, size_t out_tile_stride_bytes, void* stream);
/* Same, but returns the un-quantised canvas: d_out_f64 = [n_jobs][H][W][4]
 * premultiplied f64 RGBA == TilePixels::pixels of the centre tile after
 * blend_unfinished_pixels(false) (tile_pixels.rs:154-158) — what the label pass
 * of the reference would continue from. */
int osmt_render_scene_f64(osmt_ctx* ctx, osmt_scene* scene, void* d_out_f64, void* stream);
/* Individual stages of osmt_render_scene (for profiling/tests): 1 = project
 * (Point::from_node), 2 = per-op extents + traveled distances, 4 = raster. */
int osmt_render_scene_stages(osmt_ctx* ctx, osmt_scene* scene, uint32_t stage_mask, void* d_out_rgba,
                             size_t out_tile_stride_bytes, void* stream);
/* Attaches the label pass of every tile of the scene (Drawer::draw_labels,
 * drawer.rs:107-125,221-262); osmt_render_scene then returns the pixels after
 * blend_unfinished_pixels(true).  NULL / n_labels == 0 detaches.  Coordinates must
 * be finite and |v| <= 2^20.  A text whose coverage window — its rows inside the label box [-W, 2W), times the
 * columns its draw_line calls span — has more than 2^24 cells is refused with OSMT_UNSUPPORTED ("coverage window of
 * C x R cells is too large"), and so is a batch whose windows add up to more than 2^31 cells: nothing is attached.
 * osmt_render_scene_f64 keeps returning the canvas BEFORE labels. */
int osmt_scene_set_labels(osmt_ctx* ctx, osmt_scene* scene, const osmt_label_batch* labels);
/* Label statuses of the last osmt_render_scene (label_generation_statuses,
 * tile_pixels.rs:160-162): ok[i] = 1 if label i succeeded.  Synchronises the stream.  Before the first render after
 * osmt_scene_set_labels every status is 0 (nothing has been placed yet). */
int osmt_scene_read_label_status(osmt_ctx* ctx, osmt_scene* scene, uint8_t* ok);
/* Waits for the launches that read the scene (not for the device) and reports what they could not report themselves:
 * osmt_render_scene is asynchronous, so a kernel-side internal error — a pre-pass arena that does not fit, which the
 * sizing at upload rules out — would otherwise show as blank tiles.  OSMT_OK, or OSMT_HIP_ERROR with the detail in
 * osmt_last_error().  The host-buffer calls (osmt_render_batch*) make the same check before they return.  (No analogue in
 * the reference: its canvas is written synchronously by the calling thread, src/draw/drawer.rs:60-131.) */
int osmt_scene_check(osmt_ctx* ctx, osmt_scene* scene);
/* Copies the projected integer points of the scene back: xy = [n_pts][2]. */
int osmt_scene_read_points(osmt_ctx* ctx, osmt_scene* scene, int32_t* xy);

/* ---- label text as glyph runs (see osmt_glyph_label_batch) ------------------------------------ */
/* Appends n_glyphs outlines to the context's glyph table; glyph i is v[vertex_off[i] .. vertex_off[i + 1]) (vertex_off:
 * n_glyphs + 1 non-decreasing entries, vertex_off[0] == 0) and gets id *out_first_id + i.  An empty outline is legal (a
 * glyph with `shape: None`, the space).  Vertex types must be 1..3.  The table is append-only with the snapshot
 * semantics of osmt_register_image: a render that holds an older snapshot never reads freed memory. */
int osmt_register_glyphs(osmt_ctx* ctx, const osmt_glyph_vertex* v, const uint32_t* vertex_off, uint32_t n_glyphs,
                         uint32_t* out_first_id);
/* osmt_scene_set_labels with glyph-run text: the glyph instances are expanded on the GPU into the draw_line calls of
 * the glyph walk (a count pass, one read-back of ~20 bytes per label, an emit pass); the label kernels then run exactly
 * as with osmt_scene_set_labels on those calls.  NULL / n_labels == 0 detaches.  Errors, never silent:
 *   - OSMT_INVALID_ARG: NULL pools, glyph ids outside the table, an instance range out of bounds, an unknown form, a
 *     scale or used parameter that is not finite;
 *   - OSMT_UNSUPPORTED: a produced draw_line coordinate that is not finite or has |v| > 2^20 (as osmt_scene_set_labels),
 *     or a curve whose subdivision is deeper than the device walk's cap (62 levels; never a truncated outline). */
int osmt_scene_set_glyph_labels(osmt_ctx* ctx, osmt_scene* scene, const osmt_glyph_label_batch* labels);
/* osmt_render_batch_rgb with glyph-run labels: scene, osmt_scene_set_glyph_labels, render, packed RGB8 out. */
int osmt_render_batch_rgb_glyphs(osmt_ctx* ctx, const osmt_batch* batch, const osmt_glyph_label_batch* labels, uint8_t* out_rgb,
                                 size_t out_tile_stride_bytes);
/* Inspection: the scene's draw_line arena as the label kernels read it, out = [n][4] (x0, y0, x1, y1).  For glyph-run
 * labels it is in label order (label, glyph, vertex, subdivision); for segment labels it is the caller's segs.  *n is
 * always set; out may be NULL to ask for the size; cap (in calls) < *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_scene_read_label_segs(osmt_ctx* ctx, osmt_scene* scene, double* out, size_t cap, size_t* n);
/* Inspection: the coverage plane of label `label` of the attached label batch (any of the three forms) as the last
 * render's label stage left it: window = { ry0, ry1, cx0, cols } as sized at upload, out = [ry1 - ry0 + 1][cols] with
 * out[r][c] = the f64 total of cell (cx0 + c, ry0 + r) — min(a + s_acc, 1.0) of save_to_figure
 * (font/rasterizer.rs:121-143), 0 where the stripe has no key; k_raster blends it, total > 0 is the pixel set the
 * collision test sees.  Synchronises the stream.  A label without a window (no text, no draw_line call, or no stripe
 * inside the label area's rows) reports window = { 1, 0, 0, 0 } and *n = 0: not an error.  *n (in cells) is set
 * whenever the label has a window; out may be NULL to ask for the size; cap (in cells) < *n with a non-NULL out is
 * OSMT_INVALID_ARG, and so is a label index beyond the batch.  The planes are written by a render: between
 * osmt_scene_set_*labels and the next osmt_render_scene the call fails with OSMT_INVALID_ARG rather than hand back
 * memory nobody has written. */
int osmt_scene_read_label_cover(osmt_ctx* ctx, osmt_scene* scene, uint32_t label, int32_t window[4], double* out, size_t cap,
                                size_t* n);

/* ---- label text as text runs (see osmt_text_label_batch) ---------------------------------------- */
/* The checks osmt_scene_set_text_labels runs first, without a device.  OSMT_OK, or with the reason in osmt_last_error():
 *   - OSMT_INVALID_ARG: NULL pools; job_label_off not running from 0 to n_labels monotonically; a glyph or way-point
 *     range outside its table; glyph ranges of two labels that overlap (a slot has one owner: one wave writes a
 *     label's slots); an unknown position; a scale, centre or used way_sincos entry that is not finite; |advance| or
 *     |kern| > 65535; y_offset > 2^20; |center| > 2^20;
 *   - OSMT_UNSUPPORTED: a way point with |v| > 2^28 (the i32 differences of Point::dist must not overflow).
 * Only labels with has_text are looked at; n_segs == 0 and a LINE run with n_pts < 2 are legal and place nothing. */
int osmt_validate_text_labels(const osmt_text_label_batch* labels, size_t n_jobs);
/* osmt_scene_set_labels with text-run text: TextPlacer::place runs on the device (k_text_place, one wave per label)
 * and writes one osmt_glyph_instance per glyph — slot seg_off + k is glyph k of the label — which the count / emit
 * passes of osmt_scene_set_glyph_labels expand on the same stream; the label kernels run unchanged behind them.  NULL /
 * n_labels == 0 detaches.  Errors: those of osmt_validate_text_labels, OSMT_INVALID_ARG for a glyph id outside the
 * table, and everything osmt_scene_set_glyph_labels reports downstream (a produced draw_line coordinate that is not
 * finite or beyond 2^20 is OSMT_UNSUPPORTED). */
int osmt_scene_set_text_labels(osmt_ctx* ctx, osmt_scene* scene, const osmt_text_label_batch* labels);
/* osmt_render_batch_rgb with text-run labels: scene, osmt_scene_set_text_labels, render, packed RGB8 out. */
int osmt_render_batch_rgb_text(osmt_ctx* ctx, const osmt_batch* batch, const osmt_text_label_batch* labels, uint8_t* out_rgb,
                               size_t out_tile_stride_bytes);
/* Inspection: the glyph instances the last osmt_scene_set_text_labels placed, out = [n] in slot order (n = the batch's
 * n_glyphs).  CENTER instances carry p[0..1], LINE instances p[0..5], skipped texts OSMT_GLYPH_NONE; unused entries of p
 * and slots no has_text label names read as zero.  With any other label form attached *n is 0.  *n is always set; out
 * may be NULL to ask for the size; cap < *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_scene_read_glyph_instances(osmt_ctx* ctx, osmt_scene* scene, osmt_glyph_instance* out, size_t cap, size_t* n);

/* ---- label text as strings (see osmt_string_label_batch) ---------------------------------------- */
/* Appends one font to the context's font table and returns its id.  Append-only with the snapshot semantics of
 * osmt_register_image / osmt_register_glyphs: a render that holds an older snapshot never reads freed memory, and a font
 * registered after a scene was set does not disturb that scene.  OSMT_INVALID_ARG, with the offender named in
 * osmt_last_error(): NULL tables (kern may be NULL when n_kern == 0; cmap when n_cmap == 0) or n_glyphs == 0; cmap or
 * kern not strictly increasing; a glyph index >= n_glyphs in cmap or kern; |advance| or |kern value| > 65535; an
 * outline_id that is not in the glyph table (register the outlines first); a code point > 0x10FFFF or in 0xD800-0xDFFF;
 * ascent - descent == 0. */
int osmt_register_font(osmt_ctx* ctx, const osmt_font_desc* font, uint32_t* out_font_id);
/* The checks osmt_scene_set_string_labels runs first, without a device (`ctx` is only asked for its fonts): everything
 * osmt_validate_text_labels checks — the char ranges in the place of the glyph ranges — plus, as OSMT_INVALID_ARG, an
 * unknown font_id, a code point that is not a Rust `char` (> 0x10FFFF, or a surrogate) and a font_size that is not finite
 * or whose scale is not.  A valid code point the font does not have is NOT an error: it shapes to glyph 0 with glyph 0's
 * advance and outline, as the reference does. */
int osmt_validate_string_labels(const osmt_string_label_batch* labels, size_t n_jobs, osmt_ctx* ctx);
/* osmt_scene_set_text_labels with string text: k_text_shape (one lane per char) writes the osmt_text_glyph records,
 * k_text_place and the count / emit passes run behind it on the same stream, unchanged.  NULL / n_labels == 0 detaches.
 * Errors: those of osmt_validate_string_labels and everything osmt_scene_set_text_labels reports downstream. */
int osmt_scene_set_string_labels(osmt_ctx* ctx, osmt_scene* scene, const osmt_string_label_batch* labels);
/* osmt_render_batch_rgb with string labels: scene, osmt_scene_set_string_labels, render, packed RGB8 out. */
int osmt_render_batch_rgb_strings(osmt_ctx* ctx, const osmt_batch* batch, const osmt_string_label_batch* labels, uint8_t* out_rgb,
                                  size_t out_tile_stride_bytes);
/* Inspection: the records the last osmt_scene_set_string_labels shaped, out = [n] in slot order (n = the batch's
 * n_chars; slot seg_off + k is char k of its label): exactly what a text-run caller would have uploaded — glyph_id is
 * the OUTLINE id, kern of a label's first char is 0.  Slots no has_text label names read as zero.  Kept with the scene
 * like the glyph instances (which osmt_scene_read_glyph_instances returns after a string set call as after a text one),
 * gone with the next set call; with any other label form attached *n is 0.  *n is always set; out may be NULL to ask for
 * the size; cap < *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_scene_read_text_glyphs(osmt_ctx* ctx, osmt_scene* scene, osmt_text_glyph* out, size_t cap, size_t* n);
/* Diagnostics: out[i] = the device hypot of (xy[2i], xy[2i + 1]) — the function the glyph walk flattens curves with. */
int osmt_debug_hypot(osmt_ctx* ctx, const double* xy, size_t n, double* out);

/* ---- label anchors: where a polygon's label goes (src/draw/labelable.rs:191-204) ------------------------------ */
/* Labelable::get_label_position of a Way or Multipolygon — the start of every icon (labeler.rs:56) and every centred
 * text (text_placer.rs:113) — for a whole batch of polygons per call: the largest ring is chosen, rings not inside it
 * are dropped (filter_polygons, :206-232) and the "polylabel" search (:125-189) runs on the device, one wave per request,
 * step for step as the reference runs it (pop order with std's BinaryHeap tie order, stop rule, first cell of the best
 * fitness).  x and y have the bits the reference returns.
 *
 * A request is n_rings consecutive osmt_ring entries (a way: one ring; a multipolygon: polygon_count() rings in file
 * order) over one pool of double[n_pts][2].  Points are what nodes_to_points produces (:61-68):
 * coords_to_xy_tile_relative(node, tile) * scale, UNROUNDED f64.  The host projects: the device projection's tan / log are
 * only exact behind Point::from_node's rounding to i32, and a last-bit difference here can flip a branch of the search —
 * there is no (lat, lon) input form.  Points must be finite with |v| <= 2^28.  (The form that takes no points at all —
 * an entity and a tile per request, projected on the device from Mercator factors the caller registered with its own libm —
 * is osmt_label_positions_tiles below.) */
typedef struct osmt_label_request {
    uint32_t ring_off; /* first entry in osmt_label_request_batch.rings */
    uint32_t n_rings;
    double scale;      /* the `scale` get_label_position receives: precision = max(w, h) / 100.0 * scale */
} osmt_label_request;

typedef struct osmt_label_request_batch {
    const osmt_label_request* requests;
    size_t n_requests;
    const osmt_ring* rings; /* first_pt / n_pts index `points` */
    size_t n_rings;
    const double* points;   /* [n_pts][2] = (x, y) */
    size_t n_pts;
} osmt_label_request_batch;

#define OSMT_LABEL_OK 0u        /* (x, y) is the label position */
#define OSMT_LABEL_NONE 1u      /* the reference returns None: no rings, or the first ring AS GIVEN is empty (labelable.rs:194) */
#define OSMT_LABEL_TOO_LARGE 2u /* the reference's run would hold more than OSMT_LABEL_MAX_CELLS cells in its queue at once, or
                                 * pop more than OSMT_LABEL_MAX_CELLS cells: not computed (x = y = 0).  Exactly then and only
                                 * then; osmt::LabelPositions (host/osmt_labelable.hpp) computes such a request on the host. */
#define OSMT_LABEL_MAX_CELLS 65536u

/* 24 bytes per request.  Never a wrong or truncated position: status says what x and y are. */
typedef struct osmt_label_position {
    double x, y;
    uint32_t status; /* OSMT_LABEL_* */
    uint32_t _pad;
} osmt_label_position;

/* Validates on the host (nothing is uploaded before it passes, `out` is not touched when it fails), uploads, runs the
 * kernels, reads `out` back: n_requests records.  OSMT_INVALID_ARG: NULL pointers, ring or point ranges outside the
 * tables, a scale that is not finite; OSMT_UNSUPPORTED: a coordinate that is not finite or has |v| > 2^28.  Zero
 * requests: OSMT_OK, no device is touched. */
int osmt_label_positions(osmt_ctx* ctx, const osmt_label_request_batch* batch, osmt_label_position* out);
/* The same call in two halves, as osmt_render_batch_png_begin / _end: _begin validates, uploads and queues the kernels
 * and the read-back and returns without waiting; _end waits, copies the records into `out` and frees the job whatever it
 * returns.  The arrays of `batch` must stay valid until _end returns.  A server thread begins the anchors of batch k + 1
 * while the GPU renders batch k. */
typedef struct osmt_label_job osmt_label_job;
int osmt_label_positions_begin(osmt_ctx* ctx, const osmt_label_request_batch* batch, osmt_label_job** out_job);
int osmt_label_positions_end(osmt_label_job* job, osmt_label_position* out);
/* Inspection (tests, tools): what the last completed osmt_label_positions / _end on this context did — stats[0] = its
 * requests, stats[1] = those whose queue outgrew the LDS tier and were run again with a queue in device memory,
 * stats[2] = those answered OSMT_LABEL_TOO_LARGE. */
int osmt_label_positions_stats(osmt_ctx* ctx, uint64_t stats[3]);

/* ---- display lists built on the GPU from registered geodata and styles ------------------ */
/* The third way to a scene: instead of an osmt_batch the caller registers, once per context, the topology of a geodata file
 * (reader.rs:291-336: nodes, ways, polygons, multipolygons) and the Style records of its stylesheet (styler.rs:48-71), and then
 * names per tile the (entity, style) pairs Styler::style_entities pushes — 8 bytes each.  The GPU does what
 * Styler::style_areas (styler.rs:168-203) and the three passes of Drawer::draw_to_pixels (drawer.rs:60-99,133-219) do: it
 * sorts every tile's areas into draw order and writes jobs, ops, rings, node references and dashes where the renderer reads
 * them.  The result is an ordinary scene with coord_kind == OSMT_COORD_NODE_REF: byte for byte the display list
 * osmt::SceneBuilder (host/osmt_styled.hpp) builds on the host.  Only osmt_scene_build_styled starts from a styled batch; the
 * PNG, worker and multi-GPU entries take osmt_batch. */

#define OSMT_STYLED_MAX_TILE_AREAS 65536u /* (entity, style) pairs of one tile */
#define OSMT_STYLED_LDS_AREAS 2048u       /* up to here a tile is sorted in LDS (16-byte keys: 32 KB), beyond in device memory */

/* The flat arrays of one geodata file, as GeodataReader hands them out (osmt::GeodataDesc in host/osmt_geodata.hpp fills
 * one).  Borrowed for the call; the library keeps device copies.  Every *_off array has count + 1 non-decreasing entries, the
 * first 0 and the last the length of the array it indexes. */
typedef struct osmt_geodata_desc {
    const double* nodes; /* [n_nodes][2] = (lat, lon) degrees */
    size_t n_nodes;
    const uint64_t* way_ids;      /* [n_ways] global ids (Way::global_id) */
    const uint32_t* way_node_off; /* [n_ways + 1] into way_nodes */
    size_t n_ways;
    const uint32_t* way_nodes; /* node indices */
    size_t n_way_nodes;
    const uint32_t* polygon_node_off; /* [n_polygons + 1] into polygon_nodes */
    size_t n_polygons;
    const uint32_t* polygon_nodes; /* node indices */
    size_t n_polygon_nodes;
    const uint64_t* multipolygon_ids;         /* [n_multipolygons] global ids */
    const uint32_t* multipolygon_polygon_off; /* [n_multipolygons + 1] into multipolygon_polygons */
    size_t n_multipolygons;
    const uint32_t* multipolygon_polygons; /* polygon indices */
    size_t n_multipolygon_polygons;
} osmt_geodata_desc;

/* mapcss::styler::Style (styler.rs:48-71) as a POD of 96 bytes: an Option is a has_* byte in front of its value, a dash list
 * a range of the pool handed over with the records (UNSCALED, as the stylesheet has them), a line cap an osmt_line_cap.
 * A value whose has_* byte is 0 is ignored, whatever its bits. */
typedef struct osmt_style_rec {
    int64_t layer;
    double z_index;
    double opacity, fill_opacity, width, casing_width;
    uint32_t fill_image; /* id from osmt_register_image */
    uint32_t dashes_off, n_dashes, casing_dashes_off, n_casing_dashes;
    uint8_t has_layer, is_foreground_fill;
    uint8_t has_color, color[3];
    uint8_t has_fill_color, fill_color[3];
    uint8_t has_opacity, has_fill_opacity, has_width, has_dashes, line_cap;
    uint8_t has_casing_color, casing_color[3];
    uint8_t has_casing_width, has_casing_dashes, casing_line_cap, has_fill_image;
    uint8_t has_background_color, background_color[3]; /* carried for completeness: no area op reads it */
    uint8_t _pad;
} osmt_style_rec;

/* One element of what Styler::style_entities returns for the areas of a tile; 8 bytes. */
#define OSMT_STYLED_MULTIPOLYGON 0x80000000u
typedef struct osmt_styled_area {
    uint32_t entity; /* local id in the registered geodata (< 2^31); | OSMT_STYLED_MULTIPOLYGON: a multipolygon, else a way */
    uint32_t style;  /* id from osmt_register_styles */
} osmt_styled_area;

/* One Drawer::draw_to_pixels call, minus labels; 24 bytes. */
typedef struct osmt_styled_tile {
    uint32_t x, y;
    uint8_t zoom;
    uint8_t has_canvas;    /* 0: canvas = opaque black */
    uint8_t canvas_rgb[3]; /* Styler::canvas_fill_color */
    uint8_t _pad[3];
    uint32_t area_off; /* the tile's areas: areas[area_off .. area_off + n_areas), ways in entity order among themselves, */
    uint32_t n_areas;  /* multipolygons too; how the two kinds interleave carries no meaning */
} osmt_styled_tile;

typedef struct osmt_styled_batch {
    const osmt_styled_tile* tiles;
    size_t n_tiles;
    const osmt_styled_area* areas;
    size_t n_areas;
    uint32_t geodata_id; /* id from osmt_register_geodata */
    uint32_t scale;      /* 1 .. OSMT_MAX_SCALE */
    uint32_t use_caps_for_dashes; /* Styler::use_caps_for_dashes: 0 / 1 */
    uint32_t _pad;
} osmt_styled_batch;

/* The checks osmt_register_geodata runs first, without a device.  OSMT_INVALID_ARG with the offender named in
 * osmt_last_error(): a NULL array with a non-zero count; offsets that do not start at 0, decrease, or do not end at the length of
 * the array they index; a node or polygon index out of range; a node that is not finite or lies outside the Web-Mercator
 * square (what osmt_validate_batch refuses of a node table).  OSMT_UNSUPPORTED: more than 2^31 - 1 ways or multipolygons, or
 * node-index arrays that together do not fit 32-bit offsets. */
int osmt_validate_geodata(const osmt_geodata_desc* geodata);
/* Uploads one geodata file's topology and returns its id.  Append-only with the snapshot semantics of osmt_register_image /
 * osmt_register_font: a file's tables get one device allocation that never moves and lives as long as the context, so a scene
 * built from it — whose node table IS the registered one; the scene neither owns nor frees it — is not disturbed by a later
 * registration. */
int osmt_register_geodata(osmt_ctx* ctx, const osmt_geodata_desc* geodata, uint32_t* out_geodata_id);
/* The checks osmt_register_styles runs first, without a device (`ctx` is only asked for its icons): everything that would make
 * an op built from the style one that osmt_validate_batch refuses.  OSMT_INVALID_ARG, naming the style: a NaN z_index; opacity or
 * fill_opacity outside [0, 2^52]; a width or casing_width that is not finite or is not finite after multiplication by
 * OSMT_MAX_SCALE; an unknown line cap; a dash list that is Some([]) or outside the pool; a fill_image that is not
 * registered.  OSMT_UNSUPPORTED: more than OSMT_MAX_DASHES dashes; |width| * OSMT_MAX_SCALE > 65536.  Only values whose has_*
 * byte is set are looked at.  A NULL `ctx` has no icons. */
int osmt_validate_styles(const osmt_style_rec* styles, size_t n, const double* dashes, size_t n_dashes, osmt_ctx* ctx);
/* Appends n styles (and their dash pool) to the context's style table; style i gets id *out_first_style_id + i.  Same
 * snapshot rules as above. */
int osmt_register_styles(osmt_ctx* ctx, const osmt_style_rec* styles, size_t n, const double* dashes, size_t n_dashes,
                         uint32_t* out_first_style_id);
/* The checks osmt_scene_build_styled runs first, without a device, O(n_areas).  OSMT_INVALID_ARG: NULL arrays, an unknown
 * geodata id, a way, multipolygon or style id out of range, zoom > OSMT_MAX_ZOOM, scale outside 1..OSMT_MAX_SCALE, a tile's
 * area range outside the area array or overlapping another tile's.  OSMT_UNSUPPORTED: a tile with more than
 * OSMT_STYLED_MAX_TILE_AREAS areas, or more areas in all than 32-bit element indices hold.  The batch's own shape is checked
 * first, its ids against the context's tables last; a NULL `ctx` has nothing registered. */
int osmt_validate_styled_batch(const osmt_styled_batch* batch, osmt_ctx* ctx);
/* Builds the scene of a styled batch on the device: per tile a sort under the total order of compare_styled_entities +
 * style_areas' merge (layer or 0, is_foreground_fill, z_index, global id, multipolygon before way, input position), a count
 * pass over (tile, pass in Fill / Casing / Stroke, area), one read-back of eight totals, and an emit pass into the scene's
 * own arrays.  Errors: those of osmt_validate_styled_batch; OSMT_UNSUPPORTED when the ops, rings, node references, dashes,
 * 64-edge blocks or virtual stroke segments of the batch do not fit 32-bit indices.  *out_scene is NULL on every error:
 * never a truncated or mis-ordered list. */
int osmt_scene_build_styled(osmt_ctx* ctx, const osmt_styled_batch* batch, osmt_scene** out_scene);
/* Inspection: the device-resident display list of ANY scene, uploaded or built, copied back.  counts = { jobs, ops, rings,
 * node references (0 unless the scene is OSMT_COORD_NODE_REF), dashes } is always set; each output may be NULL (all NULL:
 * ask for the sizes). */
int osmt_scene_read_display_list(osmt_ctx* ctx, osmt_scene* scene, osmt_tile_job* jobs, osmt_op* ops, osmt_ring* rings,
                                 uint32_t* node_refs, double* dashes, size_t counts[5]);
/* Inspection: the most ops of any tile of the scene, as the renderer knows it (a batch of at most 64 tiles runs the list
 * kernel only if this exceeds 128).  Counted on the host for an uploaded scene, by k_styled_tilemax for a built one. */
int osmt_scene_max_tile_ops(osmt_ctx* ctx, osmt_scene* scene, uint32_t* out_max_ops);

/* ---- scenes built from tile coordinates: the tile query and the style lookup on the GPU ------------------------ */
/* The fourth way to a scene.  With the z18 tile index of a registered geodata file (reader.rs:217-229) and a table
 * "entity -> the styles Styler::style_entities pushes for it" registered too, a tile is 16 bytes: (zoom, x, y) and its
 * canvas.  The GPU does GeodataReader::get_entities_in_tile_with_neighbors (reader.rs:60-133) — the z18 tiles of the 3 x 3
 * neighbourhood, their way and multipolygon lists gathered, sorted, made unique, multipolygons without polygons dropped —
 * expands every entity by its bound styles and hands the resulting styled batch to the build of osmt_scene_build_styled:
 * byte for byte the display list that call builds from the batch osmt::styled_areas_of_tile (host/osmt_tilequery.hpp)
 * makes on the host.  The osm_ids filter of the reference is osmt_scene_build_tiles_filtered below. */

/* way (or multipolygon) references gathered for ONE tile before dedup: from the z18 index every z18 reference of the
 * neighbourhood, from a pyramid level (osmt_register_tile_pyramid) at most roughly 9 x its distinct entities */
#define OSMT_QUERY_MAX_TILE_CANDIDATES (1u << 20)
#define OSMT_QUERY_LDS_CANDIDATES 8192u           /* up to here a tile's candidates are sorted in LDS (32 KB of u32) */
#define OSMT_BINDINGS_NONE 0xFFFFFFFFu

/* the z18 tile storage of a geodata file (reader.rs:217-229, saver.rs:167-226), ways and multipolygons only */
typedef struct osmt_tile_index_desc {
    const uint32_t* tile_xy; /* [n_tiles][2] = (x, y) at zoom 18, STRICTLY ascending lexicographically */
    size_t n_tiles;
    const uint32_t* way_off; /* [n_tiles + 1] into ways */
    const uint32_t* ways;    /* local way ids, any order, duplicates allowed */
    size_t n_way_refs;
    const uint32_t* multipolygon_off; /* [n_tiles + 1] into multipolygons */
    const uint32_t* multipolygons;
    size_t n_multipolygon_refs;
} osmt_tile_index_desc;

/* (entity -> style ids) for a range of zooms: what Styler::style_entities pushes for the entity, in push order */
typedef struct osmt_style_bindings_desc {
    uint32_t geodata_id;
    uint8_t zoom_lo, zoom_hi, _pad[2]; /* inclusive */
    const uint32_t* way_style_off;     /* [n_ways + 1] */
    const uint32_t* way_styles;        /* ids from osmt_register_styles */
    size_t n_way_styles;
    const uint32_t* multipolygon_style_off; /* [n_multipolygons + 1] */
    const uint32_t* multipolygon_styles;
    size_t n_multipolygon_styles;
} osmt_style_bindings_desc;

typedef struct osmt_query_tile { /* 16 bytes */
    uint32_t x, y;
    uint8_t zoom, has_canvas, canvas_rgb[3], _pad[3];
} osmt_query_tile;

typedef struct osmt_tile_batch {
    const osmt_query_tile* tiles;
    size_t n_tiles;
    uint32_t geodata_id, scale, use_caps_for_dashes, _pad;
    uint32_t bindings_of_zoom[OSMT_MAX_ZOOM + 1]; /* id from osmt_register_style_bindings, or OSMT_BINDINGS_NONE */
} osmt_tile_batch;

/* The checks osmt_register_tile_index runs first, without a device.  OSMT_INVALID_ARG, naming the offender: a NULL array with a
 * non-zero count; offsets that do not start at 0, decrease or do not end at the pool length; tile_xy not strictly ascending; a
 * coordinate >= 2^18 (with it the reference's u32 wrap at the world's edge is a plain clip: a neighbour column at x = -1 or
 * x = 2^zoom holds no tile); a way or multipolygon id >= n_ways / n_multipolygons. */
int osmt_validate_tile_index(const osmt_tile_index_desc* index, size_t n_ways, size_t n_multipolygons);
/* Uploads the tile index of a registered geodata file: one allocation that never moves and lives as long as the context,
 * together with a column directory (the distinct x and the first tile of each) built here.  One index per geodata id: a second
 * registration is OSMT_INVALID_ARG. */
int osmt_register_tile_index(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tile_index_desc* index);
/* OSMT_INVALID_ARG: an unknown geodata id (a NULL `ctx` has none), zoom_lo > zoom_hi or zoom_hi > OSMT_MAX_ZOOM, bad offsets
 * (as above), a style id that is not registered at the time of the call. */
int osmt_validate_style_bindings(const osmt_style_bindings_desc* b, osmt_ctx* ctx);
/* Appends a bindings table.  Append-only with the snapshot semantics of images, fonts and styles: a table's device copy never
 * moves, a later registration never disturbs a scene that is already built. */
int osmt_register_style_bindings(osmt_ctx* ctx, const osmt_style_bindings_desc* b, uint32_t* out_bindings_id);
/* OSMT_INVALID_ARG: zoom > 18, x or y >= 2^zoom, scale outside 1..OSMT_MAX_SCALE, an unknown geodata id or one without a tile
 * index, a tile whose zoom has OSMT_BINDINGS_NONE, a bindings id that is unknown, belongs to another geodata id or does not
 * cover that zoom.  The same tile may appear any number of times; 0 tiles are a valid batch. */
int osmt_validate_tile_batch(const osmt_tile_batch* batch, osmt_ctx* ctx);
/* Query, style lookup and display-list build on the device (csrc/osmt_tilequery.hip, then the kernels of
 * osmt_scene_build_styled).  OSMT_UNSUPPORTED with the exact figure: a tile that gathers more than
 * OSMT_QUERY_MAX_TILE_CANDIDATES references of one kind, a candidate or area total that does not fit 32 bits, a tile with more
 * than OSMT_STYLED_MAX_TILE_AREAS areas; and whatever osmt_scene_build_styled refuses.  *out_scene is NULL on every error and
 * the context stays usable.  The scene is an ordinary OSMT_COORD_NODE_REF scene. */
int osmt_scene_build_tiles(osmt_ctx* ctx, const osmt_tile_batch* batch, osmt_scene** out_scene);
/* Inspection: the styled batch the device derived for a scene of osmt_scene_build_tiles (tiles[i].area_off / n_areas index
 * `areas`); NULL outputs ask for sizes (*n_areas is always set; the tile count is the scene's).  OSMT_INVALID_ARG for a scene
 * from any other source, or when areas_cap is less than *n_areas. */
int osmt_scene_read_styled_areas(osmt_ctx* ctx, osmt_scene* scene, osmt_styled_tile* tiles, osmt_styled_area* areas,
                                 size_t areas_cap, size_t* n_areas);

/* ---- the tile index pyramid: coarser levels of the z18 index, built on the GPU ---------------------------------- */
/* The geodata file holds the z18 level only, so a tile of zoom z gathers from 9 * 4^(18 - z) index tiles, and an entity is
 * gathered once for every z18 tile of its bounding range inside the neighbourhood.  Level L (0 <= L <= 18, s = 18 - L) of a
 * registered tile index has the tiles (x >> s, y >> s) of ALL its tiles (a tile with empty lists still gives its parent a
 * tile), strictly ascending by (x, y), and per tile and kind the union of the lists of its z18 children, ascending and without
 * repeats.  The kinds are ways, multipolygons and — iff a node index (osmt_register_node_index) is registered for the geodata
 * id at the moment of the call — nodes.  Level 18 is the registered index with every list sorted and made unique.  The
 * registered index itself stays as it is.
 *
 * The rectangle of a tile's neighbourhood has z18 bounds that are multiples of 2^(18 - L) for every L >= zoom, so it covers a
 * z18 tile iff it covers the tile's parent at level L: gathered from level L, the tile's entity SET is the one gathered from
 * z18, and everything behind the dedup sees the same input.  Every tile query of the library (osmt_scene_build_tiles[_filtered],
 * both label builds, the tile server, the worker's tile requests) reads, per tile, the SMALLEST REGISTERED LEVEL >= THE TILE'S
 * ZOOM, and the z18 index where there is none (the node query: the z18 node index unless that level has node lists).  With
 * level z a tile gathers from at most 9 index tiles and names an entity at most 9 times.
 *
 * The limits are judged on what is gathered: OSMT_QUERY_MAX_TILE_CANDIDATES then bounds roughly 9 x the distinct entities of a
 * neighbourhood instead of its z18 references.  A build that was accepted without a pyramid is accepted with one (a level never
 * gathers more than z18 does), and a pyramid moves the refusal of a dense extract several zooms down — not to zoom 0: the
 * distinct entities of a large extract exceed the limit by themselves.
 *
 * The levels are built on the device (csrc/osmt_tilepyramid.hip: an LSD radix sort of (parent tile, id) pairs per kind, each
 * level from the next finer one that is being built, the finest from the registered index).  A level is one allocation that
 * never moves and lives as long as the context; one pyramid per geodata id. */
#define OSMT_PYRAMID_ALL_LEVELS 0x7FFFFu /* bits 0 .. 18 */
/* OSMT_INVALID_ARG, naming the offender: a mask of 0 or with bits above 18 (these need no context); an unknown geodata id (a
 * NULL `ctx` has none), one without a tile index, one that has a pyramid already. */
int osmt_validate_tile_pyramid(uint32_t geodata_id, uint32_t level_mask, osmt_ctx* ctx);
/* Builds the levels of `level_mask` (bit L = level L).  OSMT_UNSUPPORTED with the exact figure and the level: a pair total or a
 * reference total that does not fit 32 bits.  A failed call registers nothing and leaves the context usable. */
int osmt_register_tile_pyramid(osmt_ctx* ctx, uint32_t geodata_id, uint32_t level_mask);
/* Which levels exist (0: no pyramid) and which of them have node lists. */
int osmt_tile_pyramid_levels(osmt_ctx* ctx, uint32_t geodata_id, uint32_t* out_mask, uint32_t* out_node_mask);
/* Inspection: one level copied back.  counts = { tiles, way refs, multipolygon refs, node refs } is always set; each output may
 * be NULL (all NULL: ask for the sizes); caps = the capacities of { tile_xy (in tiles), ways, mps, nodes } (NULL: not checked), an
 * output that is too small is OSMT_INVALID_ARG.  The offset arrays have tiles + 1 entries.  A level without node lists has 0
 * node refs and writes node_off as zeros.  OSMT_INVALID_ARG for a level that was not registered. */
int osmt_read_tile_pyramid(osmt_ctx* ctx, uint32_t geodata_id, uint32_t level, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways,
                           uint32_t* mp_off, uint32_t* mps, uint32_t* node_off, uint32_t* nodes, const size_t caps[4], size_t counts[4]);
/* Of the last completed tile query of this context: { (tile, column) items, way candidates, multipolygon candidates, node
 * candidates } as gathered, before dedup — what tests and tools use to see that a level was read.  A query of ways and
 * multipolygons (osmt_scene_build_tiles[_filtered], the area labels) reports 0 node candidates, the node query of the tile labels
 * 0 way and multipolygon candidates. */
int osmt_tile_query_stats(osmt_ctx* ctx, uint64_t stats[4]);

/* ---- the z18 tile index itself, built on the GPU from nodes, ways and multipolygons -------------------------------- */
/* get_tile_references (saver.rs:167-226) over the registered geodata and its registered Mercator factors
 * (osmt_register_node_mercator), for a caller whose geodata does not come from the importer's file:
 *
 *   node tile    with the factors (fx, fy) of a node, x = (u32)(fx * 2^26) >> 8, y = (u32)(fy * 2^26) >> 8 (tile.rs:30-38: the
 *                product with a power of two is exact, `as u32` truncates, / 256 is the shift).  Every node is listed in its tile.
 *   ways         a way with at least one node is listed in every tile of the inclusive rectangle [min x, max x] x [min y, max y]
 *                over its nodes' tiles, the tiles none of its nodes touches included; a way without nodes is listed nowhere.
 *   multipolygons the same over all nodes of all their polygons; a polygon without nodes contributes nothing, a multipolygon
 *                without polygons or with empty polygons only is listed nowhere.
 *   tiles        a tile exists iff a node, a way or a multipolygon is listed in it; tiles ascend by (x, y), every list ascends
 *                without repeats (the BTreeMap / BTreeSet order the file holds).
 *   factor 1.0   gives coordinate 2^18, which osmt_validate_tile_index refuses and no query reaches: the build is refused with
 *                OSMT_UNSUPPORTED, naming the lowest such node and whether it is its x or its y factor.  Never guessed, never
 *                clamped.
 *
 * The result equals the importer's index FOR THE REGISTERED FACTORS.  Reproducing a given file's index bit for bit needs factors
 * computed the way the importer's libm computes them: a node whose factor lies within an ulp of a tile edge can land in the
 * neighbouring tile under another tan / log.
 *
 * The built index is the geodata id's tile index: tile queries, both label builds, the pyramid, the id filter, the tile server and
 * the worker entries read it as they read a registered one.  One tile index per file, registered or built. */
/* OSMT_INVALID_ARG, naming the offender: an unknown geodata id (a NULL `ctx` has none), one without Mercator factors, one that
 * has a tile index already; node_ids non-NULL with n_nodes different from the geodata's, or while a node index is registered. */
int osmt_validate_tile_index_build(uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes, osmt_ctx* ctx);
/* Builds and installs the index.  The node lists are always built; with node_ids ([n_nodes] the nodes' global ids) the node index
 * is registered in the same call as osmt_register_node_index would leave it, with NULL none is (osmt_read_tile_index gives the
 * lists, osmt_register_node_index takes them later).  OSMT_UNSUPPORTED with the exact figure, decided before the pairs get a
 * buffer: a way, multipolygon or node reference total, or a total of tile keys (the kinds' distinct tiles, summed), that does
 * not fit 32 bits (>= 2^32 - 1); a factor of exactly 1.0.  A second build, or two threads building one id: one OSMT_OK, the other
 * OSMT_INVALID_ARG.  A failed call registers nothing, gives its buffers back and leaves the context usable. */
int osmt_build_tile_index(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* node_ids, size_t n_nodes);
/* Inspection, in the shape of osmt_read_tile_pyramid: the geodata id's tile index, built or registered (a registered one in its
 * registered order).  The node lists come back if a node index is registered or the index was built; otherwise there are 0 node
 * refs and node_off is zeros.  OSMT_INVALID_ARG without a tile index. */
int osmt_read_tile_index(osmt_ctx* ctx, uint32_t geodata_id, uint32_t* tile_xy, uint32_t* way_off, uint32_t* ways, uint32_t* mp_off,
                         uint32_t* mps, uint32_t* node_off, uint32_t* nodes, const size_t caps[4], size_t counts[4]);

/* ---- multipolygon rings assembled on the GPU from relations' member ways ------------------------------------------ */
/* find_polygons_in_multipolygon (find_polygons.rs, called from importer.rs:278-293 over RawRelation::to_segments,
 * importer.rs:516-537), for a caller whose geodata does not come from the importer's file: OSM relations with `inner` / `outer`
 * member ways in, the polygon and multipolygon arrays of osmt_geodata_desc out.  Per relation, in relation order:
 *
 *   segments     for every way reference in order and every idx in 1 .. len(way): (node[idx - 1], node[idx], role).  Ways come in
 *                as they are stored: postprocess_node_refs ran before, in osmt_resolve_refs (below) or at the caller.
 *   connections  per POSITION — the bits of (lat, lon): -0.0 and 0.0 are two vertices, two NaNs of equal bits are one — the list of
 *                (other side, segment), filled for idx ascending with node1's entry, then node2's: the order inside a list is
 *                2 * idx + side.  A segment whose two positions are equal stands twice on one list.
 *   rings        for start ascending over the segments still available: first = node1's position, walk from node2's.  Each
 *                step takes the FIRST entry of the current position's list that has the start segment's role, is available, and
 *                whose other side is no vertex this ring has used, unless it is `first`.  The ring closes when the other side is
 *                `first` and is valid with at least 3 segments.  No candidate, or a short ring: the WHOLE relation is rejected,
 *                with the two figures of the importer's message — complete rings so far, segments unmatched before this ring.
 *   polygons     per ring node1's id of its first segment, then per segment node2's id if the last id pushed equals node1's id,
 *                else node1's id: a comparison of IDS, where the search compares positions.
 *   multipolygons an accepted relation is one multipolygon with the relation's global id, its polygons appended in ring order; a
 *                relation without segments is accepted with no polygons; a rejected one leaves nothing behind.
 *
 * The search is greedy and order-dependent: the arrays equal the importer's for the same input, ring by ring.  The host twin
 * is osmt::assemble_multipolygons_host (host/osmt_polygons.hpp). */
typedef struct osmt_relations_desc {
    const double* nodes; /* [n_nodes][2] = (lat, lon); compared by their bits, any bit pattern is allowed */
    size_t n_nodes;
    const uint32_t* way_node_off; /* [n_ways + 1] into way_nodes; offsets as in osmt_geodata_desc */
    size_t n_ways;
    const uint32_t* way_nodes; /* node indices */
    size_t n_way_nodes;
    const uint64_t* relation_ids;     /* [n_relations] global ids */
    const uint32_t* relation_way_off; /* [n_relations + 1] into relation_ways / relation_way_inner */
    size_t n_relations;
    const uint32_t* relation_ways;     /* way indices */
    const uint8_t* relation_way_inner; /* the reference's role: 0 outer, 1 inner */
    size_t n_relation_ways;
} osmt_relations_desc;

/* what became of one relation; rings_built and unmatched are the figures of the importer's message for a rejected relation
 * (an accepted one: its ring count and 0) */
typedef struct osmt_relation_status {
    uint32_t accepted, rings_built, unmatched;
} osmt_relation_status;

typedef struct osmt_polygons osmt_polygons; /* an assembly's result, on the device until it is freed */

/* The checks osmt_assemble_multipolygons runs first, without a device.  OSMT_INVALID_ARG, naming the offender: a NULL array with
 * a non-zero count; bad offsets; a node or way index out of range; a role byte above 1.  OSMT_UNSUPPORTED, with the figure: a
 * segment total of 2^31 or more (an endpoint is 2 * segment + side in 32 bits); n_nodes at or above 2^32 - 1. */
int osmt_validate_relations(const osmt_relations_desc* relations);
/* Uploads the arrays, assembles every relation on the device (csrc/osmt_polygons.hip) and waits for the result.  A refused or
 * failed call allocates no result, gives its buffers back and leaves the context usable. */
int osmt_assemble_multipolygons(osmt_ctx* ctx, const osmt_relations_desc* relations, osmt_polygons** out);
/* counts = { polygons, polygon nodes, multipolygons, multipolygon polygons } */
int osmt_polygons_counts(const osmt_polygons* p, size_t counts[4]);
/* The arrays in exactly the form osmt_geodata_desc takes: polygon_node_off [counts[0] + 1], polygon_nodes [counts[1]],
 * multipolygon_ids [counts[2]], multipolygon_polygon_off [counts[2] + 1], multipolygon_polygons [counts[3]]; status
 * [n_relations]; multipolygon_relation [counts[2]]: the index of the relation a multipolygon came from, so the caller can carry
 * its tags over.  A NULL output is skipped; the caller's buffers have the sizes osmt_polygons_counts gave. */
int osmt_polygons_read(osmt_ctx* ctx, const osmt_polygons* p, uint32_t* polygon_node_off, uint32_t* polygon_nodes, uint64_t* multipolygon_ids,
                       uint32_t* multipolygon_polygon_off, uint32_t* multipolygon_polygons, osmt_relation_status* status,
                       uint32_t* multipolygon_relation);
void osmt_polygons_free(osmt_polygons* p);
/* Test hook in the spirit of osmt_debug_match_hash_bits: the vertex table of later assemblies of this context keeps only the
 * low `bits` bits of the position hash (32 = all; 0 puts every vertex into one probe chain).  The result must not change. */
int osmt_debug_vertex_hash_bits(osmt_ctx* ctx, uint32_t bits);

/* ---- OSM ids resolved on the GPU: way and relation references to local indices, ways deduped ----------------------- */
/* The three steps of importer.rs between the elements a parser hands over and the local indices every other call takes:
 * OsmEntityStorage::translate_id (importer.rs:45-71), the silent drop of references that do not resolve
 * (importer.rs:365-400) and postprocess_node_refs (importer.rs:334-353, called at importer.rs:260).  Elements come per kind
 * and in file order; selecting relations by type=multipolygon and dropping members that are no ways stay with the caller.
 *
 *   translate    a reference g of way w resolves to the LARGEST node index i < way_nodes_seen[w] with node_ids[i] == g:
 *                HashMap::insert overwrites, so a later element of an id wins, and an element not yet read does not exist.
 *                way_nodes_seen NULL: every way sees every node (a file that writes nodes, then ways, then relations).
 *                Relation members resolve the same way over way_ids / relation_ways_seen and carry their role byte along.
 *   drop         a reference without such an index is dropped; the others keep their order.  Every element stays stored: a
 *                shadowed duplicate keeps its index and is never referenced.
 *   dedup        over a way's references AFTER the drop: position 0 is kept; position idx >= 1 is kept iff no position
 *                1 <= j < idx has the same UNORDERED pair {refs[j], refs[j - 1]} — refs is the list before any removal, so
 *                the predecessor is the original neighbour, not the last one kept.  ([a,b,a,c] gives [a,b,c].)  This is what
 *                the importer's running HashSet computes: every visited pair is in the set afterwards in one orientation
 *                or the other, so "not seen" is "the first occurrence of the unordered pair in this way" (DESIGN.md
 *                section 3.20).  Relation members are not deduped: the importer does not dedup them.
 *
 * The result is in exactly the form osmt_relations_desc and osmt_geodata_desc take.  The host twin is
 * osmt::resolve_refs_host (host/osmt_resolve.hpp). */
typedef struct osmt_raw_osm_desc {
    const uint64_t* node_ids; /* [n_nodes] global ids, any 64 bits */
    size_t n_nodes;
    const uint64_t* way_ids;     /* [n_ways] */
    const uint32_t* way_ref_off; /* [n_ways + 1] into way_refs */
    size_t n_ways;
    const uint64_t* way_refs; /* the `nd ref` values in order */
    size_t n_way_refs;
    const uint32_t* relation_ref_off; /* [n_relations + 1] into relation_refs / relation_ref_inner */
    size_t n_relations;
    const uint64_t* relation_refs;     /* the ids of the type="way" members in order */
    const uint8_t* relation_ref_inner; /* role == "inner": 0 / 1 */
    size_t n_relation_refs;
    const uint32_t* way_nodes_seen;     /* [n_ways] nodes that precede the way in the file, or NULL: all of them */
    const uint32_t* relation_ways_seen; /* [n_relations] ways that precede the relation in the file, or NULL: all of them */
} osmt_raw_osm_desc;

typedef struct osmt_resolved osmt_resolved; /* a resolution's result, on the device until it is freed */

/* The checks osmt_resolve_refs runs first, without a device.  OSMT_INVALID_ARG, naming the offender: a NULL array with a
 * non-zero count; bad offsets; a role byte above 1; a *_seen value above its element count.  OSMT_UNSUPPORTED, with the
 * figure: n_nodes, n_ways or n_relations at or above 2^32 - 1 (an index is 32 bits and all ones marks "none"); a reference
 * total at or above 2^32 - 1. */
int osmt_validate_resolve(const osmt_raw_osm_desc* raw);
/* Uploads the arrays, resolves every reference on the device (csrc/osmt_resolve.hip) and waits for the result.  A refused or
 * failed call allocates no result, gives its buffers back and leaves the context usable. */
int osmt_resolve_refs(osmt_ctx* ctx, const osmt_raw_osm_desc* raw, osmt_resolved** out);
/* counts = { way nodes kept, relation ways kept, node references unresolved, node references removed as repeats, way
 * references unresolved } */
int osmt_resolved_counts(const osmt_resolved* r, size_t counts[5]);
/* way_node_off [n_ways + 1], way_nodes [counts[0]], relation_way_off [n_relations + 1], relation_ways [counts[1]],
 * relation_way_inner [counts[1]].  A NULL output is skipped. */
int osmt_resolved_read(osmt_ctx* ctx, const osmt_resolved* r, uint32_t* way_node_off, uint32_t* way_nodes, uint32_t* relation_way_off,
                       uint32_t* relation_ways, uint8_t* relation_way_inner);
void osmt_resolved_free(osmt_resolved* r);
/* Test hook in the spirit of osmt_debug_vertex_hash_bits: ways of up to `n` resolved references (at most 1024) of later
 * resolutions of this context find their repeats in LDS, one wave per way; longer ways go through the global sort.  0 sends
 * every way through the sort.  The result must not change. */
int osmt_debug_resolve_short_way_max(osmt_ctx* ctx, uint32_t n);

/* ---- the osm_ids filter: a set of global ids as bit-planes on the GPU -------------------------------------------- */
/* The one argument of get_entities_in_tile_with_neighbors(tile, osm_ids) (reader.rs:60,95-99): filter_entities_by_ids
 * (reader.rs:254-262) keeps an entity iff its global_id() is in the set.  ONE set serves nodes, ways and multipolygons alike
 * (the reference holds one HashSet<u64>): an id that a node and a way share keeps both.  `ids` may come in any order, with
 * repeats; n == 0 is a valid filter that keeps nothing (Some(empty)) and is not OSMT_ID_FILTER_NONE (None).
 *
 * Registration sorts and dedups the set on the host (once per filter, small), uploads it, and the device builds one bit-plane
 * per kind, 1 bit per entity of the geodata file (csrc/osmt_idfilter.hip): a lower-bound bisection per entity.  A registered
 * filter is one allocation that never moves; append-only with the snapshot rule of bindings, styles and fonts: a later
 * registration never disturbs a scene that is already built.  The node plane is built iff a node index
 * (osmt_register_node_index: it carries the nodes' global ids) is registered for the geodata id AT THAT MOMENT.
 *
 * Order of the drops and the limits, as in the reference, which gathers, sorts, dedups, drops polygon-less multipolygons and
 * filters LAST: the per-tile candidate limit OSMT_QUERY_MAX_TILE_CANDIDATES and the candidate totals are judged BEFORE the
 * filter (a filtered build gathers what an unfiltered one gathers); the area limit OSMT_STYLED_MAX_TILE_AREAS, the label limit
 * OSMT_TILE_LABELS_MAX and the area and label totals are judged AFTER it. */
#define OSMT_ID_FILTER_NONE 0xFFFFFFFFu
/* OSMT_INVALID_ARG, naming the offender: n >= 2^31; a NULL array with a non-zero count; an unknown geodata id (a NULL `ctx`
 * has none).  The first two need no context. */
int osmt_validate_id_filter(const uint64_t* ids, size_t n, uint32_t geodata_id, osmt_ctx* ctx);
/* Validates, builds the planes and returns the filter's id. */
int osmt_register_id_filter(osmt_ctx* ctx, uint32_t geodata_id, const uint64_t* ids, size_t n, uint32_t* out_filter_id);
/* Inspection: the three bit-planes as 32-bit words, entity e = bit e % 32 of word e / 32; a plane has whole 64-bit words and the
 * bits past the entity count are 0.  counts = { way words, multipolygon words, node words (0 without a node plane) } is always
 * set; caps bound what is written (a smaller cap with a non-NULL output is OSMT_INVALID_ARG); each output may be NULL. */
int osmt_read_id_filter(osmt_ctx* ctx, uint32_t filter_id, uint32_t* way_words, uint32_t* mp_words, uint32_t* node_words,
                        const size_t caps[3], size_t counts[3]);
/* osmt_scene_build_tiles with the filter: with OSMT_ID_FILTER_NONE it IS that call; otherwise the scene holds the filter's
 * snapshot, and osmt_scene_build_tile_labels and osmt_scene_build_tile_labels_all apply it to nodes, ways and multipolygons —
 * one filter per scene, as there is one per request in the reference.  OSMT_INVALID_ARG: an unknown filter id, a filter of
 * another geodata id than the batch's.  A label build with node bindings on a scene whose filter has no node plane is
 * OSMT_INVALID_ARG: register the node index first, then the filter.  A handed-in anchor
 * (osmt_scene_build_tile_labels_all) whose entity the filter removed is treated as every listed pair that has no labels in
 * its tile: it is validated like the others and then not looked at. */
int osmt_scene_build_tiles_filtered(osmt_ctx* ctx, const osmt_tile_batch* batch, uint32_t filter_id, osmt_scene** out_scene);

/* ---- label anchors from tile coordinates: the exact projection on the GPU ---------------------------------------- */
/* osmt_label_positions for callers that hold a registered geodata file: a request is 8 bytes — an entity and a tile — and
 * the device does what nodes_to_points does (labelable.rs:61-68), bit for bit.  The one libm step of coords_to_xy
 * (tile.rs:88-95), PI - tan(..).ln(), and the division by 2 PI behind it depend on the node alone, not on zoom or tile: the
 * caller computes them once per node and registers them.  Everything after that is exact IEEE arithmetic that every machine
 * rounds alike: factor * f64::from(256 << zoom) (a power of two), - f64::from(tile.x * 256) (one rounding), * scale (one
 * rounding).  The kernels (csrc/osmt_anchors.hip) run the three operations unfused and call no tan or log.
 *
 * factors[i] = ((lon_rad + PI) / (2 PI), (PI - ln(tan(PI / 4 + lat_rad / 2))) / (2 PI)) of node i, lat_rad = lat * (PI / 180)
 * as f64::to_radians; osmt::mercator_factors (host/osmt_geodata.hpp) is that formula, INTEGRATION.md has the Rust line.
 *
 * Why no point is range-checked afterwards: a factor f lies in [0, 1] and dim = 256 << zoom <= 2^26 at zoom <= 18, so f * dim
 * lies in [0, 2^26] (a multiplication by a power of two is exact); the tile offset 256 * x lies in [0, 2^26 - 256]; the
 * difference therefore has magnitude <= 2^26 and, rounding being monotonic, so has its rounded value; times scale <=
 * OSMT_MAX_SCALE = 4 that is <= 2^28 — the bound the polylabel kernels admit. */

/* The checks osmt_register_node_mercator runs first, on the host.  OSMT_INVALID_ARG, naming the offender: NULL with a count; a
 * factor that is not finite or lies outside [0, 1]; an unknown geodata id (a NULL `ctx` has none); n_nodes that is not the
 * geodata's; a geodata id that has its factors already. */
int osmt_validate_node_mercator(const double* factors /* [n_nodes][2] */, size_t n_nodes, uint32_t geodata_id, osmt_ctx* ctx);
/* Uploads the factors of every node of a registered geodata file: one allocation that never moves and lives as long as the
 * context (the snapshot rule of the tile index).  One table per geodata id: a second registration is OSMT_INVALID_ARG. */
int osmt_register_node_mercator(osmt_ctx* ctx, uint32_t geodata_id, const double* factors /* [n_nodes][2] */);

typedef struct osmt_label_tile_request { /* 8 bytes */
    uint32_t entity; /* local id of a way; of a multipolygon: | OSMT_STYLED_MULTIPOLYGON */
    uint32_t tile;   /* index into osmt_label_tile_batch.tiles */
} osmt_label_tile_request;

typedef struct osmt_label_tile_batch {
    const osmt_label_tile_request* requests;
    size_t n_requests;
    const osmt_query_tile* tiles; /* the array a caller hands to osmt_scene_build_tiles; the canvas fields are ignored */
    size_t n_tiles;
    uint32_t geodata_id, scale; /* scale 1 .. OSMT_MAX_SCALE: the factor of nodes_to_points AND the `scale` of get_label_position */
} osmt_label_tile_batch;

/* Host only.  OSMT_INVALID_ARG, naming the offender: a NULL pool with a non-zero count; scale outside 1..OSMT_MAX_SCALE; a
 * tile with zoom > 18 or x or y >= 2^zoom; a request whose tile index is >= n_tiles; an unknown geodata id (a NULL `ctx` has
 * none) or one without registered factors; an entity id that is not a way / multipolygon of the geodata. */
int osmt_validate_label_tile_batch(const osmt_label_tile_batch* batch, osmt_ctx* ctx);
/* get_label_position of every request: a way is ONE ring of its nodes, a multipolygon ALL polygon_count() polygons in file
 * order, polygons of 0 or 1 node included (labelable.rs:41-59) — not the >= 2-node rings a display list draws.  `out` gets
 * n_requests records with the meaning they have in osmt_label_positions (OK, NONE, TOO_LARGE), and
 * osmt_label_positions_stats reports the call.  Validates first (`out` is not touched when it fails).  OSMT_UNSUPPORTED with
 * the exact figure: a ring total or a point total of the batch that does not fit 32 bits (decided from the device's 64-bit
 * totals before anything is allocated for rings or points).  Zero requests: OSMT_OK, no device is touched. */
int osmt_label_positions_tiles(osmt_ctx* ctx, const osmt_label_tile_batch* batch, osmt_label_position* out);
/* The same call in two halves; the job ends with osmt_label_positions_end.  _begin waits for one small read-back (the
 * totals that size the point pool) and returns with the projection, the search and the read-back of the positions queued. */
int osmt_label_positions_tiles_begin(osmt_ctx* ctx, const osmt_label_tile_batch* batch, osmt_label_job** out_job);
/* Inspection (tests, tools): the rings and points the search of this batch would be given — rings[i].first_pt / n_pts index
 * `points` ([n][2], x then y), rings in request order.  counts[0] = rings, counts[1] = points, always set when the batch is
 * accepted; NULL for both outputs asks for the sizes; a capacity below a count with a non-NULL output is OSMT_INVALID_ARG. */
int osmt_label_tile_batch_expand(osmt_ctx* ctx, const osmt_label_tile_batch* batch, osmt_ring* rings, double* points, size_t rings_cap,
                                 size_t points_cap, size_t counts[2]);

/* ---- node labels of tile-built scenes: query, order and label records on the GPU --------------------------------- */
/* What Drawer::draw_labels does for the NODES of a tile (drawer.rs:251-260), for a scene of osmt_scene_build_tiles: the 3 x 3
 * neighbourhood query over the node lists of the tile index (reader.rs:60-133), the styles bound to every node under the
 * tile's zoom, the stable sort of Styler::style_entities(nodes, zoom, true) (styler.rs:163, compare_styled_entities with
 * for_labels: layer or 0, z_index, global id), and per (node, style) the osmt_label + osmt_string_run Labeler::label_entity
 * implies (labeler.rs:16-106, text_placer.rs:24-58): the anchor is Point::from_node (labelable.rs:15-24), the default text
 * position of a node is Center.  The batch goes through the string-label path of osmt_scene_set_string_labels.  Labels of
 * ways and multipolygons may be handed in host-built: they are drawn in front of the nodes' (drawer.rs:229-250);
 * osmt_scene_build_tile_labels_all below builds them on the device too.  The host twin is osmt::node_labels_of_tile (host/osmt_tilelabels.hpp). */

#define OSMT_TILE_LABELS_MAX 65536u /* (node, style) labels of one tile */
#define OSMT_TEXT_NONE 0xFFFFFFFFu  /* osmt_label_binding.text: the tag text_style.text names is absent (text_placer.rs:42-45) */

#define OSMT_LABEL_POSITION_NONE 0u   /* text_style.text_position is None: the default of the entity kind (a node: Center) */
#define OSMT_LABEL_POSITION_CENTER 1u
#define OSMT_LABEL_POSITION_LINE 2u   /* on a node: nothing is rasterized, save_to_figure of an empty figure is true */

/* the node half of the z18 tile storage (reader.rs:217-229, tile_local_ids(i, 0)), for the tiles of the tile index already
 * registered for the geodata id, plus the nodes' global ids */
typedef struct osmt_node_index_desc {
    const uint64_t* node_ids; /* [n_nodes] global ids (Node::global_id) */
    size_t n_nodes;           /* the geodata's node count */
    const uint32_t* node_off; /* [n_tiles + 1] into nodes, n_tiles = the registered tile index's */
    const uint32_t* nodes;    /* local node ids, any order, duplicates allowed */
    size_t n_node_refs;
} osmt_node_index_desc;

/* The label half of mapcss::styler::Style (styler.rs:42-72) as a POD of 48 bytes; a value whose has_* byte is 0 is ignored. */
typedef struct osmt_label_style_rec {
    int64_t layer;
    double z_index;
    double font_size;    /* text_style.font_size, as property_map_to_style produced it (unscaled) */
    uint32_t icon_image; /* id from osmt_register_image; an icon missing from the cache is has_icon = 0 (labeler.rs:55-66) */
    uint32_t font_id;    /* id from osmt_register_font; read when has_text_style and has_font_size */
    uint8_t has_layer, has_icon, has_text_style, has_font_size;
    uint8_t has_text_color, text_color[3];
    uint8_t text_position; /* OSMT_LABEL_POSITION_* */
    uint8_t _pad[7];
} osmt_label_style_rec;

typedef struct osmt_label_binding { /* one element Styler::style_entities pushes for a node */
    uint32_t style;                 /* id from osmt_register_label_styles */
    uint32_t text;                  /* index into the table's text pool, or OSMT_TEXT_NONE */
} osmt_label_binding;

/* (node -> label style, text) for a range of zooms, in push order, and the texts the bindings name */
typedef struct osmt_label_bindings_desc {
    uint32_t geodata_id;
    uint8_t zoom_lo, zoom_hi, _pad[2]; /* inclusive */
    const uint32_t* node_off;          /* [n_nodes + 1] into bindings */
    const osmt_label_binding* bindings;
    size_t n_bindings;
    const uint32_t* text_off; /* [n_texts + 1] into chars */
    size_t n_texts;
    const uint32_t* chars; /* Unicode scalar values, as osmt_string_label_batch.chars */
    size_t n_chars;
} osmt_label_bindings_desc;

/* OSMT_INVALID_ARG: an unknown geodata id (a NULL `ctx` has none) or one without a tile index; n_nodes different from the
 * geodata's; offsets that do not start at 0, decrease or do not end at the pool length; a node id >= n_nodes.
 * OSMT_UNSUPPORTED: more than 2^32 - 2 references. */
int osmt_validate_node_index(const osmt_node_index_desc* index, uint32_t geodata_id, osmt_ctx* ctx);
/* Uploads the node lists of a registered tile index and the nodes' global ids: one allocation that never moves and lives as
 * long as the context.  One per geodata id: a second registration is OSMT_INVALID_ARG. */
int osmt_register_node_index(osmt_ctx* ctx, uint32_t geodata_id, const osmt_node_index_desc* index);
/* OSMT_INVALID_ARG, naming the style: a NaN z_index; an icon_image or font_id that is not registered (`ctx` is only asked for
 * its icons and fonts, a NULL one has none); a font_size that is not finite or is not finite after multiplication by
 * OSMT_MAX_SCALE; an unknown text_position.  Only values whose has_* byte is set are looked at. */
int osmt_validate_label_styles(const osmt_label_style_rec* styles, size_t n, osmt_ctx* ctx);
/* Appends n label styles; style i gets id *out_first_style_id + i.  Append-only with the snapshot rules of
 * osmt_register_styles; the dense rank of every style under (layer or 0, z_index with -0.0 == +0.0) is recomputed when
 * the table has grown. */
int osmt_register_label_styles(osmt_ctx* ctx, const osmt_label_style_rec* styles, size_t n, uint32_t* out_first_style_id);
/* OSMT_INVALID_ARG: an unknown geodata id, zoom_lo > zoom_hi or zoom_hi > OSMT_MAX_ZOOM, bad offsets (as above), a style id
 * that is not registered at the time of the call, a text id that is neither in the pool nor OSMT_TEXT_NONE, a char that is
 * not a Unicode scalar value. */
int osmt_validate_label_bindings(const osmt_label_bindings_desc* b, osmt_ctx* ctx);
/* Appends a label bindings table (one device allocation that never moves) and returns its id. */
int osmt_register_label_bindings(osmt_ctx* ctx, const osmt_label_bindings_desc* b, uint32_t* out_bindings_id);
/* Builds the node labels of every tile of `scene` on the device (csrc/osmt_tilelabels.hip), reads the batch back, puts
 * each tile's `area_labels` (may be NULL; job_label_off over the scene's tiles) in front of its node labels and attaches the
 * result as osmt_scene_set_string_labels does.  label_bindings_of_zoom[z]: id from osmt_register_label_bindings or
 * OSMT_BINDINGS_NONE.  OSMT_INVALID_ARG: a scene that osmt_scene_build_tiles did not build, a geodata id without node
 * index, a tile whose zoom has no bindings or bindings of another geodata id or zoom range; OSMT_UNSUPPORTED with the exact
 * figure: a tile that gathers more than OSMT_QUERY_MAX_TILE_CANDIDATES node references or has more than
 * OSMT_TILE_LABELS_MAX labels, a label or char total that does not fit 32 bits; and whatever osmt_scene_set_string_labels
 * refuses.  On an error of the build the scene keeps the labels it had; an error of the attach leaves it without labels, as
 * osmt_scene_set_string_labels does. */
int osmt_scene_build_tile_labels(osmt_ctx* ctx, osmt_scene* scene, const uint32_t label_bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                                 const osmt_string_label_batch* area_labels);
/* Inspection: the node batch the device built in the last osmt_scene_build_tile_labels of the scene, before the splice.
 * counts = { labels, chars } is always set; caps = { labels, chars } bound what is written (a smaller cap with a non-NULL
 * output is OSMT_INVALID_ARG); each output may be NULL; job_label_off gets n_tiles + 1 entries. */
int osmt_scene_read_tile_labels(osmt_ctx* ctx, osmt_scene* scene, osmt_label* labels, osmt_string_run* runs, uint32_t* chars,
                                uint32_t* job_label_off, const size_t caps[2], size_t counts[2]);

/* ---- area labels of tile-built scenes: order, anchors and way text on the GPU ------------------------------------ */
/* What Drawer::draw_labels does for the WAYS and MULTIPOLYGONS of a tile (drawer.rs:229-250), for a scene of
 * osmt_scene_build_tiles: the 3 x 3 neighbourhood query over the way and multipolygon lists of the tile index, the label
 * styles bound to every entity under the tile's zoom, the order of style_areas(.., for_labels = true) (styler.rs:168-203: each
 * kind stably sorted by layer or 0, z_index, global id; merged with the multipolygon first on a tie), and per (entity, style)
 * what Labeler::label_entity does (labeler.rs:16-106, text_placer.rs:24-168): the anchor get_label_position of the entity
 * under the tile (the kernels of osmt_label_positions_tiles, fed on the device) for the icon and a centred text, the way's
 * points in walking order for a text along the line.  The default text position is Line for a way and Center for a
 * multipolygon; Line on a multipolygon and Center without an anchor rasterize nothing.  The angles of a text along a way —
 * atan2, sin, cos of integer differences — are filled in by the library ON THE HOST, with the libm of the process, in the batch
 * it reads back: the libm the caller's own code would have called.  The host twin is osmt::area_labels_of_tile
 * (host/osmt_arealabels.hpp). */

/* (way -> label style, text), (multipolygon -> label style, text) for a range of zooms, in push order, and the text pool */
typedef struct osmt_area_label_bindings_desc {
    uint32_t geodata_id;
    uint8_t zoom_lo, zoom_hi, _pad[2]; /* inclusive */
    const uint32_t* way_off;           /* [n_ways + 1] into way_bindings */
    const osmt_label_binding* way_bindings; /* style: id from osmt_register_label_styles; text_position NONE: the kind's default */
    size_t n_way_bindings;
    const uint32_t* multipolygon_off; /* [n_multipolygons + 1] into multipolygon_bindings */
    const osmt_label_binding* multipolygon_bindings;
    size_t n_multipolygon_bindings;
    const uint32_t* text_off; /* [n_texts + 1] into chars */
    size_t n_texts;
    const uint32_t* chars; /* Unicode scalar values */
    size_t n_chars;
} osmt_area_label_bindings_desc;

/* The anchor of one (tile, entity) pair: what the search declined (osmt_scene_read_declined_anchors) and what the caller hands
 * back computed (osmt_scene_build_tile_labels_all); 32 bytes. */
typedef struct osmt_area_anchor {
    uint32_t tile;   /* index of the tile in the scene */
    uint32_t entity; /* local id of a way; of a multipolygon: | OSMT_STYLED_MULTIPOLYGON */
    double x, y;
    uint32_t status; /* OSMT_LABEL_OK / OSMT_LABEL_NONE (handed in); OSMT_LABEL_TOO_LARGE (read as declined) */
    uint32_t _pad;
} osmt_area_anchor;

/* OSMT_INVALID_ARG, naming the offender: an unknown geodata id (a NULL `ctx` has none), one without a tile index
 * (osmt_register_tile_index) or without Mercator factors (osmt_register_node_mercator); zoom_lo > zoom_hi or zoom_hi >
 * OSMT_MAX_ZOOM; offsets that do not start at 0, decrease or do not end at the pool length (their counts are the geodata's);
 * a style id that is not registered at the time of the call; a text id that is neither in the pool nor OSMT_TEXT_NONE; a char
 * that is not a Unicode scalar value.  OSMT_UNSUPPORTED: a pool too large for 32-bit indices. */
int osmt_validate_area_label_bindings(const osmt_area_label_bindings_desc* b, osmt_ctx* ctx);
/* Appends an area label bindings table (one device allocation that never moves) and returns its id; ids are counted apart
 * from those of osmt_register_label_bindings. */
int osmt_register_area_label_bindings(osmt_ctx* ctx, const osmt_area_label_bindings_desc* b, uint32_t* out_bindings_id);
/* Builds the area labels of every tile of `scene` on the device (csrc/osmt_arealabels.hip), then its node labels as
 * osmt_scene_build_tile_labels does, and attaches each tile's area labels in front of its node labels as ONE string batch.
 * area_bindings_of_zoom[z]: id from osmt_register_area_label_bindings; node_bindings_of_zoom[z]: id from
 * osmt_register_label_bindings; either array may be NULL (no labels of that kind), an entry of a zoom some tile has may not
 * be OSMT_BINDINGS_NONE.  `anchors` (may be NULL with n_anchors 0): anchors the caller computed for pairs an earlier call
 * declined — strictly ascending by (tile, entity), status OK or NONE, x and y finite with |v| <= 2^28, tile and entity in
 * range, else OSMT_INVALID_ARG; a listed pair is not searched.
 * OSMT_UNSUPPORTED with the exact figure: a tile with more than OSMT_TILE_LABELS_MAX area labels; label, char, way point,
 * ring or point totals that do not fit 32 bits; and: the anchor search declined pairs (OSMT_LABEL_TOO_LARGE) — the message
 * names their number and the first (tile, entity), osmt_scene_read_declined_anchors returns all of them; compute them
 * (osmt::get_label_position over osmt::label_rings_of) and call again.  A label is never wrong and never dropped.
 * On an error of the build the scene keeps the labels it had and the context stays usable; an error of the attach leaves it
 * without labels, as osmt_scene_set_string_labels does. */
int osmt_scene_build_tile_labels_all(osmt_ctx* ctx, osmt_scene* scene, const uint32_t area_bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                                     const uint32_t node_bindings_of_zoom[OSMT_MAX_ZOOM + 1], const osmt_area_anchor* anchors, size_t n_anchors);
/* The pairs the last osmt_scene_build_tile_labels_all of the scene declined, ascending by (tile, entity), status
 * OSMT_LABEL_TOO_LARGE, x = y = 0; none after a call that did not decline.  *n is always set; out may be NULL to ask for the
 * size; cap < *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_scene_read_declined_anchors(osmt_ctx* ctx, osmt_scene* scene, osmt_area_anchor* out, size_t cap, size_t* n);
/* Inspection: the area batch the last successful osmt_scene_build_tile_labels_all of the scene built, before the splice
 * (osmt_scene_read_tile_labels keeps returning the node batch).  counts = { labels, chars, way points } is always set; caps
 * bound what is written (a smaller cap with a non-NULL output is OSMT_INVALID_ARG); each output may be NULL; way_pts is
 * int32 [n][2], way_sincos double [n][2]; job_label_off gets n_tiles + 1 entries. */
int osmt_scene_read_tile_area_labels(osmt_ctx* ctx, osmt_scene* scene, osmt_label* labels, osmt_string_run* runs, uint32_t* chars,
                                     int32_t* way_pts, double* way_sincos, uint32_t* job_label_off, const size_t caps[3], size_t counts[3]);

/* ---- style bindings from tags: MapCSS selector matching on the GPU ------------------------------------------------ */
/* Rule matching (Styler::style_area -> area_matches -> matches_by_tags, mapcss/styler.rs:205-242,450-520) for every entity
 * of a registered geodata file at once: which selectors of a registered selector set match each node, way and
 * multipolygon (zoom left aside), and the entities' CLASSES.  A class is what the reference's style cache keys on
 * (mapcss/style_cache.rs) plus what property_map_to_style reads of the entity: (cache slot, tags["layer"].parse::<i64>(),
 * the matched selector ids ascending).  Entities of one class get the same styles at every zoom, so the caller cascades
 * once per class and zoom and registers the result with osmt_register_style_bindings_matched.  Parsing MapCSS, the cascade
 * and property_map_to_style stay with the caller; DESIGN.md 3.13 has the stages and the arguments. */

#define OSMT_MATCH_MAX_SELECTORS 16384u    /* selectors of one set */
#define OSMT_MATCH_MAX_SELECTOR_TESTS 16u  /* tests of one selector */

/* the tags of a geodata file as the file has them (reader.rs:339-398): per kind a CSR over (k_off, k_len, v_off, v_len)
 * quadruples into one string pool */
typedef struct osmt_tags_desc {
    const uint32_t* node_tag_off; /* [n_nodes + 1] into node_tags (in quadruples) */
    const uint32_t* node_tags;    /* [n_node_tags][4] */
    size_t n_nodes, n_node_tags;
    const uint32_t* way_tag_off; /* [n_ways + 1] */
    const uint32_t* way_tags;
    size_t n_ways, n_way_tags;
    const uint32_t* multipolygon_tag_off; /* [n_multipolygons + 1] */
    const uint32_t* multipolygon_tags;
    size_t n_multipolygons, n_multipolygon_tags;
    const uint8_t* strings;
    size_t n_string_bytes;
} osmt_tags_desc;

enum { OSMT_SEL_NODE = 0, OSMT_SEL_WAY = 1, OSMT_SEL_AREA = 2, OSMT_SEL_OTHER = 3 }; /* OTHER: All, Canvas, Meta — matches nothing */
enum {
    OSMT_TEST_EXISTS = 0,
    OSMT_TEST_NOT_EXISTS,
    OSMT_TEST_TRUE,
    OSMT_TEST_FALSE,
    OSMT_TEST_EQUAL,
    OSMT_TEST_NOT_EQUAL,
    OSMT_TEST_LESS,
    OSMT_TEST_LESS_OR_EQUAL,
    OSMT_TEST_GREATER,
    OSMT_TEST_GREATER_OR_EQUAL,
    OSMT_TEST_KINDS
};
typedef struct osmt_selector_test { /* 32 bytes */
    uint32_t kind;                 /* OSMT_TEST_* */
    uint32_t key_off, key_len;     /* the tag name, in the descriptor's string pool */
    uint32_t value_off, value_len; /* EQUAL / NOT_EQUAL: the value; 0, 0 otherwise */
    uint32_t _pad;
    double value;                  /* the four numeric kinds: the right-hand side; 0 otherwise */
} osmt_selector_test;
typedef struct osmt_selector_rec { /* 16 bytes */
    uint8_t object_type;           /* OSMT_SEL_* */
    uint8_t has_min_zoom, min_zoom, has_max_zoom, max_zoom, _pad[3]; /* carried for the caller (osmt::selectors_at_zoom); the device ignores zoom */
    uint32_t test_off, n_tests;    /* into tests */
} osmt_selector_rec;
/* selectors in stylesheet order: rule by rule, selector by selector */
typedef struct osmt_selectors_desc {
    const osmt_selector_rec* selectors;
    size_t n_selectors;
    const osmt_selector_test* tests;
    size_t n_tests;
    const uint8_t* strings;
    size_t n_string_bytes;
} osmt_selectors_desc;

typedef struct osmt_match osmt_match;
typedef struct osmt_number_override { /* 24 bytes: str::parse::<f64> of the tag value strings[v_off .. v_off + v_len) */
    uint32_t v_off, v_len;
    uint32_t has_value, _pad; /* 0: the parse is an error */
    double value;
} osmt_number_override;
typedef struct osmt_declined_number { /* 8 bytes */
    uint32_t v_off, v_len;
} osmt_declined_number;
typedef struct osmt_match_class { /* 24 bytes */
    int64_t layer;                 /* 0 without */
    uint32_t sel_off, n_sels;      /* into the pooled selector ids, ascending */
    uint32_t first_entity;         /* the lowest-numbered member; entities are numbered nodes, then ways, then multipolygons */
    uint8_t slot, has_layer, _pad[2]; /* slot: 0 node, 1 closed way, 2 open way, 3 multipolygon (styler.rs:559-579) */
} osmt_match_class;

/* The checks osmt_register_tags runs first, without a device.  OSMT_INVALID_ARG, naming the offender: NULL with a non-zero
 * count; offsets that do not start at 0, decrease or do not end at the pool length; a key or value range outside the string
 * pool; an entity whose keys are not STRICTLY ascending as unsigned bytes (the saver writes a BTreeMap; under that
 * condition the bisection of Tags::get_by_key, reader.rs:351-373, equals any correct lookup); with a context, a geodata id
 * that is unknown or entity counts that are not the registered file's (a NULL `ctx` skips these two).  OSMT_UNSUPPORTED:
 * tags or string bytes beyond 32-bit indices. */
int osmt_validate_tags(const osmt_tags_desc* tags, uint32_t geodata_id, osmt_ctx* ctx);
/* Uploads the tags of a registered geodata file: one allocation that lives as long as the context.  One per geodata id: a
 * second registration is OSMT_INVALID_ARG. */
int osmt_register_tags(osmt_ctx* ctx, uint32_t geodata_id, const osmt_tags_desc* tags);
/* The checks osmt_register_selectors runs first, without a device.  OSMT_INVALID_ARG: NULL with a non-zero count, an object
 * type or test kind outside the enums, a test range outside `tests`, a string range outside the pool, a zoom flag that is
 * not 0 or 1.  OSMT_UNSUPPORTED with the figure: more than OSMT_MATCH_MAX_SELECTORS selectors, a selector with more than
 * OSMT_MATCH_MAX_SELECTOR_TESTS tests. */
int osmt_validate_selectors(const osmt_selectors_desc* selectors);
/* Appends a selector set (append-only, the snapshot rules of styles and bindings: a set's device copy never moves).  At
 * registration the distinct test keys are sorted byte-wise and numbered, and per key the distinct EQUAL / NOT_EQUAL values. */
int osmt_register_selectors(osmt_ctx* ctx, const osmt_selectors_desc* selectors, uint32_t* out_selectors_id);
/* Runs the match on the device (csrc/osmt_selmatch.hip).  `ov` (n_ov entries, STRICTLY ascending by (v_off, v_len), ranges
 * inside the tags' string pool, has_value 0 or 1; anything else is OSMT_INVALID_ARG) lists tag values whose f64 the caller
 * supplies: a listed value is not parsed on the device.
 * Numbers are exact or declined, never guessed.  A tag value is parsed as f64 only where a numeric test names its key.  The
 * device accepts the grammar of str::parse::<f64> and converts when the conversion is exact by construction: inf, infinity,
 * nan, zero significands; otherwise the digits without leading zeros and trailing zeros form an integer w <= 2^53
 * and the decimal exponent e left over has |e| <= 22, so the value is RN(w * 10^e) or RN(w / 10^-e) — one
 * correctly rounded operation on two exact doubles.  A grammar error is an error (every comparison false), not a decline.
 * Every other value is DECLINED: the call returns OSMT_UNSUPPORTED naming how many distinct (v_off, v_len) were declined and
 * the first, and *out is a match that answers only osmt_match_read_declined_numbers and osmt_match_free.  The caller
 * computes those values (osmt::HostNumbers, host/osmt_selmatch.hpp) and calls again with them as `ov`.
 * tags["layer"] is parsed as i64 in full (sign, leading zeros, overflow = error) and is never declined.
 * OSMT_INVALID_ARG: unknown ids, a geodata id without tags.  *out is NULL on every other error. */
int osmt_match_selectors(osmt_ctx* ctx, uint32_t geodata_id, uint32_t selectors_id, const osmt_number_override* ov, size_t n_ov,
                         osmt_match** out);
void osmt_match_free(osmt_match* match);
/* The distinct declined tag values, ascending by (v_off, v_len); none for a complete match.  *n is always set; out may be
 * NULL to ask for the size; cap < *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_match_read_declined_numbers(osmt_match* match, osmt_declined_number* out, size_t cap, size_t* n);
/* The result of a complete match (a declined one is OSMT_INVALID_ARG).  counts = { entities, classes, pooled selector ids }
 * is always set; NULL outputs ask for sizes; caps bound what is written (a smaller cap with a non-NULL output is
 * OSMT_INVALID_ARG).  entity_class: the class of every node, then way, then multipolygon.  Class ids are a pure function of
 * the input: classes are numbered by their lowest-numbered member.  An entity that matches nothing still has a class. */
int osmt_match_read(osmt_match* match, uint32_t* entity_class, osmt_match_class* classes, uint32_t* class_selectors, const size_t caps[3],
                    size_t counts[3]);
/* Bindings per class: class_style_off[n + 1] / class_styles give every class its style ids in push order for zooms
 * zoom_lo..zoom_hi; the device expands them over the ways and multipolygons (count, scan, emit) into a table of exactly
 * the form osmt_register_style_bindings makes from the per-entity lists; the id serves osmt_tile_batch::bindings_of_zoom like
 * any other.  OSMT_INVALID_ARG: a match of another context or a declined one, n that is not the class count, bad offsets,
 * a style id that is not registered, a bad zoom range.  OSMT_UNSUPPORTED: more than 2^32 - 2 bindings of one kind. */
int osmt_register_style_bindings_matched(osmt_ctx* ctx, osmt_match* match, uint8_t zoom_lo, uint8_t zoom_hi, const uint32_t* class_style_off,
                                         const uint32_t* class_styles, size_t n, uint32_t* out_bindings_id);
/* Test hook in the spirit of osmt_debug_hypot: the class table of later osmt_match_selectors calls of this context keeps only
 * the low `bits` bits of the key hash (32 = all; 0 puts every key into one probe chain).  The result must not change. */
int osmt_debug_match_hash_bits(osmt_ctx* ctx, uint32_t bits);

/* ---- label bindings from tags: per-class expansion and tag text on the GPU --------------------------------------- */
/* What osmt_register_label_bindings / osmt_register_area_label_bindings take finished — per entity the (label style, text id)
 * pairs and the text pool — made on the device (csrc/osmt_labelbind.hip) from the match, the registered tags and label
 * bindings given PER CLASS.  An entity of class c gets, in push order, one osmt_label_binding per element of c's list: `style`
 * is copied; `text` is OSMT_TEXT_NONE when text_key is OSMT_TEXT_NONE or the entity has no tag whose key equals the key's
 * bytes (Tags::get_by_key(&text_style.text), text_placer.rs:42-45, reader.rs:351-373; &str order: unsigned bytes, a proper
 * prefix sorts first), else the text of that tag's value.  The lookup is made whatever the style's has_* bytes say.
 * The text pool: a text is a distinct value range (v_off, v_len) among the tags some binding of THIS table uses (the
 * reference's saver interns whole strings, saver.rs:141-152: in its files equal strings are equal ranges).  Texts are
 * numbered by their lowest-numbered user in the table's tag order — the node tags for the node table; the way tags, then the
 * multipolygon tags for the area table — a pure function of the input.  A text's chars are the value decoded as UTF-8; an
 * empty value is a text of 0 chars, not OSMT_TEXT_NONE.  A USED value that is not well-formed UTF-8 (Unicode Table 3-7: no
 * overlong forms, no surrogates, nothing above U+10FFFF, no sequence cut off by the end of the value) is OSMT_INVALID_ARG
 * naming the lowest-numbered offending tag (kind, entity, v_off), and nothing is registered; a value no binding uses is not
 * looked at; no byte at or past v_off + v_len is read. */

#define OSMT_LABEL_TEXT_KEYS_MAX 256u /* keys of one osmt_class_label_bindings_desc */

typedef struct osmt_class_label_binding { /* 8 bytes: one element style_entities pushes for every member of the class */
    uint32_t style;                       /* id from osmt_register_label_styles */
    uint32_t text_key;                    /* index into the descriptor's keys (the tag text_style.text names), or OSMT_TEXT_NONE */
} osmt_class_label_binding;

typedef struct osmt_class_label_bindings_desc {
    uint8_t zoom_lo, zoom_hi, _pad[6]; /* inclusive */
    const uint32_t* class_off;         /* [n_classes + 1] into bindings, push order inside a class */
    const osmt_class_label_binding* bindings;
    size_t n_classes, n_bindings;
    const uint32_t* key_off; /* [n_keys + 1] into key_bytes; keys need be neither sorted nor distinct; an empty key is legal */
    const uint8_t* key_bytes;
    size_t n_keys, n_key_bytes; /* n_keys <= OSMT_LABEL_TEXT_KEYS_MAX */
} osmt_class_label_bindings_desc;

/* The checks the two registrations below run first, without a device.  `match` and `ctx` may be NULL: the class count is
 * then not compared and the style ids are not looked up.  OSMT_INVALID_ARG: a match of another context or a declined one;
 * n_classes that is not the match's class count; offsets that do not start at 0, decrease or do not end at the pool length; a
 * style id that is not registered at the time of the call; a text_key that is neither below n_keys nor OSMT_TEXT_NONE; a bad
 * zoom range.  OSMT_UNSUPPORTED with the figure: more than OSMT_LABEL_TEXT_KEYS_MAX keys; pools beyond 32-bit indices.
 * Lists of classes that hold no entity of the table's kinds are validated and otherwise unused. */
int osmt_validate_class_label_bindings(const osmt_class_label_bindings_desc* d, osmt_match* match, osmt_ctx* ctx);
/* The node table: an id of the kind osmt_register_label_bindings returns, for the geodata id of the match; the device table
 * has exactly the layout that call makes and does not depend on the match after the call returns.  Beyond the validator:
 * OSMT_INVALID_ARG for what osmt_validate_label_bindings demands of the geodata id and for ill-formed UTF-8 (above);
 * OSMT_UNSUPPORTED with the figure for more than 2^32 - 2 bindings, 2^32 - 1 or more texts or chars. */
int osmt_register_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, const osmt_class_label_bindings_desc* d, uint32_t* out_bindings_id);
/* The area table (ways + multipolygons): an id of the kind osmt_register_area_label_bindings returns; the geodata id needs
 * what osmt_validate_area_label_bindings demands (tile index, Mercator factors).  Otherwise as above, the binding limit per
 * kind. */
int osmt_register_area_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, const osmt_class_label_bindings_desc* d, uint32_t* out_bindings_id);
/* Inspection of ANY registered label bindings table, host-made ones included.  counts = { bindings, texts, chars } is always
 * set; NULL outputs ask for sizes; caps bound what is written (a smaller cap with a non-NULL output is OSMT_INVALID_ARG);
 * node_off gets n_nodes + 1 entries, text_off n_texts + 1. */
int osmt_read_label_bindings(osmt_ctx* ctx, uint32_t id, uint32_t* node_off, osmt_label_binding* bindings, uint32_t* text_off, uint32_t* chars,
                             const size_t caps[3], size_t counts[3]);
/* The same for an area table; counts = { way bindings, multipolygon bindings, texts, chars }. */
int osmt_read_area_label_bindings(osmt_ctx* ctx, uint32_t id, uint32_t* way_off, osmt_label_binding* way_bindings, uint32_t* multipolygon_off,
                                  osmt_label_binding* multipolygon_bindings, uint32_t* text_off, uint32_t* chars, const size_t caps[4],
                                  size_t counts[4]);

/* ---- the cascade: styles per class and zoom from registered rules ------------------------------------------------ */
/* The step of Styler::style_entities between the match and the tables (mapcss/styler.rs:128-160,205-242,277-429), on the
 * device (csrc/osmt_cascade.hip): per class of an osmt_match and zoom 0 .. OSMT_MAX_ZOOM the fold of style_area over the
 * class's selectors that admit the zoom (area_matches' zoom half, 501-515), then property_map_to_style of every layer but
 * "*", in insertion order.  The styles of all (class, zoom, layer) are made distinct — as area records (osmt_style_rec with
 * their dashes) and as label records (osmt_label_style_rec) — and numbered by their lowest user, user number
 * ((class * 19) + zoom) * 8 + position (positions 0 .. 7; for a rule set registered with OSMT_RULES_CLASS_LAYERS positions
 * 0 .. 15, user number ((class * 19) + zoom) * 16 + position): styles are numbered by their lowest user in (class, zoom,
 * position) order either way, so ids remain a pure function of the input.  Zooms at which every class has the same lists
 * as at the zoom below are joined into ranges.  Nothing is approximate: casing_width = base + multiplier * w is a multiplication and an addition, never fused.
 * What the device cannot know the caller resolves per property: from_color_name of an identifier, and the registered image
 * of an icon-image / fill-image string (not in the icon cache: no icon, no image fill; drawer.rs:179-183,
 * labeler.rs:53-66).  The host twin is osmt::cascade_host (host/osmt_cascade.hpp); DESIGN.md 3.15. */

#define OSMT_CASCADE_MAX_LAYERS 8u       /* distinct layer names of one rule set, "*" and "default" included */
/* With OSMT_RULES_CLASS_LAYERS the names of the set and the layers of one class are bounded apart: layer numbers are local
 * to a class (numbered by first appearance among the class's selectors), so a sheet may name many layers as long as no
 * entity class collects more than OSMT_CASCADE_MAX_CLASS_LAYERS of them. */
#define OSMT_RULES_CLASS_LAYERS 1u        /* flags of osmt_validate_rules_ex / osmt_register_rules_ex */
#define OSMT_CASCADE_MAX_LAYER_NAMES 255u /* flagged set: distinct layer names, "*" and "default" included (a selector's layer is a byte) */
#define OSMT_CASCADE_MAX_CLASS_LAYERS 16u /* flagged set: distinct layers over the selectors of ONE class, all zooms, "*" and "default" counted */
#define OSMT_LAYER_DEFAULT 0xFFFFFFFFu   /* osmt_rules_desc.selector_layer: the selector names no layer */

enum { /* the 20 property names property_map_to_style reads; every other name is OSMT_PROP_OTHER and is dropped */
    OSMT_PROP_Z_INDEX = 0,
    OSMT_PROP_FILL_POSITION,
    OSMT_PROP_WIDTH,
    OSMT_PROP_CASING_WIDTH,
    OSMT_PROP_TEXT,
    OSMT_PROP_FONT_SIZE,
    OSMT_PROP_TEXT_COLOR,
    OSMT_PROP_TEXT_POSITION,
    OSMT_PROP_COLOR,
    OSMT_PROP_FILL_COLOR,
    OSMT_PROP_BACKGROUND_COLOR,
    OSMT_PROP_OPACITY,
    OSMT_PROP_FILL_OPACITY,
    OSMT_PROP_DASHES,
    OSMT_PROP_LINECAP,
    OSMT_PROP_CASING_COLOR,
    OSMT_PROP_CASING_DASHES,
    OSMT_PROP_CASING_LINECAP,
    OSMT_PROP_ICON_IMAGE,
    OSMT_PROP_FILL_IMAGE,
    OSMT_PROP_NAMES, /* 20 */
    OSMT_PROP_OTHER = OSMT_PROP_NAMES
};
enum { OSMT_PV_IDENTIFIER = 0, OSMT_PV_STRING, OSMT_PV_COLOR, OSMT_PV_NUMBERS, OSMT_PV_WIDTH_DELTA, OSMT_PV_KINDS }; /* parser.rs PropertyValue */

typedef struct osmt_rule_prop { /* 40 bytes: one `name: value;` of a rule */
    uint8_t name;               /* OSMT_PROP_* */
    uint8_t kind;               /* OSMT_PV_* */
    uint8_t has_color;          /* COLOR: 1.  IDENTIFIER: from_color_name found it.  Otherwise 0 */
    uint8_t rgb[3];             /* read when has_color */
    uint8_t has_image;          /* IDENTIFIER / STRING of icon-image or fill-image: the string's icon is registered */
    uint8_t _pad;
    uint32_t image;             /* read when has_image: id from osmt_register_image */
    uint32_t str_off, str_len;  /* IDENTIFIER / STRING: the bytes, in `strings` */
    uint32_t num_off, n_nums;   /* NUMBERS: the list, in `numbers` */
    uint32_t _pad2;
    double delta;               /* WIDTH_DELTA */
} osmt_rule_prop;

typedef struct osmt_rules_desc {
    uint32_t selectors_id;          /* the registered selector set the rules' selectors are */
    uint32_t font_id;               /* id from osmt_register_font: the font of every label style with a font size */
    const uint32_t* selector_rule;  /* [n_selectors] non-decreasing rule index */
    const uint32_t* selector_layer; /* [n_selectors] index into the layer names, or OSMT_LAYER_DEFAULT */
    size_t n_selectors;             /* the selector set's */
    const uint32_t* layer_off;      /* [n_layers + 1] into layer_bytes; "*" and "default" are recognised by their bytes; equal names are one layer */
    const uint8_t* layer_bytes;
    size_t n_layers, n_layer_bytes;
    const uint32_t* rule_prop_off; /* [n_rules + 1] into props, file order inside a rule */
    const osmt_rule_prop* props;
    size_t n_rules, n_props;
    const double* numbers;
    size_t n_numbers;
    const uint8_t* strings;
    size_t n_string_bytes;
    double casing_width_multiplier; /* Styler::casing_width_multiplier */
    double font_size_multiplier;    /* read when has_font_size_multiplier */
    uint32_t has_font_size_multiplier, _pad;
} osmt_rules_desc;

typedef struct osmt_cascade osmt_cascade;

/* The checks osmt_register_rules runs first, without a device; a NULL `ctx` skips the lookups of ids.  OSMT_INVALID_ARG,
 * naming the offender: NULL with a non-zero count; offsets that do not start at 0, decrease or do not end at the pool
 * length; a selector_rule that decreases or is >= n_rules; n_selectors that is not the selector set's; a name, kind or flag
 * outside its values; a COLOR without has_color, has_color on a value that is neither COLOR nor IDENTIFIER, has_image on
 * anything but an IDENTIFIER / STRING of icon-image or fill-image; a range outside its pool; an image that is not registered; a font_id that is not registered (asked
 * only when some rule writes font-size); a multiplier that is NaN.  OSMT_UNSUPPORTED with the figure: more than
 * OSMT_CASCADE_MAX_LAYERS distinct layer names ("*" and "default" counted, used by a selector or not); more than
 * OSMT_LABEL_TEXT_KEYS_MAX distinct `text` strings; pools beyond 32-bit indices. */
int osmt_validate_rules(const osmt_rules_desc* rules, osmt_ctx* ctx);
/* Appends a rule set (append-only, the snapshot rules of selectors and styles).  At registration, on the host: per rule and
 * name the LAST property of that name; the identifiers of line caps, text positions and fill-position as small codes; the
 * distinct `text` strings (IDENTIFIER or STRING alike) pooled as keys, numbered by first appearance in file order.  No kernel
 * touches a string. */
int osmt_register_rules(osmt_ctx* ctx, const osmt_rules_desc* rules, uint32_t* out_rules_id);
/* The same two calls with flags; flags = 0 IS osmt_validate_rules / osmt_register_rules (same checks, same messages).  A bit
 * other than OSMT_RULES_CLASS_LAYERS is OSMT_INVALID_ARG naming the value.  With OSMT_RULES_CLASS_LAYERS the bound on the
 * names is OSMT_CASCADE_MAX_LAYER_NAMES (more: OSMT_UNSUPPORTED with the figure), and what bounds the cascade is the number
 * of layers of one class, which only a match knows: osmt_cascade_classes checks it.  Over the same match a set of at most
 * OSMT_CASCADE_MAX_LAYERS names gives the same bytes registered either way. */
int osmt_validate_rules_ex(const osmt_rules_desc* rules, uint32_t flags, osmt_ctx* ctx);
int osmt_register_rules_ex(osmt_ctx* ctx, const osmt_rules_desc* rules, uint32_t flags, uint32_t* out_rules_id);
/* Runs the cascade on the device.  labels_all = 1: every style is also a label binding, as the reference pushes them;
 * 0: only styles with an icon or a text style (the others draw nothing, labeler.rs:28-36).  OSMT_INVALID_ARG: a match of
 * another context, a declined match, a match whose selector set is not the rules' set, an unknown rules id, labels_all that
 * is not 0 or 1; whatever osmt_validate_styles / osmt_validate_label_styles refuse of a produced distinct record (checked
 * on the host after the read-back, naming the record and the lowest (class, zoom, position) that produced it).
 * OSMT_UNSUPPORTED with the figure: more than 2^31 styles over all (class, zoom) pairs (the table of distinct records has twice
 * as many slots), more than 2^32 - 2 dashes, class styles or class label bindings over the zoom ranges; for a rule set registered
 * with OSMT_RULES_CLASS_LAYERS, a class whose selectors, taken over all zooms, name more than OSMT_CASCADE_MAX_CLASS_LAYERS
 * distinct layers ("*" and "default" counted) — the message names the lowest such class and its exact layer count, nothing
 * is registered and the context stays usable.  *out is NULL on every error. */
int osmt_cascade_classes(osmt_ctx* ctx, osmt_match* match, uint32_t rules_id, uint32_t labels_all, osmt_cascade** out);
void osmt_cascade_free(osmt_cascade* cascade);
/* counts = { distinct styles, dashes, distinct label styles, key bytes, keys, zoom ranges, class styles of all ranges, class
 * label bindings of all ranges, classes } is always set; NULL outputs ask for sizes; caps[0 .. 8) bound what is written (a
 * smaller cap with a non-NULL output is OSMT_INVALID_ARG).  zoom_lo / zoom_hi: the ranges, ascending, inclusive, together
 * 0 .. OSMT_MAX_ZOOM.  Range r has class_style_off[r * (classes + 1) ..][classes + 1] into ITS part of class_styles, which
 * starts at range_style_base[r] (ranges + 1 entries), and the same with class_off / bindings / range_binding_base.  Style
 * indices are into the distinct lists of this cascade; text_key is into the keys or OSMT_TEXT_NONE. */
int osmt_cascade_read(osmt_cascade* cascade, osmt_style_rec* styles, double* dashes, osmt_label_style_rec* label_styles, uint8_t* key_bytes,
                      uint32_t* key_off, uint8_t* zoom_lo, uint8_t* zoom_hi, uint32_t* class_style_off, uint32_t* class_styles,
                      uint32_t* range_style_base, uint32_t* class_off, osmt_class_label_binding* bindings, uint32_t* range_binding_base,
                      const size_t caps[8], size_t counts[9]);
#define OSMT_CASCADE_AREA_STYLES 1u /* osmt_register_styles + osmt_register_style_bindings_matched */
#define OSMT_CASCADE_NODE_LABELS 2u /* osmt_register_label_styles + osmt_register_label_bindings_matched */
#define OSMT_CASCADE_AREA_LABELS 4u /* osmt_register_label_styles + osmt_register_area_label_bindings_matched */
/* Registers the distinct styles / label styles once and, per zoom range, the tables `what` asks for through the existing
 * matched registrations (whose prerequisites and errors hold unchanged), and fills the per-zoom id arrays osmt_tile_batch and
 * the two label builders take; an array `what` does not ask for may be NULL and is otherwise filled with OSMT_BINDINGS_NONE.
 * `match` is the match the cascade was made from.  Registrations are append-only: an error half way leaves what was
 * registered before it. */
int osmt_cascade_register(osmt_ctx* ctx, osmt_cascade* cascade, osmt_match* match, uint32_t what, uint32_t bindings_of_zoom[OSMT_MAX_ZOOM + 1],
                          uint32_t label_bindings_of_zoom[OSMT_MAX_ZOOM + 1], uint32_t area_label_bindings_of_zoom[OSMT_MAX_ZOOM + 1]);

/* ---- projection only (tile.rs:88-106 + point.rs:11-19) ------------------ */
/* xy[i] = round(coords_to_xy_tile_relative(latlon[i], tile) * scale) as i32, latlon = n pairs (lat, lon) in degrees.
 * The contract, as tests/test_gpu_projection_domain.py tests it against the bounded model of tests/_projection_model.py:
 *   x  is identical to the reference's for every input: the longitude path is IEEE arithmetic alone.
 *   y  passes through the device's tan and log, the reference's through its host's.  It is identical to the reference's
 *      unless the real value of ry * scale lies within the derived bound of a round() tie (k + 1/2): with tan within 5 ulp
 *      and log within 3 ulp of the correctly rounded value (the OpenCL full-profile bounds the device library conforms to)
 *      that bound is at most 2.4e-7 px (zoom 18, scale 4; it halves with every zoom below).  Inside it the answer is one of
 *      the two neighbouring integers.
 *   Coordinates are NOT checked by this entry (the batch entries refuse what lies outside |lat| <= OSMT_MAX_ABS_LAT,
 *   |lon| <= 180): a NaN gives 0, what does not fit an i32 saturates, as `f64 as i32` does.
 * zoom > OSMT_MAX_ZOOM is refused with OSMT_INVALID_ARG; tile_x / tile_y are taken as they are. */
int osmt_project(osmt_ctx* ctx, const double* latlon, size_t n, uint8_t zoom, uint32_t tile_x, uint32_t tile_y,
                 double scale, int32_t* xy);

/* ---- layer compositing only (tile_pixels.rs:205-223 + :164-181) ---------- */
/* planes: [n][L][H][W][4] premultiplied f64 RGBA (NextPixel.color of L
 * successive generations); canvas_rgba: premultiplied f64[4]; result per pixel:
 * dst = canvas; for l in 0..L: dst = src_l + (1 - src_l.a) * dst; then
 * un-premultiply + truncate to u8 -> out_rgba [n][H][W][4], A = 255.
 * W*H must be a multiple of 64 (true for every (256*scale)^2 tile). */
int osmt_composite(osmt_ctx* ctx, const double* planes, const double canvas_rgba[4], uint32_t n, uint32_t L,
                   uint32_t W, uint32_t H, uint8_t* out_rgba);
/* DEVICE pointers; asynchronous on `stream`. */
int osmt_composite_device(osmt_ctx* ctx, const void* d_planes, const double canvas_rgba[4], uint32_t n, uint32_t L,
                          uint32_t W, uint32_t H, void* d_out_rgba, void* stream);

/* ---- PNG encoding of a rendered tile (host side) ------- */
/* rgb_triples_to_png (src/draw/png_writer.rs:4-21), the tail of Drawer::draw_tile
 * (drawer.rs:40-58): RGB8 PNG of an RGBA8 framebuffer tile (A dropped).  The reference's
 * tests compare DECODED pixels only, so filter / compression choices are free.
 * level: zlib 0..9 (other values: zlib default).  out_capacity >= osmt_png_bound(). */
size_t osmt_png_bound(uint32_t width, uint32_t height);
int osmt_encode_png(const uint8_t* rgba, uint32_t width, uint32_t height, size_t row_stride_bytes, int level,
                    uint8_t* out_png, size_t out_capacity, size_t* out_len);

/* ---- PNG files produced on the GPU ---------------------------------------- */
/* The same file format as above (RGB8, one IDAT) written by a HIP kernel, one workgroup per tile: Paeth-filtered
 * rows, one deflate block with distance-1 run matches under a prefix code fitted to map tiles (the same "dynamic
 * Huffman" header in every file), Adler-32 and chunk CRCs computed on the device.  Decoded pixels equal the
 * framebuffer; a map tile shrinks 5-8x, so a server moves 30-50 KB per tile over PCIe instead of 256 KB and spends
 * no host time in zlib.
 * d_rgba: n framebuffers (RGBA8, rows tightly packed) tile_stride bytes apart; d_png: n slots png_stride >=
 * osmt_png_device_bound(W, H) bytes apart (multiples of 4); d_len[i] = size of file i.  W multiple of 4, <= 1024;
 * H <= 1024.  Anything else is OSMT_UNSUPPORTED before a kernel is launched (osmt_last_error names the width or the height). */
size_t osmt_png_device_bound(uint32_t width, uint32_t height);
int osmt_encode_png_device(osmt_ctx* ctx, const void* d_rgba, size_t tile_stride_bytes, uint32_t n, uint32_t width, uint32_t height,
                           void* d_png, size_t png_stride_bytes, uint32_t* d_len, void* stream);
/* Drawer::draw_tile for a batch (drawer.rs:40-58): display lists (+ labels, may be NULL) in, PNG files out.
 * File i = out_png[out_off[i] .. out_off[i + 1]); out_off has n_jobs + 1 entries (filled even when out_capacity
 * is too small, so the call can be repeated with out_off[n_jobs] bytes). */
int osmt_render_batch_png(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels, uint8_t* out_png, size_t out_capacity,
                          uint64_t* out_off);
/* The same call in two halves, for a caller thread that renders batch after batch (the reference answers request after
 * request, src/http_server.rs:183-201): _begin validates, uploads and queues every kernel of the batch and returns
 * without waiting; _end waits for the files, compacts them and copies them into out_png (same out_png / out_off
 * contract as the one-piece call, same errors), and frees the job whatever it returns.  With batch k + 1 begun before
 * batch k is ended, the validation and upload of k + 1 run on the host while the GPU renders and encodes k, and the
 * read-back of k runs under the kernels of k + 1: one thread reaches what several threads of one-piece calls reach.
 * The arrays of `batch` / `labels` must stay valid until _end returns (uploads are stream-ordered).  Every job holds its
 * device buffers until it is ended: ~0.9 GB per 1024 tiles of 256 x 256 (PNG slots at 12 bits per filtered byte, the
 * compacted blob, two chunks of framebuffers; kept in the context's buffer cache afterwards). */
typedef struct osmt_png_job osmt_png_job;
int osmt_render_batch_png_begin(osmt_ctx* ctx, const osmt_batch* batch, const osmt_label_batch* labels /* may be NULL */, osmt_png_job** out_job);
int osmt_render_batch_png_end(osmt_png_job* job, uint8_t* out_png, size_t out_capacity, uint64_t* out_off);

/* ---- host pixels and PNG files from any scene (Drawer::draw_tile for tile coordinates, drawer.rs:40-58) ----------
 * The entries above start from a host-built osmt_batch.  These start from a scene of the context — osmt_scene_upload,
 * osmt_scene_build_styled or osmt_scene_build_tiles, with whatever labels osmt_scene_set_*labels or
 * osmt_scene_build_tile_labels[_all] attached — so a caller without a HIP runtime of its own goes from tile coordinates to
 * files.  The scene is BORROWED: it is never consumed and renders the same afterwards, through any entry.
 * Work runs on private streams of the context.  Before its first launch a call waits for the scene's own earlier launches
 * (the pre-pass rewrites the scene's lists), so a second call — or a second _begin — on the SAME scene while a job is in
 * flight is correct but serialised.  As with osmt_render_scene, one scene is driven by one thread at a time; different
 * scenes of one context may be driven from different threads and run concurrently.  A scene of 0 tiles is valid.
 * OSMT_INVALID_ARG: NULL arguments, a scene of another context, an unknown format, a stride below the tile size
 * (W*W*4, RGB8: W*W*3), RGB8 with `out` or the stride not a multiple of 4.
 *
 * osmt_render_scene_host: the pixels of every tile at out + i * out_tile_stride_bytes, complete on return; the same three
 * routes as osmt_render_batch* (zero-copy for at most OSMT_ZERO_COPY_TILES tiles into pinned memory, a two-stream chunked
 * read-back for big pinned outputs, one copy otherwise).
 * osmt_render_scene_png / _begin: the out_png / out_off contract of osmt_render_batch_png.  A job begun from a scene is
 * ended by osmt_render_batch_png_end like any other (capacity too small: out_off[n_jobs] is the size needed; the job is
 * freed whatever _end returns).  The job does not own the scene: the SCENE MUST OUTLIVE THE JOB — end (or abandon) the job
 * before osmt_scene_free. */
#define OSMT_PIXELS_RGBA8 0u
#define OSMT_PIXELS_RGB8 1u /* packed triples, the memory of RgbTriples */
int osmt_render_scene_host(osmt_ctx* ctx, osmt_scene* scene, uint32_t format, uint8_t* out, size_t out_tile_stride_bytes);
int osmt_render_scene_png(osmt_ctx* ctx, osmt_scene* scene, uint8_t* out_png, size_t out_capacity, uint64_t* out_off);
int osmt_render_scene_png_begin(osmt_ctx* ctx, osmt_scene* scene, osmt_png_job** out_job);

/* The asynchronous device form: render, encode, file offsets and compaction are QUEUED on the caller's stream and nothing is
 * waited for (the rules of osmt_render_scene).  Afterwards, in stream order: d_off[0 .. n_jobs] are the file offsets
 * (exclusive 64-bit scan of the lengths, complete in every case), *d_status is 0 and file i is d_png[d_off[i] .. d_off[i+1]),
 * or *d_status is 1 because d_off[n_jobs] > png_capacity and NOTHING was written to d_png.
 * d_work: osmt_scene_png_work_bytes(ctx, scene) bytes of device memory, aligned to 256 — n framebuffers of W*W*4 bytes, then n
 * slots of osmt_png_device_bound(W, W) bytes, then n 32-bit lengths, each part rounded up to a multiple of 256 bytes
 * (W = OSMT_TILE_SIZE * scale; 0 tiles: 0 bytes, d_work and d_png may be NULL).  d_off is 8-byte aligned device memory.
 * osmt_scene_png_work_bytes returns 0 on bad arguments. */
size_t osmt_scene_png_work_bytes(osmt_ctx* ctx, osmt_scene* scene);
int osmt_render_scene_png_device(osmt_ctx* ctx, osmt_scene* scene, void* d_work, size_t work_bytes, void* d_png, size_t png_capacity,
                                 uint64_t* d_off /* [n_jobs + 1] */, uint32_t* d_status, void* stream);
/* Test hook in the spirit of osmt_debug_hypot: the offset scan of the device form alone (k_png_offsets: one workgroup of
 * OSMT_PNG_OFFSETS_GROUP threads walks n <= 2^31 lengths in passes).  d_len[n], d_off[n + 1] and d_status are device memory;
 * queued on `stream`. */
#define OSMT_PNG_OFFSETS_GROUP 256u
int osmt_debug_png_offsets(osmt_ctx* ctx, const uint32_t* d_len, uint32_t n, uint64_t capacity, uint64_t* d_off, uint32_t* d_status,
                           void* stream);

/* ---- the per-request entry: one worker handle per server thread (SURVEY.md 8(b) "Threading") ----------------
 * The reference's server gives every request — ONE tile — to one of available_parallelism() worker threads, each
 * with a TilePixels of its own (src/http_server.rs:50-83,105-108,134-181: handle_connection -> draw_tile_png).
 * An osmt_worker is that per-thread handle.  osmt_worker_render is osmt_render_batch_rgb for the calling thread
 * (same arguments, same pixels, same errors, blocks until out_rgb holds the tiles), but requests of different
 * workers of one context that are in flight at the same moment are gathered into ONE launch sequence on the device:
 * a request that finds the device free starts at once, alone; requests that arrive while it renders wait and go out
 * together with the next one (at most 64 tiles per group, OSMT_WORKER_INFLIGHT = 2 groups on the device at a time).
 * Sixteen threads calling the batch entry with one tile each queue up behind each other instead (round 3: 17 k
 * tiles/s at p99 9.6 ms).  Any thread may use any worker; a worker keeps its context alive like a scene does.
 * Batches of more than 64 tiles are rendered directly. */
typedef struct osmt_worker osmt_worker;
int osmt_worker_create(osmt_ctx* ctx, osmt_worker** out_worker);
void osmt_worker_destroy(osmt_worker* worker);
int osmt_worker_render(osmt_worker* worker, const osmt_batch* batch, const osmt_label_batch* labels /* may be NULL */, uint8_t* out_rgb,
                       size_t out_tile_stride_bytes);

/* ---- tile requests: (z, x, y, scale) in, PNG out ------------------------------------------------------------------ */
/* The reference's request handler (try_handle_connection, src/http_server.rs:134-181) as one step: what a server renders
 * its requests with — geodata, bindings per zoom, canvas, filter — is stated ONCE, in a tile server; a request is then tile
 * coordinates and a scale.  The server is immutable, holds a reference on its context like a scene or a worker, and is
 * validated once: every id known, of this geodata id and covering the zoom it is listed under, the filter of this geodata id,
 * a node index (and, with a filter, a node plane) where node labels are bound.  A label array that is all
 * OSMT_BINDINGS_NONE means no labels of that kind. */
typedef struct osmt_tile_server_desc {
    uint32_t geodata_id, use_caps_for_dashes;
    uint32_t id_filter; /* from osmt_register_id_filter, or OSMT_ID_FILTER_NONE */
    uint8_t has_canvas, canvas_rgb[3];
    uint32_t bindings_of_zoom[OSMT_MAX_ZOOM + 1];            /* osmt_register_style_bindings[_matched] / osmt_cascade_register */
    uint32_t area_label_bindings_of_zoom[OSMT_MAX_ZOOM + 1]; /* all OSMT_BINDINGS_NONE: no labels of that kind */
    uint32_t node_label_bindings_of_zoom[OSMT_MAX_ZOOM + 1];
} osmt_tile_server_desc;
typedef struct osmt_tile_server osmt_tile_server;
typedef struct osmt_tile_coord { /* 12 bytes */
    uint32_t x, y, zoom;
} osmt_tile_coord;

/* OSMT_INVALID_ARG, naming the offender (a NULL `ctx` knows no geodata id). */
int osmt_validate_tile_server(const osmt_tile_server_desc* d, osmt_ctx* ctx);
int osmt_tile_server_create(osmt_ctx* ctx, const osmt_tile_server_desc* d, osmt_tile_server** out);
void osmt_tile_server_free(osmt_tile_server* s);
/* Tiles in, files out, in one call, on the library's own streams: osmt_scene_build_tiles[_filtered], then — if a label array
 * is not all-NONE — osmt_scene_build_tile_labels_all, then osmt_render_scene_png, then the scene is freed.  out_png / out_off
 * [n + 1] follow the osmt_render_batch_png contract: the offsets are filled even when out_capacity is too small
 * (OSMT_INVALID_ARG), so the call can be repeated; n * osmt_png_device_bound(W, W) always suffices.  n == 0 is OSMT_OK and
 * touches no device.  A tile at a zoom whose style bindings are OSMT_BINDINGS_NONE is OSMT_INVALID_ARG, and so is one at a
 * zoom with NONE in a label array that is not all-NONE: judged for this call alone, by the rules of osmt_validate_tile_batch
 * and osmt_scene_build_tile_labels_all.  `anchors` follow the osmt_scene_build_tile_labels_all contract (tile = index into
 * `tiles`).  When the anchor search declines pairs the call is OSMT_UNSUPPORTED as that call is, and the declined list is kept
 * for the calling thread (osmt_last_declined_anchors): compute the anchors and call again.  A label is never wrong and
 * never dropped. */
int osmt_tile_server_render_png(osmt_tile_server* s, const osmt_tile_coord* tiles, size_t n, uint32_t scale,
                                const osmt_area_anchor* anchors, size_t n_anchors, uint8_t* out_png, size_t out_capacity,
                                uint64_t* out_off /* [n + 1] */);
/* The pairs the last osmt_tile_server_render_png / osmt_worker_render_tile_png call of THIS thread declined (tile = index into
 * that call's tiles; empty after a call that declined nothing).  Thread-local like osmt_last_error.  *n is always set; out
 * may be NULL; a cap below *n with a non-NULL out is OSMT_INVALID_ARG. */
int osmt_last_declined_anchors(osmt_area_anchor* out, size_t cap, size_t* n);
/* The per-request entry: one tile, one file.  Group commit exactly as osmt_worker_render does it: the requester validates its
 * own request and queues it; a request that finds fewer than OSMT_WORKER_INFLIGHT groups on the device (a count it shares with
 * osmt_worker_render) becomes leader and takes the waiting requests of the server and scale at the head of the queue, in
 * arrival order, up to the first request of another server or scale (the next leader's) and up to 64 tiles — mixed zooms share
 * a group — and runs the body of osmt_tile_server_render_png once into pinned staging; every
 * requester copies its own file out.  No timer: a lone request never waits.  If the group's run fails for any reason every
 * member is run alone, so a bad request or a declined anchor fails alone and the others get their files; a member's declined
 * list (tile 0 in each) is left for ITS thread.  anchors: tile == 0 in each.  out_capacity too small: OSMT_INVALID_ARG,
 * *out_len is the size needed and nothing is written; osmt_png_device_bound(W, W) always suffices. */
int osmt_worker_render_tile_png(osmt_worker* w, osmt_tile_server* s, const osmt_tile_coord* tile, uint32_t scale,
                                const osmt_area_anchor* anchors, size_t n_anchors, uint8_t* out_png, size_t out_capacity,
                                size_t* out_len);
/* Inspection: stats = { requests queued, groups run, tiles of the largest group } of osmt_worker_render_tile_png since the
 * context was created. */
int osmt_worker_tile_stats(osmt_ctx* ctx, uint64_t stats[3]);

/* ---- one node, several GPUs ------------------------------------------------ */
/* The reference deals tiles round-robin to its worker threads, each with its own TilePixels
 * (src/http_server.rs:50-83,105-108); tiles never exchange data (neighbours' geometry is duplicated into every
 * tile's entity list, reader.rs:60-100).  Here a worker is a GPU: tile i of a batch belongs to shard i mod world. */

/* The display list of one shard: jobs rank, rank + world, ... of `batch` with their ops, rings, points and dashes
 * re-packed into pools of their own (a valid osmt_batch: the shard's op ranges partition its op pool).  The node table
 * of OSMT_COORD_NODE_REF is shared, not copied: `batch->nodes` must outlive the shard.  Host only. */
typedef struct osmt_batch_shard osmt_batch_shard;
int osmt_batch_shard_create(const osmt_batch* batch, uint32_t rank, uint32_t world, osmt_batch_shard** out_shard);
const osmt_batch* osmt_batch_shard_get(const osmt_batch_shard* shard);
void osmt_batch_shard_free(osmt_batch_shard* shard);

/* One call, n GPUs of one node: one host thread per context builds its shard and runs osmt_render_batch on it
 * (upload, kernels and the chunked read-back pipeline of each GPU overlap with the others'); tile i lands at
 * out_rgba + i * out_tile_stride_bytes exactly as with one GPU — every GPU writes its own interleaved slices of the
 * one buffer (pinned memory from osmt_host_alloc of ANY of the contexts keeps the copies asynchronous).
 * *out_tile_count (optional) = the all-reduced number of rendered tiles: over RCCL when osmt_comm_init_local has
 * joined the contexts, summed on the host otherwise; it equals batch->n_jobs on success. */
int osmt_render_batch_multi(osmt_ctx* const* ctxs, uint32_t n_ctx, const osmt_batch* batch, uint8_t* out_rgba,
                            size_t out_tile_stride_bytes, uint64_t* out_tile_count);
/* The same with what the reference's workers always do after the areas — Drawer::draw_labels per tile
 * (drawer.rs:107-125) — and with the reference's own output format: `labels` (may be NULL) is sliced per shard by
 * job_label_off (tile i's labels travel with tile i, segments re-packed); flags & OSMT_MULTI_RGB8 writes packed RGB8
 * (out_tile_stride_bytes >= W*H*3, the layout of osmt_render_batch_rgb) instead of RGBA8.  Image ids of the labels /
 * FILL_IMAGE ops are per context: register the same icons in the same order on every context. */
#define OSMT_MULTI_RGB8 1u
int osmt_render_batch_multi_ex(osmt_ctx* const* ctxs, uint32_t n_ctx, const osmt_batch* batch, const osmt_label_batch* labels,
                               uint32_t flags, uint8_t* out, size_t out_tile_stride_bytes, uint64_t* out_tile_count);

/* RCCL communicators for the tile-count reduction (the path's only collective: 8 bytes, latency-bound).  The library
 * is loaded at the first of these calls (dlopen: an already loaded RCCL — e.g. PyTorch's — is reused).
 *   one process, n GPUs:  osmt_comm_init_local(ctxs, n)                                   (ncclCommInitAll)
 *   one process per GPU:  rank 0 calls osmt_comm_unique_id and sends the 128 bytes to the other ranks by its own
 *                         means; every rank then calls osmt_comm_init_rank(ctx, id, rank, nranks)  (ncclCommInitRank) */
#define OSMT_COMM_ID_BYTES 128
int osmt_comm_unique_id(uint8_t id[OSMT_COMM_ID_BYTES]);
int osmt_comm_init_rank(osmt_ctx* ctx, const uint8_t id[OSMT_COMM_ID_BYTES], uint32_t rank, uint32_t nranks);
int osmt_comm_init_local(osmt_ctx* const* ctxs, uint32_t n_ctx);
/* ncclAllReduce(sum) of one uint64 over the communicator of `ctx`; collective: every rank calls it.  Blocks until the
 * result is on the host. */
int osmt_allreduce_tile_count(osmt_ctx* ctx, uint64_t local, uint64_t* out_global);
/* The same reduction behind the kernels of a render: enqueued on `stream` (the stream the batch was rendered on), no
 * host synchronisation, so the next batch's kernels queue up behind it.  `..._result` copies the most recent sum back
 * and waits for `stream` only.  Collective: every rank enqueues the same number of reductions. */
int osmt_allreduce_tile_count_enqueue(osmt_ctx* ctx, uint64_t local, void* stream);
int osmt_allreduce_tile_count_result(osmt_ctx* ctx, void* stream, uint64_t* out_global);
/* the same for the contexts of ONE process (a grouped call over all of them) */
int osmt_allreduce_tile_count_local(osmt_ctx* const* ctxs, uint32_t n_ctx, const uint64_t* locals, uint64_t* out_global);

/* ---- diagnostics ------------------------------------------------------------------------------ */
/* What "HBM speed" is on this device: a 16-byte-per-lane grid-stride stream over `bytes`, `iters` launches timed with
 * HIP events after one warm-up.  *out_copy_gb_per_s = copy (bytes read + bytes written); *out_read_gb_per_s (optional)
 * = the same stream read only — the ceiling of a read-dominated pass such as the layer composite.  bench.py quotes
 * roofline fractions against these next to the 8 TB/s datasheet figure. */
int osmt_hbm_copy_probe(osmt_ctx* ctx, size_t bytes, uint32_t iters, double* out_copy_gb_per_s, double* out_read_gb_per_s);
/* 1 when the process runs with OSMT_POISON_ALLOC=1: every device buffer and every pinned staging buffer the library hands
 * out — fresh or recycled from its caches — is filled with 0xA5 first.  The reference resets every pixel and pending entry
 * per tile (src/draw/tile_pixels.rs:89-105); the library recycles buffers un-zeroed, so a kernel may only read what this
 * render wrote.  The GPU tests and the fuzz run under it (tests/conftest.py); production leaves it off (one memset per
 * allocation). */
int osmt_debug_poison_enabled(void);

#ifdef __cplusplus
}
#endif
#endif /* OSMTILE_H */
