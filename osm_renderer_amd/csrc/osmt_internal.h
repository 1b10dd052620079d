/* osmt_internal.h — device-side records shared by the kernels and the host library. */
#ifndef OSMT_INTERNAL_H
#define OSMT_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/osmtile.h"
#include "osmt_glyph.h"
#include "osmt_list_slices.h"
#include "osmt_fill_slots.h"

/* Sub-tile geometry of k_raster: OSMT_SUB_W x OSMT_SUB_H pixels per workgroup.  Sub-tile
 * coverage masks (osmt_raster_args.submask) have one 32-bit word per sub-tile ROW. */
#define OSMT_SUB_W 32
#ifndef OSMT_SUB_H_LOG2
#define OSMT_SUB_H_LOG2 4
#endif
#define OSMT_SUB_H (1 << OSMT_SUB_H_LOG2)

/* even dash indices (<= 8) + the first dash repeated (opacity_calculator.rs:105-106) */
#define OSMT_MAX_DASH_SEGS 10

/* DashSegment, opacity_calculator.rs:88-96 */
struct osmt_dash_seg {
    double start_from, start_to, end_from, end_to, opacity_mul;
    double orig_a, orig_b; /* original_endpoints (valid when table.has_orig) */
    double r_start, r_end; /* RN(1 / (start_to - start_from)), RN(1 / (end_to - end_from)): the two ramp divisions as osmt_div_exact */
};

/* A cap stub of draw_lines (line.rs:33-57): p1 -> p1.push_away_from(p2, half_width) of the first edge, p2 ->
 * p2.push_away_from(p1, half_width) of the last one; k_opinfo's working record (the stubs reach the binning kernel as the op's
 * last two virtual segments). */
struct osmt_cap_seg {
    int32_t p1x, p1y, p2x, p2y;
    int32_t valid; /* the edge is not degenerate and the cap is Round/Square */
    uint32_t cand_off; /* first slot of the stub's sub-tile window in the op's slice of the stroke arena */
    double denom;  /* center_dist_denom of the stub */
};

/* The per-op constants of a STROKE op (k_opinfo -> k_raster): 192 bytes, written as three whole 64-byte lines.
 * draw_lines builds two OpacityCalculators (line.rs:21-22): `main` for the edges — its DashSegments (up to
 * OSMT_MAX_DASH_SEGS, only when the op has dashes) live in a table of their own, osmt_*_args::dseg[aux index][..], so that an
 * un-dashed op writes and reads nothing of it — and the one for the outer cap stubs, which always has exactly ONE segment
 * (compute_segments over dashes = [0.0]) and total_len 0.  (Until round 4 the record held both tables in full, 1608 bytes,
 * and the cap stubs a second time: k_opinfo wrote five partial cache lines per stroke op — most of its 1.9 GB on config 5.) */
struct alignas(64) osmt_stroke_aux {
    double half_width;
    /* get_opacity_by_center_distance terms for cap_dist == 0 (opacity_calculator.rs:36,171-176):
     * hlw0 = sqrt(h*h - 0*0), feather_from/to/dist and opacity_mul of hlw0 */
    double hlw0, ff0, ft0, fd0, mul0;
    double rfd0; /* RN(1 / fd0): the feather division of the walk becomes osmt_div_exact */
    /* OpacityCalculator `main` minus half_line_width / traveled (opacity_calculator.rs:3-8) */
    int32_t main_n_segs;
    int32_t main_has_orig; /* line cap is Round and use_caps_for_dashes: original_endpoints = Some(..) */
    double main_total_len;
    double main_r_total;   /* RN(1 / total_len): quotient estimate of the exact `dist_rem % total_len` */
    /* opacity_calculator_for_outer_caps: n_segs == 1, total_len == 0 */
    int32_t caps_has_orig;
    int32_t _pad;
    osmt_dash_seg caps_seg;
};
static_assert(sizeof(osmt_stroke_aux) == 192, "three 64-byte lines");

/* Everything k_raster needs to start on an op, in ONE 64-byte record (one s_load_dwordx16): the op header fields it
 * uses and the results of the pre-pass — k_raster never touches ops, rings or points. */
struct osmt_opinfo {
    int32_t x0, y0, x1, y1; /* inclusive extent of the op's points (empty: x0 > x1) */
    uint32_t aux;           /* STROKE: index into the stroke_aux table */
    uint32_t n_edges;       /* total edges over all rings */
    uint32_t first_pt;      /* first point of the op's FIRST ring: a one-ring polygon is binned without touching osmt_op / osmt_ring */
    uint32_t n_rings;       /* osmt_op.n_rings */
    uint8_t kind, cap, color[3], _pad[3]; /* osmt_op.kind / cap / color */
    /* FILL: first 64-byte group (16 row words of one sub-tile) of the op's coverage masks in the fill arena;
     * STROKE: first record of the op in the stroke-record arena */
    uint32_t arena_off;
    uint32_t rec_cap;   /* STROKE: slots of the op in the stroke arena = sum over its virtual segments of the sub-tiles
                         * in each one's window; slot order = segment order (edges, then the two cap stubs), window row-major */
    union {
        struct {
            /* FILL: sub-tile window the masks cover: sr0 | c0 << 8 | ncols << 16 | nsr << 24 (nsr == 0: no covered row inside the tile) */
            uint32_t fill_geom;
            uint32_t image_id; /* FILL_IMAGE: osmt_op.image_id */
        };
        double stroke_ft; /* STROKE: max(|half_width| + 0.5, 1.0), the feather_to the binning bounds a run's reach with */
    };
    double opacity;     /* osmt_op.opacity */
};
static_assert(sizeof(osmt_opinfo) == 64, "osmt_opinfo must be one 64-byte record");

/* ---- pre-pass products (implementation traffic, not algorithmic bytes) --------------------------
 * Fill arena: for every FILL op, for every sub-tile (sr, c) of its window, 16 words = the coverage of rows
 * 16*sr .. 16*sr+15 restricted to columns 32*c .. 32*c+31 (bit x of the word of row y = fill_contour sets pixel (x, y),
 * fill.rs:23-45).  Group index = arena_off + (sr - sr0) * ncols + (c - c0).  Written by k_fill_rows once per op — the
 * rows of an op are evaluated ONCE per tile, not once per sub-tile column.
 *
 * Stroke arena: one SLOT per (virtual segment, sub-tile of its window), written by k_stroke_bin: the step ranges of
 * the segment's perpendicular runs for that sub-tile when it can draw there, a hole otherwise.  The slots of one op
 * are contiguous (arena_off .. + rec_cap) and in segment order — no atomics, the layout is a pure function of the
 * scene; `key` = the sub-tile of a slot (0xFFFFFFFF: hole), kept in its own array so that a wave filters 64 slots with
 * one coalesced load. */
struct alignas(16) osmt_srec {
    int32_t p1x, p1y, p2x, p2y;
    double traveled;      /* line.rs:31, before this edge (0 for a cap stub) */
    double denom;         /* center_dist_denom (line.rs:104) */
    double rdenom;        /* 1 / denom, correctly rounded (exact-division shortcut of the walk) */
    int32_t k_lo0, k_lo1; /* main perpendiculars: steps [k_lo, k_lo + k_n) per side */
    int32_t m_lo0, m_lo1; /* extra perpendiculars (line.rs:152-154): events [m_lo, m_lo + n_x) per side */
    uint16_t k_n0, k_n1, n_x0, n_x1; /* <= sub-tile extent + OSMT_REACH_MAX */
};
static_assert(sizeof(osmt_srec) == 64, "osmt_srec is one 64-byte line: four 16-byte stores by k_stroke_bin, four loads by k_raster");

/* What k_opinfo leaves per VIRTUAL SEGMENT (an edge of a stroke op, or one of its two cap stubs; index = op_vseg[op] + running
 * edge, the stubs last) for the binning kernel, as ONE 48-byte record: three 16-byte stores by the op's lane, three loads by the
 * segment's lane.  (Round 6: with k_opinfo no longer queueing behind its atomics, the bytes it writes show — pre-pass of 256
 * config-5 tiles 2.77 -> 2.73 ms, 64 tiles 0.935 -> 0.906, config 2 0.207 -> 0.2055; profiles/r06_n_vseg_aos_stage_times.txt.) */
struct alignas(16) osmt_vseg {
    int32_t p1x, p1y, p2x, p2y; /* p1 == p2: draws nothing (a degenerate edge, line.rs:73-75, or an invalid stub) */
    double trav;                /* traveled before the edge (line.rs:31); 0 for a stub */
    double den, rden;           /* |p2 - p1| = center_dist_denom (line.rs:104) and its correctly rounded reciprocal */
    uint32_t cand_off;          /* first slot (relative to the op) of the segment's sub-tile window */
    uint32_t vop;               /* the op; bit 31: the segment is a cap stub */
};
static_assert(sizeof(osmt_vseg) == 48, "three 16-byte words");

/* Ops with more than 64 edges get one bounding box per block of 64 consecutive edges (running
 * edge index over all rings): k_fill_rows skips the blocks whose rows miss the rows it is working on. */
struct osmt_blk_bbox {
    int32_t x0, y0, x1, y1; /* over the end points of the block's edges (empty block: x0 > x1) */
};

/* ---- per-sub-tile display lists (k_sublist -> k_raster) -----------------------------------------------------------
 * After the binning kernels have set the exact "op draws into sub-tile" bits, k_sublist turns them round: for every
 * (tile, sub-tile) the ops that draw there, in display-list order (= generation order, drawer.rs:218), each with what
 * k_raster needs to start on it resolved for THAT sub-tile.  k_raster then streams its own short list instead of
 * scanning the op bits of the whole tile (config 5: 9000 bits for ~100 drawing ops) and never touches osmt_opinfo. */
struct alignas(16) osmt_ent {
    uint32_t arena;      /* FILL: first word of the 16 coverage words of THIS sub-tile; STROKE: first slot of the op */
    uint32_t kind_color; /* kind | r << 8 | g << 16 | b << 24 */
    double opacity;
    uint32_t aux;        /* STROKE: index into the stroke_aux table; FILL_IMAGE: image id */
    uint32_t nv;         /* STROKE: slots of the op in the stroke arena (rec_cap) */
    uint32_t stage;      /* k_raster's own use while the entry sits in LDS */
    uint32_t _pad;
};
static_assert(sizeof(osmt_ent) == 32, "osmt_ent is two 16-byte loads");

struct osmt_image_desc {
    uint64_t offset; /* first pixel in the image pool (double4 units) */
    uint32_t width, height;
};

/* ---- label pass ------------------------------------------------------ */
/* One Rasterizer::draw_line call, pre-digested (label_seg_prep, font/rasterizer.rs:27-41):
 * everything that does not depend on the stripe y. */
struct osmt_label_seg {
    double x0, y0;
    double slope, slope_recip; /* (x1 - x0) / delta and its f64::recip */
    double y_min, y_max;
    double sign;               /* +1.0 / -1.0 */
    int32_t yf, yl;            /* floor(y_min) as i32 ..= floor(y_max) as i32; yf > yl: delta == 0.0, no-op */
};
static_assert(sizeof(osmt_label_seg) == 64, "osmt_label_seg must be one 64-byte record");

/* One Labeler::label_entity call with its coverage plane: the dense window
 * [cx0, cx0 + cols) x [ry0, ry1] of the Rasterizer's stripes (rows clipped to labels_bb,
 * tile_pixels.rs:67-72; columns cover every key the clipped rows can receive). */
struct osmt_labelinfo {
    uint32_t seg_off, n_segs;
    int32_t ry0, ry1; /* empty (ry0 > ry1): no text pixels can land inside labels_bb */
    int32_t cx0;
    uint32_t cols;
    uint64_t plane_off; /* first cell of the window in the A pool */
    int32_t icon_x, icon_y; /* get_start_coord (labeler.rs:92-95) */
    uint32_t icon_w, icon_h; /* 0 x 0: no icon */
    uint64_t icon_off;       /* first pixel in the image pool (double4 units) */
    uint8_t has_text, color[3];
    /* windows wider than the LDS band: first cell of a 64-stripe S scratch (k_label_cover_wide); all others: first
     * 64-bit word of the label's coverage bit streams (one per band, see osmt_label_band) */
    uint32_t wide_off;
};
static_assert(sizeof(osmt_labelinfo) == 64, "osmt_labelinfo must be one 64-byte record");

/* Accumulator cells (A and S each) one k_label_cover workgroup keeps in LDS: a label's window is processed in
 * bands of OSMT_LABEL_LDS_CELLS / cols stripes; windows with more columns take k_label_cover_wide.  576: with the
 * hand-over buffers a workgroup takes 20 336 B, eight fit a CU (640 cells: seven; measured 448 .. 896, profiles/). */
#ifndef OSMT_LABEL_LDS_CELLS
#define OSMT_LABEL_LDS_CELLS 576
#endif

/* k_label_resolve -> k_raster: a succeeded label that reaches into the tile, with the box to test sub-tiles against */
struct osmt_tile_label {
    int16_t x0, y0, x1, y1;
    uint32_t label;
    uint32_t _pad;
};

/* One k_label_cover wave: OSMT_LABEL_LDS_CELLS / cols stripes of one label's window, starting at stripe `rbase`.  Stripes
 * never share a cell, so the bands of a label are independent waves; the list is ordered by falling work
 * (draw_line calls to scan), so that the longest bands start first and the kernel does not end on one straggler. */
struct osmt_label_band {
    uint32_t label, rbase;
};
/* Besides the f64 totals a band leaves ONE BIT per cell (total > 0) for k_label_resolve, in cell order, 64 cells
 * per word; band b of a label starts at word wide_off + b * osmt_label_band_words(cols). */
__host__ __device__ static inline uint32_t osmt_label_band_rows(uint32_t cols) {
    const uint32_t r = OSMT_LABEL_LDS_CELLS / cols;
    return r < 64u ? r : 64u;
}
__host__ __device__ static inline uint32_t osmt_label_band_words(uint32_t cols) { return (osmt_label_band_rows(cols) * cols + 63u) / 64u; }

struct osmt_label_launch {
    const osmt_labelinfo* info;
    const osmt_label_band* bands;
    uint32_t n_bands;
    uint32_t n_labels, n_jobs, scale, n_wide;
    const uint32_t* job_label_off;
    const double* segs;
    const uint32_t* wide; /* labels that need k_label_cover_wide */
    double* plane_a;
    unsigned long long* cell_bits; /* coverage bit streams (osmt_label_band_words) */
    double* plane_s_wide;
    uint32_t* bitmap; /* scale > 1 only */
    uint8_t* ok;
    uint32_t* err;
    osmt_tile_label* tile_labels;
    uint32_t* tile_label_cnt;
};

struct osmt_label_args {
    const osmt_labelinfo* info; /* [n_labels] */
    uint32_t n_labels;
    const uint32_t* job_label_off; /* [n_jobs + 1] */
    const osmt_tile_label* tile_labels; /* [n_labels], tile i's entries start at job_label_off[i] (k_label_resolve) */
    const uint32_t* tile_label_cnt;     /* [n_jobs] */
    const double* plane;           /* A pool after k_label_cover: min(a + s_acc, 1.0) per cell, 0 where no key */
};

/* glyph-run labels (osmt_glyphs.hip): one (label, glyph instance) pair per wave, pairs in label order */
struct osmt_glyph_pass {
    const osmt_glyph_vertex* verts; /* the context's glyph table snapshot */
    const uint32_t* voff;           /* [n_glyphs + 1] */
    const osmt_glyph_instance* inst;
    const uint32_t* pair_inst;  /* [n_pairs] instance of the pair */
    const uint32_t* pair_label; /* [n_pairs] its label */
    uint32_t n_pairs;
    int32_t W;                 /* tile width in pixels */
    osmt_label_extent* sum;    /* [n_labels] per-label window summary (count pass) */
    uint32_t* pair_cnt;        /* [n_pairs] draw_line calls of the pair (count pass) */
    uint32_t* pair_base;       /* [n_pairs] exclusive scan inside blocks of 1024 pairs */
    uint32_t* blk;             /* [n_pairs / 1024 + 1] block totals -> their exclusive scan */
    uint32_t* err;             /* OSMT_GLYPH_ERR_* */
    double* segs;              /* emit pass: the label pass's draw_line arena, n_segs calls */
    uint32_t n_segs;
};

/* SMALL batches (the one-tile request, a gathered worker group): a tile with at most this many ops gets no per-sub-tile lists
 * from k_sublist — one word of op bits per lane (two rounds) and a ballot give a sub-tile wave its list in op order directly,
 * and a launch (8 us of a 105 us request) is saved.  Big batches keep the lists: there the scattered reads of the op bits by
 * 131 072 waves cost k_raster more (0.615 -> 0.670 ms on config 2) than the list kernel does (0.032 ms). */
#define OSMT_FOLD_MAX_OPS 128u
#define OSMT_FOLD_MAX_JOBS 64u

struct osmt_raster_args {
    const osmt_tile_job* jobs;
    uint32_t n_jobs;
    uint32_t scale;
    const osmt_stroke_aux* aux;
    const osmt_dash_seg* dseg; /* [stroke][OSMT_MAX_DASH_SEGS]: DashSegments of the `main` calculators (dashed ops only) */
    const uint2* hdr;        /* [n_jobs][nsub]: (first entry, entry count) of the sub-tile's list (k_sublist) */
    const osmt_ent* ent;     /* the lists */
    const uint32_t* fmask;   /* fill arena (words) */
    const osmt_srec* srec;   /* stroke arena */
    /* tiles of at most fold_max_ops ops have no lists: their sub-tile waves read the op bits and the op records themselves */
    uint32_t fold_max_ops;   /* 0: every tile has lists */
    uint32_t _pad1;
    const osmt_opinfo* info;
    const uint32_t* submask; /* [op][sub-tile row]: bit sx = the op draws into sub-tile (sx, row) */
    const uint2* skey;       /* per stroke slot: (its sub-tile sy * subs_per_row + sx, or 0xFFFFFFFF for a hole; item count | cap flag << 31) */
    const osmt_image_desc* images;
    const double4* image_pool;
    uint32_t n_images;
    uint32_t out_rgb8;       /* 1: packed RGB8 (the memory of to_rgb_triples' Vec<(u8, u8, u8)>) instead of RGBA8; tile stride a multiple of 4 */
    void* out;
    size_t out_tile_stride; /* bytes (RGBA8 / RGB8 output) */
    osmt_label_args labels;  /* info == NULL: no label pass */
};

/* The per-op pre-pass and the two binning kernels (stage 2). */
struct osmt_prepass_args {
    const osmt_tile_job* jobs;
    uint32_t n_jobs;
    const osmt_op* ops;
    uint32_t n_ops;
    const osmt_ring* rings;
    const int2* pts;
    const double* dashes;
    const uint32_t* op_aux;   /* op -> stroke slot */
    const uint32_t* op_job;   /* op -> job */
    const uint32_t* op_blk;   /* op -> first 64-edge block bbox (0xFFFFFFFF: none) */
    const uint32_t* op_vseg;  /* op -> its first virtual segment (stroke ops that have segments) */
    uint32_t n_vsegs;
    uint32_t scale;
    uint32_t sub_rows;
    uint32_t max_job_ops;  /* most ops of any tile */
    uint32_t fold_max_ops; /* tiles of at most this many ops get no lists (0: all do); max_job_ops <= fold_max_ops = no k_sublist launch */
    osmt_opinfo* info;
    osmt_stroke_aux* aux;
    osmt_dash_seg* dseg; /* [stroke][OSMT_MAX_DASH_SEGS] */
    osmt_blk_bbox* blk;
    uint32_t* submask;
    /* per VIRTUAL SEGMENT (index = op_vseg[op] + running edge index, so ops that share rings do not collide): what the binning
     * kernel needs of an edge / cap stub in ONE record, one level of loads (round 3 went vseg -> table slot -> op -> opinfo ->
     * osmt_op -> ring -> points; rounds 4-5 kept six arrays: six scattered partial-line stores per edge) */
    osmt_vseg* vseg;
    unsigned long long* cursors; /* [0] fill arena (64-byte groups), [1] stroke arena (records), [2] list entries, [3] fill slots
                                  * (osmt_fill_slots.h; four times the pass count of k_prebin's fill role); zeroed by the launcher */
    osmt_fill_slot* slots;       /* [slot_cap] one descriptor per (fill op, sub-tile row of its window), written by k_opinfo */
    unsigned long long slot_cap; /* a multiple of four; 0 in the sizing pass (only the cursor is produced) */
    uint32_t n_fill_pass;        /* passes of k_prebin's fill role where the sizing run counted them (the launcher makes its fill blocks
                                  * from this count), else 0: ceil(n_ops / 2) blocks that stride through the passes the cursor shows */
    uint32_t* cnt;      /* [n_jobs][nsub], right behind the cursors (zeroed with them): ops that draw into the sub-tile; behind the
                         * counts, zeroed with them, the cursors of the list arena's slices (osmt_list_slices.h) */
    uint2* hdr;         /* [n_jobs][nsub]: k_sublist's (first entry, count) */
    osmt_ent* ent;      /* list arena: osmt_list_layout_make(n_jobs, ent_cap).total entries */
    unsigned long long ent_cap; /* list entries the binning can produce */
    uint32_t* fmask;
    osmt_srec* srec;
    uint2* skey;
    unsigned long long fmask_cap, srec_cap; /* arena capacities (groups / records); 0 = sizing pass: only the cursors are produced */
    /* host-mapped (pinned, coherent) word of the scene, or NULL: a kernel whose arena reservation does not fit — it cannot,
     * the arenas are sized by the same code; a future change to the binning that breaks the invariant must not show as
     * silently blank tiles — stores an OSMT_PREPASS_ERR_* code here, the host looks at it after its own synchronisation */
    uint32_t* err;
};
#define OSMT_PREPASS_ERR_FILL_ARENA 1u
#define OSMT_PREPASS_ERR_STROKE_ARENA 2u
#define OSMT_PREPASS_ERR_LIST_ARENA 4u

/* ---- label anchors (osmt_polylabel.hip) ----------------------------------------------------------------------- */
/* one request as the kernels read it */
struct osmt_pl_req {
    uint32_t ring_off, n_rings;
    uint32_t keep_off; /* first word of the request's slice of `keep` (n_rings words: the rings filter_polygons keeps, the largest first) */
    uint32_t _pad;
    double scale;
};
static_assert(sizeof(osmt_pl_req) == 24, "osmt_pl_req");

#define OSMT_PL_GLOBAL_CELLS OSMT_LABEL_MAX_CELLS /* queue capacity of the second tier = the cap of the contract */
#define OSMT_PL_CELL_DOUBLES 5u                   /* centre x, y, half size, fitness, max fitness */
#define OSMT_PL_ERR_HEAP 1u   /* a sift walked more levels than a heap of 2^32 cells has */
#define OSMT_PL_ERR_KEEP 2u   /* the kept-ring list names a ring outside the table */
#define OSMT_PL_ERR_GRID 4u   /* the grid walk outran the queue cap without a push failing */
#define OSMT_PL_ERR_LIST 8u   /* the second tier took more rounds than there are requests */
#define OSMT_PL_ERR_TIER1 16u /* (where: first / second tier) */
#define OSMT_PL_ERR_TIER2 32u
#define OSMT_PL_MAX_SLOTS 64u                     /* second-tier queues (2.6 MB each) a call allocates at most */

struct osmt_polylabel_args {
    const osmt_pl_req* req;
    uint32_t n_req;
    const osmt_ring* rings;
    uint32_t n_rings;
    const double2* pts;
    uint32_t* keep;           /* [sum of n_rings] */
    osmt_label_position* out; /* [n_req] */
    uint32_t* over;           /* [n_req] requests whose queue outgrew the LDS tier, in no particular order */
    uint32_t* cnt;            /* [0] entries of `over`, [1] the second tier's cursor into it, [2] requests answered TOO_LARGE, [3] OSMT_PL_ERR_*; zeroed by the launcher */
    double* ws;               /* [n_slots][OSMT_PL_CELL_DOUBLES][OSMT_PL_GLOBAL_CELLS] */
    uint32_t n_slots;
};
/* zeroes cnt, then k_polylabel (one wave per request, queue in LDS) and k_polylabel_big (n_slots waves work through `over`) */
hipError_t osmt_launch_polylabel(const osmt_polylabel_args& a, hipStream_t st);

/* zero / n_zero (optional): 32-bit words the kernel clears on the way — the cursors and list counts of the pre-pass that follows */
hipError_t osmt_launch_project(const osmt_tile_job* jobs, const uint32_t* pt_job, const double* latlon, const uint32_t* refs,
                               uint32_t n_pts, double scale, int32_t* pts, hipStream_t st, uint32_t* zero = nullptr, size_t n_zero = 0);
size_t osmt_prepass_zero_words(const osmt_prepass_args& a);
/* point -> job table on the device: pt_job[i] = j for the points of job j, 0xFFFFFFFF for points no job owns */
hipError_t osmt_launch_ptjob(const osmt_tile_job* jobs, uint32_t n_jobs, uint32_t* pt_job, uint32_t n_pts, hipStream_t st);
hipError_t osmt_launch_project_single(const double* latlon, uint32_t n, uint32_t zoom, uint32_t tx, uint32_t ty,
                                      double scale, int32_t* pts, hipStream_t st);
/* k_opinfo -> k_fill_rows -> k_stroke_bin on `st` (sizing pass: k_opinfo only) */
hipError_t osmt_launch_prepass(const osmt_prepass_args& a, hipStream_t st, bool zeroed = false);
hipError_t osmt_launch_raster(const osmt_raster_args& a, bool out_f64, hipStream_t st);
/* label pass: cover (one wave per label) -> resolve (one workgroup per tile, labels in order) */
hipError_t osmt_launch_labels(const osmt_label_launch& a, hipStream_t st);
/* glyph-run labels: k_glyph_init + k_glyph_count (window summaries, pair counts, error word) */
hipError_t osmt_launch_glyph_count(const osmt_glyph_pass& a, uint32_t n_labels, hipStream_t st);
/* the scan of the pair counts + k_glyph_emit (draw_line calls into a.segs) */
hipError_t osmt_launch_glyph_emit(const osmt_glyph_pass& a, hipStream_t st);
/* text-run labels (osmt_textplace.hip): one label per wave; the batch has passed osmt::validate_text_labels */
struct osmt_text_pass {
    const osmt_label* labels;
    uint32_t n_labels;
    const osmt_text_run* runs;     /* [n_labels] */
    const osmt_text_glyph* glyphs; /* a label's text: glyphs[seg_off .. seg_off + n_segs) */
    const int32_t* way_pts;        /* [n_way_pts][2] */
    const double* way_sincos;      /* [n_way_pts][2] */
    osmt_glyph_instance* inst;     /* out: slot seg_off + k = glyph k of its label */
};
/* k_text_place: TextPlacer::place of every label with text, glyph instances into a.inst */
hipError_t osmt_launch_text_place(const osmt_text_pass& a, hipStream_t st);
/* string labels (osmt_textshape.hip): a registered font as the kernel reads it.  The tables of a font are uploaded once
 * and never move; only the array of these records is replaced when a font is appended. */
struct osmt_font_dev {
    const osmt_cmap_entry* cmap;
    const int32_t* advance;     /* [n_glyphs] */
    const uint32_t* outline;    /* [n_glyphs] ids in the glyph table */
    const osmt_kern_pair* kern; /* NULL when n_kern == 0 */
    uint32_t n_cmap, n_kern, n_glyphs, _pad;
};
/* one char per lane, over the (slot, label) pairs of the glyph expansion; the batch has passed osmt::validate_string_labels */
struct osmt_shape_pass {
    const osmt_label* labels;
    const uint32_t* label_font; /* [n_labels] font id (read for the labels the pairs name) */
    const uint32_t* pair_inst;  /* [n_pairs] slot of the pair = index into chars and out */
    const uint32_t* pair_label; /* [n_pairs] its label */
    uint32_t n_pairs;
    const uint32_t* chars;
    const osmt_font_dev* fonts; /* the context's font table snapshot */
    osmt_text_glyph* out;       /* slot seg_off + k = char k of its label */
};
/* k_text_shape: TextPlacer::text_to_glyphs of every label with text, osmt_text_glyph records into a.out */
hipError_t osmt_launch_text_shape(const osmt_shape_pass& a, hipStream_t st);
/* ---- display lists built on the device (osmt_styled.hip) ------------------------------------------------------- */
/* a registered geodata file as the kernels read it: one allocation that never moves */
struct osmt_geo_dev {
    const double* nodes;      /* [n_nodes][2] */
    const uint64_t* way_gid;  /* [n_ways] */
    const uint64_t* mp_gid;   /* [n_mps] */
    const uint32_t* way_off;  /* [n_ways + 1] into idx */
    const uint32_t* poly_off; /* [n_polys + 1] into idx (the polygons' nodes sit behind the ways': already shifted) */
    const uint32_t* mp_off;   /* [n_mps + 1] into mp_polys */
    const uint32_t* mp_polys; /* polygon indices */
    const uint32_t* idx;      /* node indices: the ways', then the polygons' */
    const uint2* mp_sum;      /* [n_mps]: (rings of >= 2 nodes, their nodes in all), summed once at registration */
};

/* what is counted per (tile, pass, area) element and scanned in that order */
enum { OSMT_SQ_OPS = 0, OSMT_SQ_RINGS, OSMT_SQ_REFS, OSMT_SQ_DASHES, OSMT_SQ_STROKES, OSMT_SQ_BLOCKS, OSMT_SQ_VSEGS, OSMT_SQ_N };
#define OSMT_STYLED_TOTALS (OSMT_SQ_N + 1) /* the totals of the scans + the most ops of any tile */

struct osmt_styled_pass {
    osmt_geo_dev geo;
    const osmt_style_rec* styles;
    const uint32_t* style_rank; /* [n_styles]: dense rank under (layer or 0, is_foreground_fill, z_index); equal keys, equal rank */
    const double* style_dashes; /* the styles' pool, unscaled */
    const osmt_styled_tile* tiles;
    const uint32_t* tile_base; /* [n_tiles + 1]: areas of the tiles in front (the tiles' ranges may lie anywhere in `areas`) */
    const osmt_styled_area* areas;
    uint32_t n_tiles;
    uint32_t n_elems; /* 3 * tile_base[n_tiles]: element (t, p, k) = 3 * tile_base[t] + p * n_areas(t) + k */
    uint32_t scale, use_caps;
    /* work areas */
    ulonglong2* keys;         /* [tile_base[n_tiles]]: the sort keys of tiles beyond the LDS tier */
    uint32_t* sorted;         /* [tile_base[n_tiles]]: absolute area index, tile by tile in draw order */
    uint32_t* pre;            /* [OSMT_SQ_N][n_elems + 1]: counts, then their exclusive scans (mod 2^32: exact once the totals fit) */
    unsigned long long* blk;  /* [OSMT_SQ_N][blocks of 256 elements]: block totals, then their exclusive scan */
    unsigned long long* totals; /* [OSMT_STYLED_TOTALS] */
    /* the scene's arrays (emit pass) */
    osmt_tile_job* jobs;
    osmt_op* ops;
    osmt_ring* rings;
    uint32_t* refs;
    double* dashes;
    uint32_t *op_job, *op_aux, *op_blk, *op_vseg;
    uint32_t* ring_src; /* [n_rings]: where in geo.idx a ring's nodes start */
    uint32_t n_rings, n_refs;
};
/* k_styled_sort -> k_styled_count -> k_styled_scan_blocks -> k_styled_scan_apply -> k_styled_tilemax: everything up to the totals */
hipError_t osmt_launch_styled_count(const osmt_styled_pass& a, hipStream_t st);
/* k_styled_emit -> k_styled_jobs -> k_styled_refs */
hipError_t osmt_launch_styled_emit(const osmt_styled_pass& a, hipStream_t st);

/* ---- scenes built from tile coordinates (osmt_tilequery.hip) --------------------------------------------------- */
/* a registered z18 tile index as the kernels read it: one allocation that never moves.  The tiles are sorted by (x, y), so a
 * column (one x) is a contiguous run of them and its tiles' reference lists are ONE contiguous slice of each pool. */
struct osmt_tq_index_dev {
    const uint32_t* col_x;     /* [n_cols] the distinct x, ascending (the column directory, built at registration) */
    const uint32_t* col_first; /* [n_cols + 1] first index tile of the column */
    const uint32_t* tile_y;    /* [n_tiles] */
    const uint32_t* way_off;   /* [n_tiles + 1] into ways */
    const uint32_t* ways;
    const uint32_t* mp_off;    /* [n_tiles + 1] into mps */
    const uint32_t* mps;
    uint32_t n_cols, n_tiles;
    uint32_t level; /* the zoom of its tiles: OSMT_MAX_ZOOM for the registered index, L for level L of its pyramid */
};
/* a registered bindings table: entity -> its style ids, in push order */
struct osmt_tq_bind_dev {
    const uint32_t *way_off, *way_styles, *mp_off, *mp_styles;
};
/* words of osmt_tq_pass::tot */
enum {
    OSMT_TQ_ITEMS = 0,  /* (tile, column) items */
    OSMT_TQ_WAYS,       /* way candidates */
    OSMT_TQ_MPS,        /* multipolygon candidates */
    OSMT_TQ_MAX_CAND,   /* the largest per-tile count of either kind */
    OSMT_TQ_OVER_CAND,  /* the first tile with more than OSMT_QUERY_MAX_TILE_CANDIDATES of one kind (none: all ones) */
    OSMT_TQ_AREAS,      /* areas */
    OSMT_TQ_MAX_AREAS,  /* the most areas of any tile */
    OSMT_TQ_OVER_AREAS, /* the first tile with more than OSMT_STYLED_MAX_TILE_AREAS (none: all ones) */
    OSMT_TQ_N
};
struct osmt_tq_pass {
    osmt_tq_index_dev ix; /* the registered z18 index: what every tile reads while ixz is NULL */
    /* [OSMT_MAX_ZOOM + 1], device memory: the index a tile of each zoom reads — the smallest level >= the zoom of the geodata's
     * pyramid (osmt_tilepyramid.hip), the z18 index where there is none.  NULL: no pyramid, every kernel reads `ix` and computes
     * what it computed before there were levels.  A tile's items slice the pools of its zoom's index. */
    const osmt_tq_index_dev* ixz;
    const uint32_t* geo_mp_off;  /* osmt_geo_dev::mp_off: a multipolygon without polygons is dropped */
    const osmt_tq_bind_dev* bind; /* [OSMT_MAX_ZOOM + 1] the bindings of each zoom (zooms no tile has: never read) */
    const osmt_query_tile* q;     /* [n_tiles] */
    /* the planes of a registered id filter (osmt_idfilter.hip), bit `id` of word id / 32; NULL: no filter.  A candidate whose bit
     * is 0 counts nothing: the filter is the last drop, behind the repeats and the multipolygons without polygons */
    const uint32_t *keep_way, *keep_mp;
    uint32_t n_tiles, n_items, n_ways, n_mps; /* the last three: totals, known once they have been read back */
    /* per tile */
    uint32_t* span_c0;   /* [n_tiles] first present column of the tile's rectangle */
    uint32_t* item_base; /* [n_tiles + 1] span widths, then their exclusive scan: the tile's (tile, column) items */
    uint32_t* t_wbase;   /* [n_tiles + 1] way candidates of the tiles in front */
    uint32_t* t_mbase;   /* [n_tiles + 1] */
    /* per item */
    uint32_t* item_tile;
    uint32_t *item_wsrc, *item_msrc; /* where in ix.ways / ix.mps the item's slice starts */
    uint32_t *wbase, *mbase;         /* [n_items + 1] slice lengths, then their exclusive scans */
    /* per candidate; a tile's ways, then its multipolygons, tile by tile: slot = t_wbase[t] + t_mbase[t] (+ way count) + k */
    uint32_t* cand; /* ids: gathered, sorted in place per (tile, kind) */
    uint32_t* apos; /* [n_ways + n_mps + 1] areas of the candidate (0 for a repeat), then their exclusive scan */
    /* scans */
    unsigned long long* blk; /* block totals of the scan under way */
    unsigned long long* tot; /* [OSMT_TQ_N] */
    /* the derived styled batch */
    osmt_styled_tile* tiles;
    uint32_t* tile_base; /* [n_tiles + 1] */
    osmt_styled_area* areas;
};
/* k_tq_span + scan: the tiles' column ranges, tot[OSMT_TQ_ITEMS] */
hipError_t osmt_launch_tq_span(const osmt_tq_pass& a, hipStream_t st);
/* k_tq_columns + two scans + k_tq_tilecand: per-item slices, per-tile candidate counts, the first read-back's words */
hipError_t osmt_launch_tq_columns(const osmt_tq_pass& a, hipStream_t st);
/* k_tq_gather (both kinds) */
hipError_t osmt_launch_tq_gather(const osmt_tq_pass& a, hipStream_t st);
/* k_tq_sort (one workgroup per tile and kind) */
hipError_t osmt_launch_tq_sort(const osmt_tq_pass& a, hipStream_t st);
/* k_tq_mark + scan + k_tq_tiles: area positions, styled tiles, tile_base, the second read-back's words */
hipError_t osmt_launch_tq_mark(const osmt_tq_pass& a, hipStream_t st);
/* k_tq_emit: the styled areas */
hipError_t osmt_launch_tq_emit(const osmt_tq_pass& a, hipStream_t st);

/* ---- the tile index pyramid (osmt_tilepyramid.hip) ------------------------------------------------------------- */
#define OSMT_PYR_SORT_BLOCK 1024u /* pairs one workgroup of the sort takes */
#define OSMT_PYR_DIGITS 9u        /* 8-bit digits of a pair: 0..3 of the id, 4..8 of the 36-bit key (x << 18 | y) */
/* one kind's lists of the finer index a level is built from (the registered index, or a level): n_refs = off[n_tiles], read
 * back by the host; a source of references has at least one tile, and a tile at least one column */
struct osmt_pyr_src {
    const uint32_t *col_x, *col_first, *tile_y, *off, *pool;
    uint32_t n_cols, n_tiles, n_refs;
    uint32_t shift; /* a parent coordinate = the source's >> shift */
};
/* k_pyr_pairs: key[r], id[r] of every reference r < s.n_refs */
hipError_t osmt_launch_pyr_pairs(const osmt_pyr_src& s, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_pyr_tilekeys: (parent key, 0) of every source tile */
hipError_t osmt_launch_pyr_tilekeys(const osmt_pyr_src& s, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_pyr_digits: hist[OSMT_PYR_DIGITS][256] of n pairs (zeroed here) */
hipError_t osmt_launch_pyr_digits(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t* hist, hipStream_t st);
/* A pass sorts on any digit below OSMT_PYR_PASS_DIGITS: 4 + b is byte b of the key, b = 0..7.  The histogram above stops at
 * OSMT_PYR_DIGITS because its callers' keys have 36 bits; a caller whose key is any 64 bits and whose ids already ascend
 * (the id resolution, osmt_resolve.hip) takes k_pyr_keydigits instead: hist[OSMT_PYR_KEY_DIGITS][256] of the key's bytes
 * alone (zeroed here), row b for pass digit 4 + b. */
#define OSMT_PYR_KEY_DIGITS 8u
#define OSMT_PYR_PASS_DIGITS 12u
hipError_t osmt_launch_pyr_keydigits(const unsigned long long* key, uint32_t n, uint32_t* hist, hipStream_t st);
/* one stable pass over `digit`: k_pyr_hist -> osmt_tq_scan -> k_pyr_scatter.  counts: 256 * blocks + 1 words, blk: blocks + 1,
 * with blocks = ceil(n / OSMT_PYR_SORT_BLOCK); tot: one word */
hipError_t osmt_launch_pyr_pass(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t digit, uint32_t* counts, unsigned long long* blk,
                                unsigned long long* tot, unsigned long long* out_key, uint32_t* out_id, hipStream_t st);
/* k_pyr_mark + scans over sorted pairs: pos[n + 1] numbers the distinct pairs (tot[0]); cpos[n + 1] (or NULL) the distinct x
 * (tot[1]); blk: n / 256 + 1 words */
hipError_t osmt_launch_pyr_mark(const unsigned long long* key, const uint32_t* id, uint32_t n, uint32_t* pos, uint32_t* cpos, unsigned long long* blk,
                                unsigned long long* tot, hipStream_t st);
/* the level's tiles and column directory from the tiles' job: tile_x, tile_y [n_tiles], col_x [n_cols], col_first [n_cols + 1] */
hipError_t osmt_launch_pyr_emit_tiles(const unsigned long long* key, uint32_t n, const uint32_t* pos, const uint32_t* cpos, uint32_t n_tiles, uint32_t n_cols,
                                      uint32_t* tile_x, uint32_t* tile_y, uint32_t* col_x, uint32_t* col_first, hipStream_t st);
/* one kind's lists from its job: off [n_tiles + 1], pool [pos[n]]; tile_x, tile_y: what osmt_launch_pyr_emit_tiles wrote */
hipError_t osmt_launch_pyr_emit_lists(const unsigned long long* key, const uint32_t* id, uint32_t n, const uint32_t* pos, const uint32_t* tile_x,
                                      const uint32_t* tile_y, uint32_t n_tiles, uint32_t* off, uint32_t* pool, hipStream_t st);

/* ---- the z18 tile index built from geometry (osmt_tileindex.hip) ------------------------------------------------- */
/* words of osmt_tix_pass::words */
enum {
    OSMT_TIX_OFFENDER = 0, /* the lowest 2 * node + axis (0: x, 1: y) whose factor is exactly 1.0; none: all ones */
    OSMT_TIX_WAY_REFS,     /* the exact (tile, way) total */
    OSMT_TIX_MP_REFS,      /* the exact (tile, multipolygon) total */
    OSMT_TIX_SCAN,         /* the total of the scan under way (saturated counts: not read back) */
    OSMT_TIX_WORDS
};
struct osmt_tix_pass {
    osmt_geo_dev geo;
    const double2* factors; /* [n_nodes] */
    uint32_t n_nodes, n_ways, n_polys, n_mps, n_way_nodes, n_poly_nodes, n_mp_polys;
    uint32_t *tx, *ty;                  /* [n_nodes] the nodes' tiles */
    uint4 *way_box, *poly_box, *mp_box; /* {min_x, max_x, min_y, max_y}; {~0, 0, ~0, 0}: no node */
    uint32_t *way_cnt, *mp_cnt;         /* [n + 1] tiles of the entity (saturated), then their exclusive scan */
    unsigned long long* blk;            /* max(n_ways, n_mps) / 256 + 1 words */
    unsigned long long* words;          /* [OSMT_TIX_WORDS] */
};
/* k_tix_init, k_tix_node_tiles, k_tix_bbox (ways, polygons), k_tix_mp_bbox, k_tix_count + scan (ways, multipolygons):
 * everything up to the words the host reads back */
hipError_t osmt_launch_tix_boxes(const osmt_tix_pass& a, hipStream_t st);
/* k_tix_pairs: the n_refs = off[n_ent] (key, entity) pairs of one kind */
hipError_t osmt_launch_tix_pairs(const uint32_t* off, uint32_t n_ent, const uint4* box, uint32_t n_refs, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_tix_node_pairs: (key of the node's tile, node) */
hipError_t osmt_launch_tix_node_pairs(const uint32_t* tx, const uint32_t* ty, uint32_t n, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_tix_keymark + scan over n sorted pairs: head[n + 1] numbers the distinct keys, *tot their count; blk: n / 256 + 1 words */
hipError_t osmt_launch_tix_keymark(const unsigned long long* key, uint32_t n, uint32_t* head, unsigned long long* blk, unsigned long long* tot, hipStream_t st);
/* k_tix_keycompact: (distinct key, 0) into out_key / out_id [head[n]] */
hipError_t osmt_launch_tix_keycompact(const unsigned long long* key, uint32_t n, const uint32_t* head, unsigned long long* out_key, uint32_t* out_id,
                                      hipStream_t st);

/* ---- multipolygon rings from relations' member ways (osmt_polygons.hip) ------------------------------------------ */
/* words of osmt_mpa_pass::words */
enum {
    OSMT_MPA_SEGMENTS = 0, /* the exact segment total */
    OSMT_MPA_SCAN,         /* the total of the way references' scan (equal to the above when it fits 32 bits) */
    OSMT_MPA_MPS,          /* accepted relations */
    OSMT_MPA_POLYS,        /* their rings */
    OSMT_MPA_NODES,        /* their polygon nodes */
    OSMT_MPA_WORDS
};
struct osmt_mpa_pass {
    /* the caller's arrays on the device */
    const ulonglong2* node_bits; /* [n_nodes] the bits of (lat, lon) */
    const uint32_t *way_off, *way_nodes, *rel_way_off, *rel_ways;
    const uint8_t* rel_inner;
    const uint64_t* rel_ids;
    uint32_t n_nodes, n_ways, n_rels, n_refs;
    uint32_t* ref_off;  /* [n_refs + 1] segments of a way reference, then their exclusive scan */
    uint32_t* rel_seg;  /* [n_rels + 1] a relation's first segment */
    uint32_t *rel_acc, *rel_rings, *rel_nodes; /* [n_rels + 1] what the walk found, then their exclusive scans */
    unsigned long long *blk, *words; /* max(n_refs, n_rels) / 256 + 1 words; [OSMT_MPA_WORDS] */
    /* sized once the segment total is known; e = 2 * segment + side is an endpoint */
    uint32_t n_segs;
    uint32_t hash_bits, table_mask; /* osmt_debug_vertex_hash_bits; slots - 1 */
    uint32_t* seg_nodes; /* [2 * n_segs] the node of an endpoint */
    uint32_t* seg_rel;   /* [n_segs] */
    uint8_t* seg_state;  /* [n_segs] role | 2 while the segment is available */
    uint32_t* table;     /* [table_mask + 1] lowest endpoint of a (relation, position) */
    uint32_t* canon;     /* [2 * n_segs] the vertex of an endpoint: the lowest endpoint of its relation at its position */
    uint2* ent;          /* [2 * n_segs] sorted adjacency: {endpoint, vertex of its other side}, both less the relation's 2 * first segment */
    uint32_t* gstart;    /* [2 * n_segs] by endpoint: where its list starts if it is a vertex, else all ones; relation-local */
    uint32_t* stamp;     /* [2 * n_segs] by vertex: the serial of the last ring that used it */
    uint32_t* ring_seg;  /* [n_segs] the segments of a relation's rings in walk order, relation-local */
    uint32_t* ring_end;  /* [n_segs / 3 + 1] at n_first_segment / 3 + k: segments walked when ring k closed */
    osmt_relation_status* status; /* [n_rels] */
    /* the result */
    uint32_t *poly_node_off, *poly_nodes, *mp_poly_off, *mp_polys, *mp_rel;
    uint64_t* mp_ids;
};
/* k_mpa_count + scan + k_mpa_reloff: ref_off, rel_seg and words[OSMT_MPA_SEGMENTS] (words zeroed here) */
hipError_t osmt_launch_mpa_count(const osmt_mpa_pass& a, hipStream_t st);
/* k_mpa_segments, k_mpa_fill + k_mpa_vertices + k_mpa_canon: segments, the vertex table, canon and the (vertex, endpoint)
 * pairs to sort */
hipError_t osmt_launch_mpa_vertices(const osmt_mpa_pass& a, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_mpa_adjacency over the sorted pairs, k_mpa_walk, the scans of what it found */
hipError_t osmt_launch_mpa_walk(const osmt_mpa_pass& a, const unsigned long long* key, const uint32_t* id, hipStream_t st);
/* k_mpa_emit: the five arrays and mp_rel */
hipError_t osmt_launch_mpa_emit(const osmt_mpa_pass& a, hipStream_t st);

/* ---- OSM ids resolved to local indices (osmt_resolve.hip) -------------------------------------------------------- */
#define OSMT_RES_SHORT_WAY_CAP 1024u    /* the most osmt_debug_resolve_short_way_max takes: 24 KiB of LDS for one wave */
#define OSMT_RES_SHORT_WAY_DEFAULT 256u /* ways up to this many resolved references find their repeats in LDS */
/* one kind's references on their way from global ids to local indices: ways' node references, or relations' way members */
struct osmt_res_refs {
    const unsigned long long* table_key; /* [n_table] the elements' global ids, sorted; equal ids in index order */
    const uint32_t* table_id;            /* [n_table] their indices */
    uint32_t n_table;
    const uint32_t* off;             /* [n_owners + 1] into refs */
    const uint32_t* seen;            /* [n_owners] elements an owner's references may resolve to, or NULL: n_table */
    const unsigned long long* refs;  /* [n_refs] global ids */
    const uint8_t* role;             /* [n_refs] carried along, or NULL */
    uint32_t n_owners, n_refs;
    uint32_t* local;  /* [n_refs] the index a reference resolves to, all ones: none */
    uint32_t* pos;    /* [n_refs + 1] 1: resolved, then its exclusive scan */
    uint32_t* out_off;   /* [n_owners + 1] */
    uint32_t* out_local; /* [pos[n_refs]] */
    uint8_t* out_role;   /* [pos[n_refs]], or NULL */
    unsigned long long *blk, *tot; /* n_refs / 256 + 1 words; one word: references resolved */
};
/* id[i] = i for i < n: the indices of a table before its sort */
hipError_t osmt_launch_res_iota(uint32_t* id, uint32_t n, hipStream_t st);
/* k_res_translate + scan + k_res_compact: local, pos, out_off, out_local, out_role, *tot */
hipError_t osmt_launch_res_translate(const osmt_res_refs& a, hipStream_t st);
/* the dedup of the ways' resolved references: off [n_ways + 1], refs [off[n_ways]] as osmt_launch_res_translate wrote them */
struct osmt_res_dedup {
    const uint32_t *off, *refs;
    uint32_t n_ways, short_max; /* osmt_debug_resolve_short_way_max */
    uint32_t* keep;             /* [n_refs_cap + 1] 1: kept, then its exclusive scan */
    uint32_t* long_pos;         /* [n_ways + 1] pairs a way sends through the sort, then their exclusive scan */
    unsigned long long *blk, *tot; /* max(n_refs_cap, n_ways) / 256 + 1 words; tot[0]: pairs to sort, tot[1]: references kept */
};
/* k_res_short (one wave per way of up to short_max references, LDS) and k_res_longcount + scan: keep of the short ways and of
 * every position 0, long_pos, tot[0] */
hipError_t osmt_launch_res_short(const osmt_res_dedup& a, hipStream_t st);
/* k_res_longpairs: key = min << 32 | max, id = the position in refs, of the n_pairs = tot[0] pairs of the long ways */
hipError_t osmt_launch_res_longpairs(const osmt_res_dedup& a, uint32_t n_pairs, unsigned long long* key, uint32_t* id, hipStream_t st);
/* k_res_longmark over the sorted pairs (none: nothing), then the scan of keep over n_refs references: tot[1] */
hipError_t osmt_launch_res_mark(const osmt_res_dedup& a, uint32_t n_pairs, const unsigned long long* key, const uint32_t* id, uint32_t n_refs, hipStream_t st);
/* k_res_emit: out_off [n_ways + 1], out_nodes [tot[1]] */
hipError_t osmt_launch_res_emit(const osmt_res_dedup& a, uint32_t n_refs, uint32_t* out_off, uint32_t* out_nodes, hipStream_t st);

/* ---- the id filter (osmt_idfilter.hip) -------------------------------------------------------------------------- */
/* k_idf_plane: bit e of `plane` = gid[e] is in ids[0 .. n_ids) (ascending, unique); plane has ceil(n / 64) 64-bit words and every
 * one of them is written; n == 0 launches nothing */
hipError_t osmt_launch_idf_plane(const uint64_t* gid, uint32_t n, const uint64_t* ids, uint32_t n_ids, uint32_t* plane, hipStream_t st);

/* ---- node labels of tile-built scenes (osmt_tilelabels.hip) ----------------------------------------------------- */
/* The query half is the k_tq_* stages over the NODE pools: osmt_tq_pass::ix with way_off / ways = the node lists and
 * mp_off = an array of zeros (no second kind), so span, columns, gather and sort run unchanged. */
/* the scan of the tile query: a[0 .. n) -> its exclusive scan (mod 2^32), a[n] = the total (mod 2^32), *tot = the 64-bit total;
 * blk: one word per 256 elements, at least one */
hipError_t osmt_tq_scan(uint32_t* a, uint32_t n, unsigned long long* blk, unsigned long long* tot, hipStream_t st);
/* a registered label bindings table: node -> (label style, text) in push order, and the text pool */
struct osmt_tl_bind_dev {
    const uint32_t* node_off;
    const osmt_label_binding* bindings;
    const uint32_t* text_off;
    const uint32_t* chars;
};
/* words of osmt_tl_pass::tot */
enum {
    OSMT_TL_LABELS = 0, /* labels of the batch */
    OSMT_TL_MAX_LABELS, /* the most labels of any tile */
    OSMT_TL_OVER,       /* the first tile with more than OSMT_TILE_LABELS_MAX labels (none: all ones) */
    OSMT_TL_CHARS,      /* chars of the batch */
    OSMT_TL_N
};
struct osmt_tl_pass {
    const osmt_query_tile* q;        /* [n_tiles] */
    const osmt_tl_bind_dev* bind;    /* [OSMT_MAX_ZOOM + 1] (zooms no tile has: never read) */
    const double* nodes;             /* the geodata's node table [n_nodes][2] */
    const uint64_t* node_gid;        /* [n_nodes] */
    const osmt_label_style_rec* styles;
    const uint32_t* style_rank;      /* dense rank under (layer or 0, z_index) */
    const uint32_t* icon_h;          /* [images of the snapshot] heights */
    uint32_t n_tiles, n_cand, n_labels, n_chars; /* the last three: totals, known once they have been read back */
    uint32_t scale;
    const uint32_t* t_base; /* [n_tiles + 1] candidates of the tiles in front (osmt_tq_pass::t_wbase) */
    const uint32_t* cand;   /* sorted per tile */
    const uint32_t* keep_node; /* the node plane of a registered id filter, or NULL: no filter */
    uint32_t* lpos;         /* [n_cand + 1] labels of the candidate (0 for a repeat), then their exclusive scan */
    uint32_t* job_label_off; /* [n_tiles + 1] */
    ulonglong2* keys;       /* [n_labels] rank:32 | gid:64 | element position in the tile:32, sorted in place per tile */
    uint32_t* el_bind;      /* [n_labels] the element's binding (absolute index in its table), by unsorted position */
    uint32_t* el_node;      /* [n_labels] its node */
    uint32_t* chpos;        /* [n_labels + 1] chars of the sorted label, then their exclusive scan */
    uint32_t* ch_src;       /* [n_labels] where in its table's char pool the label's text starts */
    unsigned long long* blk;
    unsigned long long* tot; /* [OSMT_TL_N] */
    osmt_label* labels;      /* [n_labels] */
    osmt_string_run* runs;   /* [n_labels] */
    uint32_t* chars;         /* [n_chars] */
};
/* k_tl_mark + scan + k_tl_tiles: label positions, job_label_off, tot[LABELS, MAX_LABELS, OVER] */
hipError_t osmt_launch_tl_mark(const osmt_tl_pass& a, hipStream_t st);
/* k_tl_expand + k_tl_sort + k_tl_count + scan: keys in draw order, char positions, tot[CHARS] */
hipError_t osmt_launch_tl_order(const osmt_tl_pass& a, hipStream_t st);
/* k_tl_emit + k_tl_chars: the records and the char pool */
hipError_t osmt_launch_tl_emit(const osmt_tl_pass& a, hipStream_t st);

/* ---- label anchors from tile coordinates (osmt_anchors.hip) ----------------------------------------------------- */
/* words of osmt_an_pass::tot; the points of the batch are tot[POINTS] + tot[HIGH] */
enum {
    OSMT_AN_RINGS = 0,   /* rings of the batch */
    OSMT_AN_POINTS,      /* the sum of the requests' point counts, each taken mod 2^32 */
    OSMT_AN_HIGH,        /* what the requests' point counts hold above 32 bits */
    OSMT_AN_RING_POINTS, /* the total of the per-ring scan (= the points again; not read back) */
    OSMT_AN_N
};
struct osmt_an_pass {
    osmt_geo_dev geo;
    const double2* factors;             /* [n_nodes] the registered Mercator factors */
    const osmt_label_tile_request* req; /* [n_req] */
    const osmt_query_tile* tiles;
    uint32_t n_req, n_rings, n_pts; /* the last two: totals, known once they have been read back */
    uint32_t scale;
    uint32_t* rpos;          /* [n_req + 1] rings of the request, then their exclusive scan */
    uint32_t* ppos;          /* [n_req + 1] points of the request (mod 2^32), then their exclusive scan */
    unsigned long long* blk; /* block totals of the scan under way: one word per 256 elements, at least one */
    unsigned long long* tot; /* [OSMT_AN_N] */
    uint32_t* ring_base;     /* [n_rings + 1] points of the ring, then their exclusive scan: the ring's first point */
    uint32_t* ring_src;      /* [n_rings] where in geo.idx the ring's nodes start */
    uint32_t* ring_req;      /* [n_rings] its request */
    /* what osmt_launch_polylabel takes */
    osmt_pl_req* pl_req; /* [n_req] */
    osmt_ring* rings;    /* [n_rings] */
    double2* pts;        /* [n_pts] */
};
/* zeroes tot, then k_an_count + two scans: everything up to the totals */
hipError_t osmt_launch_an_count(const osmt_an_pass& a, hipStream_t st);
/* k_an_rings + scan + k_an_records + k_an_points: pl_req, rings and pts */
hipError_t osmt_launch_an_expand(const osmt_an_pass& a, hipStream_t st);

/* ---- area labels of tile-built scenes (osmt_arealabels.hip) ------------------------------------------------------ */
/* The query half is the k_tq_* stages over the way and multipolygon pools, up to and including osmt_launch_tq_mark with an
 * osmt_tq_bind_dev whose offsets are the LABEL bindings' (mark and tiles read no style id): apos is then the first label of
 * every candidate, tile_base the tiles' job_label_off, ways numbered in front of multipolygons. */
/* k_tl_sort alone: reads a.keys, a.job_label_off and a.n_tiles only */
hipError_t osmt_launch_tl_sort(const osmt_tl_pass& a, hipStream_t st);
/* a registered area label bindings table */
struct osmt_al_bind_dev {
    const uint32_t *way_off, *mp_off;
    const osmt_label_binding *way_bind, *mp_bind;
    const uint32_t *text_off, *chars;
};
/* words of osmt_al_pass::tot */
enum {
    OSMT_AL_REQS = 0,       /* (tile, entity) pairs that need the anchor search */
    OSMT_AL_CHARS,          /* chars of the batch */
    OSMT_AL_PTS,            /* way points of the batch */
    OSMT_AL_DECLINED,       /* requests answered OSMT_LABEL_TOO_LARGE */
    OSMT_AL_FIRST_DECLINED, /* the first of them (none: all ones) */
    OSMT_AL_N
};
#define OSMT_AL_NO_ANCHOR 3u /* beside OSMT_LABEL_*: the pair asked for no anchor */
struct osmt_al_pass {
    osmt_geo_dev geo;
    const osmt_query_tile* q;     /* [n_tiles] */
    const osmt_al_bind_dev* bind; /* [OSMT_MAX_ZOOM + 1] (zooms no tile has: never read) */
    const osmt_label_style_rec* styles;
    const uint32_t* style_rank;
    const uint32_t* icon_h;
    const osmt_area_anchor* anchors; /* [n_anchors] ascending by (tile, entity) */
    uint32_t n_tiles, n_cand, n_labels, n_req, n_chars, n_pts, n_anchors, scale;
    /* what the query left (osmt_tq_pass) */
    const uint32_t *t_wbase, *t_mbase; /* [n_tiles + 1] */
    const uint32_t* cand;              /* sorted per (tile, kind), a tile's ways in front of its multipolygons */
    const uint32_t* apos;              /* [n_cand + 1] first label of the candidate in query numbering */
    const uint32_t* job_label_off;     /* [n_tiles + 1] */
    /* per candidate */
    uint32_t* need; /* [n_cand + 1] 1: the pair is searched; then the exclusive scan: its request */
    uint32_t* ov;   /* [n_cand] the pair's entry in `anchors`, or all ones */
    /* per element, by position before the sort (multipolygons in front of ways) */
    ulonglong2* keys;  /* rank:32 | gid:64 | position in the tile:32, sorted in place per tile */
    uint32_t* el_bind; /* the binding: absolute index in its kind's pool */
    uint32_t* el_slot; /* the candidate slot */
    /* per sorted label */
    uint32_t* chpos;  /* [n_labels + 1] chars, then their exclusive scan */
    uint32_t* ch_src; /* [n_labels] */
    uint32_t* ptpos;  /* [n_labels + 1] way points, then their exclusive scan */
    uint32_t* pt_src; /* [n_labels] where in geo.idx the way's nodes start */
    unsigned long long* blk;
    unsigned long long* tot; /* [OSMT_AL_N] */
    /* anchors */
    osmt_label_tile_request* req;   /* [n_req] */
    const osmt_label_position* pos; /* [n_req] what osmt_launch_polylabel wrote */
    /* the batch */
    osmt_label* labels;
    osmt_string_run* runs;
    uint32_t* chars;
    int2* pts_fwd; /* [n_pts] the runs' points in the way's own order */
    int2* pts;     /* [n_pts] in walking order */
};
/* zeroes tot, k_al_expand + the scan of `need`: keys, element tables, tot[REQS] */
hipError_t osmt_launch_al_expand(const osmt_al_pass& a, hipStream_t st);
/* k_al_requests: the osmt_label_tile_request records of the pairs that are searched */
hipError_t osmt_launch_al_requests(const osmt_al_pass& a, hipStream_t st);
/* k_al_declined (after the search) + k_al_count + two scans: tot[DECLINED, FIRST_DECLINED, CHARS, PTS]; the keys are sorted */
hipError_t osmt_launch_al_count(const osmt_al_pass& a, hipStream_t st);
/* k_al_project + k_al_waypts + k_al_emit + k_al_chars */
hipError_t osmt_launch_al_emit(const osmt_al_pass& a, hipStream_t st);

/* ---- selector matching (osmt_selmatch.hip) ------------------------------------------------------------------------ */
/* the registered tags of a geodata file: the three kinds' CSRs joined, entities numbered nodes, ways, multipolygons */
struct osmt_sm_tags_dev {
    const uint32_t* tag_off; /* [n_ent + 1] into tags */
    const uint4* tags;       /* (k_off, k_len, v_off, v_len) */
    const uint8_t* strings;
    uint32_t n_nodes, n_ways, n_mps, n_tags;
};
/* a registered selector set.  keys: the distinct test keys ascending as unsigned bytes; vals: per key its distinct EQUAL /
 * NOT_EQUAL values, ascending too */
struct osmt_sm_key {
    uint32_t off, len;        /* in strings */
    uint32_t val_first, n_vals;
    uint32_t numeric, _pad;   /* some numeric test names the key */
};
struct osmt_sm_test { /* 24 bytes */
    uint32_t kind, key; /* OSMT_TEST_*, index into keys */
    uint32_t vid, _pad; /* EQUAL / NOT_EQUAL: the value's index among the key's values */
    double value;
};
struct osmt_sm_sel {
    uint32_t type, test_off, n_tests, _pad;
};
struct osmt_sm_sels_dev {
    const osmt_sm_key* keys;
    const uint2* vals; /* (off, len) in strings */
    const uint8_t* strings;
    const osmt_sm_sel* sels;
    const osmt_sm_test* tests;
    uint32_t n_keys, n_sels;
};
#define OSMT_SM_NONE 0xFFFFFFFFu
/* osmt_sm_pass::tag_vf[].y */
#define OSMT_SM_TRUE 1u     /* the value is yes, true or 1 */
#define OSMT_SM_NUM 2u      /* tag_num holds its f64 */
#define OSMT_SM_DECLINED 4u /* a numeric key's value the fast path declines and no override lists */
/* words of osmt_sm_pass::tot */
enum { OSMT_SM_T_DECLINED = 0, OSMT_SM_T_MATCHED, OSMT_SM_T_CLASSES, OSMT_SM_T_CLASS_SELS, OSMT_SM_T_N };
struct osmt_sm_pass {
    osmt_geo_dev geo;
    osmt_sm_tags_dev tg;
    osmt_sm_sels_dev ss;
    const osmt_number_override* ov; /* [n_ov] ascending by (v_off, v_len) */
    uint32_t n_ov, n_ent;
    uint32_t n_declined, n_matched, n_classes, n_class_sels; /* totals, known once they have been read back */
    uint32_t hash_mask, table_mask; /* the debug knob; table size - 1 (a power of two >= 2 n_ent) */
    /* per tag */
    uint32_t* tag_code; /* 2 k + 1: the tag's key is test key k; 2 k: it sorts in front of test key k (k = n_keys: behind all) */
    uint2* tag_vf;      /* (value id among its key's values or NONE, OSMT_SM_* flags) */
    double* tag_num;
    uint32_t* decl_pos; /* [n_tags + 1] 1: declined; then the exclusive scan */
    osmt_declined_number* declined; /* [n_declined] in tag order, duplicates included */
    /* per entity */
    uint32_t* sel_pos;  /* [n_ent + 1] matched selectors, then their exclusive scan */
    uint32_t* ent_sels; /* [n_matched] */
    long long* ent_layer; /* 0 without */
    uint32_t* ent_key;  /* slot | has_layer << 2 */
    uint32_t* ent_hash;
    uint32_t* ent_tslot; /* the entity's class in the table */
    uint32_t* first_pos; /* [n_ent + 1] 1: the lowest member of its class; then the exclusive scan: the class id */
    uint32_t* ent_class; /* the result */
    /* the class table: open addressing over representative entity numbers */
    uint32_t* table;  /* [table_mask + 1] */
    uint32_t* lowest; /* [table_mask + 1] the lowest member */
    /* per class */
    uint32_t* cls_pos;   /* [n_classes + 1] selectors, then their exclusive scan */
    uint32_t* cls_first; /* [n_classes] */
    osmt_match_class* classes;
    uint32_t* class_sels; /* [n_class_sels] */
    unsigned long long* blk;
    unsigned long long* tot; /* [OSMT_SM_T_N] */
};
/* k_sm_tags + scan: per-tag codes, value ids, flags and numbers; tot[DECLINED] */
hipError_t osmt_launch_sm_tags(const osmt_sm_pass& a, hipStream_t st);
/* k_sm_declined: the (v_off, v_len) of the declined tags */
hipError_t osmt_launch_sm_declined(const osmt_sm_pass& a, hipStream_t st);
/* k_sm_match (count) + scan: tot[MATCHED] */
hipError_t osmt_launch_sm_count(const osmt_sm_pass& a, hipStream_t st);
/* k_sm_match (emit) + k_sm_class_insert + k_sm_class_mark + scan: tot[CLASSES] */
hipError_t osmt_launch_sm_classes(const osmt_sm_pass& a, hipStream_t st);
/* k_sm_class_count + scan: tot[CLASS_SELS] */
hipError_t osmt_launch_sm_class_count(const osmt_sm_pass& a, hipStream_t st);
/* k_sm_class_emit + k_sm_ent_class */
hipError_t osmt_launch_sm_emit(const osmt_sm_pass& a, hipStream_t st);
/* bindings per class, one kind: pos[0 .. n) = styles of the entity's class, scanned (*tot the 64-bit total) */
hipError_t osmt_launch_sm_bind_count(const uint32_t* ent_class, const uint32_t* class_off, uint32_t n, uint32_t* pos, unsigned long long* blk,
                                     unsigned long long* tot, hipStream_t st);
/* out[pos[i] ..) = the styles of entity i's class */
hipError_t osmt_launch_sm_bind_emit(const uint32_t* ent_class, const uint32_t* class_off, const uint32_t* class_styles, uint32_t n, const uint32_t* pos,
                                    uint32_t* out, hipStream_t st);

/* ---- label bindings per class (osmt_labelbind.hip) ---------------------------------------------------------------- */
/* words of osmt_lb_pass::tot; FIRST_BAD is the one word that is not a scan total */
enum {
    OSMT_LB_T_BIND0 = 0, /* bindings of the first kind (nodes, or ways) */
    OSMT_LB_T_BIND1,     /* bindings of the second kind (multipolygons) */
    OSMT_LB_T_TEXTS,     /* distinct value ranges some binding uses */
    OSMT_LB_T_CHARS,     /* their scalars */
    OSMT_LB_T_FIRST_BAD, /* the lowest-numbered tag of the table whose used value is not well-formed UTF-8 (none: all ones) */
    OSMT_LB_T_N
};
/* One table: the node table has one kind (the nodes) and numbers the node tags; the area table has two (ways, then
 * multipolygons) and numbers the way tags in front of the multipolygon tags.  Tag t of the table is tags[tag_base + t]. */
struct osmt_lb_pass {
    osmt_sm_tags_dev tg;
    const uint32_t* ent_class;  /* the match's, [nodes + ways + multipolygons] */
    const uint32_t* class_off;  /* [n_classes + 1] into class_bind */
    const uint2* class_bind;    /* osmt_class_label_binding: (style, text_key) */
    const uint2* keys;          /* [n_keys] (offset in key_bytes, a multiple of 4; length) */
    const uint8_t* key_bytes;   /* the device copy starts every key on a 4-byte boundary */
    uint32_t tag_base, n_tt;    /* the table's tags */
    uint32_t n_texts, n_chars;  /* totals, known once they have been read back */
    uint32_t hash_mask, table_mask; /* the debug knob; table size - 1 (a power of two >= 2 n_tt) */
    /* per tag of the table */
    uint32_t* used;      /* 1: some binding reads the tag's value; cleared first */
    uint32_t* tslot;     /* a used tag's slot in the table */
    uint32_t* first_pos; /* [n_tt + 1] 1: the lowest used tag of its value range; then the exclusive scan: the text id */
    /* the text table: open addressing over representative tag numbers */
    uint32_t* table;  /* [table_mask + 1] */
    uint32_t* lowest; /* [table_mask + 1] the lowest member */
    /* per text */
    uint32_t* text_tag; /* [n_texts] its lowest user */
    uint32_t* text_off; /* [n_texts + 1] scalars, then their exclusive scan */
    uint32_t* chars;    /* [n_chars] */
    unsigned long long* blk;
    unsigned long long* tot; /* [OSMT_LB_T_N] */
};
/* sets tot[FIRST_BAD] to all ones and clears `used` */
hipError_t osmt_launch_lb_begin(const osmt_lb_pass& a, hipStream_t st);
/* k_lb_count + scan, one kind: pos[0 .. n) = bindings of the class of entity first + i, scanned (*tot the 64-bit total) */
hipError_t osmt_launch_lb_count(const osmt_lb_pass& a, uint32_t first, uint32_t n, uint32_t* pos, unsigned long long* tot, hipStream_t st);
/* k_lb_emit, one kind: out[pos[i] ..) = the bindings of entity first + i with the tag's number in the table as text; `used` */
hipError_t osmt_launch_lb_emit(const osmt_lb_pass& a, uint32_t first, uint32_t n, const uint32_t* pos, osmt_label_binding* out, hipStream_t st);
/* k_lb_text_insert + k_lb_text_mark + scan: tot[TEXTS] */
hipError_t osmt_launch_lb_texts(const osmt_lb_pass& a, hipStream_t st);
/* k_lb_text_list + k_lb_measure + scan: text_tag, text_off, tot[CHARS], tot[FIRST_BAD] */
hipError_t osmt_launch_lb_measure(const osmt_lb_pass& a, hipStream_t st);
/* k_lb_decode: chars */
hipError_t osmt_launch_lb_decode(const osmt_lb_pass& a, hipStream_t st);
/* k_lb_patch: the provisional tag numbers of bind[0 .. n) replaced by text ids */
hipError_t osmt_launch_lb_patch(const osmt_lb_pass& a, osmt_label_binding* bind, uint32_t n, hipStream_t st);

/* ---- the cascade (osmt_cascade.hip) ------------------------------------------------------------------------------- */
struct osmt_cs_prop;
/* a registered rule set */
struct osmt_cs_rules_dev {
    const osmt_cs_prop* props;
    const uint32_t* rule_last;  /* [n_rules][OSMT_PROP_NAMES] */
    const uint32_t* sel_rule;   /* [n_sels] */
    const uint8_t* sel_layer;   /* [n_sels] 0 .. n_layers - 1: the set-wide layer number (below 8, or below 255 with CLASS_LAYERS) */
    const uint8_t* sel_zoom;    /* [n_sels][2] the zooms the selector admits, inclusive (0, 255 without bounds) */
    const double* numbers;
    uint32_t n_sels, n_layers, star, base; /* star / base: the layers "*" and "default", or OSMT_CS_NONE */
    uint32_t font_id, flags;    /* flags: OSMT_RULES_* of the registration */
    double casing_width_multiplier, font_size_multiplier;
};
/* words of osmt_cs_pass::tot; BAD_CLASS is read back together with STYLES */
enum { OSMT_CS_T_BAD_CLASS = 0, OSMT_CS_T_STYLES, OSMT_CS_T_BINDINGS, OSMT_CS_T_AREA, OSMT_CS_T_LABEL, OSMT_CS_T_DASHES, OSMT_CS_T_RANGE_STYLES, OSMT_CS_T_RANGE_BINDINGS, OSMT_CS_T_N };
/* osmt_cs_pass::class_info: one word per class */
#define OSMT_CS_CI_STAR(w) ((w) & 0xFFu)          /* the class's local number of "*", 0xFF: the class has none */
#define OSMT_CS_CI_BASE(w) (((w) >> 8) & 0xFFu)   /* of "default" */
#define OSMT_CS_CI_LAYERS(w) ((w) >> 16)          /* the class's distinct layers, exact, at most 255 */
struct osmt_cs_pass {
    osmt_cs_rules_dev R;
    const osmt_match_class* classes;
    const uint32_t* class_sels;
    /* a set registered with OSMT_RULES_CLASS_LAYERS only (k_cs_class_layers writes them, k_cs_count and k_cs_fold read them) */
    uint8_t* sel_local;           /* [n_class_sels], parallel to class_sels: the selector's layer numbered inside its class by first
                                     appearance, 0 .. 15 (clamped to 15 in a class over the bound, whose cascade is refused) */
    uint32_t* class_info;         /* [n_classes] OSMT_CS_CI_* */
    uint32_t n_classes, n_pairs;  /* pairs: (class, zoom), number class * 19 + zoom */
    uint32_t n_styles, n_bindings, n_area, n_label, n_ranges; /* totals, known once they have been read back */
    uint32_t labels_all;
    uint32_t hash_mask, table_mask;
    /* per pair */
    uint32_t* pair_pos; /* [n_pairs + 1] styles, then their exclusive scan */
    /* per style (user): number = position in pair order, monotonic in ((class * 19) + zoom) * 8 + position (* 16 with CLASS_LAYERS) */
    uint32_t* rows;             /* [n_styles][OSMT_CS_ROW_WORDS] */
    osmt_style_rec* area;       /* [n_styles] dashes as ranges of R.numbers */
    osmt_label_style_rec* label;
    uint32_t* text_key;
    uint32_t* bind_pos;         /* [n_styles + 1] 1: the style is a label binding; then the exclusive scan */
    uint32_t* hash[2];          /* area, label */
    uint32_t* tslot[2];
    uint32_t* first_pos[2];     /* [n_styles + 1] 1: the lowest user of its record; then the scan: the distinct id */
    uint32_t* id[2];            /* the distinct id of the style's record (label: of a binding's, else undefined) */
    uint32_t* table[2];         /* [table_mask + 1] */
    uint32_t* lowest[2];
    /* per distinct record */
    uint32_t* dash_pos;         /* [n_area + 1] dashes of the record, then the scan */
    osmt_style_rec* out_area;   /* [n_area] dashes as ranges of out_dashes */
    double* out_dashes;
    osmt_label_style_rec* out_label; /* [n_label] */
    uint32_t* rep[2];           /* [n_area], [n_label] the lowest user */
    /* zooms */
    uint32_t* zoom_differs;     /* [19] 1: some class's lists at z differ from those at z - 1 (z >= 1) */
    uint8_t range_zoom[OSMT_MAX_ZOOM + 1]; /* the first zoom of range r */
    /* per (range, class), number range * n_classes + class */
    uint32_t* rs_pos;           /* [n_ranges * n_classes + 1] styles, then the scan */
    uint32_t* rb_pos;           /* the same for label bindings */
    uint32_t* out_style_off;    /* [n_ranges][n_classes + 1] rebased to the range */
    uint32_t* out_styles;       /* distinct area ids */
    uint32_t* out_bind_off;
    osmt_class_label_binding* out_binds;
    unsigned long long* blk;
    unsigned long long* tot; /* [OSMT_CS_T_N] */
};
/* k_cs_class_layers (a CLASS_LAYERS set only; otherwise nothing is launched): sel_local, class_info, tot[BAD_CLASS] = the lowest
 * class of more than OSMT_CASCADE_MAX_CLASS_LAYERS layers, or all ones */
hipError_t osmt_launch_cs_class_layers(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_count + scan: tot[STYLES] */
hipError_t osmt_launch_cs_count(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_fold + k_cs_records + scan: rows, records, hashes, tot[BINDINGS] */
hipError_t osmt_launch_cs_fold(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_insert + k_cs_mark + scan, both kinds: tot[AREA], tot[LABEL] */
hipError_t osmt_launch_cs_distinct(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_rank + scan: id, rep, dash_pos, tot[DASHES] */
hipError_t osmt_launch_cs_rank(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_compact + k_cs_zoom_differs: out_area, out_dashes, out_label, zoom_differs */
hipError_t osmt_launch_cs_compact(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_range_count + scans: tot[RANGE_STYLES], tot[RANGE_BINDINGS] */
hipError_t osmt_launch_cs_range_count(const osmt_cs_pass& a, hipStream_t st);
/* k_cs_range_emit */
hipError_t osmt_launch_cs_range_emit(const osmt_cs_pass& a, hipStream_t st);

/* out[i] = osmt_hypot(xy[2i], xy[2i + 1]) */
hipError_t osmt_launch_hypot(const double* xy, uint32_t n, double* out, hipStream_t st);
/* RGBA8 framebuffers -> complete RGB8 PNG files, one per tile, out_len[i] bytes at out + i * out_stride */
hipError_t osmt_launch_png(const void* rgba, size_t tile_stride, uint32_t n, uint32_t W, uint32_t H, uint32_t ihdr_crc, void* out,
                           size_t out_stride, uint32_t* out_len, hipStream_t st);
/* status != NULL: the guarded form, which writes nothing when *status (device memory, set earlier on `st`) is not 0 */
hipError_t osmt_launch_png_compact(const void* slots, size_t slot_stride, const uint32_t* len, const unsigned long long* off, uint32_t n,
                                   void* blob, hipStream_t st, const uint32_t* status = nullptr);
/* exclusive 64-bit scan of n <= 2^31 lengths into off[0 .. n]; *status = off[n] > capacity */
hipError_t osmt_launch_png_offsets(const uint32_t* len, uint32_t n, unsigned long long capacity, unsigned long long* off, uint32_t* status,
                                   hipStream_t st);
hipError_t osmt_launch_copy16(const void* src, void* dst, size_t n16, bool read_only, hipStream_t st);
hipError_t osmt_launch_composite(const void* planes, const double canvas[4], uint32_t n, uint32_t L, uint32_t npx,
                                 void* out, hipStream_t st);

#endif
