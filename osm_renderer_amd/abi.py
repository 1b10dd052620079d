"""ctypes mirror of include/osmtile.h (data layout only — no compute).

The struct layouts here must match the C header byte for byte; tests/test_abi.py
checks sizes/offsets against the library's own sizeof probes.
"""
import ctypes as C

TILE_SIZE = 256  # reference: src/tile.rs:6
MAX_ZOOM = 18  # reference: src/tile.rs:5
MAX_DASHES = 16

OK, INVALID_ARG, OOM, HIP_ERROR, UNSUPPORTED, NO_DEVICE, RCCL_ERROR = 0, -1, -2, -3, -4, -5, -6
PIXELS_RGBA8, PIXELS_RGB8 = 0, 1  # osmt_render_scene_host formats
PNG_OFFSETS_GROUP = 256  # threads of k_png_offsets' one workgroup = lengths per pass (OSMT_PNG_OFFSETS_GROUP)
COMM_ID_BYTES = 128
MULTI_RGB8 = 1  # osmt_render_batch_multi_ex flags

OP_NONE, OP_FILL_COLOR, OP_FILL_IMAGE, OP_STROKE = 0, 1, 2, 3
CAP_NONE, CAP_BUTT, CAP_ROUND, CAP_SQUARE = 0, 1, 2, 3
COORD_LATLON_F64, COORD_POINT_I32, COORD_NODE_REF = 0, 1, 2

STAGE_PROJECT, STAGE_OPINFO, STAGE_RASTER = 1, 2, 4

GLYPH_MOVE_TO, GLYPH_LINE_TO, GLYPH_CURVE_TO = 1, 2, 3  # osmt_glyph_vertex.type (stb_truetype's Vertex)
LABEL_OK, LABEL_NONE, LABEL_TOO_LARGE = 0, 1, 2  # osmt_label_position.status
LABEL_MAX_CELLS = 65536
GLYPH_CENTER, GLYPH_LINE = 0, 1  # osmt_glyph_instance.form: TextPlacer::place's two `tr` closures
GLYPH_NONE = 2  # a glyph of a text place() skipped (seen through osmt_scene_read_glyph_instances only)
TEXT_CENTER, TEXT_LINE = 0, 1  # osmt_text_run.position: TextPosition
STYLED_MAX_TILE_AREAS = 65536  # (entity, style) pairs of one tile of an osmt_styled_batch
STYLED_LDS_AREAS = 2048  # up to here osmt_scene_build_styled sorts a tile in LDS
STYLED_MULTIPOLYGON = 0x80000000  # osmt_styled_area.entity: the entity is a multipolygon
MAX_SCALE = 4
MAX_FILL_GROUPS = 1 << 28  # fill groups (fill op x sub-tile of its window) of one scene: 2^28 or more are refused
QUERY_MAX_TILE_CANDIDATES = 1 << 20  # references of one kind osmt_scene_build_tiles gathers for one tile before dedup
QUERY_LDS_CANDIDATES = 8192  # up to here a tile's candidates are sorted in LDS
BINDINGS_NONE = 0xFFFFFFFF  # osmt_tile_batch.bindings_of_zoom: the zoom has no bindings
PYRAMID_ALL_LEVELS = 0x7FFFF  # osmt_register_tile_pyramid: bits 0 .. 18, one per level
ID_FILTER_NONE = 0xFFFFFFFF  # osmt_scene_build_tiles_filtered: no osm_ids filter (an EMPTY filter keeps nothing)
TILE_LABELS_MAX = 65536  # (node, style) labels osmt_scene_build_tile_labels builds for one tile
TEXT_NONE = 0xFFFFFFFF  # osmt_label_binding.text: the tag text_style.text names is absent on the node
LABEL_POSITION_NONE, LABEL_POSITION_CENTER, LABEL_POSITION_LINE = 0, 1, 2  # osmt_label_style_rec.text_position


class Op(C.Structure):
    _fields_ = [
        ("kind", C.c_uint8),
        ("cap", C.c_uint8),
        ("use_caps_for_dashes", C.c_uint8),
        ("has_dashes", C.c_uint8),
        ("color", C.c_uint8 * 3),
        ("_pad0", C.c_uint8),
        ("opacity", C.c_double),
        ("width", C.c_double),
        ("n_dashes", C.c_uint32),
        ("dashes_off", C.c_uint32),
        ("n_rings", C.c_uint32),
        ("ring_off", C.c_uint32),
        ("image_id", C.c_uint32),
        ("_reserved", C.c_uint32 * 5),
    ]


class Ring(C.Structure):
    _fields_ = [("first_pt", C.c_uint32), ("n_pts", C.c_uint32)]


class TileJob(C.Structure):
    _fields_ = [
        ("x", C.c_uint32),
        ("y", C.c_uint32),
        ("zoom", C.c_uint8),
        ("has_canvas", C.c_uint8),
        ("canvas_rgb", C.c_uint8 * 3),
        ("_pad", C.c_uint8 * 3),
        ("n_ops", C.c_uint32),
        ("op_off", C.c_uint32),
        ("n_pts", C.c_uint32),
        ("pt_off", C.c_uint32),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("jobs", C.POINTER(TileJob)),
        ("n_jobs", C.c_size_t),
        ("ops", C.POINTER(Op)),
        ("n_ops", C.c_size_t),
        ("rings", C.POINTER(Ring)),
        ("n_rings", C.c_size_t),
        ("coord_kind", C.c_uint32),
        ("scale", C.c_uint32),
        ("latlon", C.POINTER(C.c_double)),
        ("points", C.POINTER(C.c_int32)),
        ("n_pts", C.c_size_t),
        ("dashes", C.POINTER(C.c_double)),
        ("n_dashes", C.c_size_t),
        ("nodes", C.POINTER(C.c_double)),
        ("n_nodes", C.c_size_t),
        ("node_refs", C.POINTER(C.c_uint32)),
    ]


class Label(C.Structure):
    _fields_ = [
        ("has_icon", C.c_uint8),
        ("has_text", C.c_uint8),
        ("text_color", C.c_uint8 * 3),
        ("_pad", C.c_uint8 * 3),
        ("image_id", C.c_uint32),
        ("seg_off", C.c_uint32),
        ("n_segs", C.c_uint32),
        ("_reserved", C.c_uint32),
        ("icon_center_x", C.c_double),
        ("icon_center_y", C.c_double),
    ]


class LabelBatch(C.Structure):
    _fields_ = [
        ("labels", C.POINTER(Label)),
        ("n_labels", C.c_size_t),
        ("job_label_off", C.POINTER(C.c_uint32)),
        ("segs", C.POINTER(C.c_double)),
        ("n_segs", C.c_size_t),
    ]


class GlyphVertex(C.Structure):
    _fields_ = [
        ("x", C.c_int16),
        ("y", C.c_int16),
        ("cx", C.c_int16),
        ("cy", C.c_int16),
        ("type", C.c_uint8),
        ("_pad", C.c_uint8),
    ]


class GlyphInstance(C.Structure):
    _fields_ = [
        ("glyph_id", C.c_uint32),
        ("form", C.c_uint32),
        ("scale", C.c_double),
        ("p", C.c_double * 6),
    ]


class GlyphLabelBatch(C.Structure):
    _fields_ = [
        ("labels", C.POINTER(Label)),
        ("n_labels", C.c_size_t),
        ("job_label_off", C.POINTER(C.c_uint32)),
        ("glyphs", C.POINTER(GlyphInstance)),
        ("n_glyphs", C.c_size_t),
    ]


class TextGlyph(C.Structure):
    _fields_ = [("glyph_id", C.c_uint32), ("advance", C.c_int32), ("kern", C.c_int32), ("flags", C.c_uint32)]


class TextRun(C.Structure):
    _fields_ = [
        ("position", C.c_uint32),
        ("y_offset", C.c_uint32),
        ("pt_off", C.c_uint32),
        ("n_pts", C.c_uint32),
        ("scale", C.c_double),
        ("ascent", C.c_int32),
        ("descent", C.c_int32),
        ("line_gap", C.c_int32),
        ("_pad", C.c_int32),
        ("center_x", C.c_double),
        ("center_y", C.c_double),
        ("_reserved", C.c_double),
    ]


class TextLabelBatch(C.Structure):
    _fields_ = [
        ("labels", C.POINTER(Label)),
        ("n_labels", C.c_size_t),
        ("job_label_off", C.POINTER(C.c_uint32)),
        ("runs", C.POINTER(TextRun)),
        ("glyphs", C.POINTER(TextGlyph)),
        ("n_glyphs", C.c_size_t),
        ("way_pts", C.POINTER(C.c_int32)),
        ("way_sincos", C.POINTER(C.c_double)),
        ("n_way_pts", C.c_size_t),
    ]


class CmapEntry(C.Structure):
    _fields_ = [("code_point", C.c_uint32), ("glyph", C.c_uint32)]


class KernPair(C.Structure):
    _fields_ = [("left", C.c_uint32), ("right", C.c_uint32), ("value", C.c_int32)]


class FontDesc(C.Structure):
    _fields_ = [
        ("cmap", C.POINTER(CmapEntry)),
        ("n_cmap", C.c_size_t),
        ("advance", C.POINTER(C.c_int32)),
        ("outline_id", C.POINTER(C.c_uint32)),
        ("n_glyphs", C.c_size_t),
        ("kern", C.POINTER(KernPair)),
        ("n_kern", C.c_size_t),
        ("ascent", C.c_int32),
        ("descent", C.c_int32),
        ("line_gap", C.c_int32),
        ("_pad", C.c_int32),
    ]


class StringRun(C.Structure):
    _fields_ = [
        ("position", C.c_uint32),
        ("y_offset", C.c_uint32),
        ("pt_off", C.c_uint32),
        ("n_pts", C.c_uint32),
        ("font_id", C.c_uint32),
        ("_pad", C.c_uint32),
        ("font_size", C.c_double),
        ("center_x", C.c_double),
        ("center_y", C.c_double),
        ("_reserved", C.c_double * 2),
    ]


class StringLabelBatch(C.Structure):
    _fields_ = [
        ("labels", C.POINTER(Label)),
        ("n_labels", C.c_size_t),
        ("job_label_off", C.POINTER(C.c_uint32)),
        ("runs", C.POINTER(StringRun)),
        ("chars", C.POINTER(C.c_uint32)),
        ("n_chars", C.c_size_t),
        ("way_pts", C.POINTER(C.c_int32)),
        ("way_sincos", C.POINTER(C.c_double)),
        ("n_way_pts", C.c_size_t),
    ]


class LabelRequest(C.Structure):
    _fields_ = [("ring_off", C.c_uint32), ("n_rings", C.c_uint32), ("scale", C.c_double)]


class LabelRequestBatch(C.Structure):
    _fields_ = [
        ("requests", C.POINTER(LabelRequest)),
        ("n_requests", C.c_size_t),
        ("rings", C.POINTER(Ring)),
        ("n_rings", C.c_size_t),
        ("points", C.POINTER(C.c_double)),
        ("n_pts", C.c_size_t),
    ]


class LabelPosition(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("status", C.c_uint32), ("_pad", C.c_uint32)]


class LabelTileRequest(C.Structure):
    _fields_ = [("entity", C.c_uint32), ("tile", C.c_uint32)]


class GeodataDesc(C.Structure):
    _fields_ = [
        ("nodes", C.POINTER(C.c_double)),
        ("n_nodes", C.c_size_t),
        ("way_ids", C.POINTER(C.c_uint64)),
        ("way_node_off", C.POINTER(C.c_uint32)),
        ("n_ways", C.c_size_t),
        ("way_nodes", C.POINTER(C.c_uint32)),
        ("n_way_nodes", C.c_size_t),
        ("polygon_node_off", C.POINTER(C.c_uint32)),
        ("n_polygons", C.c_size_t),
        ("polygon_nodes", C.POINTER(C.c_uint32)),
        ("n_polygon_nodes", C.c_size_t),
        ("multipolygon_ids", C.POINTER(C.c_uint64)),
        ("multipolygon_polygon_off", C.POINTER(C.c_uint32)),
        ("n_multipolygons", C.c_size_t),
        ("multipolygon_polygons", C.POINTER(C.c_uint32)),
        ("n_multipolygon_polygons", C.c_size_t),
    ]


class RelationsDesc(C.Structure):  # osmt_relations_desc
    _fields_ = [
        ("nodes", C.POINTER(C.c_double)),
        ("n_nodes", C.c_size_t),
        ("way_node_off", C.POINTER(C.c_uint32)),
        ("n_ways", C.c_size_t),
        ("way_nodes", C.POINTER(C.c_uint32)),
        ("n_way_nodes", C.c_size_t),
        ("relation_ids", C.POINTER(C.c_uint64)),
        ("relation_way_off", C.POINTER(C.c_uint32)),
        ("n_relations", C.c_size_t),
        ("relation_ways", C.POINTER(C.c_uint32)),
        ("relation_way_inner", C.POINTER(C.c_uint8)),
        ("n_relation_ways", C.c_size_t),
    ]


class RawOsmDesc(C.Structure):  # osmt_raw_osm_desc
    _fields_ = [
        ("node_ids", C.POINTER(C.c_uint64)),
        ("n_nodes", C.c_size_t),
        ("way_ids", C.POINTER(C.c_uint64)),
        ("way_ref_off", C.POINTER(C.c_uint32)),
        ("n_ways", C.c_size_t),
        ("way_refs", C.POINTER(C.c_uint64)),
        ("n_way_refs", C.c_size_t),
        ("relation_ref_off", C.POINTER(C.c_uint32)),
        ("n_relations", C.c_size_t),
        ("relation_refs", C.POINTER(C.c_uint64)),
        ("relation_ref_inner", C.POINTER(C.c_uint8)),
        ("n_relation_refs", C.c_size_t),
        ("way_nodes_seen", C.POINTER(C.c_uint32)),
        ("relation_ways_seen", C.POINTER(C.c_uint32)),
    ]


class StyleRec(C.Structure):
    _fields_ = [
        ("layer", C.c_int64),
        ("z_index", C.c_double),
        ("opacity", C.c_double),
        ("fill_opacity", C.c_double),
        ("width", C.c_double),
        ("casing_width", C.c_double),
        ("fill_image", C.c_uint32),
        ("dashes_off", C.c_uint32),
        ("n_dashes", C.c_uint32),
        ("casing_dashes_off", C.c_uint32),
        ("n_casing_dashes", C.c_uint32),
        ("has_layer", C.c_uint8),
        ("is_foreground_fill", C.c_uint8),
        ("has_color", C.c_uint8),
        ("color", C.c_uint8 * 3),
        ("has_fill_color", C.c_uint8),
        ("fill_color", C.c_uint8 * 3),
        ("has_opacity", C.c_uint8),
        ("has_fill_opacity", C.c_uint8),
        ("has_width", C.c_uint8),
        ("has_dashes", C.c_uint8),
        ("line_cap", C.c_uint8),
        ("has_casing_color", C.c_uint8),
        ("casing_color", C.c_uint8 * 3),
        ("has_casing_width", C.c_uint8),
        ("has_casing_dashes", C.c_uint8),
        ("casing_line_cap", C.c_uint8),
        ("has_fill_image", C.c_uint8),
        ("has_background_color", C.c_uint8),
        ("background_color", C.c_uint8 * 3),
        ("_pad", C.c_uint8),
    ]


class StyledArea(C.Structure):
    _fields_ = [("entity", C.c_uint32), ("style", C.c_uint32)]


class StyledTile(C.Structure):
    _fields_ = [
        ("x", C.c_uint32),
        ("y", C.c_uint32),
        ("zoom", C.c_uint8),
        ("has_canvas", C.c_uint8),
        ("canvas_rgb", C.c_uint8 * 3),
        ("_pad", C.c_uint8 * 3),
        ("area_off", C.c_uint32),
        ("n_areas", C.c_uint32),
    ]


class StyledBatch(C.Structure):
    _fields_ = [
        ("tiles", C.POINTER(StyledTile)),
        ("n_tiles", C.c_size_t),
        ("areas", C.POINTER(StyledArea)),
        ("n_areas", C.c_size_t),
        ("geodata_id", C.c_uint32),
        ("scale", C.c_uint32),
        ("use_caps_for_dashes", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class TileIndexDesc(C.Structure):
    _fields_ = [
        ("tile_xy", C.POINTER(C.c_uint32)),
        ("n_tiles", C.c_size_t),
        ("way_off", C.POINTER(C.c_uint32)),
        ("ways", C.POINTER(C.c_uint32)),
        ("n_way_refs", C.c_size_t),
        ("multipolygon_off", C.POINTER(C.c_uint32)),
        ("multipolygons", C.POINTER(C.c_uint32)),
        ("n_multipolygon_refs", C.c_size_t),
    ]


class StyleBindingsDesc(C.Structure):
    _fields_ = [
        ("geodata_id", C.c_uint32),
        ("zoom_lo", C.c_uint8),
        ("zoom_hi", C.c_uint8),
        ("_pad", C.c_uint8 * 2),
        ("way_style_off", C.POINTER(C.c_uint32)),
        ("way_styles", C.POINTER(C.c_uint32)),
        ("n_way_styles", C.c_size_t),
        ("multipolygon_style_off", C.POINTER(C.c_uint32)),
        ("multipolygon_styles", C.POINTER(C.c_uint32)),
        ("n_multipolygon_styles", C.c_size_t),
    ]


class QueryTile(C.Structure):
    _fields_ = [
        ("x", C.c_uint32),
        ("y", C.c_uint32),
        ("zoom", C.c_uint8),
        ("has_canvas", C.c_uint8),
        ("canvas_rgb", C.c_uint8 * 3),
        ("_pad", C.c_uint8 * 3),
    ]


class TileBatch(C.Structure):
    _fields_ = [
        ("tiles", C.POINTER(QueryTile)),
        ("n_tiles", C.c_size_t),
        ("geodata_id", C.c_uint32),
        ("scale", C.c_uint32),
        ("use_caps_for_dashes", C.c_uint32),
        ("_pad", C.c_uint32),
        ("bindings_of_zoom", C.c_uint32 * (MAX_ZOOM + 1)),
    ]


class LabelTileBatch(C.Structure):
    _fields_ = [
        ("requests", C.POINTER(LabelTileRequest)),
        ("n_requests", C.c_size_t),
        ("tiles", C.POINTER(QueryTile)),
        ("n_tiles", C.c_size_t),
        ("geodata_id", C.c_uint32),
        ("scale", C.c_uint32),
    ]


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32)]


assert C.sizeof(Op) == 64
assert C.sizeof(Ring) == 8
assert C.sizeof(TileJob) == 32
assert C.sizeof(Label) == 40
assert C.sizeof(GlyphVertex) == 10
assert C.sizeof(GlyphInstance) == 64
assert C.sizeof(TextGlyph) == 16
assert C.sizeof(TextRun) == 64
assert C.sizeof(CmapEntry) == 8
assert C.sizeof(KernPair) == 12
assert C.sizeof(StringRun) == 64
assert C.sizeof(LabelRequest) == 16
assert C.sizeof(LabelPosition) == 24
assert C.sizeof(StyleRec) == 96
assert C.sizeof(StyledArea) == 8
assert C.sizeof(StyledTile) == 24
assert C.sizeof(StyledBatch) == 48
assert C.sizeof(GeodataDesc) == 128
assert C.sizeof(TileIndexDesc) == 64
assert C.sizeof(StyleBindingsDesc) == 56
assert C.sizeof(QueryTile) == 16
assert C.sizeof(TileBatch) == 112
assert C.sizeof(LabelTileRequest) == 8
assert C.sizeof(LabelTileBatch) == 40


class NodeIndexDesc(C.Structure):
    _fields_ = [
        ("node_ids", C.POINTER(C.c_uint64)),
        ("n_nodes", C.c_size_t),
        ("node_off", C.POINTER(C.c_uint32)),
        ("nodes", C.POINTER(C.c_uint32)),
        ("n_node_refs", C.c_size_t),
    ]


class LabelStyleRec(C.Structure):
    _fields_ = [
        ("layer", C.c_int64),
        ("z_index", C.c_double),
        ("font_size", C.c_double),
        ("icon_image", C.c_uint32),
        ("font_id", C.c_uint32),
        ("has_layer", C.c_uint8),
        ("has_icon", C.c_uint8),
        ("has_text_style", C.c_uint8),
        ("has_font_size", C.c_uint8),
        ("has_text_color", C.c_uint8),
        ("text_color", C.c_uint8 * 3),
        ("text_position", C.c_uint8),
        ("_pad", C.c_uint8 * 7),
    ]


class LabelBinding(C.Structure):
    _fields_ = [("style", C.c_uint32), ("text", C.c_uint32)]


class LabelBindingsDesc(C.Structure):
    _fields_ = [
        ("geodata_id", C.c_uint32),
        ("zoom_lo", C.c_uint8),
        ("zoom_hi", C.c_uint8),
        ("_pad", C.c_uint8 * 2),
        ("node_off", C.POINTER(C.c_uint32)),
        ("bindings", C.POINTER(LabelBinding)),
        ("n_bindings", C.c_size_t),
        ("text_off", C.POINTER(C.c_uint32)),
        ("n_texts", C.c_size_t),
        ("chars", C.POINTER(C.c_uint32)),
        ("n_chars", C.c_size_t),
    ]


class AreaLabelBindingsDesc(C.Structure):
    _fields_ = [
        ("geodata_id", C.c_uint32),
        ("zoom_lo", C.c_uint8),
        ("zoom_hi", C.c_uint8),
        ("_pad", C.c_uint8 * 2),
        ("way_off", C.POINTER(C.c_uint32)),
        ("way_bindings", C.POINTER(LabelBinding)),
        ("n_way_bindings", C.c_size_t),
        ("multipolygon_off", C.POINTER(C.c_uint32)),
        ("multipolygon_bindings", C.POINTER(LabelBinding)),
        ("n_multipolygon_bindings", C.c_size_t),
        ("text_off", C.POINTER(C.c_uint32)),
        ("n_texts", C.c_size_t),
        ("chars", C.POINTER(C.c_uint32)),
        ("n_chars", C.c_size_t),
    ]


class AreaAnchor(C.Structure):  # osmt_area_anchor
    _fields_ = [("tile", C.c_uint32), ("entity", C.c_uint32), ("x", C.c_double), ("y", C.c_double), ("status", C.c_uint32), ("_pad", C.c_uint32)]


assert C.sizeof(AreaLabelBindingsDesc) == 88
assert C.sizeof(AreaAnchor) == 32


# ---- tile requests (osmt_tile_server_*, osmt_worker_render_tile_png) ------------------------------------------------
class TileServerDesc(C.Structure):  # osmt_tile_server_desc
    _fields_ = [
        ("geodata_id", C.c_uint32),
        ("use_caps_for_dashes", C.c_uint32),
        ("id_filter", C.c_uint32),
        ("has_canvas", C.c_uint8),
        ("canvas_rgb", C.c_uint8 * 3),
        ("bindings_of_zoom", C.c_uint32 * (MAX_ZOOM + 1)),
        ("area_label_bindings_of_zoom", C.c_uint32 * (MAX_ZOOM + 1)),
        ("node_label_bindings_of_zoom", C.c_uint32 * (MAX_ZOOM + 1)),
    ]


class TileCoord(C.Structure):  # osmt_tile_coord
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("zoom", C.c_uint32)]


assert C.sizeof(TileServerDesc) == 16 + 3 * 4 * (MAX_ZOOM + 1) and C.sizeof(TileCoord) == 12


# ---- selector matching (osmt_match_selectors) ----------------------------------------------------------------------
MATCH_MAX_SELECTORS = 16384
MATCH_MAX_SELECTOR_TESTS = 16
SEL_NODE, SEL_WAY, SEL_AREA, SEL_OTHER = 0, 1, 2, 3
(TEST_EXISTS, TEST_NOT_EXISTS, TEST_TRUE, TEST_FALSE, TEST_EQUAL, TEST_NOT_EQUAL, TEST_LESS, TEST_LESS_OR_EQUAL, TEST_GREATER,
 TEST_GREATER_OR_EQUAL) = range(10)


class TagsDesc(C.Structure):
    _fields_ = [
        ("node_tag_off", C.POINTER(C.c_uint32)),
        ("node_tags", C.POINTER(C.c_uint32)),
        ("n_nodes", C.c_size_t),
        ("n_node_tags", C.c_size_t),
        ("way_tag_off", C.POINTER(C.c_uint32)),
        ("way_tags", C.POINTER(C.c_uint32)),
        ("n_ways", C.c_size_t),
        ("n_way_tags", C.c_size_t),
        ("multipolygon_tag_off", C.POINTER(C.c_uint32)),
        ("multipolygon_tags", C.POINTER(C.c_uint32)),
        ("n_multipolygons", C.c_size_t),
        ("n_multipolygon_tags", C.c_size_t),
        ("strings", C.POINTER(C.c_uint8)),
        ("n_string_bytes", C.c_size_t),
    ]


class SelectorTest(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("key_off", C.c_uint32), ("key_len", C.c_uint32), ("value_off", C.c_uint32), ("value_len", C.c_uint32),
                ("_pad", C.c_uint32), ("value", C.c_double)]


class SelectorRec(C.Structure):
    _fields_ = [("object_type", C.c_uint8), ("has_min_zoom", C.c_uint8), ("min_zoom", C.c_uint8), ("has_max_zoom", C.c_uint8), ("max_zoom", C.c_uint8),
                ("_pad", C.c_uint8 * 3), ("test_off", C.c_uint32), ("n_tests", C.c_uint32)]


class SelectorsDesc(C.Structure):
    _fields_ = [("selectors", C.POINTER(SelectorRec)), ("n_selectors", C.c_size_t), ("tests", C.POINTER(SelectorTest)), ("n_tests", C.c_size_t),
                ("strings", C.POINTER(C.c_uint8)), ("n_string_bytes", C.c_size_t)]


class NumberOverride(C.Structure):
    _fields_ = [("v_off", C.c_uint32), ("v_len", C.c_uint32), ("has_value", C.c_uint32), ("_pad", C.c_uint32), ("value", C.c_double)]


class DeclinedNumber(C.Structure):
    _fields_ = [("v_off", C.c_uint32), ("v_len", C.c_uint32)]


class MatchClass(C.Structure):
    _fields_ = [("layer", C.c_int64), ("sel_off", C.c_uint32), ("n_sels", C.c_uint32), ("first_entity", C.c_uint32), ("slot", C.c_uint8),
                ("has_layer", C.c_uint8), ("_pad", C.c_uint8 * 2)]


LABEL_TEXT_KEYS_MAX = 256  # keys of one osmt_class_label_bindings_desc


class ClassLabelBinding(C.Structure):
    _fields_ = [("style", C.c_uint32), ("text_key", C.c_uint32)]


class ClassLabelBindingsDesc(C.Structure):
    _fields_ = [
        ("zoom_lo", C.c_uint8),
        ("zoom_hi", C.c_uint8),
        ("_pad", C.c_uint8 * 6),
        ("class_off", C.POINTER(C.c_uint32)),
        ("bindings", C.POINTER(ClassLabelBinding)),
        ("n_classes", C.c_size_t),
        ("n_bindings", C.c_size_t),
        ("key_off", C.POINTER(C.c_uint32)),
        ("key_bytes", C.POINTER(C.c_uint8)),
        ("n_keys", C.c_size_t),
        ("n_key_bytes", C.c_size_t),
    ]


assert C.sizeof(ClassLabelBinding) == 8
assert C.sizeof(ClassLabelBindingsDesc) == 72
assert C.sizeof(TagsDesc) == 112
assert C.sizeof(SelectorTest) == 32
assert C.sizeof(SelectorRec) == 16
assert C.sizeof(SelectorsDesc) == 48
assert C.sizeof(NumberOverride) == 24
assert C.sizeof(DeclinedNumber) == 8
assert C.sizeof(MatchClass) == 24


# ---- the cascade: styles per class and zoom from registered rules ----
CASCADE_MAX_LAYERS = 8
RULES_CLASS_LAYERS = 1  # flags of osmt_validate_rules_ex / osmt_register_rules_ex: layer numbers local to a class
CASCADE_MAX_LAYER_NAMES = 255
CASCADE_MAX_CLASS_LAYERS = 16
LAYER_DEFAULT = 0xFFFFFFFF  # osmt_rules_desc.selector_layer: the selector names no layer
PROP_NAMES = ("z-index", "fill-position", "width", "casing-width", "text", "font-size", "text-color", "text-position", "color", "fill-color",
              "background-color", "opacity", "fill-opacity", "dashes", "linecap", "casing-color", "casing-dashes", "casing-linecap", "icon-image",
              "fill-image")  # OSMT_PROP_*: the index is the value
PROP_OTHER = len(PROP_NAMES)
PV_IDENTIFIER, PV_STRING, PV_COLOR, PV_NUMBERS, PV_WIDTH_DELTA = range(5)
CASCADE_AREA_STYLES, CASCADE_NODE_LABELS, CASCADE_AREA_LABELS = 1, 2, 4


class RuleProp(C.Structure):
    _fields_ = [("name", C.c_uint8), ("kind", C.c_uint8), ("has_color", C.c_uint8), ("rgb", C.c_uint8 * 3), ("has_image", C.c_uint8), ("_pad", C.c_uint8),
                ("image", C.c_uint32), ("str_off", C.c_uint32), ("str_len", C.c_uint32), ("num_off", C.c_uint32), ("n_nums", C.c_uint32),
                ("_pad2", C.c_uint32), ("delta", C.c_double)]


class RulesDesc(C.Structure):
    _fields_ = [
        ("selectors_id", C.c_uint32),
        ("font_id", C.c_uint32),
        ("selector_rule", C.POINTER(C.c_uint32)),
        ("selector_layer", C.POINTER(C.c_uint32)),
        ("n_selectors", C.c_size_t),
        ("layer_off", C.POINTER(C.c_uint32)),
        ("layer_bytes", C.POINTER(C.c_uint8)),
        ("n_layers", C.c_size_t),
        ("n_layer_bytes", C.c_size_t),
        ("rule_prop_off", C.POINTER(C.c_uint32)),
        ("props", C.POINTER(RuleProp)),
        ("n_rules", C.c_size_t),
        ("n_props", C.c_size_t),
        ("numbers", C.POINTER(C.c_double)),
        ("n_numbers", C.c_size_t),
        ("strings", C.POINTER(C.c_uint8)),
        ("n_string_bytes", C.c_size_t),
        ("casing_width_multiplier", C.c_double),
        ("font_size_multiplier", C.c_double),
        ("has_font_size_multiplier", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


assert C.sizeof(RuleProp) == 40
assert C.sizeof(RulesDesc) == 152
