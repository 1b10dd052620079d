"""ctypes binding of libosmtile.so — the C ABI of include/osmtile.h.

There is no fallback: if the HIP library is missing or no GPU is present the
calls raise.  torch is imported first on purpose: it brings its own
libamdhip64.so.7 into the process and the dynamic linker then resolves our
NEEDED entry of the same soname to that copy, so device pointers and streams
are shared between torch tensors and the kernels.
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# OSMT_LIB selects an alternative build of the same library (kernel-variant experiments only)
LIB_PATH = os.environ.get("OSMT_LIB") or os.path.join(_HERE, "libosmtile.so")
_lib = None

EXPORTS = [
    "osmt_create", "osmt_destroy", "osmt_last_error", "osmt_version", "osmt_register_image", "osmt_render_batch",
    "osmt_scene_upload", "osmt_scene_free", "osmt_render_scene", "osmt_render_scene_f64", "osmt_render_scene_stages",
    "osmt_scene_read_points", "osmt_project", "osmt_composite", "osmt_composite_device", "osmt_png_bound",
    "osmt_encode_png", "osmt_render_batch_labels", "osmt_render_batch_rgb", "osmt_scene_set_labels", "osmt_scene_read_label_status",
    "osmt_scene_check", "osmt_worker_create", "osmt_worker_destroy", "osmt_worker_render",
    "osmt_render_batch_png_begin", "osmt_render_batch_png_end",
    "osmt_host_alloc", "osmt_host_free", "osmt_png_device_bound", "osmt_encode_png_device", "osmt_render_batch_png",
    "osmt_validate_batch", "osmt_batch_shard_create", "osmt_batch_shard_get", "osmt_batch_shard_free", "osmt_render_batch_multi",
    "osmt_render_batch_multi_ex",
    "osmt_comm_unique_id", "osmt_comm_init_rank", "osmt_comm_init_local", "osmt_allreduce_tile_count",
    "osmt_allreduce_tile_count_local", "osmt_allreduce_tile_count_enqueue", "osmt_allreduce_tile_count_result", "osmt_hbm_copy_probe",
    "osmt_debug_poison_enabled",
    "osmt_register_glyphs", "osmt_scene_set_glyph_labels", "osmt_render_batch_rgb_glyphs", "osmt_scene_read_label_segs",
    "osmt_debug_hypot", "osmt_scene_read_label_cover",
    "osmt_validate_text_labels", "osmt_scene_set_text_labels", "osmt_render_batch_rgb_text", "osmt_scene_read_glyph_instances",
    "osmt_register_font", "osmt_validate_string_labels", "osmt_scene_set_string_labels", "osmt_render_batch_rgb_strings",
    "osmt_scene_read_text_glyphs",
    "osmt_label_positions", "osmt_label_positions_begin", "osmt_label_positions_end", "osmt_label_positions_stats",
    "osmt_validate_geodata", "osmt_register_geodata", "osmt_validate_styles", "osmt_register_styles", "osmt_validate_styled_batch",
    "osmt_scene_build_styled", "osmt_scene_read_display_list", "osmt_scene_max_tile_ops",
    "osmt_validate_tile_index", "osmt_register_tile_index", "osmt_validate_style_bindings", "osmt_register_style_bindings",
    "osmt_validate_tile_batch", "osmt_scene_build_tiles", "osmt_scene_read_styled_areas",
    "osmt_validate_node_index", "osmt_register_node_index", "osmt_validate_label_styles", "osmt_register_label_styles",
    "osmt_validate_label_bindings", "osmt_register_label_bindings", "osmt_scene_build_tile_labels", "osmt_scene_read_tile_labels",
    "osmt_validate_node_mercator", "osmt_register_node_mercator", "osmt_validate_label_tile_batch", "osmt_label_positions_tiles",
    "osmt_label_positions_tiles_begin", "osmt_label_tile_batch_expand",
    "osmt_validate_area_label_bindings", "osmt_register_area_label_bindings", "osmt_scene_build_tile_labels_all",
    "osmt_scene_read_declined_anchors", "osmt_scene_read_tile_area_labels",
    "osmt_validate_tags", "osmt_register_tags", "osmt_validate_selectors", "osmt_register_selectors", "osmt_match_selectors",
    "osmt_match_free", "osmt_match_read_declined_numbers", "osmt_match_read", "osmt_register_style_bindings_matched",
    "osmt_debug_match_hash_bits",
    "osmt_validate_class_label_bindings", "osmt_register_label_bindings_matched", "osmt_register_area_label_bindings_matched",
    "osmt_read_label_bindings", "osmt_read_area_label_bindings",
    "osmt_validate_rules", "osmt_register_rules", "osmt_validate_rules_ex", "osmt_register_rules_ex", "osmt_cascade_classes", "osmt_cascade_free", "osmt_cascade_read", "osmt_cascade_register",
    "osmt_render_scene_host", "osmt_render_scene_png", "osmt_render_scene_png_begin", "osmt_scene_png_work_bytes",
    "osmt_render_scene_png_device", "osmt_debug_png_offsets",
    "osmt_validate_id_filter", "osmt_register_id_filter", "osmt_read_id_filter", "osmt_scene_build_tiles_filtered",
    "osmt_validate_tile_server", "osmt_tile_server_create", "osmt_tile_server_free", "osmt_tile_server_render_png",
    "osmt_last_declined_anchors", "osmt_worker_render_tile_png", "osmt_worker_tile_stats",
    "osmt_validate_tile_pyramid", "osmt_register_tile_pyramid", "osmt_tile_pyramid_levels", "osmt_read_tile_pyramid", "osmt_tile_query_stats",
    "osmt_validate_tile_index_build", "osmt_build_tile_index", "osmt_read_tile_index",
    "osmt_validate_relations", "osmt_assemble_multipolygons", "osmt_polygons_counts", "osmt_polygons_read", "osmt_polygons_free",
    "osmt_debug_vertex_hash_bits",
    "osmt_validate_resolve", "osmt_resolve_refs", "osmt_resolved_counts", "osmt_resolved_read", "osmt_resolved_free",
    "osmt_debug_resolve_short_way_max",
]


class OsmtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"osmtile error {code}: {msg}")
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m osm_renderer_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback"
        )
    import torch  # noqa: F401  (loads the HIP runtime this library binds to)

    L = C.CDLL(LIB_PATH)
    vp, dp, ip, u8p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.osmt_version.restype = C.c_uint32
    L.osmt_last_error.restype = C.c_char_p
    L.osmt_create.argtypes = [C.POINTER(abi.Config), C.POINTER(vp)]
    L.osmt_destroy.argtypes = [vp]
    L.osmt_destroy.restype = None
    L.osmt_register_image.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.osmt_render_batch.argtypes = [vp, C.POINTER(abi.Batch), u8p, C.c_size_t]
    L.osmt_validate_batch.argtypes = [C.POINTER(abi.Batch)]
    L.osmt_batch_shard_create.argtypes = [C.POINTER(abi.Batch), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.osmt_batch_shard_get.argtypes = [vp]
    L.osmt_batch_shard_get.restype = C.POINTER(abi.Batch)
    L.osmt_batch_shard_free.argtypes = [vp]
    L.osmt_batch_shard_free.restype = None
    L.osmt_render_batch_multi.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(abi.Batch), u8p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.osmt_render_batch_multi_ex.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), C.c_uint32, u8p,
                                             C.c_size_t, C.POINTER(C.c_uint64)]
    L.osmt_comm_unique_id.argtypes = [u8p]
    L.osmt_comm_init_rank.argtypes = [vp, u8p, C.c_uint32, C.c_uint32]
    L.osmt_comm_init_local.argtypes = [C.POINTER(vp), C.c_uint32]
    L.osmt_allreduce_tile_count.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.osmt_allreduce_tile_count_enqueue.argtypes = [vp, C.c_uint64, vp]
    L.osmt_allreduce_tile_count_result.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.osmt_allreduce_tile_count_local.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.osmt_hbm_copy_probe.argtypes = [vp, C.c_size_t, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.osmt_scene_upload.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(vp)]
    L.osmt_scene_free.argtypes = [vp]
    L.osmt_scene_free.restype = None
    L.osmt_render_scene.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.osmt_render_scene_f64.argtypes = [vp, vp, vp, vp]
    L.osmt_render_scene_stages.argtypes = [vp, vp, C.c_uint32, vp, C.c_size_t, vp]
    L.osmt_scene_read_points.argtypes = [vp, vp, ip]
    L.osmt_project.argtypes = [vp, dp, C.c_size_t, C.c_uint8, C.c_uint32, C.c_uint32, C.c_double, ip]
    L.osmt_composite.argtypes = [vp, dp, dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u8p]
    L.osmt_composite_device.argtypes = [vp, vp, dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.osmt_render_batch_labels.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), u8p, C.c_size_t]
    L.osmt_render_batch_rgb.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), u8p, C.c_size_t]
    L.osmt_scene_set_labels.argtypes = [vp, vp, C.POINTER(abi.LabelBatch)]
    L.osmt_scene_read_label_status.argtypes = [vp, vp, u8p]
    if hasattr(L, "osmt_scene_check"):  # absent only from older variant builds loaded through OSMT_LIB (A/B timing runs)
        L.osmt_scene_check.argtypes = [vp, vp]
        L.osmt_worker_create.argtypes = [vp, C.POINTER(vp)]
        L.osmt_worker_destroy.argtypes = [vp]
        L.osmt_worker_destroy.restype = None
        L.osmt_worker_render.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), u8p, C.c_size_t]
    if hasattr(L, "osmt_render_batch_png_begin"):
        L.osmt_render_batch_png_begin.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), C.POINTER(vp)]
        L.osmt_render_batch_png_end.argtypes = [vp, u8p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.osmt_png_device_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.osmt_png_device_bound.restype = C.c_size_t
    L.osmt_encode_png_device.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.osmt_render_batch_png.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.LabelBatch), u8p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.osmt_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.osmt_host_free.argtypes = [vp, vp]
    L.osmt_host_free.restype = None
    if hasattr(L, "osmt_register_glyphs"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_register_glyphs.argtypes = [vp, C.POINTER(abi.GlyphVertex), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        L.osmt_scene_set_glyph_labels.argtypes = [vp, vp, C.POINTER(abi.GlyphLabelBatch)]
        L.osmt_render_batch_rgb_glyphs.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.GlyphLabelBatch), u8p, C.c_size_t]
        L.osmt_scene_read_label_segs.argtypes = [vp, vp, dp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.osmt_debug_hypot.argtypes = [vp, dp, C.c_size_t, dp]
    if hasattr(L, "osmt_scene_set_text_labels"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_text_labels.argtypes = [C.POINTER(abi.TextLabelBatch), C.c_size_t]
        L.osmt_scene_set_text_labels.argtypes = [vp, vp, C.POINTER(abi.TextLabelBatch)]
        L.osmt_render_batch_rgb_text.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.TextLabelBatch), u8p, C.c_size_t]
        L.osmt_scene_read_glyph_instances.argtypes = [vp, vp, C.POINTER(abi.GlyphInstance), C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_scene_set_string_labels"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_register_font.argtypes = [vp, C.POINTER(abi.FontDesc), C.POINTER(C.c_uint32)]
        L.osmt_validate_string_labels.argtypes = [C.POINTER(abi.StringLabelBatch), C.c_size_t, vp]
        L.osmt_scene_set_string_labels.argtypes = [vp, vp, C.POINTER(abi.StringLabelBatch)]
        L.osmt_render_batch_rgb_strings.argtypes = [vp, C.POINTER(abi.Batch), C.POINTER(abi.StringLabelBatch), u8p, C.c_size_t]
        L.osmt_scene_read_text_glyphs.argtypes = [vp, vp, C.POINTER(abi.TextGlyph), C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_label_positions"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_label_positions.argtypes = [vp, C.POINTER(abi.LabelRequestBatch), vp]
        L.osmt_label_positions_begin.argtypes = [vp, C.POINTER(abi.LabelRequestBatch), C.POINTER(vp)]
        L.osmt_label_positions_end.argtypes = [vp, vp]
        L.osmt_label_positions_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "osmt_scene_read_label_cover"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_scene_read_label_cover.argtypes = [vp, vp, C.c_uint32, ip, dp, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_scene_build_styled"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_geodata.argtypes = [C.POINTER(abi.GeodataDesc)]
        L.osmt_register_geodata.argtypes = [vp, C.POINTER(abi.GeodataDesc), C.POINTER(C.c_uint32)]
        L.osmt_validate_styles.argtypes = [C.POINTER(abi.StyleRec), C.c_size_t, dp, C.c_size_t, vp]
        L.osmt_register_styles.argtypes = [vp, C.POINTER(abi.StyleRec), C.c_size_t, dp, C.c_size_t, C.POINTER(C.c_uint32)]
        L.osmt_validate_styled_batch.argtypes = [C.POINTER(abi.StyledBatch), vp]
        L.osmt_scene_build_styled.argtypes = [vp, C.POINTER(abi.StyledBatch), C.POINTER(vp)]
        L.osmt_scene_read_display_list.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]
        L.osmt_scene_max_tile_ops.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "osmt_scene_build_tiles"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_tile_index.argtypes = [C.POINTER(abi.TileIndexDesc), C.c_size_t, C.c_size_t]
        L.osmt_register_tile_index.argtypes = [vp, C.c_uint32, C.POINTER(abi.TileIndexDesc)]
        L.osmt_validate_style_bindings.argtypes = [C.POINTER(abi.StyleBindingsDesc), vp]
        L.osmt_register_style_bindings.argtypes = [vp, C.POINTER(abi.StyleBindingsDesc), C.POINTER(C.c_uint32)]
        L.osmt_validate_tile_batch.argtypes = [C.POINTER(abi.TileBatch), vp]
        L.osmt_scene_build_tiles.argtypes = [vp, C.POINTER(abi.TileBatch), C.POINTER(vp)]
        L.osmt_scene_read_styled_areas.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_scene_build_tile_labels"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_node_index.argtypes = [C.POINTER(abi.NodeIndexDesc), C.c_uint32, vp]
        L.osmt_register_node_index.argtypes = [vp, C.c_uint32, C.POINTER(abi.NodeIndexDesc)]
        L.osmt_validate_label_styles.argtypes = [C.POINTER(abi.LabelStyleRec), C.c_size_t, vp]
        L.osmt_register_label_styles.argtypes = [vp, C.POINTER(abi.LabelStyleRec), C.c_size_t, C.POINTER(C.c_uint32)]
        L.osmt_validate_label_bindings.argtypes = [C.POINTER(abi.LabelBindingsDesc), vp]
        L.osmt_register_label_bindings.argtypes = [vp, C.POINTER(abi.LabelBindingsDesc), C.POINTER(C.c_uint32)]
        L.osmt_scene_build_tile_labels.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(abi.StringLabelBatch)]
        L.osmt_scene_read_tile_labels.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_scene_build_tile_labels_all"):  # absent only from older variant builds loaded through OSMT_LIB
        for name in ("osmt_validate_area_label_bindings", "osmt_register_area_label_bindings", "osmt_scene_build_tile_labels_all",
                     "osmt_scene_read_declined_anchors", "osmt_scene_read_tile_area_labels"):
            getattr(L, name).restype = C.c_int
        L.osmt_validate_area_label_bindings.argtypes = [C.POINTER(abi.AreaLabelBindingsDesc), vp]
        L.osmt_register_area_label_bindings.argtypes = [vp, C.POINTER(abi.AreaLabelBindingsDesc), C.POINTER(C.c_uint32)]
        L.osmt_scene_build_tile_labels_all.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.c_size_t]
        L.osmt_scene_read_declined_anchors.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.osmt_scene_read_tile_area_labels.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_match_selectors"):  # absent only from older variant builds loaded through OSMT_LIB
        sz = C.POINTER(C.c_size_t)
        L.osmt_validate_tags.argtypes = [C.POINTER(abi.TagsDesc), C.c_uint32, vp]
        L.osmt_register_tags.argtypes = [vp, C.c_uint32, C.POINTER(abi.TagsDesc)]
        L.osmt_validate_selectors.argtypes = [C.POINTER(abi.SelectorsDesc)]
        L.osmt_register_selectors.argtypes = [vp, C.POINTER(abi.SelectorsDesc), C.POINTER(C.c_uint32)]
        L.osmt_match_selectors.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.POINTER(vp)]
        L.osmt_match_free.argtypes = [vp]
        L.osmt_match_free.restype = None
        L.osmt_match_read_declined_numbers.argtypes = [vp, vp, C.c_size_t, sz]
        L.osmt_match_read.argtypes = [vp, vp, vp, vp, sz, sz]
        L.osmt_register_style_bindings_matched.argtypes = [vp, vp, C.c_uint8, C.c_uint8, vp, vp, C.c_size_t, C.POINTER(C.c_uint32)]
        L.osmt_debug_match_hash_bits.argtypes = [vp, C.c_uint32]
    if hasattr(L, "osmt_register_label_bindings_matched"):  # absent only from older variant builds loaded through OSMT_LIB
        sz = C.POINTER(C.c_size_t)
        L.osmt_validate_class_label_bindings.argtypes = [C.POINTER(abi.ClassLabelBindingsDesc), vp, vp]
        L.osmt_register_label_bindings_matched.argtypes = [vp, vp, C.POINTER(abi.ClassLabelBindingsDesc), C.POINTER(C.c_uint32)]
        L.osmt_register_area_label_bindings_matched.argtypes = [vp, vp, C.POINTER(abi.ClassLabelBindingsDesc), C.POINTER(C.c_uint32)]
        L.osmt_read_label_bindings.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, sz, sz]
        L.osmt_read_area_label_bindings.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, sz, sz]
    if hasattr(L, "osmt_cascade_classes"):  # absent only from older variant builds loaded through OSMT_LIB
        sz = C.POINTER(C.c_size_t)
        L.osmt_validate_rules.argtypes = [C.POINTER(abi.RulesDesc), vp]
        L.osmt_register_rules.argtypes = [vp, C.POINTER(abi.RulesDesc), C.POINTER(C.c_uint32)]
        if hasattr(L, "osmt_register_rules_ex"):  # absent only from older variant builds loaded through OSMT_LIB
            L.osmt_validate_rules_ex.argtypes = [C.POINTER(abi.RulesDesc), C.c_uint32, vp]
            L.osmt_register_rules_ex.argtypes = [vp, C.POINTER(abi.RulesDesc), C.c_uint32, C.POINTER(C.c_uint32)]
        L.osmt_cascade_classes.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.osmt_cascade_free.argtypes = [vp]
        L.osmt_cascade_free.restype = None
        L.osmt_cascade_read.argtypes = [vp] * 14 + [sz, sz]
        L.osmt_cascade_register.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp]
    if hasattr(L, "osmt_label_positions_tiles"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_node_mercator.argtypes = [dp, C.c_size_t, C.c_uint32, vp]
        L.osmt_register_node_mercator.argtypes = [vp, C.c_uint32, dp]
        L.osmt_validate_label_tile_batch.argtypes = [C.POINTER(abi.LabelTileBatch), vp]
        L.osmt_label_positions_tiles.argtypes = [vp, C.POINTER(abi.LabelTileBatch), vp]
        L.osmt_label_positions_tiles_begin.argtypes = [vp, C.POINTER(abi.LabelTileBatch), C.POINTER(vp)]
        L.osmt_label_tile_batch_expand.argtypes = [vp, C.POINTER(abi.LabelTileBatch), vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "osmt_render_scene_png"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_render_scene_host.argtypes = [vp, vp, C.c_uint32, vp, C.c_size_t]
        L.osmt_render_scene_png.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.osmt_render_scene_png_begin.argtypes = [vp, vp, C.POINTER(vp)]
        L.osmt_scene_png_work_bytes.argtypes = [vp, vp]
        L.osmt_scene_png_work_bytes.restype = C.c_size_t
        L.osmt_render_scene_png_device.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]
        L.osmt_debug_png_offsets.argtypes = [vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp]
    if hasattr(L, "osmt_register_id_filter"):  # absent only from older variant builds loaded through OSMT_LIB
        u64p, sz = C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.osmt_validate_id_filter.argtypes = [u64p, C.c_size_t, C.c_uint32, vp]
        L.osmt_register_id_filter.argtypes = [vp, C.c_uint32, u64p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.osmt_read_id_filter.argtypes = [vp, C.c_uint32, vp, vp, vp, sz, sz]
        L.osmt_scene_build_tiles_filtered.argtypes = [vp, C.POINTER(abi.TileBatch), C.c_uint32, C.POINTER(vp)]
    if hasattr(L, "osmt_tile_server_create"):  # absent only from older variant builds loaded through OSMT_LIB
        sz = C.POINTER(C.c_size_t)
        L.osmt_validate_tile_server.argtypes = [C.POINTER(abi.TileServerDesc), vp]
        L.osmt_tile_server_create.argtypes = [vp, C.POINTER(abi.TileServerDesc), C.POINTER(vp)]
        L.osmt_tile_server_free.argtypes = [vp]
        L.osmt_tile_server_free.restype = None
        L.osmt_tile_server_render_png.argtypes = [vp, C.POINTER(abi.TileCoord), C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.osmt_last_declined_anchors.argtypes = [vp, C.c_size_t, sz]
        L.osmt_worker_render_tile_png.argtypes = [vp, vp, C.POINTER(abi.TileCoord), C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, sz]
        L.osmt_worker_tile_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "osmt_register_tile_pyramid"):  # absent only from older variant builds loaded through OSMT_LIB
        u32p, sz = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)
        L.osmt_validate_tile_pyramid.argtypes = [C.c_uint32, C.c_uint32, vp]
        L.osmt_register_tile_pyramid.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.osmt_tile_pyramid_levels.argtypes = [vp, C.c_uint32, u32p, u32p]
        L.osmt_read_tile_pyramid.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, sz, sz]
        L.osmt_tile_query_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "osmt_build_tile_index"):  # absent only from older variant builds loaded through OSMT_LIB
        u64p, sz = C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.osmt_validate_tile_index_build.argtypes = [C.c_uint32, u64p, C.c_size_t, vp]
        L.osmt_build_tile_index.argtypes = [vp, C.c_uint32, u64p, C.c_size_t]
        L.osmt_read_tile_index.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, sz, sz]
    if hasattr(L, "osmt_assemble_multipolygons"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_relations.argtypes = [vp]
        L.osmt_assemble_multipolygons.argtypes = [vp, vp, C.POINTER(vp)]
        L.osmt_polygons_counts.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.osmt_polygons_read.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.osmt_polygons_free.argtypes = [vp]
        L.osmt_polygons_free.restype = None
        L.osmt_debug_vertex_hash_bits.argtypes = [vp, C.c_uint32]
    if hasattr(L, "osmt_resolve_refs"):  # absent only from older variant builds loaded through OSMT_LIB
        L.osmt_validate_resolve.argtypes = [vp]
        L.osmt_resolve_refs.argtypes = [vp, vp, C.POINTER(vp)]
        L.osmt_resolved_counts.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.osmt_resolved_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.osmt_resolved_free.argtypes = [vp]
        L.osmt_resolved_free.restype = None
        L.osmt_debug_resolve_short_way_max.argtypes = [vp, C.c_uint32]
    L.osmt_png_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.osmt_png_bound.restype = C.c_size_t
    L.osmt_encode_png.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_int, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    _lib = L
    return L


def check(rc):
    if rc != abi.OK:
        raise OsmtError(rc, load().osmt_last_error().decode("utf-8", "replace"))
