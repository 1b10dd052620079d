"""Styled batches: the inputs of osmt_scene_build_styled, backed by numpy arrays.

Instead of a display list the caller registers a geodata file's topology (Geodata) and its stylesheet's Style records
(STYLE_REC_DTYPE) once per context and sends, per tile, the (entity, style) pairs Styler::style_entities pushes
(reference: src/mapcss/styler.rs:86-92,163-203); the GPU builds the display list.  The dtypes mirror include/osmtile.h.
"""
import ctypes as C

import numpy as np

from . import abi

STYLE_REC_DTYPE = np.dtype(
    [
        ("layer", "<i8"), ("z_index", "<f8"), ("opacity", "<f8"), ("fill_opacity", "<f8"), ("width", "<f8"), ("casing_width", "<f8"),
        ("fill_image", "<u4"), ("dashes_off", "<u4"), ("n_dashes", "<u4"), ("casing_dashes_off", "<u4"), ("n_casing_dashes", "<u4"),
        ("has_layer", "u1"), ("is_foreground_fill", "u1"),
        ("has_color", "u1"), ("color", "u1", (3,)),
        ("has_fill_color", "u1"), ("fill_color", "u1", (3,)),
        ("has_opacity", "u1"), ("has_fill_opacity", "u1"), ("has_width", "u1"), ("has_dashes", "u1"), ("line_cap", "u1"),
        ("has_casing_color", "u1"), ("casing_color", "u1", (3,)),
        ("has_casing_width", "u1"), ("has_casing_dashes", "u1"), ("casing_line_cap", "u1"), ("has_fill_image", "u1"),
        ("has_background_color", "u1"), ("background_color", "u1", (3,)),
        ("_pad", "u1"),
    ]
)
STYLED_AREA_DTYPE = np.dtype([("entity", "<u4"), ("style", "<u4")])
STYLED_TILE_DTYPE = np.dtype(
    [("x", "<u4"), ("y", "<u4"), ("zoom", "u1"), ("has_canvas", "u1"), ("canvas_rgb", "u1", (3,)), ("_pad", "u1", (3,)), ("area_off", "<u4"),
     ("n_areas", "<u4")]
)
QUERY_TILE_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("zoom", "u1"), ("has_canvas", "u1"), ("canvas_rgb", "u1", (3,)), ("_pad", "u1", (3,))])
assert QUERY_TILE_DTYPE.itemsize == 16
assert STYLE_REC_DTYPE.itemsize == 96 and STYLED_AREA_DTYPE.itemsize == 8 and STYLED_TILE_DTYPE.itemsize == 24


def _csr(lists, dtype=np.uint32):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    if len(lists):
        off[1:] = np.cumsum([len(v) for v in lists])
    flat = np.array([x for v in lists for x in v], dtype=dtype)
    return off, flat


class Geodata:
    """The flat arrays of osmt_geodata_desc.  nodes: [n, 2] (lat, lon); ways: [(global id, [node idx])]; polygons:
    [[node idx]]; multipolygons: [(global id, [polygon idx])]."""

    def __init__(self, nodes, ways=(), polygons=(), multipolygons=()):
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 2)
        self.way_ids = np.array([w[0] for w in ways], dtype=np.uint64)
        self.way_node_off, self.way_nodes = _csr([w[1] for w in ways])
        self.polygon_node_off, self.polygon_nodes = _csr(list(polygons))
        self.multipolygon_ids = np.array([m[0] for m in multipolygons], dtype=np.uint64)
        self.multipolygon_polygon_off, self.multipolygon_polygons = _csr([m[1] for m in multipolygons])

    @classmethod
    def from_arrays(cls, nodes, way_ids, way_node_off, way_nodes, polygons):
        """A Geodata over flat arrays: the ways as they are, the polygon and multipolygon arrays from `polygons`, the dict
        Context.assemble_multipolygons returns (or any with its five array names)."""
        g = cls(nodes)
        g.way_ids = np.ascontiguousarray(way_ids, dtype=np.uint64).reshape(-1)
        g.way_node_off, g.way_nodes = np.ascontiguousarray(way_node_off, dtype=np.uint32), np.ascontiguousarray(way_nodes, dtype=np.uint32)
        g.polygon_node_off, g.polygon_nodes = np.ascontiguousarray(polygons["polygon_node_off"], dtype=np.uint32), np.ascontiguousarray(polygons["polygon_nodes"], dtype=np.uint32)
        g.multipolygon_ids = np.ascontiguousarray(polygons["multipolygon_ids"], dtype=np.uint64)
        g.multipolygon_polygon_off = np.ascontiguousarray(polygons["multipolygon_polygon_off"], dtype=np.uint32)
        g.multipolygon_polygons = np.ascontiguousarray(polygons["multipolygon_polygons"], dtype=np.uint32)
        return g

    def as_desc(self):
        """ctypes osmt_geodata_desc pointing into this object's arrays (keep `self` alive)."""
        u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        d = abi.GeodataDesc()
        d.nodes, d.n_nodes = self.nodes.ctypes.data_as(C.POINTER(C.c_double)), len(self.nodes)
        d.way_ids, d.way_node_off, d.n_ways = self.way_ids.ctypes.data_as(u64), self.way_node_off.ctypes.data_as(u32), len(self.way_ids)
        d.way_nodes, d.n_way_nodes = self.way_nodes.ctypes.data_as(u32), len(self.way_nodes)
        d.polygon_node_off, d.n_polygons = self.polygon_node_off.ctypes.data_as(u32), len(self.polygon_node_off) - 1
        d.polygon_nodes, d.n_polygon_nodes = self.polygon_nodes.ctypes.data_as(u32), len(self.polygon_nodes)
        d.multipolygon_ids, d.multipolygon_polygon_off = self.multipolygon_ids.ctypes.data_as(u64), self.multipolygon_polygon_off.ctypes.data_as(u32)
        d.n_multipolygons = len(self.multipolygon_ids)
        d.multipolygon_polygons, d.n_multipolygon_polygons = self.multipolygon_polygons.ctypes.data_as(u32), len(self.multipolygon_polygons)
        return d


RELATION_STATUS_DTYPE = np.dtype([("accepted", "<u4"), ("rings_built", "<u4"), ("unmatched", "<u4")])
assert RELATION_STATUS_DTYPE.itemsize == 12


class Relations:
    """The flat arrays of osmt_relations_desc.  nodes: [n, 2] (lat, lon), compared by their bits; ways: [[node idx]];
    relations: [(global id, [(way idx, inner)])] with inner 0 / 1 (the importer's role)."""

    def __init__(self, nodes, ways=(), relations=()):
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 2)
        self.way_node_off, self.way_nodes = _csr([list(w) for w in ways])
        self.relation_ids = np.array([r[0] for r in relations], dtype=np.uint64)
        self.relation_way_off, self.relation_ways = _csr([[w for w, _ in r[1]] for r in relations])
        self.relation_way_inner = np.array([i for r in relations for _, i in r[1]], dtype=np.uint8)

    @classmethod
    def from_resolved(cls, nodes, relation_ids, resolved):
        """The relations of a resolution: `resolved` is the dict Context.resolve_refs returns (or any with its five array
        names), relation_ids the relations' global ids in the order the RawOsm listed them."""
        r = cls(nodes)
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        r.way_node_off, r.way_nodes = u32(resolved["way_node_off"]), u32(resolved["way_nodes"])
        r.relation_ids = np.ascontiguousarray(relation_ids, dtype=np.uint64).reshape(-1)
        r.relation_way_off, r.relation_ways = u32(resolved["relation_way_off"]), u32(resolved["relation_ways"])
        r.relation_way_inner = np.ascontiguousarray(resolved["relation_way_inner"], dtype=np.uint8).reshape(-1)
        if len(r.relation_way_off) != len(r.relation_ids) + 1:
            raise ValueError(f"{len(r.relation_ids)} relation ids for {len(r.relation_way_off) - 1} resolved relations")
        return r

    def as_desc(self):
        """ctypes osmt_relations_desc pointing into this object's arrays (keep `self` alive)."""
        u32 = C.POINTER(C.c_uint32)
        d = abi.RelationsDesc()
        d.nodes, d.n_nodes = self.nodes.ctypes.data_as(C.POINTER(C.c_double)), len(self.nodes)
        d.way_node_off, d.n_ways = self.way_node_off.ctypes.data_as(u32), len(self.way_node_off) - 1
        d.way_nodes, d.n_way_nodes = self.way_nodes.ctypes.data_as(u32), len(self.way_nodes)
        d.relation_ids, d.relation_way_off = self.relation_ids.ctypes.data_as(C.POINTER(C.c_uint64)), self.relation_way_off.ctypes.data_as(u32)
        d.n_relations = len(self.relation_ids)
        d.relation_ways, d.relation_way_inner = self.relation_ways.ctypes.data_as(u32), self.relation_way_inner.ctypes.data_as(C.POINTER(C.c_uint8))
        d.n_relation_ways = len(self.relation_ways)
        return d


class RawOsm:
    """The flat arrays of osmt_raw_osm_desc: elements as a parser hands them over, per kind and in file order.  node_ids:
    global ids; ways: [(global id, [node id])]; relations: [(global id, [(way id, inner)])] with the type="way" members only
    and inner 0 / 1.  nodes_seen [n ways] / ways_seen [n relations]: how many nodes (ways) precede each way (relation) in the
    file, None: all of them.  relation_ids is kept for styled.Relations.from_resolved; the resolution does not read it."""

    def __init__(self, node_ids, ways=(), relations=(), nodes_seen=None, ways_seen=None):
        u64 = lambda v: np.array([int(x) for x in v], dtype=np.uint64)
        self.node_ids = u64(node_ids)
        self.way_ids = u64([w[0] for w in ways])
        self.way_ref_off = np.concatenate([[0], np.cumsum([len(w[1]) for w in ways], dtype=np.int64)]).astype(np.uint32)
        self.way_refs = u64([g for w in ways for g in w[1]])
        self.relation_ids = u64([r[0] for r in relations])
        self.relation_ref_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in relations], dtype=np.int64)]).astype(np.uint32)
        self.relation_refs = u64([g for r in relations for g, _ in r[1]])
        self.relation_ref_inner = np.array([i for r in relations for _, i in r[1]], dtype=np.uint8)
        self.way_nodes_seen = None if nodes_seen is None else np.array(nodes_seen, dtype=np.uint32).reshape(-1)
        self.relation_ways_seen = None if ways_seen is None else np.array(ways_seen, dtype=np.uint32).reshape(-1)
        if self.way_nodes_seen is not None and len(self.way_nodes_seen) != len(self.way_ids):
            raise ValueError(f"nodes_seen has {len(self.way_nodes_seen)} entries for {len(self.way_ids)} ways")
        if self.relation_ways_seen is not None and len(self.relation_ways_seen) != len(self.relation_ids):
            raise ValueError(f"ways_seen has {len(self.relation_ways_seen)} entries for {len(self.relation_ids)} relations")

    def as_desc(self):
        """ctypes osmt_raw_osm_desc pointing into this object's arrays (keep `self` alive)."""
        u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        d = abi.RawOsmDesc()
        d.node_ids, d.n_nodes = self.node_ids.ctypes.data_as(u64), len(self.node_ids)
        d.way_ids, d.way_ref_off, d.n_ways = self.way_ids.ctypes.data_as(u64), self.way_ref_off.ctypes.data_as(u32), len(self.way_ids)
        d.way_refs, d.n_way_refs = self.way_refs.ctypes.data_as(u64), len(self.way_refs)
        d.relation_ref_off, d.n_relations = self.relation_ref_off.ctypes.data_as(u32), len(self.relation_ref_off) - 1
        d.relation_refs, d.relation_ref_inner = self.relation_refs.ctypes.data_as(u64), self.relation_ref_inner.ctypes.data_as(C.POINTER(C.c_uint8))
        d.n_relation_refs = len(self.relation_refs)
        if self.way_nodes_seen is not None:
            d.way_nodes_seen = self.way_nodes_seen.ctypes.data_as(u32)
        if self.relation_ways_seen is not None:
            d.relation_ways_seen = self.relation_ways_seen.ctypes.data_as(u32)
        return d


class StyledBatch:
    """osmt_styled_batch.  tiles: [(zoom, x, y, ways, multipolygons)] with ways / multipolygons lists of (local id, style
    id) in the order Styler::style_entities pushes them; canvas: (r, g, b) or None."""

    def __init__(self, geodata_id, tiles, scale=1, use_caps_for_dashes=True, canvas=(241, 238, 232)):
        self.geodata_id, self.scale, self.use_caps_for_dashes = int(geodata_id), int(scale), bool(use_caps_for_dashes)
        self.tiles = np.zeros(len(tiles), STYLED_TILE_DTYPE)
        areas = []
        for t, (zoom, x, y, ways, mps) in zip(self.tiles, tiles):
            t["zoom"], t["x"], t["y"] = zoom, x, y
            if canvas is not None:
                t["has_canvas"], t["canvas_rgb"] = 1, canvas
            t["area_off"], t["n_areas"] = len(areas), len(ways) + len(mps)
            areas += [(int(i), int(s)) for i, s in ways] + [(int(i) | abi.STYLED_MULTIPOLYGON, int(s)) for i, s in mps]
        self.areas = np.array(areas, dtype=STYLED_AREA_DTYPE).reshape(-1)

    @property
    def n_jobs(self):
        return len(self.tiles)

    def as_batch(self):
        b = abi.StyledBatch()
        b.tiles, b.n_tiles = self.tiles.ctypes.data_as(C.POINTER(abi.StyledTile)), len(self.tiles)
        b.areas, b.n_areas = self.areas.ctypes.data_as(C.POINTER(abi.StyledArea)), len(self.areas)
        b.geodata_id, b.scale, b.use_caps_for_dashes = self.geodata_id, self.scale, int(self.use_caps_for_dashes)
        return b


class TileIndex:
    """osmt_tile_index_desc: the z18 tile storage of a geodata file.  tiles: {(x, y): (way ids, multipolygon ids)} or a
    list of ((x, y), way ids, multipolygon ids) in the order to hand over (strictly ascending (x, y) is what registers)."""

    def __init__(self, tiles):
        if isinstance(tiles, dict):
            tiles = [(k, tiles[k][0], tiles[k][1]) for k in sorted(tiles)]
        self.tile_xy = np.array([k for k, _, _ in tiles], dtype=np.uint32).reshape(-1, 2)
        self.way_off, self.ways = _csr([list(w) for _, w, _ in tiles])
        self.multipolygon_off, self.multipolygons = _csr([list(m) for _, _, m in tiles])

    def as_desc(self):
        """ctypes osmt_tile_index_desc pointing into this object's arrays (keep `self` alive)."""
        u32 = C.POINTER(C.c_uint32)
        d = abi.TileIndexDesc()
        d.tile_xy, d.n_tiles = self.tile_xy.ctypes.data_as(u32), len(self.tile_xy)
        d.way_off, d.ways, d.n_way_refs = self.way_off.ctypes.data_as(u32), self.ways.ctypes.data_as(u32), len(self.ways)
        d.multipolygon_off, d.multipolygons = self.multipolygon_off.ctypes.data_as(u32), self.multipolygons.ctypes.data_as(u32)
        d.n_multipolygon_refs = len(self.multipolygons)
        return d


class StyleBindings:
    """osmt_style_bindings_desc: per way and per multipolygon the style ids Styler::style_entities pushes for it at zooms
    zoom_lo..zoom_hi, in push order.  way_styles / multipolygon_styles: one list of style ids per entity."""

    def __init__(self, geodata_id, zoom_lo, zoom_hi, way_styles, multipolygon_styles=()):
        self.geodata_id, self.zoom_lo, self.zoom_hi = int(geodata_id), int(zoom_lo), int(zoom_hi)
        self.way_style_off, self.way_styles = _csr([list(v) for v in way_styles])
        self.multipolygon_style_off, self.multipolygon_styles = _csr([list(v) for v in multipolygon_styles])

    def as_desc(self):
        u32 = C.POINTER(C.c_uint32)
        d = abi.StyleBindingsDesc()
        d.geodata_id, d.zoom_lo, d.zoom_hi = self.geodata_id, self.zoom_lo, self.zoom_hi
        d.way_style_off, d.way_styles, d.n_way_styles = self.way_style_off.ctypes.data_as(u32), self.way_styles.ctypes.data_as(u32), len(self.way_styles)
        d.multipolygon_style_off, d.multipolygon_styles = self.multipolygon_style_off.ctypes.data_as(u32), self.multipolygon_styles.ctypes.data_as(u32)
        d.n_multipolygon_styles = len(self.multipolygon_styles)
        return d


class TileBatch:
    """osmt_tile_batch.  tiles: [(zoom, x, y)]; bindings: {zoom: bindings id} (a zoom that is missing has none); canvas:
    (r, g, b) or None."""

    def __init__(self, geodata_id, tiles, bindings, scale=1, use_caps_for_dashes=True, canvas=(241, 238, 232)):
        self.geodata_id, self.scale, self.use_caps_for_dashes = int(geodata_id), int(scale), bool(use_caps_for_dashes)
        self.bindings = {int(z): int(i) for z, i in dict(bindings).items()}
        self.tiles = np.zeros(len(tiles), QUERY_TILE_DTYPE)
        for t, (zoom, x, y) in zip(self.tiles, tiles):
            t["zoom"], t["x"], t["y"] = zoom, x, y
            if canvas is not None:
                t["has_canvas"], t["canvas_rgb"] = 1, canvas

    @property
    def n_jobs(self):
        return len(self.tiles)

    def as_batch(self):
        b = abi.TileBatch()
        b.tiles, b.n_tiles = self.tiles.ctypes.data_as(C.POINTER(abi.QueryTile)), len(self.tiles)
        b.geodata_id, b.scale, b.use_caps_for_dashes = self.geodata_id, self.scale, int(self.use_caps_for_dashes)
        for z in range(abi.MAX_ZOOM + 1):
            b.bindings_of_zoom[z] = self.bindings.get(z, abi.BINDINGS_NONE)
        return b


LABEL_STYLE_REC_DTYPE = np.dtype(
    [
        ("layer", "<i8"), ("z_index", "<f8"), ("font_size", "<f8"), ("icon_image", "<u4"), ("font_id", "<u4"),
        ("has_layer", "u1"), ("has_icon", "u1"), ("has_text_style", "u1"), ("has_font_size", "u1"),
        ("has_text_color", "u1"), ("text_color", "u1", (3,)), ("text_position", "u1"), ("_pad", "u1", (7,)),
    ]
)
LABEL_BINDING_DTYPE = np.dtype([("style", "<u4"), ("text", "<u4")])
assert LABEL_STYLE_REC_DTYPE.itemsize == 48 and LABEL_BINDING_DTYPE.itemsize == 8


class NodeIndex:
    """osmt_node_index_desc: the nodes' global ids and the node lists of the z18 tiles of the TileIndex registered for the
    same geodata id.  tiles: one list of local node ids per index tile, in the index's order."""

    def __init__(self, node_ids, tiles):
        self.node_ids = np.array(node_ids, dtype=np.uint64).reshape(-1)
        self.node_off, self.nodes = _csr([list(v) for v in tiles])

    def as_desc(self):
        u32 = C.POINTER(C.c_uint32)
        d = abi.NodeIndexDesc()
        d.node_ids, d.n_nodes = self.node_ids.ctypes.data_as(C.POINTER(C.c_uint64)), len(self.node_ids)
        d.node_off, d.nodes, d.n_node_refs = self.node_off.ctypes.data_as(u32), self.nodes.ctypes.data_as(u32), len(self.nodes)
        return d


class LabelBindings:
    """osmt_label_bindings_desc: per node the (label style id, text id) pairs Styler::style_entities pushes for it at zooms
    zoom_lo..zoom_hi, in push order.  node_bindings: one list of (style, text id or None) per node; texts: the pool, each a
    str or a list of code points."""

    def __init__(self, geodata_id, zoom_lo, zoom_hi, node_bindings, texts=()):
        self.geodata_id, self.zoom_lo, self.zoom_hi = int(geodata_id), int(zoom_lo), int(zoom_hi)
        self.node_off = np.zeros(len(node_bindings) + 1, dtype=np.uint32)
        if len(node_bindings):
            self.node_off[1:] = np.cumsum([len(v) for v in node_bindings])
        flat = [(int(s), abi.TEXT_NONE if t is None else int(t)) for v in node_bindings for s, t in v]
        self.bindings = np.array(flat, dtype=LABEL_BINDING_DTYPE).reshape(-1)
        self.text_off, self.chars = _csr([[ord(c) for c in t] if isinstance(t, str) else list(t) for t in texts])

    def as_desc(self):
        u32 = C.POINTER(C.c_uint32)
        d = abi.LabelBindingsDesc()
        d.geodata_id, d.zoom_lo, d.zoom_hi = self.geodata_id, self.zoom_lo, self.zoom_hi
        d.node_off, d.bindings, d.n_bindings = self.node_off.ctypes.data_as(u32), self.bindings.ctypes.data_as(C.POINTER(abi.LabelBinding)), len(self.bindings)
        d.text_off, d.n_texts = self.text_off.ctypes.data_as(u32), len(self.text_off) - 1
        d.chars, d.n_chars = self.chars.ctypes.data_as(u32), len(self.chars)
        return d


class AreaLabelBindings:
    """osmt_area_label_bindings_desc: per way and per multipolygon the (label style id, text id) pairs
    Styler::style_entities pushes for it at zooms zoom_lo..zoom_hi, in push order.  way_bindings / multipolygon_bindings: one
    list of (style, text id or None) per entity; texts: the pool, each a str or a list of code points."""

    def __init__(self, geodata_id, zoom_lo, zoom_hi, way_bindings, multipolygon_bindings, texts=()):
        self.geodata_id, self.zoom_lo, self.zoom_hi = int(geodata_id), int(zoom_lo), int(zoom_hi)

        def csr(rows):
            off = np.zeros(len(rows) + 1, dtype=np.uint32)
            if len(rows):
                off[1:] = np.cumsum([len(v) for v in rows])
            flat = [(int(s), abi.TEXT_NONE if t is None else int(t)) for v in rows for s, t in v]
            return off, np.array(flat, dtype=LABEL_BINDING_DTYPE).reshape(-1)

        self.way_off, self.way_bindings = csr(way_bindings)
        self.multipolygon_off, self.multipolygon_bindings = csr(multipolygon_bindings)
        self.text_off, self.chars = _csr([[ord(c) for c in t] if isinstance(t, str) else list(t) for t in texts])

    def as_desc(self):
        u32, lb = C.POINTER(C.c_uint32), C.POINTER(abi.LabelBinding)
        d = abi.AreaLabelBindingsDesc()
        d.geodata_id, d.zoom_lo, d.zoom_hi = self.geodata_id, self.zoom_lo, self.zoom_hi
        d.way_off, d.way_bindings, d.n_way_bindings = self.way_off.ctypes.data_as(u32), self.way_bindings.ctypes.data_as(lb), len(self.way_bindings)
        d.multipolygon_off, d.multipolygon_bindings = self.multipolygon_off.ctypes.data_as(u32), self.multipolygon_bindings.ctypes.data_as(lb)
        d.n_multipolygon_bindings = len(self.multipolygon_bindings)
        d.text_off, d.n_texts = self.text_off.ctypes.data_as(u32), len(self.text_off) - 1
        d.chars, d.n_chars = self.chars.ctypes.data_as(u32), len(self.chars)
        return d
