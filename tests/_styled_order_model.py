"""The draw order of a tile's styled areas, stated once more and independently of osmt::SceneBuilder, k_styled_sort and the
Python twin of tests/test_styled_builder.py: one numpy lexsort over the ordering rules of Styler::style_areas
(mapcss/styler.rs:163-203,246-272) — layer (0 without one), background fill before foreground fill, z-index with
-0.0 == +0.0, global id as an unsigned 64-bit number, the relation before the way where all of that is equal
(styler.rs:186), then input order (Rust's sort_by is stable).

An order is read OUT of a display list through marks: where every style has colours of its own and every entity owns its
nodes, (colour, first node reference of the op's first ring) names (style, entity).  Two areas with the same entity and
style emit identical ops; their mutual order cannot be seen and does not matter."""
import numpy as np


def draw_order(way_pairs, mp_pairs, st, way_gids, mp_gids):
    """way_pairs / mp_pairs: [(local id, style index)] in input order -> (order, entity, style, is_way): `order` indexes
    the concatenation ways + multipolygons, which the other three arrays describe"""
    w = np.array(way_pairs, dtype=np.int64).reshape(-1, 2)
    m = np.array(mp_pairs, dtype=np.int64).reshape(-1, 2)
    entity, style = np.concatenate([w[:, 0], m[:, 0]]), np.concatenate([w[:, 1], m[:, 1]])
    is_way = np.concatenate([np.ones(len(w), np.uint8), np.zeros(len(m), np.uint8)])
    gid = np.concatenate([np.array(way_gids, dtype=np.uint64)[w[:, 0]], np.array(mp_gids, dtype=np.uint64)[m[:, 0]]])
    s = st[style]
    layer = np.where(s["has_layer"] != 0, s["layer"], 0)
    position = np.arange(len(entity))
    order = np.lexsort((position, is_way, gid, s["z_index"] + 0.0, s["is_foreground_fill"] != 0, layer))
    return order, entity, style, is_way


def _mark(colour, node):
    c = np.asarray(colour, dtype=np.uint64).reshape(-1, 3)
    return (c[:, 0] << np.uint64(48)) | (c[:, 1] << np.uint64(40)) | (c[:, 2] << np.uint64(32)) | np.asarray(node, dtype=np.uint64)


def expected_marks(way_pairs, mp_pairs, st, way_gids, mp_gids, way_first_node, mp_first_node):
    """the marks of the ops the three passes of Drawer::draw_to_pixels (drawer.rs:60-99) emit for the tile; *_first_node: per
    entity the first node of its first ring of at least two nodes, -1 where it has none (no op)"""
    order, entity, style, is_way = draw_order(way_pairs, mp_pairs, st, way_gids, mp_gids)
    entity, style, is_way = entity[order], style[order], is_way[order] != 0
    wf, mf = np.asarray(way_first_node, dtype=np.int64), np.asarray(mp_first_node, dtype=np.int64)
    first = np.where(is_way, wf[np.where(is_way, entity, 0)] if len(wf) else -1, mf[np.where(is_way, 0, entity)] if len(mf) else -1)
    s = st[style]
    out = []
    passes = ((s["has_fill_color"] != 0, "fill_color"), ((s["has_casing_color"] != 0) & (s["has_casing_width"] != 0) & is_way, "casing_color"),
              ((s["has_color"] != 0) & is_way, "color"))
    for draws, key in passes:
        sel = draws & (first >= 0)
        out.append(_mark(s[key][sel], first[sel]))
    return np.concatenate(out)


def seen_marks(dl, j):
    """the marks of the ops of job j of a display list with node references"""
    job = dl.jobs[j]
    ops = dl.ops[int(job["op_off"]) : int(job["op_off"]) + int(job["n_ops"])]
    if len(ops) == 0:
        return np.zeros(0, np.uint64)
    return _mark(ops["color"], dl.coords[dl.rings["first_pt"][ops["ring_off"]]])


def first_nodes(r):
    """(per way, per multipolygon) of a tests._geodata.Reader: the first node of the first ring of at least two nodes, or -1"""
    ways = []
    for i in range(r.n_ways):
        n = r.way_nodes(i)
        ways.append(n[0] if len(n) >= 2 else -1)
    mps = []
    for i in range(r.n_multipolygons):
        rings = [r.polygon_nodes(p) for p in r.multipolygon_polygons(i)]
        mps.append(next((n[0] for n in rings if len(n) >= 2), -1))
    return ways, mps


def gids(r):
    return [r.global_id(1, i) for i in range(r.n_ways)], [r.global_id(2, i) for i in range(r.n_multipolygons)]
