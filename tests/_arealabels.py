"""Shared helpers of the area-label tests (tests/test_area_labels_cpu.py, tests/test_gpu_area_labels.py): the shim over
osm_renderer_amd/host/osmt_arealabels.hpp (osmt::AreaLabelBindings, the host mirror osmt::area_labels_of_tile), a Python
restatement of the way and multipolygon labels of a tile written from styler.rs, labeler.rs, text_placer.rs and reader.rs
alone — the order literally as sort, sort, merge, and once more as the device's one sort — and a small world of ways,
polygons and multipolygons whose shapes are stated in pixels of a z18 tile and whose tile index is placed freely."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, labels, styled
from osm_renderer_amd.labels import LABEL_DTYPE, STRING_RUN_DTYPE, StringLabelList
from tests._anchors import latlon_of_px
from tests._geodata import ROOT, Reader, write_geodata
from tests._tilequery import rect

MP = abi.STYLED_MULTIPOLYGON
SHIM = os.path.join(ROOT, "tests", "_build", "libarealabels_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "arealabels_host_main")
HOST_DEMO = os.path.join(ROOT, "tests", "_build", "arealabels_host_demo")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h)
         for h in ("osmt_arealabels.hpp", "osmt_tilelabels.hpp", "osmt_labelable.hpp", "osmt_styled.hpp", "osmt_draw.hpp", "osmt_geodata.hpp")]
_HDRS.append(os.path.join(ROOT, "include", "osmtile.h"))
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "arealabels_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.al_bindings_new.restype = vp
        L.al_bindings_new.argtypes = [C.c_uint32, C.c_uint8, C.c_uint8, sz, u32p, vp, sz, u32p, vp, sz, u32p, u32p]
        L.al_bindings_get.restype = C.POINTER(abi.AreaLabelBindingsDesc)
        L.al_bindings_get.argtypes = [vp]
        L.al_bindings_free.argtypes = [vp]
        L.al_labels.restype = None
        L.al_labels.argtypes = [vp, vp, vp, u32p, sz, C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
        L.al_sizeof.restype = sz
        L.al_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt_arealabels.hpp, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "arealabels_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def build_demo():
    """tests/arealabels_host_demo.cpp: TileScene::build_all_labels of host/osmt_draw.hpp, linked to libosmtile.so"""
    src = os.path.join(ROOT, "tests", "arealabels_host_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    lib = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(lib), "build libosmtile.so first (__graft_entry__.build())"
    if _stale(HOST_DEMO, [src, lib, os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_tilequery.hpp")] + _HDRS):
        os.makedirs(os.path.dirname(HOST_DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", HOST_DEMO, src, "-L" + libdir, "-losmtile",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    return HOST_DEMO


# ---- a world of ways and multipolygons ----------------------------------------------------------------------------------
class World:
    """Shapes are stated in pixels of the z18 tile `tile`; ways / polygons / multipolygons name the nodes; `refs` places every
    way and multipolygon in index tiles of the caller's choice.  write() -> (Reader, refs as written)."""

    def __init__(self, tile):
        self.tile = tile
        self.nodes, self.ways, self.polygons, self.mps, self.refs = [], [], [], [], {}

    def shape(self, pts_px, tile=None):
        ids = []
        for px, py in np.asarray(pts_px, np.float64).reshape(-1, 2):
            lat, lon = latlon_of_px(float(px), float(py), tile or self.tile)
            self.nodes.append((7000 + len(self.nodes), lat, lon, {}))
            ids.append(len(self.nodes) - 1)
        return ids

    def way(self, node_ids, gid, tiles=None):
        self.ways.append((int(gid), list(node_ids), {}))
        for k in tiles if tiles is not None else [self.tile]:
            self.refs.setdefault(tuple(k), ([], [], []))[1].append(len(self.ways) - 1)
        return len(self.ways) - 1

    def polygon(self, node_ids):
        self.polygons.append(list(node_ids))
        return len(self.polygons) - 1

    def mp(self, polygon_ids, gid, tiles=None):
        self.mps.append((int(gid), list(polygon_ids), {}))
        for k in tiles if tiles is not None else [self.tile]:
            self.refs.setdefault(tuple(k), ([], [], []))[2].append(len(self.mps) - 1)
        return len(self.mps) - 1

    def write(self, path):
        write_geodata(str(path), self.nodes, self.ways, self.polygons, self.mps, tile_refs=self.refs)
        return Reader(str(path)), self.refs

    # what the restatement asks
    def way_gids(self):
        return [w[0] for w in self.ways]

    def mp_gids(self):
        return [m[0] for m in self.mps]

    def mp_polygon_counts(self):
        return [len(m[1]) for m in self.mps]


def feature_world(tile, gids, w=None):
    """The shapes the label rules turn on, around the z18 tile `tile`: ways of 0, 1, 2 and 3 nodes and closed ones, one walked
    from its end (first.x > last.x), a vertical one (first.x == last.x), one with a zero-length edge; multipolygons of several
    polygons whose largest ring is not the first, one without polygons (dropped by the query), one whose first polygon is
    empty (no anchor); entities listed by two index tiles and by a far one.  gids: five global ids; gids[3] is shared by way 4
    and multipolygon 0, gids[0] by way 0 and multipolygon 3, gids[2] by way 2 and multipolygon 2."""
    w = w or World(tile)
    cx, cy = tile
    near, east, far = (cx, cy), (cx + 1, cy), (cx + 40, cy + 3)
    sq = lambda x, y, s: [(x, y), (x + s, y), (x + s, y + s), (x, y + s), (x, y)]
    w.way(w.shape(sq(20, 20, 60), near), gids[0], [near])
    w.way(w.shape([(200, 40), (120, 90), (60, 200)], near), gids[1], [near, east])       # first.x > last.x
    w.way(w.shape([(10, 10)], near), gids[2], [near])
    w.way([], 5, [near])
    w.way(w.shape([(30, 100), (30, 220)], near), gids[3], [near])                        # vertical
    w.way(w.shape(sq(300, 10, 40), near), 900, [east])
    w.way(w.shape([(5, 5), (90, 40), (250, 45)], far), 901, [far])
    w.way(w.shape([(50, 50), (50, 50), (80, 50)], near), gids[4], [near])                # a zero-length edge
    p = [w.polygon(w.shape(sq(100, 100, 30), near)), w.polygon(w.shape(sq(10, 150, 90), near)), w.polygon([]), w.polygon(w.shape(sq(40, 180, 20), near))]
    w.mp([p[0], p[1], p[3]], gids[3], [near, east])                                      # the largest ring is not the first
    w.mp([], 11, [near])                                                                 # no polygons: dropped by the query
    w.mp([p[2], p[0]], gids[2], [near])                                                  # first polygon empty: NONE
    w.mp([p[1]], gids[0], [near, far])
    w.mp([w.polygon(w.shape(sq(20, 20, 200), far))], 902, [far])
    return w


class Mirror:
    """osmt::AreaLabelBindings + osmt::area_labels_of_tile over a tests._geodata.Reader"""

    def __init__(self, r, way_bindings, mp_bindings, texts, geodata_id=0, zoom_lo=0, zoom_hi=18):
        self.r = r
        self.b = styled.AreaLabelBindings(geodata_id, zoom_lo, zoom_hi, way_bindings, mp_bindings, texts)
        b = self.b
        u32 = C.POINTER(C.c_uint32)
        self.h = shim().al_bindings_new(geodata_id, zoom_lo, zoom_hi, len(way_bindings), b.way_off.ctypes.data_as(u32), b.way_bindings.ctypes.data,
                                        len(mp_bindings), b.multipolygon_off.ctypes.data_as(u32), b.multipolygon_bindings.ctypes.data,
                                        len(b.text_off) - 1, b.text_off.ctypes.data_as(u32), b.chars.ctypes.data_as(u32))

    def desc(self):
        return shim().al_bindings_get(self.h).contents

    def labels(self, styles, icon_h, zoom, x, y, scale=1, pts=None, way_pos=None, mp_pos=None):
        """(labels, runs, chars, way_pts, way_sincos) of one tile; pts: None = the libm projection, else int32 [n_nodes, 2];
        way_pos / mp_pos: None = get_label_position on the host, else labels.LABEL_POSITION_DTYPE per way / multipolygon"""
        styles = np.ascontiguousarray(styles, dtype=styled.LABEL_STYLE_REC_DTYPE)
        icon_h = np.ascontiguousarray(icon_h, dtype=np.uint32)
        assert len(icon_h) == len(styles)
        if pts is not None:
            pts = np.ascontiguousarray(pts, dtype=np.int32)
            assert pts.shape == (self.r.n_nodes, 2)
        if way_pos is not None:
            way_pos = np.ascontiguousarray(way_pos, dtype=labels.LABEL_POSITION_DTYPE)
            mp_pos = np.ascontiguousarray(mp_pos, dtype=labels.LABEL_POSITION_DTYPE)
            assert len(way_pos) == self.r.n_ways and len(mp_pos) == self.r.n_multipolygons
            # an empty table still needs an address: the shim takes NULL for "compute on the host"
            way_pos = way_pos if len(way_pos) else np.zeros(1, labels.LABEL_POSITION_DTYPE)
            mp_pos = mp_pos if len(mp_pos) else np.zeros(1, labels.LABEL_POSITION_DTYPE)
        caps, n = (C.c_size_t * 3)(1 << 10, 1 << 12, 1 << 12), (C.c_size_t * 3)()
        while True:
            lab, runs, chars = np.zeros(caps[0], LABEL_DTYPE), np.zeros(caps[0], STRING_RUN_DTYPE), np.zeros(caps[1], np.uint32)
            wp, sc = np.zeros((caps[2], 2), np.int32), np.zeros((caps[2], 2))
            shim().al_labels(self.r.h, self.h, styles.ctypes.data, icon_h.ctypes.data_as(C.POINTER(C.c_uint32)), len(styles), zoom, x, y, scale,
                             pts.ctypes.data if pts is not None else None, way_pos.ctypes.data if way_pos is not None else None,
                             mp_pos.ctypes.data if way_pos is not None else None, lab.ctypes.data, runs.ctypes.data, chars.ctypes.data, wp.ctypes.data,
                             sc.ctypes.data, caps, n)
            if all(n[i] <= caps[i] for i in range(3)):
                return lab[: n[0]].copy(), runs[: n[0]].copy(), chars[: n[1]].copy(), wp[: n[2]].copy(), sc[: n[2]].copy()
            caps = (C.c_size_t * 3)(*[max(n[i], 1) for i in range(3)])

    def close(self):
        if self.h:
            shim().al_bindings_free(self.h)
            self.h = None


def batch_of(parts):
    """[(labels, runs, chars, way_pts, way_sincos)] per tile -> the StringLabelList of the batch: tile behind tile, seg_off
    running over the chars and pt_off over the way points"""
    lab, runs, chars, pts, scs, offs, cur, pcur = [], [], [], [], [], [0], 0, 0
    for l, r, c, p, s in parts:
        l, r = l.copy(), r.copy()
        l["seg_off"] += cur
        r["pt_off"][r["position"] == abi.TEXT_LINE] += pcur
        cur += len(c)
        pcur += len(p)
        lab.append(l), runs.append(r), chars.append(c), pts.append(p), scs.append(s)
        offs.append(offs[-1] + len(l))
    cat = lambda v, empty: np.concatenate(v) if v else empty
    return StringLabelList(cat(lab, np.zeros(0, LABEL_DTYPE)), offs, cat(runs, np.zeros(0, STRING_RUN_DTYPE)), cat(chars, np.zeros(0, np.uint32)),
                           cat(pts, np.zeros((0, 2), np.int32)), cat(scs, np.zeros((0, 2))))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _key(styles, gids):
    """compare_styled_entities(.., for_labels = true) as a sort key (styler.rs:246-272): layer or 0, z_index, global id; tuples
    compare like the chain of comparisons, and -0.0 == 0.0 in Python as in partial_cmp"""
    return lambda e: (int(styles[e[1]]["layer"]) if styles[e[1]]["has_layer"] else 0, float(styles[e[1]]["z_index"]), gids[e[0]])


def elements(tile_refs, mp_polygon_counts, way_bindings, mp_bindings, zoom, x, y):
    """reader.rs:60-133 + styler.rs:128-160: the unique ways and multipolygons of the clipped 3 x 3 rectangle (multipolygons
    without polygons dropped), each expanded by its bindings in push order: ([(way, style, text)], [(multipolygon, style, text)])"""
    x0, x1, y0, y1 = rect(zoom, x, y)
    ws, ms = [], []
    for (tx, ty), v in tile_refs.items():
        if x0 <= tx <= x1 and y0 <= ty <= y1:
            ws += list(v[1])
            ms += list(v[2])
    ms = [m for m in sorted(set(ms)) if mp_polygon_counts[m] > 0]
    return [(w, s, t) for w in sorted(set(ws)) for s, t in way_bindings[w]], [(m, s, t) for m in ms for s, t in mp_bindings[m]]


def order_literal(W, M, styles, way_gids, mp_gids):
    """Styler::style_areas (styler.rs:168-203), literally: sort, sort (Python's sorted is stable, as sort_by), merge with the
    multipolygon first unless it compares Greater.  Returns [(is_mp, id, style, text)]."""
    kw, km = _key(styles, way_gids), _key(styles, mp_gids)
    W, M = sorted(W, key=kw), sorted(M, key=km)
    out, wi, mi = [], 0, 0
    while wi < len(W) or mi < len(M):
        if mi >= len(M):
            rel = False
        elif wi >= len(W):
            rel = True
        else:
            rel = not (km(M[mi]) > kw(W[wi]))
        if rel:
            out.append((True,) + M[mi])
            mi += 1
        else:
            out.append((False,) + W[wi])
            wi += 1
    return out


def order_one_sort(W, M, styles, way_gids, mp_gids):
    """The device's order: a tile's multipolygon elements numbered in front of its way elements, each kind in (local id, push
    order); ONE sort by (dense rank of (layer or 0, z_index), global id, that number)."""
    ranks = sorted({(int(s["layer"]) if s["has_layer"] else 0, float(s["z_index"])) for s in styles})  # -0.0 and 0.0: one entry
    rank_of = lambda s: ranks.index((int(styles[s]["layer"]) if styles[s]["has_layer"] else 0, float(styles[s]["z_index"])))
    elems = [(True,) + m for m in M] + [(False,) + w for w in W]
    keyed = [((rank_of(e[2]), (mp_gids if e[0] else way_gids)[e[1]], pos), e) for pos, e in enumerate(elems)]
    return [e for _, e in sorted(keyed, key=lambda ke: ke[0])]


def records(order, texts, styles, icon_h, scale, way_nodes, point_of, anchor_of):
    """Labeler::label_entity (labeler.rs:16-106) + TextPlacer::place (text_placer.rs:24-168) per element of `order`, as the
    records of a string batch.  way_nodes(way) -> node ids; point_of(node) -> (x, y) of Point::from_node; anchor_of(entity)
    -> (status, x, y) of get_label_position.  Returns (labels, runs, chars, way_pts, way_sincos)."""
    lab, runs, chars, pts, scs = np.zeros(len(order), LABEL_DTYPE), np.zeros(len(order), STRING_RUN_DTYPE), [], [], []
    for l, r, (mp, eid, s, t) in zip(lab, runs, order):
        st = styles[s]
        pos = int(st["text_position"])
        line = (not mp) if pos == abi.LABEL_POSITION_NONE else pos == abi.LABEL_POSITION_LINE  # drawer.rs:233-250
        text = bool(st["has_text_style"]) and bool(st["has_font_size"]) and t is not None     # text_placer.rs:37-47
        status, ax, ay = abi.LABEL_NONE, 0.0, 0.0
        if st["has_icon"] or (text and not line):
            status, ax, ay = anchor_of(eid | (MP if mp else 0))
        some = status == abi.LABEL_OK
        icon = bool(st["has_icon"]) and some                                                   # labeler.rs:55-66
        has_text = text and ((not mp) if line else some)
        l["seg_off"] = len(chars)
        if some:
            l["icon_center_x"] = r["center_x"] = float(ax)
            l["icon_center_y"] = r["center_y"] = float(ay)
        if icon:
            l["has_icon"], l["image_id"], r["y_offset"] = 1, st["icon_image"], int(icon_h[s]) // 2
        if has_text:
            tx = [ord(c) for c in texts[t]] if isinstance(texts[t], str) else list(texts[t])
            l["has_text"], l["n_segs"] = 1, len(tx)
            chars += tx
            if st["has_text_color"]:
                l["text_color"] = st["text_color"]
            r["font_id"], r["font_size"] = st["font_id"], float(st["font_size"]) * float(scale)
            if line:
                p = [tuple(int(v) for v in point_of(n)) for n in way_nodes(eid)]
                if p and p[0][0] > p[-1][0]:                                                   # text_placer.rs:65-67
                    p.reverse()
                r["position"], r["pt_off"], r["n_pts"] = abi.TEXT_LINE, len(pts), len(p)
                for e in range(len(p)):
                    if e + 1 < len(p):
                        a = -math.atan2(float(p[e + 1][1] - p[e][1]), float(p[e + 1][0] - p[e][0]))
                        scs.append((math.sin(a), math.cos(a)))
                    else:
                        scs.append((0.0, 0.0))
                pts += p
    return (lab, runs, np.array(chars, dtype=np.uint32), np.array(pts, dtype=np.int32).reshape(-1, 2), np.array(scs, dtype=np.float64).reshape(-1, 2))
