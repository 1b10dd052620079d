"""Shared helpers of the tile-label tests (tests/test_tile_labels_cpu.py, tests/test_gpu_tile_labels.py): the shim over
osm_renderer_amd/host/osmt_tilelabels.hpp (osmt::NodeIndexDesc, osmt::LabelBindings, the host mirror
osmt::node_labels_of_tile), a Python restatement of the node labels of a tile written from styler.rs, labeler.rs, text_placer.rs
and reader.rs alone, and small worlds of nodes whose tile index is placed freely."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, styled
from osm_renderer_amd.labels import LABEL_DTYPE, STRING_RUN_DTYPE, StringLabelList
from tests._geodata import ROOT, Reader, write_geodata
from tests._tilequery import WORLD, rect

SHIM = os.path.join(ROOT, "tests", "_build", "libtilelabels_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "tilelabels_host_main")
HOST_DEMO = os.path.join(ROOT, "tests", "_build", "tilelabels_host_demo")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_tilelabels.hpp", "osmt_styled.hpp", "osmt_draw.hpp", "osmt_geodata.hpp")]
_HDRS.append(os.path.join(ROOT, "include", "osmtile.h"))
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "tilelabels_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SHIM, src])
        L = C.CDLL(SHIM)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.tl_index_new.restype = vp
        L.tl_index_new.argtypes = [vp]
        L.tl_index_get.restype = C.POINTER(abi.NodeIndexDesc)
        L.tl_index_get.argtypes = [vp]
        L.tl_index_free.argtypes = [vp]
        L.tl_bindings_new.restype = vp
        L.tl_bindings_new.argtypes = [C.c_uint32, C.c_uint8, C.c_uint8, sz, u32p, vp, sz, u32p, u32p]
        L.tl_bindings_get.restype = C.POINTER(abi.LabelBindingsDesc)
        L.tl_bindings_get.argtypes = [vp]
        L.tl_bindings_free.argtypes = [vp]
        L.tl_labels.restype = None
        L.tl_labels.argtypes = [vp, vp, vp, u32p, sz, C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
        L.tl_batch.restype = None
        L.tl_batch.argtypes = [vp, vp, vp, u32p, sz, vp, sz, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
        L.tl_project.restype = None
        L.tl_project.argtypes = [C.c_double, C.c_double, C.c_uint8, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_int32)]
        L.tl_sizeof.restype = sz
        L.tl_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt_tilelabels.hpp, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "tilelabels_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def build_demo():
    """tests/tilelabels_host_demo.cpp: the C++ binding of host/osmt_draw.hpp, linked to libosmtile.so"""
    src = os.path.join(ROOT, "tests", "tilelabels_host_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    lib = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(lib), "build libosmtile.so first (__graft_entry__.build())"
    if _stale(HOST_DEMO, [src, lib, os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_tilequery.hpp")] + _HDRS):
        os.makedirs(os.path.dirname(HOST_DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", HOST_DEMO, src, "-L" + libdir, "-losmtile", "-Wl,-rpath," + libdir,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
    return HOST_DEMO


def string_labels(specs):
    """One tile of host-built string labels from dicts: chars (a str), font (id), font_size, color, and either center (a
    centred text) or pts (a text along these way points, already in walking order)."""
    from osm_renderer_amd.labels import way_sincos

    lab, runs = np.zeros(len(specs), LABEL_DTYPE), np.zeros(len(specs), STRING_RUN_DTYPE)
    chars, pts = [], []
    for l, r, s in zip(lab, runs, specs):
        c = [ord(ch) for ch in s["chars"]]
        l["has_text"], l["text_color"], l["seg_off"], l["n_segs"] = 1, s.get("color", (10, 20, 30)), len(chars), len(c)
        chars += c
        r["font_id"], r["font_size"] = s["font"], s["font_size"]
        if "pts" in s:
            r["position"], r["pt_off"], r["n_pts"] = abi.TEXT_LINE, len(pts), len(s["pts"])
            pts += list(s["pts"])
        else:
            r["position"], r["center_x"], r["center_y"] = abi.TEXT_CENTER, s["center"][0], s["center"][1]
    way = np.array(pts, dtype=np.int32).reshape(-1, 2)
    sincos = np.zeros((len(way), 2))
    for r in runs:
        if r["position"] == abi.TEXT_LINE:
            a, n = int(r["pt_off"]), int(r["n_pts"])
            sincos[a : a + n] = way_sincos(way[a : a + n])
    return StringLabelList(lab, [0, len(lab)], runs, np.array(chars, dtype=np.uint32), way, sincos)


def label_styles(rows):
    """rows of dicts -> styled.LABEL_STYLE_REC_DTYPE.  Keys: layer, z_index, icon (image id), text_style (bool), font_size,
    text_color (r, g, b), text_position (abi.LABEL_POSITION_*), font_id; a key that is missing is None / absent."""
    st = np.zeros(len(rows), styled.LABEL_STYLE_REC_DTYPE)
    for s, r in zip(st, rows):
        if r.get("layer") is not None:
            s["has_layer"], s["layer"] = 1, r["layer"]
        s["z_index"] = r.get("z_index", 0.0)
        if r.get("icon") is not None:
            s["has_icon"], s["icon_image"] = 1, r["icon"]
        s["has_text_style"] = 1 if r.get("text_style", r.get("font_size") is not None) else 0
        if r.get("font_size") is not None:
            s["has_font_size"], s["font_size"] = 1, r["font_size"]
        if r.get("text_color") is not None:
            s["has_text_color"], s["text_color"] = 1, r["text_color"]
        s["text_position"] = r.get("text_position", abi.LABEL_POSITION_NONE)
        s["font_id"] = r.get("font_id", 0)
    return st


def latlon_of(zoom, fx, fy):
    """(lat, lon) of the point at fractional tile coordinates (fx, fy) of `zoom` (the inverse of tile.rs:88-106)"""
    n = float(1 << zoom)
    return math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * fy / n)))), fx / n * 360.0 - 180.0


def make_world(path, nodes, tile_refs, ways=()):
    """nodes: [(global id, lat, lon)]; tile_refs: {(x, y) at z18: node ids}; ways: [(global id, [node idx])], listed in every
    index tile.  Returns (Reader, tile_refs as written: {(x, y): (nodes, ways, multipolygons)})."""
    refs = {k: (list(v), list(range(len(ways))), []) for k, v in tile_refs.items()}
    write_geodata(str(path), [(g, la, lo, {}) for g, la, lo in nodes], [(g, n, {}) for g, n in ways], [], [], tile_refs=refs)
    return Reader(str(path)), refs


def node_index_of(r, refs, shuffle=None):
    """the node half of refs as a styled.NodeIndex; shuffle (a numpy Generator): every list in a random order"""
    gids = [r.global_id(0, i) for i in range(r.n_nodes)]
    lists = [sorted(refs[k][0]) for k in sorted(refs)]
    if shuffle is not None:
        lists = [list(shuffle.permutation(v)) for v in lists]
    return styled.NodeIndex(gids, lists)


class Mirror:
    """osmt::LabelBindings + osmt::node_labels_of_tile over a tests._geodata.Reader"""

    def __init__(self, r, node_bindings, texts, geodata_id=0, zoom_lo=0, zoom_hi=18):
        self.r = r
        self.b = styled.LabelBindings(geodata_id, zoom_lo, zoom_hi, node_bindings, texts)
        b = self.b
        u32 = C.POINTER(C.c_uint32)
        self.h = shim().tl_bindings_new(geodata_id, zoom_lo, zoom_hi, len(node_bindings), b.node_off.ctypes.data_as(u32), b.bindings.ctypes.data,
                                        len(b.text_off) - 1, b.text_off.ctypes.data_as(u32), b.chars.ctypes.data_as(u32))

    def desc(self):
        return shim().tl_bindings_get(self.h).contents

    def labels(self, styles, icon_h, zoom, x, y, scale=1, pts=None):
        """(labels, runs, chars) of one tile; pts: None = the libm projection, else int32 [n_nodes, 2]"""
        styles = np.ascontiguousarray(styles, dtype=styled.LABEL_STYLE_REC_DTYPE)
        icon_h = np.ascontiguousarray(icon_h, dtype=np.uint32)
        assert len(icon_h) == len(styles)
        if pts is not None:
            pts = np.ascontiguousarray(pts, dtype=np.int32)
            assert pts.shape == (self.r.n_nodes, 2)
        caps, n = (C.c_size_t * 2)(1 << 10, 1 << 12), (C.c_size_t * 2)()
        while True:
            lab, runs, chars = np.zeros(caps[0], LABEL_DTYPE), np.zeros(caps[0], STRING_RUN_DTYPE), np.zeros(caps[1], np.uint32)
            shim().tl_labels(self.r.h, self.h, styles.ctypes.data, icon_h.ctypes.data_as(C.POINTER(C.c_uint32)), len(styles), zoom, x, y, scale,
                             pts.ctypes.data if pts is not None else None, lab.ctypes.data, runs.ctypes.data, chars.ctypes.data, caps, n)
            if n[0] <= caps[0] and n[1] <= caps[1]:
                return lab[: n[0]].copy(), runs[: n[0]].copy(), chars[: n[1]].copy()
            caps = (C.c_size_t * 2)(max(n[0], 1), max(n[1], 1))

    def close(self):
        if self.h:
            shim().tl_bindings_free(self.h)
            self.h = None


def batch_of(parts):
    """[(labels, runs, chars)] per tile -> the StringLabelList of the batch: tile behind tile, seg_off running over the chars"""
    lab, runs, chars, offs, cur = [], [], [], [0], 0
    for l, r, c in parts:
        l = l.copy()
        l["seg_off"] += cur
        cur += len(c)
        lab.append(l), runs.append(r), chars.append(c)
        offs.append(offs[-1] + len(l))
    return StringLabelList(np.concatenate(lab) if lab else np.zeros(0, LABEL_DTYPE), offs, np.concatenate(runs) if runs else np.zeros(0, STRING_RUN_DTYPE),
                           np.concatenate(chars) if chars else np.zeros(0, np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 2)))


def restate(tile_refs, gids, node_bindings, texts, styles, icon_h, zoom, x, y, scale, point_of):
    """The node labels of a tile, from the specification alone.  reader.rs:60-133: the clipped 3 x 3 rectangle over the
    tile_refs dict, sorted(set()).  styler.rs:128-165: every node's (style, text) pairs in push order, then a STABLE sort by
    (layer or 0, z_index, global id) — Python's sorted is stable, and -0.0 == 0.0 there as in partial_cmp.  labeler.rs,
    text_placer.rs:37-58: the icon, y_offset = height / 2, text only with a font size, the tag and a position that is not
    Line.  point_of(node) -> (x, y).  Returns (labels, runs, chars)."""
    x0, x1, y0, y1 = rect(zoom, x, y)
    nodes = []
    for (tx, ty), v in tile_refs.items():
        if x0 <= tx <= x1 and y0 <= ty <= y1:
            nodes += list(v[0])
    elems = [(n, s, t) for n in sorted(set(nodes)) for s, t in node_bindings[n]]
    elems = sorted(elems, key=lambda e: (int(styles[e[1]]["layer"]) if styles[e[1]]["has_layer"] else 0, float(styles[e[1]]["z_index"]), gids[e[0]]))
    lab, runs, chars = np.zeros(len(elems), LABEL_DTYPE), np.zeros(len(elems), STRING_RUN_DTYPE), []
    for l, r, (n, s, t) in zip(lab, runs, elems):
        st = styles[s]
        px, py = point_of(n)
        l["icon_center_x"] = r["center_x"] = float(px)
        l["icon_center_y"] = r["center_y"] = float(py)
        l["seg_off"] = len(chars)
        if st["has_icon"]:
            l["has_icon"], l["image_id"], r["y_offset"] = 1, st["icon_image"], int(icon_h[s]) // 2
        if st["has_text_style"] and st["has_font_size"] and t is not None and st["text_position"] != abi.LABEL_POSITION_LINE:
            text = [ord(c) for c in texts[t]] if isinstance(texts[t], str) else list(texts[t])
            l["has_text"], l["n_segs"] = 1, len(text)
            chars += text
            if st["has_text_color"]:
                l["text_color"] = st["text_color"]
            r["font_id"], r["font_size"] = st["font_id"], float(st["font_size"]) * float(scale)
    return lab, runs, np.array(chars, dtype=np.uint32)


def py_project(lat, lon, zoom, tx, ty, scale):
    """Point::from_node (tile.rs:88-106, point.rs:11-19) in Python floats"""
    lat_rad, lon_rad = lat * (math.pi / 180.0), lon * (math.pi / 180.0)
    xx, yy = lon_rad + math.pi, math.pi - math.log(math.tan((math.pi / 4.0) + (lat_rad / 2.0)))
    dim = float(256 * (1 << zoom))
    rx, ry = (xx / (2.0 * math.pi)) * dim - float(tx * 256), (yy / (2.0 * math.pi)) * dim - float(ty * 256)

    def rnd(v):  # f64::round: half away from zero
        return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)

    return rnd(rx * scale), rnd(ry * scale)
