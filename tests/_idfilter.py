"""Shared helpers of the id-filter tests (tests/test_idfilter_cpu.py, tests/test_gpu_id_filter.py): the shim over the osm_ids
argument of the three host twins (osmt::styled_areas_of_tile, osmt::node_labels_of_tile, osmt::area_labels_of_tile) and over
osm_renderer_amd/host/osmt_idfilter.hpp, which takes the handles the mirrors of tests/_tilequery.py, tests/_tilelabels.py and
tests/_arealabels.py hold; the stand-alone host program under the sanitizers; and the planes of a filter stated with numpy."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import labels, styled
from osm_renderer_amd.labels import LABEL_DTYPE, STRING_RUN_DTYPE
from tests import _arealabels as _al
from tests import _tilelabels as _tl
from tests import _tilequery as _tq
from tests._geodata import ROOT, Reader, write_geodata

SHIM = os.path.join(ROOT, "tests", "_build", "libidfilter_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "idfilter_host_main")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h)
         for h in ("osmt_idfilter.hpp", "osmt_arealabels.hpp", "osmt_tilelabels.hpp", "osmt_tilequery.hpp", "osmt_labelable.hpp", "osmt_styled.hpp",
                   "osmt_geodata.hpp")]
_HDRS.append(os.path.join(ROOT, "include", "osmtile.h"))
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "idfilter_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src, "-lm"])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz, u32p, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.idf_set.restype = sz
        L.idf_set.argtypes = [u64p, sz, u64p]
        L.idf_plane.restype = sz
        L.idf_plane.argtypes = [u64p, sz, u64p, sz, u32p]
        L.idf_areas.restype = sz
        L.idf_areas.argtypes = [vp, vp, C.c_uint8, C.c_uint32, C.c_uint32, u64p, sz, C.c_int, vp, sz]
        L.idf_node_labels.restype = None
        L.idf_node_labels.argtypes = [vp, vp, vp, u32p, sz, C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64p, sz, C.c_int, vp, vp, vp, C.POINTER(sz),
                                      C.POINTER(sz)]
        L.idf_area_labels.restype = None
        L.idf_area_labels.argtypes = [vp, vp, vp, u32p, sz, C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, u64p, sz, C.c_int, vp, vp, vp, vp, vp,
                                      C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        _lib = L
    return _lib


def build_host_main():
    """tests/idfilter_host_main.cpp: the twins and the sort / dedup step in a program of their own, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "idfilter_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        tmp = f"{HOST_MAIN}.{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", tmp, src])
        os.replace(tmp, HOST_MAIN)
    return HOST_MAIN


def _ids(ids):
    """(array, pointer or None, count, has_filter) of an id list; None: no filter"""
    if ids is None:
        return None, None, 0, 0
    a = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
    return a, (a.ctypes.data_as(C.POINTER(C.c_uint64)) if len(a) else None), len(a), 1


def host_set(ids):
    """osmt::id_filter_set"""
    a, p, n, _ = _ids(ids)
    out = np.zeros(max(n, 1), np.uint64)
    k = shim().idf_set(p, n, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out[:k].copy()


def host_plane(gids, ids):
    """osmt::id_filter_plane over osmt::id_filter_set(ids)"""
    g, gp, ng, _ = _ids(gids)
    a, p, n, _ = _ids(ids)
    out = np.zeros((ng + 63) // 64 * 2 + 2, np.uint32)
    k = shim().idf_plane(gp, ng, p, n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out[:k].copy()


def numpy_plane(gids, ids):
    """the plane of a kind from np.isin alone: bit e % 32 of word e // 32, whole 64-bit words, zeros behind the last entity"""
    gids = np.asarray(gids, dtype=np.uint64)
    bits = np.zeros((len(gids) + 63) // 64 * 64, np.uint8)
    bits[: len(gids)] = np.isin(gids, np.asarray(ids, dtype=np.uint64))
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def areas(tq_mirror, zoom, x, y, ids):
    """osmt::styled_areas_of_tile(.., osm_ids) over a tests._tilequery.Mirror"""
    a, p, n, has = _ids(ids)
    cap = 1 << 12
    while True:
        out = np.zeros(cap, styled.STYLED_AREA_DTYPE)
        k = shim().idf_areas(tq_mirror.r.h, tq_mirror.h, zoom, x, y, p, n, has, out.ctypes.data, cap)
        if k <= cap:
            return out[:k].copy()
        cap = k


def node_labels(tl_mirror, styles, icon_h, zoom, x, y, scale, pts, ids):
    """osmt::node_labels_of_tile(.., osm_ids) over a tests._tilelabels.Mirror: (labels, runs, chars)"""
    a, p, n, has = _ids(ids)
    styles = np.ascontiguousarray(styles, dtype=styled.LABEL_STYLE_REC_DTYPE)
    icon_h = np.ascontiguousarray(icon_h, dtype=np.uint32)
    assert len(icon_h) == len(styles)
    if pts is not None:
        pts = np.ascontiguousarray(pts, dtype=np.int32)
        assert pts.shape == (tl_mirror.r.n_nodes, 2)
    caps, cnt = (C.c_size_t * 2)(1 << 10, 1 << 12), (C.c_size_t * 2)()
    while True:
        lab, runs, chars = np.zeros(caps[0], LABEL_DTYPE), np.zeros(caps[0], STRING_RUN_DTYPE), np.zeros(caps[1], np.uint32)
        shim().idf_node_labels(tl_mirror.r.h, tl_mirror.h, styles.ctypes.data, icon_h.ctypes.data_as(C.POINTER(C.c_uint32)), len(styles), zoom, x, y, scale,
                               pts.ctypes.data if pts is not None else None, p, n, has, lab.ctypes.data, runs.ctypes.data, chars.ctypes.data, caps, cnt)
        if cnt[0] <= caps[0] and cnt[1] <= caps[1]:
            return lab[: cnt[0]].copy(), runs[: cnt[0]].copy(), chars[: cnt[1]].copy()
        caps = (C.c_size_t * 2)(max(cnt[0], 1), max(cnt[1], 1))


def area_labels(al_mirror, styles, icon_h, zoom, x, y, scale, pts, way_pos, mp_pos, ids, want_asked=False):
    """osmt::area_labels_of_tile(.., osm_ids) over a tests._arealabels.Mirror: (labels, runs, chars, way_pts, way_sincos) and,
    with want_asked, the number of anchors the twin asked for"""
    a, p, n, has = _ids(ids)
    r = al_mirror.r
    styles = np.ascontiguousarray(styles, dtype=styled.LABEL_STYLE_REC_DTYPE)
    icon_h = np.ascontiguousarray(icon_h, dtype=np.uint32)
    assert len(icon_h) == len(styles)
    if pts is not None:
        pts = np.ascontiguousarray(pts, dtype=np.int32)
        assert pts.shape == (r.n_nodes, 2)
    if way_pos is not None:
        way_pos = np.ascontiguousarray(way_pos, dtype=labels.LABEL_POSITION_DTYPE)
        mp_pos = np.ascontiguousarray(mp_pos, dtype=labels.LABEL_POSITION_DTYPE)
        assert len(way_pos) == r.n_ways and len(mp_pos) == r.n_multipolygons
        way_pos = way_pos if len(way_pos) else np.zeros(1, labels.LABEL_POSITION_DTYPE)
        mp_pos = mp_pos if len(mp_pos) else np.zeros(1, labels.LABEL_POSITION_DTYPE)
    caps, cnt, asked = (C.c_size_t * 3)(1 << 10, 1 << 12, 1 << 12), (C.c_size_t * 3)(), C.c_size_t()
    while True:
        lab, runs, chars = np.zeros(caps[0], LABEL_DTYPE), np.zeros(caps[0], STRING_RUN_DTYPE), np.zeros(caps[1], np.uint32)
        wp, sc = np.zeros((caps[2], 2), np.int32), np.zeros((caps[2], 2))
        shim().idf_area_labels(r.h, al_mirror.h, styles.ctypes.data, icon_h.ctypes.data_as(C.POINTER(C.c_uint32)), len(styles), zoom, x, y, scale,
                               pts.ctypes.data if pts is not None else None, way_pos.ctypes.data if way_pos is not None else None,
                               mp_pos.ctypes.data if way_pos is not None else None, p, n, has, lab.ctypes.data, runs.ctypes.data, chars.ctypes.data,
                               wp.ctypes.data, sc.ctypes.data, caps, cnt, C.byref(asked))
        if all(cnt[i] <= caps[i] for i in range(3)):
            out = lab[: cnt[0]].copy(), runs[: cnt[0]].copy(), chars[: cnt[1]].copy(), wp[: cnt[2]].copy(), sc[: cnt[2]].copy()
            return (out, asked.value) if want_asked else out
        caps = (C.c_size_t * 3)(*[max(cnt[i], 1) for i in range(3)])


# ---- a labelled town behind the filter: shared by tests/test_gpu_id_filter.py and tests/test_gpu_tile_requests.py --------------------
def far_and_tiles(z, tx, ty):
    """(two tiles with no index tile near, the five-tile mix with them in the middle and at the end) around tile (z, tx, ty)"""
    far = [(z, tx + 500, ty + 500), (z, tx + 501, ty + 500)]
    return far, [(z, tx, ty), (z, tx + 1, ty), far[0], (z, tx + 2, ty + 1), far[1]]


class Feed:
    """A town-like world (a World of tests/test_gpu_area_labels.py, whose label texts are `texts`) with draw styles on ways AND multipolygons, a node index, node label bindings, and the mirrors of all three"""

    def __init__(self, ctx, W, path, texts, canvas):
        self.ctx, self.W, self.canvas = ctx, W, canvas
        r = W.r
        st = np.zeros(3, styled.STYLE_REC_DTYPE)
        st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, [(170, 200, 150), (90, 120, 200), (120, 180, 90)], 1
        st["has_color"][1], st["color"][1], st["has_width"][1], st["width"][1] = 1, (60, 60, 60), 1, 2.0
        s0 = ctx.register_styles(st)
        self.ws = [[s0 + 1] if i % 3 == 0 else [s0, s0 + 1] if i % 3 == 1 else [] for i in range(r.n_ways)]  # streets stroked, first buildings twice
        self.ms = [[s0 + 2] for _ in range(r.n_multipolygons)]
        self.draw = ctx.register_style_bindings(styled.StyleBindings(W.gid, 0, 18, self.ws, self.ms))
        self.tqm = _tq.Mirror(r, self.ws, self.ms, W.gid)
        keys = sorted(W.refs)
        node_refs = {k: ([n for wi in W.refs[k][1] for n in W.w.ways[wi][1]][:7], W.refs[k][1], W.refs[k][2]) for k in keys}
        ctx.register_node_index(W.gid, _tl.node_index_of(r, node_refs))
        # the town's file lists no nodes: the node mirror reads the same town from a file whose tiles list node_refs
        write_geodata(str(path), W.w.nodes, W.w.ways, W.w.polygons, W.w.mps, tile_refs=node_refs)
        self.r_nodes = Reader(str(path))
        self.nb = [[(W.first + 4, 4)] if i % 3 == 0 else [(W.first + 2, 0), (W.first + 1, None)] if i % 7 == 0 else [] for i in range(r.n_nodes)]
        self.node_bind = ctx.register_label_bindings(styled.LabelBindings(W.gid, 0, 18, self.nb, texts))
        self.tlm = _tl.Mirror(self.r_nodes, self.nb, texts, W.gid)
        self.way_gid = np.array([r.global_id(1, i) for i in range(r.n_ways)], dtype=np.uint64)
        self.mp_gid = np.array([r.global_id(3, i) for i in range(r.n_multipolygons)], dtype=np.uint64)
        self.node_gid = np.array([r.global_id(0, i) for i in range(r.n_nodes)], dtype=np.uint64)

    def scene(self, tiles, scale=1, flt=None):
        return self.ctx.build_tiles(styled.TileBatch(self.W.gid, tiles, {z: self.draw for z in range(19)}, scale=scale, canvas=self.canvas), id_filter=flt)

    def gid_of(self, entity):
        entity = np.asarray(entity, dtype=np.uint32)
        mp = (entity & _al.MP) != 0
        ids = entity & np.uint32(~_al.MP & 0xFFFFFFFF)
        out = np.zeros(len(entity), np.uint64)
        out[mp], out[~mp] = self.mp_gid[ids[mp]], self.way_gid[ids[~mp]]
        return out

    def want_labels(self, tiles, scale, ids):
        """(area batch, node batch) of the twins with osm_ids = ids, points and anchors from the device as World.want takes them"""
        W, area, node, memo = self.W, [], [], {}
        for z, x, y in tiles:
            if (z, x, y) not in memo:
                pts = self.ctx.project(W.ll, z, x, y, float(scale))
                wp, mp = W.anchors((z, x, y), scale)
                memo[(z, x, y)] = (area_labels(W.all[1], W.styles, W.icon_h, z, x, y, scale, pts, wp, mp, ids),
                                   node_labels(self.tlm, W.styles, W.icon_h, z, x, y, scale, pts, ids))
            area.append(memo[(z, x, y)][0]), node.append(memo[(z, x, y)][1])
        return _al.batch_of(area), _tl.batch_of(node)

    def close(self):
        self.tqm.close(), self.tlm.close(), self.r_nodes.close()


def half_of_the_ids(feed, seed=3):
    """about half of the ways, multipolygons and nodes, in any order, with repeats and ids nobody has"""
    rng = np.random.default_rng(seed)
    every = np.concatenate([feed.way_gid, feed.mp_gid, feed.node_gid])
    some = rng.choice(every, len(every) // 2, replace=False)
    return rng.permutation(np.concatenate([some, some[:50], np.array([5, (1 << 64) - 1], dtype=np.uint64)]))
