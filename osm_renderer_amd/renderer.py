"""Host-side driver over the C ABI: contexts, HBM-resident scenes, device output.

torch is used for device buffers / streams only (plumbing): every pixel is
produced by the HIP kernels behind libosmtile.so.
"""
import ctypes as C

import numpy as np

from . import abi
from .display_list import DisplayList
from .lib import check, load


def _torch():
    import torch

    return torch


def _styled():
    from . import styled

    return styled


def _stream_ptr(stream=None):
    torch = _torch()
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


def scene_png_work_layout(n_tiles, dim):
    """The d_work buffer of osmt_render_scene_png_device for n_tiles tiles of dim x dim pixels, as include/osmtile.h
    documents it: (framebuffer offset, slot offset, length offset, total bytes).  No device needed."""
    up = lambda v: (v + 255) // 256 * 256
    o_png = up(n_tiles * dim * dim * 4)
    o_len = o_png + up(n_tiles * load().osmt_png_device_bound(dim, dim))
    return 0, o_png, o_len, o_len + up(n_tiles * 4)


class Scene:
    """A display-list batch resident in HBM (osmt_scene)."""

    def __init__(self, ctx, dl: DisplayList, labels=None):
        self.ctx = ctx
        self._dl = dl
        self.n_jobs = dl.n_jobs
        self.dim = dl.dim
        b = dl.as_batch()
        h = C.c_void_p()
        check(load().osmt_scene_upload(ctx._h, C.byref(b), C.byref(h)))
        self._h = h
        self.labels = None
        if labels is not None:
            self.set_labels(labels)

    @classmethod
    def _built(cls, ctx, h, n_jobs, scale, nodes):
        """A scene osmt_scene_build_styled made: its display list lives on the device only (`dl` reads it back on demand)."""
        self = cls.__new__(cls)
        self.ctx, self._h, self.n_jobs, self.dim, self.labels = ctx, h, n_jobs, abi.TILE_SIZE * scale, None
        self._scale, self._nodes, self._dl = scale, nodes, None
        return self

    @property
    def dl(self):
        if self._dl is None:
            self._dl = self.read_display_list()
        return self._dl

    @dl.setter
    def dl(self, value):
        self._dl = value

    def read_display_list(self):
        """osmt_scene_read_display_list: the device-resident display list of this scene, uploaded or built, as a
        DisplayList (jobs, ops, rings, node references, dashes byte for byte as the renderer reads them)."""
        from .display_list import JOB_DTYPE, OP_DTYPE, RING_DTYPE

        L, n = load(), (C.c_size_t * 5)()
        check(L.osmt_scene_read_display_list(self.ctx._h, self._h, None, None, None, None, None, n))
        jobs, ops, rings = np.zeros(n[0], JOB_DTYPE), np.zeros(n[1], OP_DTYPE), np.zeros(n[2], RING_DTYPE)
        refs, dashes = np.zeros(n[3], np.uint32), np.zeros(n[4], np.float64)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        check(L.osmt_scene_read_display_list(self.ctx._h, self._h, ptr(jobs), ptr(ops), ptr(rings), ptr(refs), ptr(dashes), n))
        if self._dl is not None and self._dl.coord_kind != abi.COORD_NODE_REF:  # an uploaded scene with per-point coordinates
            return DisplayList(jobs, ops, rings, self._dl.coords, dashes, self._dl.coord_kind, self._dl.scale)
        nodes = self._dl.nodes if self._dl is not None else self._nodes
        scale = self._dl.scale if self._dl is not None else self._scale
        return DisplayList(jobs, ops, rings, refs, dashes, abi.COORD_NODE_REF, scale, nodes=nodes)

    def read_styled_areas(self):
        """osmt_scene_read_styled_areas: the styled batch the device derived for a scene of build_tiles, as (tiles in
        styled.STYLED_TILE_DTYPE, areas in styled.STYLED_AREA_DTYPE)."""
        from . import styled

        L, n = load(), C.c_size_t()
        check(L.osmt_scene_read_styled_areas(self.ctx._h, self._h, None, None, 0, C.byref(n)))
        tiles, areas = np.zeros(self.n_jobs, styled.STYLED_TILE_DTYPE), np.zeros(n.value, styled.STYLED_AREA_DTYPE)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        check(L.osmt_scene_read_styled_areas(self.ctx._h, self._h, ptr(tiles), ptr(areas), len(areas), C.byref(n)))
        return tiles, areas

    def build_tile_labels(self, label_bindings, area_labels=None):
        """osmt_scene_build_tile_labels: the node labels of every tile of a scene of Context.build_tiles, built on the GPU
        and attached as string labels.  label_bindings: {zoom: id from Context.register_label_bindings}; area_labels: a
        labels.StringLabelList of host-built way / multipolygon labels drawn in front of each tile's node labels."""
        from .labels import splice_string_labels

        ids = (C.c_uint32 * (abi.MAX_ZOOM + 1))(*[int(dict(label_bindings).get(z, abi.BINDINGS_NONE)) for z in range(abi.MAX_ZOOM + 1)])
        sb = area_labels.as_batch() if area_labels is not None else None
        check(load().osmt_scene_build_tile_labels(self.ctx._h, self._h, ids, C.byref(sb) if sb is not None else None))
        node = self.read_tile_labels()
        self.labels = node if area_labels is None else splice_string_labels(area_labels, node)
        return node

    def build_tile_labels_all(self, area_bindings=None, node_bindings=None, anchors=None):
        """osmt_scene_build_tile_labels_all: the labels of the ways and multipolygons of every tile, then of its nodes, built
        on the GPU and attached as one string batch, areas in front.  area_bindings: {zoom: id from
        Context.register_area_label_bindings} or None; node_bindings: {zoom: id from Context.register_label_bindings} or None;
        anchors: a labels.AREA_ANCHOR_DTYPE array of anchors computed on the host for pairs an earlier call declined
        (read_declined_anchors).  Returns (area batch, node batch) as labels.StringLabelList."""
        from .labels import AREA_ANCHOR_DTYPE, splice_string_labels

        def ids_of(b):
            if b is None:
                return None
            return (C.c_uint32 * (abi.MAX_ZOOM + 1))(*[int(dict(b).get(z, abi.BINDINGS_NONE)) for z in range(abi.MAX_ZOOM + 1)])

        n = 0
        if anchors is not None:
            anchors = np.ascontiguousarray(anchors, dtype=AREA_ANCHOR_DTYPE)
            n = len(anchors)
        check(load().osmt_scene_build_tile_labels_all(self.ctx._h, self._h, ids_of(area_bindings), ids_of(node_bindings),
                                                      C.c_void_p(anchors.ctypes.data) if n else None, n))
        area, node = self.read_tile_area_labels(), self.read_tile_labels()
        self.labels = splice_string_labels(area, node) if len(area.labels) else node
        return area, node

    def read_declined_anchors(self):
        """osmt_scene_read_declined_anchors: the (tile, entity) pairs the anchor search of the last build_tile_labels_all
        declined, as a labels.AREA_ANCHOR_DTYPE array."""
        from .labels import AREA_ANCHOR_DTYPE

        L, n = load(), C.c_size_t()
        check(L.osmt_scene_read_declined_anchors(self.ctx._h, self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, AREA_ANCHOR_DTYPE)
        if n.value:
            check(L.osmt_scene_read_declined_anchors(self.ctx._h, self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def read_tile_area_labels(self):
        """osmt_scene_read_tile_area_labels: the area batch the device built, before the splice, as a labels.StringLabelList."""
        from .labels import LABEL_DTYPE, STRING_RUN_DTYPE, StringLabelList

        L, n = load(), (C.c_size_t * 3)()
        check(L.osmt_scene_read_tile_area_labels(self.ctx._h, self._h, None, None, None, None, None, None, None, n))
        lab, runs, chars = np.zeros(n[0], LABEL_DTYPE), np.zeros(n[0], STRING_RUN_DTYPE), np.zeros(n[1], np.uint32)
        pts, sincos, off = np.zeros((n[2], 2), np.int32), np.zeros((n[2], 2)), np.zeros(self.n_jobs + 1, np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        caps = (C.c_size_t * 3)(n[0], n[1], n[2])
        check(L.osmt_scene_read_tile_area_labels(self.ctx._h, self._h, ptr(lab), ptr(runs), ptr(chars), ptr(pts), ptr(sincos), ptr(off), caps, n))
        return StringLabelList(lab, off, runs, chars, pts, sincos)

    def read_tile_labels(self):
        """osmt_scene_read_tile_labels: the node batch the device built, before the splice, as a labels.StringLabelList."""
        from .labels import LABEL_DTYPE, STRING_RUN_DTYPE, StringLabelList

        L, n = load(), (C.c_size_t * 2)()
        check(L.osmt_scene_read_tile_labels(self.ctx._h, self._h, None, None, None, None, None, n))
        lab, runs, chars = np.zeros(n[0], LABEL_DTYPE), np.zeros(n[0], STRING_RUN_DTYPE), np.zeros(n[1], np.uint32)
        off = np.zeros(self.n_jobs + 1, np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        caps = (C.c_size_t * 2)(n[0], n[1])
        check(L.osmt_scene_read_tile_labels(self.ctx._h, self._h, ptr(lab), ptr(runs), ptr(chars), ptr(off), caps, n))
        return StringLabelList(lab, off, runs, chars, np.zeros((0, 2), np.int32), np.zeros((0, 2)))

    def max_tile_ops(self):
        """osmt_scene_max_tile_ops: the most ops of any tile, as the renderer knows it (it picks its list kernel by it)"""
        out = C.c_uint32()
        check(load().osmt_scene_max_tile_ops(self.ctx._h, self._h, C.byref(out)))
        return out.value

    def set_labels(self, labels):
        """osmt_scene_set_labels: attach (or, with None, detach) the label pass of every tile."""
        if labels is None:
            check(load().osmt_scene_set_labels(self.ctx._h, self._h, None))
        else:
            assert labels.n_jobs == self.n_jobs
            lb = labels.as_batch()
            check(load().osmt_scene_set_labels(self.ctx._h, self._h, C.byref(lb)))
        self.labels = labels

    def set_glyph_labels(self, glyph_labels):
        """osmt_scene_set_glyph_labels: attach glyph-run labels (labels.GlyphLabelList; None detaches).  The glyph ids
        must be registered on this scene's context (Context.register_glyphs)."""
        if glyph_labels is None:
            check(load().osmt_scene_set_glyph_labels(self.ctx._h, self._h, None))
        else:
            assert glyph_labels.n_jobs == self.n_jobs
            gb = glyph_labels.as_batch()
            check(load().osmt_scene_set_glyph_labels(self.ctx._h, self._h, C.byref(gb)))
        self.labels = glyph_labels

    def set_text_labels(self, text_labels):
        """osmt_scene_set_text_labels: attach text-run labels (labels.TextLabelList; None detaches): TextPlacer::place
        runs on the device.  The glyph ids must be registered on this scene's context (Context.register_glyphs)."""
        if text_labels is None:
            check(load().osmt_scene_set_text_labels(self.ctx._h, self._h, None))
        else:
            assert text_labels.n_jobs == self.n_jobs
            tb = text_labels.as_batch()
            check(load().osmt_scene_set_text_labels(self.ctx._h, self._h, C.byref(tb)))
        self.labels = text_labels

    def set_string_labels(self, string_labels):
        """osmt_scene_set_string_labels: attach string labels (labels.StringLabelList; None detaches):
        TextPlacer::text_to_glyphs and TextPlacer::place run on the device.  The font ids must be registered on this
        scene's context (Context.register_font)."""
        if string_labels is None:
            check(load().osmt_scene_set_string_labels(self.ctx._h, self._h, None))
        else:
            assert string_labels.n_jobs == self.n_jobs
            sb = string_labels.as_batch()
            check(load().osmt_scene_set_string_labels(self.ctx._h, self._h, C.byref(sb)))
        self.labels = string_labels

    def read_text_glyphs(self):
        """osmt_scene_read_text_glyphs: the records the device shaped for the attached string labels
        (labels.TEXT_GLYPH_DTYPE [n_chars], glyph_id = the outline id); empty for the other label forms."""
        from .labels import TEXT_GLYPH_DTYPE

        L, n = load(), C.c_size_t(0)
        check(L.osmt_scene_read_text_glyphs(self.ctx._h, self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=TEXT_GLYPH_DTYPE)
        if n.value:
            check(L.osmt_scene_read_text_glyphs(self.ctx._h, self._h, out.ctypes.data_as(C.POINTER(abi.TextGlyph)), n.value, C.byref(n)))
        return out

    def read_glyph_instances(self):
        """osmt_scene_read_glyph_instances: the glyph instances the device placed for the attached text-run or string
        labels (labels.GLYPH_INSTANCE_DTYPE [n_glyphs], skipped texts with form GLYPH_NONE); empty for the other forms."""
        from .labels import GLYPH_INSTANCE_DTYPE

        L, n = load(), C.c_size_t(0)
        check(L.osmt_scene_read_glyph_instances(self.ctx._h, self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=GLYPH_INSTANCE_DTYPE)
        if n.value:
            check(L.osmt_scene_read_glyph_instances(self.ctx._h, self._h, out.ctypes.data_as(C.POINTER(abi.GlyphInstance)), n.value, C.byref(n)))
        return out

    def read_label_segs(self):
        """osmt_scene_read_label_segs: the draw_line arena the label kernels read, float64 [n, 4]."""
        L, n = load(), C.c_size_t(0)
        check(L.osmt_scene_read_label_segs(self.ctx._h, self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), dtype=np.float64)
        if n.value:
            check(L.osmt_scene_read_label_segs(self.ctx._h, self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return out

    def read_label_cover(self, label):
        """osmt_scene_read_label_cover: (ry0, cx0, plane float64 [rows, cols]) of one label of the attached batch, the
        f64 totals the last render's label stage left (cell [r, c] is pixel (cx0 + c, ry0 + r)).  A label without a
        window gives a plane of zero rows.  Raises before the first render after the labels were set."""
        L, n, win = load(), C.c_size_t(0), (C.c_int32 * 4)()
        check(L.osmt_scene_read_label_cover(self.ctx._h, self._h, int(label), win, None, 0, C.byref(n)))
        ry0, ry1, cx0, cols = (int(v) for v in win)
        rows = ry1 - ry0 + 1 if n.value else 0
        out = np.zeros((rows, cols), dtype=np.float64)
        if n.value:
            check(L.osmt_scene_read_label_cover(self.ctx._h, self._h, int(label), win, out.ctypes.data_as(C.POINTER(C.c_double)),
                                                out.size, C.byref(n)))
        return ry0, cx0, out

    def label_status(self):
        """label_generation_statuses of the last render (tile_pixels.rs:160-162)."""
        n = len(self.labels.labels) if self.labels is not None else 0
        out = np.zeros(n, dtype=np.uint8)
        if n:
            check(load().osmt_scene_read_label_status(self.ctx._h, self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def check(self):
        """osmt_scene_check: waits for the scene's launches, raises if a kernel reported an internal error."""
        check(load().osmt_scene_check(self.ctx._h, self._h))

    def free(self):
        if getattr(self, "_h", None):
            load().osmt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Worker:
    """osmt_worker: the per-thread request handle of the reference's server loop (http_server.rs:50-83); concurrent
    render() calls of the workers of one context are gathered into shared launches."""

    def __init__(self, ctx):
        h = C.c_void_p()
        check(load().osmt_worker_create(ctx._h, C.byref(h)))
        self._h = h
        self.ctx = ctx

    def render(self, dl: DisplayList, labels=None, out=None):
        """osmt_worker_render: packed RGB8 [n, W*W*3] of the display list's tiles (usually one)."""
        b = dl.as_batch()
        tight = dl.dim * dl.dim * 3
        if out is None:
            out = np.empty((dl.n_jobs, tight), dtype=np.uint8)
        lb = labels.as_batch() if labels is not None else None
        check(load().osmt_worker_render(self._h, C.byref(b), C.byref(lb) if lb is not None else None,
                                        out.ctypes.data_as(C.POINTER(C.c_uint8)), tight))
        return out

    def render_tile_png(self, server, tile, scale=1, anchors=None, out=None):
        """osmt_worker_render_tile_png: the PNG file (bytes) of one tile (zoom, x, y) of a TileServer; concurrent requests of
        the same server and scale share a group.  anchors: labels.AREA_ANCHOR_DTYPE with tile == 0, for pairs an earlier
        request declined (last_declined_anchors()).  out: a uint8 buffer of the caller's (default: the bound for the scale)."""
        from .labels import AREA_ANCHOR_DTYPE

        z, x, y = tile
        t = abi.TileCoord(int(x), int(y), int(z))
        n = 0
        if anchors is not None:
            anchors = np.ascontiguousarray(anchors, dtype=AREA_ANCHOR_DTYPE)
            n = len(anchors)
        if out is None:
            out = np.empty(load().osmt_png_device_bound(256 * scale, 256 * scale), np.uint8)
        got = C.c_size_t()
        rc = load().osmt_worker_render_tile_png(self._h, server._h, C.byref(t), scale, C.c_void_p(anchors.ctypes.data) if n else None, n,
                                                C.c_void_p(out.ctypes.data) if out.size else None, out.size, C.byref(got))
        self.last_len = got.value  # the size needed, also when the buffer was too small
        check(rc)
        return out[: got.value].tobytes()

    def close(self):
        if getattr(self, "_h", None):
            load().osmt_worker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_declined_anchors():
    """osmt_last_declined_anchors: the (tile, entity) pairs the last tile-server call of THIS thread declined, as a
    labels.AREA_ANCHOR_DTYPE array."""
    from .labels import AREA_ANCHOR_DTYPE

    L, n = load(), C.c_size_t()
    check(L.osmt_last_declined_anchors(None, 0, C.byref(n)))
    out = np.zeros(n.value, AREA_ANCHOR_DTYPE)
    if n.value:
        check(L.osmt_last_declined_anchors(C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
    return out


class TileServer:
    """osmt_tile_server: what a server renders its requests with, stated once.  bindings / area_label_bindings /
    node_label_bindings: {zoom: id} (a zoom that is missing has none; an empty dict: no labels of that kind); id_filter: from
    Context.register_id_filter or None; canvas: (r, g, b) or None."""

    def __init__(self, ctx, geodata_id, bindings, area_label_bindings=None, node_label_bindings=None, id_filter=None, canvas=(241, 238, 232),
                 use_caps_for_dashes=True):
        self.ctx = ctx
        self.desc = self.describe(geodata_id, bindings, area_label_bindings, node_label_bindings, id_filter, canvas, use_caps_for_dashes)
        h = C.c_void_p()
        check(load().osmt_tile_server_create(ctx._h, C.byref(self.desc), C.byref(h)))
        self._h = h

    @staticmethod
    def describe(geodata_id, bindings, area_label_bindings=None, node_label_bindings=None, id_filter=None, canvas=(241, 238, 232), use_caps_for_dashes=True):
        d = abi.TileServerDesc()
        d.geodata_id, d.use_caps_for_dashes = int(geodata_id), int(bool(use_caps_for_dashes))
        d.id_filter = abi.ID_FILTER_NONE if id_filter is None else int(id_filter)
        if canvas is not None:
            d.has_canvas = 1
            d.canvas_rgb[0], d.canvas_rgb[1], d.canvas_rgb[2] = canvas
        for arr, b in ((d.bindings_of_zoom, bindings), (d.area_label_bindings_of_zoom, area_label_bindings), (d.node_label_bindings_of_zoom, node_label_bindings)):
            b = dict(b or {})
            for z in range(abi.MAX_ZOOM + 1):
                arr[z] = int(b.get(z, abi.BINDINGS_NONE))
        return d

    def render_png(self, tiles, scale=1, anchors=None, out=None, as_bytes=True):
        """osmt_tile_server_render_png: the PNG files of tiles [(zoom, x, y)] — build (filtered or not), label, render, encode in
        one call.  anchors: labels.AREA_ANCHOR_DTYPE for pairs an earlier call declined (last_declined_anchors()).  Returns the
        files as a list of bytes, or with as_bytes=False (blob, offsets); `offsets` is kept on self.last_offsets either way."""
        from .labels import AREA_ANCHOR_DTYPE

        n = len(tiles)
        t = (abi.TileCoord * max(n, 1))(*[abi.TileCoord(int(x), int(y), int(z)) for z, x, y in tiles])
        na = 0
        if anchors is not None:
            anchors = np.ascontiguousarray(anchors, dtype=AREA_ANCHOR_DTYPE)
            na = len(anchors)
        if out is None:
            out = np.empty(n * load().osmt_png_device_bound(256 * scale, 256 * scale), np.uint8)
        off = (C.c_uint64 * (n + 1))()
        rc = load().osmt_tile_server_render_png(self._h, t, n, scale, C.c_void_p(anchors.ctypes.data) if na else None, na,
                                                C.c_void_p(out.ctypes.data) if out.size else None, out.size, off)
        self.last_offsets = np.array(off[:], dtype=np.uint64)
        check(rc)
        if not as_bytes:
            return out, self.last_offsets
        return [out[int(off[i]) : int(off[i + 1])].tobytes() for i in range(n)]

    def close(self):
        if getattr(self, "_h", None):
            load().osmt_tile_server_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PngJob:
    """A begun osmt_render_batch_png job.  Holds the display list (and labels) alive — the uploads are stream-ordered —
    and the native handle exactly once: png_end() takes it (the native call frees the job whatever it returns), a second
    png_end() raises instead of touching freed memory, and a job that is dropped without being ended is ended here with an
    empty buffer, which releases its device buffers (about 0.9 GB per 1024 tiles).

    A job of Context.scene_png_begin holds its Scene alive instead (`scene`; `dl` is None): the native job borrows the scene,
    which must not be freed before the job is ended."""

    def __init__(self, h, dl, labels, b, lb, scene=None):
        self._h, self.dl, self.labels, self._b, self._lb, self.scene = h, dl, labels, b, lb, scene
        self.n_jobs = scene.n_jobs if scene is not None else dl.n_jobs

    def take(self):
        if self._h is None:
            raise RuntimeError("this PNG job has already been ended (osmt_render_batch_png_end frees it whatever it returns)")
        h, self._h = self._h, None
        return h

    def abort(self):
        """Ends the job without reading the files back (frees its device buffers)."""
        if self._h is not None:
            h, self._h = self._h, None
            off = (C.c_uint64 * (self.n_jobs + 1))()
            load().osmt_render_batch_png_end(h, None, 0, off)

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class Context:
    """One GPU (osmt_ctx): analogue of the reference's Drawer + per-worker TilePixels."""

    def worker(self):
        return Worker(self)

    def tile_server(self, geodata_id, bindings, **kw):
        return TileServer(self, geodata_id, bindings, **kw)

    def worker_tile_stats(self):
        """osmt_worker_tile_stats: (requests, groups run, tiles of the largest group) of Worker.render_tile_png since the context
        was created"""
        st = (C.c_uint64 * 3)()
        check(load().osmt_worker_tile_stats(self._h, st))
        return tuple(int(v) for v in st)

    def __init__(self, device=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the MI355X raster path has no CPU fallback")
        L = load()
        cfg = abi.Config(device=device, flags=0)
        h = C.c_void_p()
        check(L.osmt_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)

    def close(self):
        if getattr(self, "_h", None):
            load().osmt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- icons -------------------------------------------------------------------
    def register_image(self, rgba8):
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        h, w, four = img.shape
        assert four == 4
        out = C.c_uint32()
        check(load().osmt_register_image(self._h, img.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, C.byref(out)))
        return out.value

    # -- display lists built on the GPU ---------------------------------------------
    def register_geodata(self, geodata):
        """osmt_register_geodata: uploads a styled.Geodata (a geodata file's topology); returns its id."""
        d = geodata.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_geodata(self._h, C.byref(d), C.byref(out)))
        self._geodata_nodes = getattr(self, "_geodata_nodes", {})
        self._geodata_nodes[out.value] = geodata.nodes
        return out.value

    def register_styles(self, styles, dashes=()):
        """osmt_register_styles: appends styled.STYLE_REC_DTYPE records and the (unscaled) dash pool their dash ranges
        index; returns the id of the first."""
        st = np.ascontiguousarray(styles, dtype=_styled().STYLE_REC_DTYPE).reshape(-1)
        pool = np.ascontiguousarray(dashes, dtype=np.float64).reshape(-1)
        out = C.c_uint32()
        check(load().osmt_register_styles(self._h, st.ctypes.data_as(C.POINTER(abi.StyleRec)) if len(st) else None, len(st),
                                          pool.ctypes.data_as(C.POINTER(C.c_double)) if len(pool) else None, len(pool), C.byref(out)))
        return out.value

    def validate_styled(self, batch):
        """osmt_validate_styled_batch against this context's registrations (host only); raises OsmtError."""
        b = batch.as_batch()
        check(load().osmt_validate_styled_batch(C.byref(b), self._h))

    def build_styled(self, batch) -> Scene:
        """osmt_scene_build_styled: the scene of a styled.StyledBatch, its display list built on the GPU."""
        b = batch.as_batch()
        h = C.c_void_p()
        check(load().osmt_scene_build_styled(self._h, C.byref(b), C.byref(h)))
        return Scene._built(self, h, batch.n_jobs, batch.scale, getattr(self, "_geodata_nodes", {}).get(batch.geodata_id))

    # -- scenes built from tile coordinates -----------------------------------------
    def register_tile_index(self, geodata_id, index):
        """osmt_register_tile_index: uploads a styled.TileIndex for a registered geodata file (one per file)."""
        d = index.as_desc()
        check(load().osmt_register_tile_index(self._h, geodata_id, C.byref(d)))

    def register_tile_pyramid(self, geodata_id, level_mask=abi.PYRAMID_ALL_LEVELS):
        """osmt_register_tile_pyramid: builds the levels of level_mask (bit L = level L) of the file's tile index on the device.
        A tile of zoom z then reads the smallest registered level >= z.  One pyramid per file."""
        check(load().osmt_register_tile_pyramid(self._h, geodata_id, level_mask))

    def tile_pyramid_levels(self, geodata_id):
        """osmt_tile_pyramid_levels: (mask of the levels that exist, mask of those with node lists); (0, 0) without a pyramid."""
        m, n = C.c_uint32(), C.c_uint32()
        check(load().osmt_tile_pyramid_levels(self._h, geodata_id, C.byref(m), C.byref(n)))
        return m.value, n.value

    def read_tile_pyramid(self, geodata_id, level):
        """osmt_read_tile_pyramid: one level as a dict of uint32 arrays — tile_xy [n][2], way_off, ways, mp_off, mps, node_off,
        nodes (a level without node lists: node_off of zeros, no nodes)."""
        L = load()
        counts = (C.c_size_t * 4)()
        check(L.osmt_read_tile_pyramid(self._h, geodata_id, level, None, None, None, None, None, None, None, None, counts))
        n, nw, nm, nn = (int(c) for c in counts)
        out = {"tile_xy": np.zeros((n, 2), np.uint32), "way_off": np.zeros(n + 1, np.uint32), "ways": np.zeros(nw, np.uint32),
               "mp_off": np.zeros(n + 1, np.uint32), "mps": np.zeros(nm, np.uint32), "node_off": np.zeros(n + 1, np.uint32),
               "nodes": np.zeros(nn, np.uint32)}
        caps = (C.c_size_t * 4)(n, nw, nm, nn)
        check(L.osmt_read_tile_pyramid(self._h, geodata_id, level, *(out[k].ctypes.data for k in ("tile_xy", "way_off", "ways", "mp_off", "mps", "node_off", "nodes")),
                                       caps, counts))
        return out

    def build_tile_index(self, geodata_id, node_ids=None):
        """osmt_build_tile_index: the file's z18 tile index built on the device from its registered Mercator factors
        (register_node_mercator) and its topology, installed as register_tile_index would install it.  node_ids: the nodes'
        global ids (uint64, one per node) registers the node index in the same call; None: the tile index alone."""
        ids, n = None, 0
        if node_ids is not None:
            a = np.ascontiguousarray(node_ids, dtype=np.uint64).reshape(-1)
            n = len(a)
            keep = a if n else np.zeros(1, np.uint64)  # never empty: a pointer to pass
            ids = keep.ctypes.data_as(C.POINTER(C.c_uint64))
        check(load().osmt_validate_tile_index_build(geodata_id, ids, n, self._h))
        check(load().osmt_build_tile_index(self._h, geodata_id, ids, n))

    def read_tile_index(self, geodata_id):
        """osmt_read_tile_index: the file's z18 tile index, built or registered, as a dict of uint32 arrays — tile_xy [n][2],
        way_off, ways, mp_off, mps, node_off, nodes (no node index and not built: node_off of zeros, no nodes)."""
        L = load()
        counts = (C.c_size_t * 4)()
        check(L.osmt_read_tile_index(self._h, geodata_id, None, None, None, None, None, None, None, None, counts))
        n, nw, nm, nn = (int(c) for c in counts)
        out = {"tile_xy": np.zeros((n, 2), np.uint32), "way_off": np.zeros(n + 1, np.uint32), "ways": np.zeros(nw, np.uint32),
               "mp_off": np.zeros(n + 1, np.uint32), "mps": np.zeros(nm, np.uint32), "node_off": np.zeros(n + 1, np.uint32),
               "nodes": np.zeros(nn, np.uint32)}
        caps = (C.c_size_t * 4)(n, nw, nm, nn)
        check(L.osmt_read_tile_index(self._h, geodata_id, *(out[k].ctypes.data for k in ("tile_xy", "way_off", "ways", "mp_off", "mps", "node_off", "nodes")),
                                     caps, counts))
        return out

    def assemble_multipolygons(self, relations):
        """osmt_assemble_multipolygons: the polygons and multipolygons of `relations` (styled.Relations), assembled on the device as
        the importer's find_polygons_in_multipolygon assembles them.  A dict of numpy arrays in the form osmt_geodata_desc takes —
        polygon_node_off, polygon_nodes, multipolygon_ids, multipolygon_polygon_off, multipolygon_polygons — plus status
        (styled.RELATION_STATUS_DTYPE, one per relation) and multipolygon_relation (the relation a multipolygon came from);
        styled.Geodata.from_arrays makes a Geodata of it."""
        from . import styled

        L = load()
        d = relations.as_desc()
        check(L.osmt_validate_relations(C.byref(d)))
        h = C.c_void_p()
        check(L.osmt_assemble_multipolygons(self._h, C.byref(d), C.byref(h)))
        try:
            counts = (C.c_size_t * 4)()
            check(L.osmt_polygons_counts(h, counts))
            n_polys, n_nodes, n_mps, n_mp_polys = (int(c) for c in counts)
            out = {"polygon_node_off": np.zeros(n_polys + 1, np.uint32), "polygon_nodes": np.zeros(n_nodes, np.uint32),
                   "multipolygon_ids": np.zeros(n_mps, np.uint64), "multipolygon_polygon_off": np.zeros(n_mps + 1, np.uint32),
                   "multipolygon_polygons": np.zeros(n_mp_polys, np.uint32), "status": np.zeros(int(d.n_relations), styled.RELATION_STATUS_DTYPE),
                   "multipolygon_relation": np.zeros(n_mps, np.uint32)}
            check(L.osmt_polygons_read(self._h, h, *(out[k].ctypes.data for k in ("polygon_node_off", "polygon_nodes", "multipolygon_ids",
                                                                                 "multipolygon_polygon_off", "multipolygon_polygons", "status",
                                                                                 "multipolygon_relation"))))
        finally:
            L.osmt_polygons_free(h)
        return out

    def debug_vertex_hash_bits(self, bits):
        """osmt_debug_vertex_hash_bits (test hook): later assemblies keep only the low `bits` bits of the position hash"""
        check(load().osmt_debug_vertex_hash_bits(self._h, bits))

    def resolve_refs(self, raw):
        """osmt_resolve_refs: the global ids of `raw` (styled.RawOsm) resolved to local indices on the device as the importer's
        translate_id, its drop of unresolved references and its postprocess_node_refs resolve them.  A dict of numpy arrays in
        the form osmt_relations_desc and osmt_geodata_desc take — way_node_off, way_nodes, relation_way_off, relation_ways,
        relation_way_inner — plus counts: (way nodes kept, relation ways kept, node references unresolved, node references
        removed as repeats, way references unresolved).  styled.Relations.from_resolved makes the Relations of it."""
        L = load()
        d = raw.as_desc()
        check(L.osmt_validate_resolve(C.byref(d)))
        h = C.c_void_p()
        check(L.osmt_resolve_refs(self._h, C.byref(d), C.byref(h)))
        try:
            counts = (C.c_size_t * 5)()
            check(L.osmt_resolved_counts(h, counts))
            counts = tuple(int(c) for c in counts)
            out = {"way_node_off": np.zeros(int(d.n_ways) + 1, np.uint32), "way_nodes": np.zeros(counts[0], np.uint32),
                   "relation_way_off": np.zeros(int(d.n_relations) + 1, np.uint32), "relation_ways": np.zeros(counts[1], np.uint32),
                   "relation_way_inner": np.zeros(counts[1], np.uint8)}
            check(L.osmt_resolved_read(self._h, h, *(out[k].ctypes.data for k in ("way_node_off", "way_nodes", "relation_way_off", "relation_ways",
                                                                                 "relation_way_inner"))))
            out["counts"] = counts
        finally:
            L.osmt_resolved_free(h)
        return out

    def debug_resolve_short_way_max(self, n):
        """osmt_debug_resolve_short_way_max (test hook): later resolutions dedup ways of up to n references in LDS, longer ones
        through the sort; 0: every way through the sort"""
        check(load().osmt_debug_resolve_short_way_max(self._h, n))

    def tile_query_stats(self):
        """osmt_tile_query_stats: ((tile, column) items, way, multipolygon, node candidates) the last completed tile query of this
        context gathered, before dedup"""
        st = (C.c_uint64 * 4)()
        check(load().osmt_tile_query_stats(self._h, st))
        return tuple(int(v) for v in st)

    def register_tags(self, geodata_id, tags):
        """osmt_register_tags: the tags of a registered geodata file (selmatch.Tags or a ctypes osmt_tags_desc)."""
        d = tags.as_desc() if hasattr(tags, "as_desc") else tags
        check(load().osmt_register_tags(self._h, geodata_id, C.byref(d)))

    def register_selectors(self, selectors):
        """osmt_register_selectors: appends a selmatch.SelectorSet; returns its id."""
        d = selectors.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_selectors(self._h, C.byref(d), C.byref(out)))
        return out.value

    def register_rules(self, rules, class_layers=False):
        """osmt_register_rules_ex: appends a selmatch.RuleSet; returns its id (Match.cascade takes it).  class_layers:
        OSMT_RULES_CLASS_LAYERS, up to 255 layer names with at most 16 layers per class instead of 8 names in all."""
        d = rules.as_desc()
        out = C.c_uint32()
        L = load()
        if class_layers or hasattr(L, "osmt_register_rules_ex"):  # absent only from older variant builds loaded through OSMT_LIB
            check(L.osmt_register_rules_ex(self._h, C.byref(d), abi.RULES_CLASS_LAYERS if class_layers else 0, C.byref(out)))
        else:
            check(L.osmt_register_rules(self._h, C.byref(d), C.byref(out)))
        return out.value

    def validate_rules(self, rules, class_layers=False):
        """osmt_validate_rules_ex against this context's registries; raises OsmtError with the refusal."""
        from . import selmatch

        selmatch.validate_rules(rules, class_layers, self)

    def match_selectors(self, geodata_id, selectors_id, overrides=None):
        """osmt_match_selectors: a selmatch.Match; raises selmatch.Declined with the values to supply as overrides."""
        from . import selmatch

        return selmatch.match(self, geodata_id, selectors_id, overrides)

    def debug_match_hash_bits(self, bits):
        """osmt_debug_match_hash_bits: the class table of later matches keeps only the low `bits` bits of the key hash."""
        check(load().osmt_debug_match_hash_bits(self._h, bits))

    def register_style_bindings(self, bindings):
        """osmt_register_style_bindings: appends a styled.StyleBindings table; returns its id."""
        d = bindings.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_style_bindings(self._h, C.byref(d), C.byref(out)))
        return out.value

    def validate_tiles(self, batch):
        """osmt_validate_tile_batch against this context's registrations (host only); raises OsmtError."""
        b = batch.as_batch()
        check(load().osmt_validate_tile_batch(C.byref(b), self._h))

    def build_tiles(self, batch, id_filter=None) -> Scene:
        """osmt_scene_build_tiles: the scene of a styled.TileBatch — tile query, style lookup and display list on the GPU.
        id_filter: an id from register_id_filter (osmt_scene_build_tiles_filtered): only listed entities are drawn, and the
        scene's label builds apply the same filter; None: no filter."""
        b = batch.as_batch()
        h = C.c_void_p()
        if id_filter is None:
            check(load().osmt_scene_build_tiles(self._h, C.byref(b), C.byref(h)))
        else:
            check(load().osmt_scene_build_tiles_filtered(self._h, C.byref(b), int(id_filter), C.byref(h)))
        return Scene._built(self, h, batch.n_jobs, batch.scale, getattr(self, "_geodata_nodes", {}).get(batch.geodata_id))

    # -- the osm_ids filter -----------------------------------------------------------
    def register_id_filter(self, geodata_id, ids):
        """osmt_register_id_filter: a set of global ids (any order, repeats allowed; empty: keeps nothing) as bit-planes over
        the nodes, ways and multipolygons of a registered geodata file; returns the filter id for build_tiles."""
        a = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        out = C.c_uint32()
        check(load().osmt_register_id_filter(self._h, geodata_id, a.ctypes.data_as(C.POINTER(C.c_uint64)) if len(a) else None, len(a), C.byref(out)))
        return out.value

    def read_id_filter(self, filter_id):
        """osmt_read_id_filter: the (way, multipolygon, node) bit-planes as uint32 arrays; entity e is bit e % 32 of word e // 32;
        the node plane is empty if no node index was registered when the filter was."""
        L, n = load(), (C.c_size_t * 3)()
        check(L.osmt_read_id_filter(self._h, filter_id, None, None, None, None, n))
        planes = [np.zeros(n[k], np.uint32) for k in range(3)]
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        caps = (C.c_size_t * 3)(n[0], n[1], n[2])
        check(L.osmt_read_id_filter(self._h, filter_id, ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), caps, n))
        return tuple(planes)

    # -- node labels of tile-built scenes ---------------------------------------------
    def register_node_index(self, geodata_id, index):
        """osmt_register_node_index: uploads a styled.NodeIndex for a geodata file whose tile index is registered."""
        d = index.as_desc()
        check(load().osmt_register_node_index(self._h, geodata_id, C.byref(d)))

    def register_label_styles(self, styles):
        """osmt_register_label_styles: appends styled.LABEL_STYLE_REC_DTYPE records; returns the id of the first."""
        from .styled import LABEL_STYLE_REC_DTYPE

        st = np.ascontiguousarray(styles, dtype=LABEL_STYLE_REC_DTYPE)
        out = C.c_uint32()
        check(load().osmt_register_label_styles(self._h, st.ctypes.data_as(C.POINTER(abi.LabelStyleRec)) if len(st) else None, len(st), C.byref(out)))
        return out.value

    def register_area_label_bindings(self, bindings):
        """osmt_register_area_label_bindings: appends a styled.AreaLabelBindings table; returns its id."""
        d = bindings.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_area_label_bindings(self._h, C.byref(d), C.byref(out)))
        return out.value

    def register_label_bindings(self, bindings):
        """osmt_register_label_bindings: appends a styled.LabelBindings table; returns its id."""
        d = bindings.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_label_bindings(self._h, C.byref(d), C.byref(out)))
        return out.value

    def read_label_bindings(self, bindings_id, n_nodes):
        """osmt_read_label_bindings of any registered node table: (node_off [n_nodes + 1], bindings
        (styled.LABEL_BINDING_DTYPE), text_off, chars) as numpy arrays."""
        from .styled import LABEL_BINDING_DTYPE

        L, n = load(), (C.c_size_t * 3)()
        check(L.osmt_read_label_bindings(self._h, bindings_id, None, None, None, None, None, n))
        off, bind = np.zeros(n_nodes + 1, np.uint32), np.zeros(n[0], LABEL_BINDING_DTYPE)
        text_off, chars = np.zeros(n[1] + 1, np.uint32), np.zeros(n[2], np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        caps = (C.c_size_t * 3)(*n)
        check(L.osmt_read_label_bindings(self._h, bindings_id, ptr(off), ptr(bind), ptr(text_off), ptr(chars), caps, n))
        return off, bind, text_off, chars

    def read_area_label_bindings(self, bindings_id, n_ways, n_multipolygons):
        """osmt_read_area_label_bindings of any registered area table: (way_off, way_bindings, multipolygon_off,
        multipolygon_bindings, text_off, chars) as numpy arrays."""
        from .styled import LABEL_BINDING_DTYPE

        L, n = load(), (C.c_size_t * 4)()
        check(L.osmt_read_area_label_bindings(self._h, bindings_id, None, None, None, None, None, None, None, n))
        way_off, way = np.zeros(n_ways + 1, np.uint32), np.zeros(n[0], LABEL_BINDING_DTYPE)
        mp_off, mp = np.zeros(n_multipolygons + 1, np.uint32), np.zeros(n[1], LABEL_BINDING_DTYPE)
        text_off, chars = np.zeros(n[2] + 1, np.uint32), np.zeros(n[3], np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        caps = (C.c_size_t * 4)(*n)
        check(L.osmt_read_area_label_bindings(self._h, bindings_id, ptr(way_off), ptr(way), ptr(mp_off), ptr(mp), ptr(text_off), ptr(chars), caps, n))
        return way_off, way, mp_off, mp, text_off, chars

    # -- glyph outlines (glyph-run labels) -----------------------------------------
    def register_glyphs(self, table):
        """osmt_register_glyphs: appends the outlines of a labels.GlyphTable; returns (and records in the table) the id
        of its first glyph."""
        verts, voff = table.arrays()
        out = C.c_uint32()
        check(load().osmt_register_glyphs(self._h, verts.ctypes.data_as(C.POINTER(abi.GlyphVertex)) if len(verts) else None,
                                          voff.ctypes.data_as(C.POINTER(C.c_uint32)), len(voff) - 1, C.byref(out)))
        table.first_id = out.value
        return out.value

    # -- fonts (string labels) -------------------------------------------------------
    def register_font(self, font):
        """osmt_register_font: appends a labels.FontTable (its outline ids must be registered already); returns (and
        records in the table) the font id."""
        d, _keep = font.as_desc()
        out = C.c_uint32()
        check(load().osmt_register_font(self._h, C.byref(d), C.byref(out)))
        font.font_id = out.value
        return out.value

    def validate_string_labels(self, string_labels, n_jobs=None):
        """osmt_validate_string_labels against this context's fonts (host only); raises OsmtError."""
        sb = string_labels.as_batch()
        check(load().osmt_validate_string_labels(C.byref(sb), string_labels.n_jobs if n_jobs is None else n_jobs, self._h))

    def debug_hypot(self, x, y):
        """osmt_debug_hypot: the device hypot of the glyph walk over pairs, float64."""
        xy = np.ascontiguousarray(np.stack([np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()], axis=1))
        out = np.empty(len(xy), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(load().osmt_debug_hypot(self._h, xy.ctypes.data_as(dp), len(xy), out.ctypes.data_as(dp)))
        return out

    # -- label anchors --------------------------------------------------------------
    def _label_request_batch(self, rings, points, requests):
        from . import labels

        rings = np.ascontiguousarray(rings, dtype=np.uint32).reshape(-1, 2)  # osmt_ring: (first_pt, n_pts)
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        requests = np.ascontiguousarray(requests, dtype=labels.LABEL_REQUEST_DTYPE)
        b = abi.LabelRequestBatch(
            requests=requests.ctypes.data_as(C.POINTER(abi.LabelRequest)), n_requests=len(requests),
            rings=rings.ctypes.data_as(C.POINTER(abi.Ring)), n_rings=len(rings),
            points=points.ctypes.data_as(C.POINTER(C.c_double)), n_pts=len(points))
        return b, (rings, points, requests)

    def label_positions(self, rings, points, requests, out=None):
        """osmt_label_positions: get_label_position (src/draw/labelable.rs:191-204) of every request on the GPU.
        rings: [n, 2] uint32 (first_pt, n_pts); points: [m, 2] float64, projected and scaled by the caller; requests:
        labels.LABEL_REQUEST_DTYPE.  Returns a labels.LABEL_POSITION_DTYPE array (status: abi.LABEL_*)."""
        from . import labels

        b, keep = self._label_request_batch(rings, points, requests)
        if out is None:
            out = np.zeros(len(keep[2]), labels.LABEL_POSITION_DTYPE)
        assert out.dtype == labels.LABEL_POSITION_DTYPE and len(out) == len(keep[2]) and out.flags.c_contiguous
        check(load().osmt_label_positions(self._h, C.byref(b), out.ctypes.data_as(C.c_void_p)))
        return out

    def label_positions_begin(self, rings, points, requests):
        """osmt_label_positions_begin: validates, uploads and queues the kernels; returns a job for label_positions_end."""
        b, keep = self._label_request_batch(rings, points, requests)
        job = C.c_void_p()
        check(load().osmt_label_positions_begin(self._h, C.byref(b), C.byref(job)))
        return job, keep

    def label_positions_end(self, job):
        from . import labels

        h, keep = job
        out = np.zeros(len(keep[2]), labels.LABEL_POSITION_DTYPE)
        check(load().osmt_label_positions_end(h, out.ctypes.data_as(C.c_void_p)))
        return out

    def label_positions_stats(self):
        """(requests, requests that left the LDS tier, requests answered TOO_LARGE) of the last completed call."""
        st = (C.c_uint64 * 3)()
        check(load().osmt_label_positions_stats(self._h, st))
        return int(st[0]), int(st[1]), int(st[2])

    # -- label anchors from tile coordinates ------------------------------------------
    def register_node_mercator(self, geodata_id, factors):
        """osmt_register_node_mercator: uploads the [n_nodes, 2] float64 Mercator factors of a registered geodata file (one
        table per file) — (lon_rad + PI) / (2 PI) and (PI - ln(tan(PI / 4 + lat_rad / 2))) / (2 PI) per node, computed by the
        caller with its own libm."""
        f = np.ascontiguousarray(factors, dtype=np.float64).reshape(-1, 2)
        # the C entry takes no count (the table's length is the file's): the validator is what compares the two
        check(load().osmt_validate_node_mercator(f.ctypes.data_as(C.POINTER(C.c_double)) if len(f) else None, len(f), geodata_id, self._h))
        check(load().osmt_register_node_mercator(self._h, geodata_id, f.ctypes.data_as(C.POINTER(C.c_double)) if len(f) else None))

    def _label_tile_batch(self, geodata_id, tiles, requests, scale):
        from . import labels, styled

        if not (isinstance(tiles, np.ndarray) and tiles.dtype == styled.QUERY_TILE_DTYPE):
            t = np.zeros(len(tiles), styled.QUERY_TILE_DTYPE)
            for rec, (zoom, x, y) in zip(t, tiles):
                rec["zoom"], rec["x"], rec["y"] = zoom, x, y
            tiles = t
        tiles = np.ascontiguousarray(tiles)
        if not (isinstance(requests, np.ndarray) and requests.dtype == labels.LABEL_TILE_REQUEST_DTYPE):
            requests = np.array([(int(e), int(t)) for e, t in requests], dtype=labels.LABEL_TILE_REQUEST_DTYPE).reshape(-1)
        requests = np.ascontiguousarray(requests)
        b = abi.LabelTileBatch(
            requests=requests.ctypes.data_as(C.POINTER(abi.LabelTileRequest)) if len(requests) else None, n_requests=len(requests),
            tiles=tiles.ctypes.data_as(C.POINTER(abi.QueryTile)) if len(tiles) else None, n_tiles=len(tiles),
            geodata_id=int(geodata_id), scale=int(scale))
        return b, (tiles, requests)

    def validate_label_tiles(self, geodata_id, tiles, requests, scale=1):
        """osmt_validate_label_tile_batch against this context's registrations (host only); raises OsmtError."""
        b, _keep = self._label_tile_batch(geodata_id, tiles, requests, scale)
        check(load().osmt_validate_label_tile_batch(C.byref(b), self._h))

    def label_positions_tiles(self, geodata_id, tiles, requests, scale=1, out=None):
        """osmt_label_positions_tiles: get_label_position of every (entity, tile) request, projected on the GPU from the
        registered Mercator factors.  tiles: [(zoom, x, y)] or a styled.QUERY_TILE_DTYPE array; requests: [(entity, tile
        index)] (a multipolygon's entity carries abi.STYLED_MULTIPOLYGON) or a labels.LABEL_TILE_REQUEST_DTYPE array.
        Returns a labels.LABEL_POSITION_DTYPE array."""
        from . import labels

        b, keep = self._label_tile_batch(geodata_id, tiles, requests, scale)
        if out is None:
            out = np.zeros(len(keep[1]), labels.LABEL_POSITION_DTYPE)
        assert out.dtype == labels.LABEL_POSITION_DTYPE and len(out) == len(keep[1]) and out.flags.c_contiguous
        check(load().osmt_label_positions_tiles(self._h, C.byref(b), out.ctypes.data_as(C.c_void_p)))
        return out

    def label_positions_tiles_begin(self, geodata_id, tiles, requests, scale=1):
        """osmt_label_positions_tiles_begin: returns a job for label_positions_end."""
        b, keep = self._label_tile_batch(geodata_id, tiles, requests, scale)
        job = C.c_void_p()
        check(load().osmt_label_positions_tiles_begin(self._h, C.byref(b), C.byref(job)))
        return job, (None, None, keep[1])

    def label_tile_batch_expand(self, geodata_id, tiles, requests, scale=1):
        """osmt_label_tile_batch_expand: (rings [n, 2] uint32 (first_pt, n_pts), points [m, 2] float64) — what the search of
        this batch is given."""
        b, _keep = self._label_tile_batch(geodata_id, tiles, requests, scale)
        counts = (C.c_size_t * 2)()
        check(load().osmt_label_tile_batch_expand(self._h, C.byref(b), None, None, 0, 0, counts))
        rings = np.zeros((counts[0], 2), np.uint32)
        points = np.zeros((counts[1], 2), np.float64)
        check(load().osmt_label_tile_batch_expand(self._h, C.byref(b), rings.ctypes.data_as(C.c_void_p), points.ctypes.data_as(C.c_void_p),
                                                  len(rings), len(points), counts))
        assert (counts[0], counts[1]) == (len(rings), len(points))
        return rings, points

    # -- whole path --------------------------------------------------------------
    def upload(self, dl: DisplayList, labels=None) -> Scene:
        return Scene(self, dl, labels)

    def render(self, scene: Scene, out=None, stream=None):
        """osmt_render_scene: returns a uint8 cuda tensor [n, H, W, 4] (asynchronous)."""
        torch = _torch()
        if out is None:
            out = torch.empty((scene.n_jobs, scene.dim, scene.dim, 4), dtype=torch.uint8, device=self.device)
        stride = scene.dim * scene.dim * 4
        check(load().osmt_render_scene(self._h, scene._h, C.c_void_p(out.data_ptr()), stride, _stream_ptr(stream)))
        return out

    def render_stages(self, scene: Scene, stage_mask, out=None, stream=None):
        stride = scene.dim * scene.dim * 4
        ptr = C.c_void_p(out.data_ptr()) if out is not None else C.c_void_p(0)
        check(load().osmt_render_scene_stages(self._h, scene._h, stage_mask, ptr, stride, _stream_ptr(stream)))
        return out

    def render_f64(self, scene: Scene, stream=None):
        """osmt_render_scene_f64: premultiplied f64 canvas [n, H, W, 4]."""
        torch = _torch()
        out = torch.empty((scene.n_jobs, scene.dim, scene.dim, 4), dtype=torch.float64, device=self.device)
        check(load().osmt_render_scene_f64(self._h, scene._h, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
        return out

    def read_points(self, scene: Scene):
        out = np.empty((len(scene.dl.coords), 2), dtype=np.int32)
        check(load().osmt_scene_read_points(self._h, scene._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def host_alloc(self, shape, dtype=np.uint8):
        """osmt_host_alloc: a pinned numpy array (free it with host_free)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(load().osmt_host_alloc(self._h, n, C.byref(p)))
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        load().osmt_host_free(self._h, p)

    def render_batch_host(self, dl: DisplayList, labels=None, out=None):
        """osmt_render_batch / osmt_render_batch_labels: host buffers in, host RGBA8 out (`out`: e.g. host_alloc())."""
        b = dl.as_batch()
        if out is None:
            out = np.empty((dl.n_jobs, dl.dim, dl.dim, 4), dtype=np.uint8)
        assert out.shape == (dl.n_jobs, dl.dim, dl.dim, 4) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        if labels is None:
            check(load().osmt_render_batch(self._h, C.byref(b), out.ctypes.data_as(C.POINTER(C.c_uint8)), dl.dim * dl.dim * 4))
        else:
            lb = labels.as_batch()
            check(load().osmt_render_batch_labels(self._h, C.byref(b), C.byref(lb), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  dl.dim * dl.dim * 4))
        return out

    def render_batch_rgb(self, dl: DisplayList, labels=None, out=None, stride=None):
        """osmt_render_batch_rgb: host buffers in, packed RGB8 out (the reference's RgbTriples layout)."""
        b = dl.as_batch()
        tight = dl.dim * dl.dim * 3
        stride = tight if stride is None else stride
        if out is None:
            out = np.empty((dl.n_jobs, stride), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= dl.n_jobs * stride
        lb = labels.as_batch() if labels is not None else None
        check(load().osmt_render_batch_rgb(self._h, C.byref(b), C.byref(lb) if lb is not None else None,
                                           out.ctypes.data_as(C.POINTER(C.c_uint8)), stride))
        return out

    def render_batch_rgb_glyphs(self, dl: DisplayList, glyph_labels, out=None, stride=None):
        """osmt_render_batch_rgb_glyphs: osmt_render_batch_rgb with glyph-run labels (labels.GlyphLabelList)."""
        b = dl.as_batch()
        tight = dl.dim * dl.dim * 3
        stride = tight if stride is None else stride
        if out is None:
            out = np.empty((dl.n_jobs, stride), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= dl.n_jobs * stride
        gb = glyph_labels.as_batch() if glyph_labels is not None else None
        check(load().osmt_render_batch_rgb_glyphs(self._h, C.byref(b), C.byref(gb) if gb is not None else None,
                                                  out.ctypes.data_as(C.POINTER(C.c_uint8)), stride))
        return out

    def render_batch_rgb_text(self, dl: DisplayList, text_labels, out=None, stride=None):
        """osmt_render_batch_rgb_text: osmt_render_batch_rgb with text-run labels (labels.TextLabelList)."""
        b = dl.as_batch()
        tight = dl.dim * dl.dim * 3
        stride = tight if stride is None else stride
        if out is None:
            out = np.empty((dl.n_jobs, stride), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= dl.n_jobs * stride
        tb = text_labels.as_batch() if text_labels is not None else None
        check(load().osmt_render_batch_rgb_text(self._h, C.byref(b), C.byref(tb) if tb is not None else None,
                                                out.ctypes.data_as(C.POINTER(C.c_uint8)), stride))
        return out

    def render_batch_rgb_strings(self, dl: DisplayList, string_labels, out=None, stride=None):
        """osmt_render_batch_rgb_strings: osmt_render_batch_rgb with string labels (labels.StringLabelList)."""
        b = dl.as_batch()
        tight = dl.dim * dl.dim * 3
        stride = tight if stride is None else stride
        if out is None:
            out = np.empty((dl.n_jobs, stride), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= dl.n_jobs * stride
        sb = string_labels.as_batch() if string_labels is not None else None
        check(load().osmt_render_batch_rgb_strings(self._h, C.byref(b), C.byref(sb) if sb is not None else None,
                                                   out.ctypes.data_as(C.POINTER(C.c_uint8)), stride))
        return out

    # -- PNG files from the GPU ----------------------------------------------------
    def encode_png_device(self, rgba, stream=None):
        """osmt_encode_png_device on a uint8 cuda tensor [n, H, W, 4]: (slots uint8 [n, bound], lengths int32 [n]).
        W is a multiple of 4 and at most 1024, H at most 1024: anything else raises OsmtError (OSMT_UNSUPPORTED) before a launch."""
        torch = _torch()
        assert rgba.is_cuda and rgba.dtype == torch.uint8 and rgba.is_contiguous()
        n, H, W, four = rgba.shape
        assert four == 4
        bound = load().osmt_png_device_bound(W, H)
        slots = torch.empty((n, bound), dtype=torch.uint8, device=rgba.device)
        lens = torch.empty((n,), dtype=torch.int32, device=rgba.device)
        check(load().osmt_encode_png_device(self._h, C.c_void_p(rgba.data_ptr()), H * W * 4, n, W, H, C.c_void_p(slots.data_ptr()), bound,
                                            C.c_void_p(lens.data_ptr()), _stream_ptr(stream)))
        return slots, lens

    def render_batch_png(self, dl: DisplayList, labels=None, out=None, as_bytes=True):
        """osmt_render_batch_png: list of PNG files (bytes), one per tile.  `out`: uint8 buffer (e.g. host_alloc) to
        receive the files back to back; as_bytes=False returns (out, offsets) without copying."""
        b = dl.as_batch()
        lb = labels.as_batch() if labels is not None else None
        off = np.zeros(dl.n_jobs + 1, dtype=np.uint64)
        if out is None:
            out = np.empty(dl.n_jobs * load().osmt_png_device_bound(dl.dim, dl.dim), dtype=np.uint8)
        cap = out.size
        check(load().osmt_render_batch_png(self._h, C.byref(b), C.byref(lb) if lb is not None else None,
                                           out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, off.ctypes.data_as(C.POINTER(C.c_uint64))))
        if not as_bytes:
            return out, off
        return [out[int(off[i]) : int(off[i + 1])].tobytes() for i in range(dl.n_jobs)]

    def png_begin(self, dl: DisplayList, labels=None):
        """osmt_render_batch_png_begin: queues the whole batch, returns a job (keeps `dl` / `labels` alive until png_end)."""
        b = dl.as_batch()
        lb = labels.as_batch() if labels is not None else None
        h = C.c_void_p()
        check(load().osmt_render_batch_png_begin(self._h, C.byref(b), C.byref(lb) if lb is not None else None, C.byref(h)))
        return PngJob(h, dl, labels, b, lb)

    def png_end(self, job, out, as_bytes=False):
        """osmt_render_batch_png_end: (out, offsets) — or the list of files with as_bytes=True.

        The native call frees the job WHATEVER it returns (include/osmtile.h): a job can be ended once.  A buffer that
        turns out too small therefore needs a new png_begin — size `out` with osmt_png_device_bound x tiles and it cannot."""
        h, n = job.take(), job.n_jobs
        off = np.zeros(n + 1, dtype=np.uint64)
        job.offsets = off  # filled even when the call fails because `out` is too small: off[n] is the size needed
        check(load().osmt_render_batch_png_end(h, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, off.ctypes.data_as(C.POINTER(C.c_uint64))))
        if not as_bytes:
            return out, off
        return [out[int(off[i]) : int(off[i + 1])].tobytes() for i in range(n)]

    # -- host pixels and PNG files from any scene -----------------------------------
    def render_scene_host(self, scene: Scene, rgb=False, out=None, stride=None):
        """osmt_render_scene_host: the scene's tiles as host pixels — RGBA8 [n, W, W, 4], or with rgb=True packed RGB8
        [n, stride].  `out`: a uint8 array to fill (e.g. host_alloc()); `stride`: bytes from tile to tile (default: tight)."""
        tight = scene.dim * scene.dim * (3 if rgb else 4)
        stride = tight if stride is None else stride
        if out is None:
            out = np.empty((scene.n_jobs, scene.dim, scene.dim, 4) if (not rgb and stride == tight) else (scene.n_jobs, stride), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= scene.n_jobs * stride
        check(load().osmt_render_scene_host(self._h, scene._h, abi.PIXELS_RGB8 if rgb else abi.PIXELS_RGBA8, C.c_void_p(out.ctypes.data), stride))
        return out

    def render_scene_png(self, scene: Scene, out=None, as_bytes=True):
        """osmt_render_scene_png: the scene's tiles as PNG files (list of bytes); as_bytes=False returns (out, offsets)."""
        n = scene.n_jobs
        off = np.zeros(n + 1, dtype=np.uint64)
        if out is None:
            out = np.empty(max(1, n * load().osmt_png_device_bound(scene.dim, scene.dim)), dtype=np.uint8)
        check(load().osmt_render_scene_png(self._h, scene._h, C.c_void_p(out.ctypes.data), out.size, off.ctypes.data_as(C.POINTER(C.c_uint64))))
        if not as_bytes:
            return out, off
        return [out[int(off[i]) : int(off[i + 1])].tobytes() for i in range(n)]

    def scene_png_begin(self, scene: Scene):
        """osmt_render_scene_png_begin: queues the scene's tiles, returns a PngJob for png_end (the job keeps `scene` alive)."""
        h = C.c_void_p()
        check(load().osmt_render_scene_png_begin(self._h, scene._h, C.byref(h)))
        return PngJob(h, None, None, None, None, scene=scene)

    def render_scene_png_device(self, scene: Scene, png=None, work=None, stream=None):
        """osmt_render_scene_png_device, all on `stream`, nothing waited for: (png uint8 cuda tensor, offsets int64 cuda
        tensor [n + 1], status int32 cuda tensor [1]).  `png`: the tensor to receive the files back to back (default: the
        worst case); status 1 = it was too small, nothing written, the offsets complete."""
        torch = _torch()
        n = scene.n_jobs
        need = load().osmt_scene_png_work_bytes(self._h, scene._h)
        if work is None:
            work = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        if png is None:
            png = torch.empty((max(1, n * load().osmt_png_device_bound(scene.dim, scene.dim)),), dtype=torch.uint8, device=self.device)
        assert png.is_cuda and png.dtype == torch.uint8 and png.is_contiguous() and work.is_cuda and work.dtype == torch.uint8
        off = torch.empty((n + 1,), dtype=torch.int64, device=self.device)
        status = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(load().osmt_render_scene_png_device(self._h, scene._h, C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(png.data_ptr()),
                                                  png.numel(), C.c_void_p(off.data_ptr()), C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
        self._png_work = work  # stream-ordered use: stays alive until the next call replaces it
        return png, off, status

    def debug_png_offsets(self, lengths, capacity, stream=None):
        """osmt_debug_png_offsets: the offset scan alone on an int32 / uint32 cuda tensor of lengths (read as uint32):
        (offsets int64 [n + 1], status int32 [1]), queued on `stream`."""
        torch = _torch()
        assert lengths.is_cuda and lengths.is_contiguous() and lengths.element_size() == 4
        n = lengths.numel()
        off = torch.empty((n + 1,), dtype=torch.int64, device=lengths.device)
        status = torch.full((1,), -1, dtype=torch.int32, device=lengths.device)
        check(load().osmt_debug_png_offsets(self._h, C.c_void_p(lengths.data_ptr()) if n else None, n, int(capacity), C.c_void_p(off.data_ptr()),
                                            C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
        return off, status

    def hbm_copy_probe(self, nbytes=1 << 30, iters=20):
        """osmt_hbm_copy_probe: (copy GB/s counting read + write, read-only GB/s) of a 16-byte-per-lane device stream."""
        cp, rd = C.c_double(0.0), C.c_double(0.0)
        check(load().osmt_hbm_copy_probe(self._h, int(nbytes), int(iters), C.byref(cp), C.byref(rd)))
        return float(cp.value), float(rd.value)

    # -- stages --------------------------------------------------------------------
    def project(self, latlon, zoom, tx, ty, scale=1.0):
        latlon = np.ascontiguousarray(latlon, dtype=np.float64).reshape(-1, 2)
        out = np.empty((len(latlon), 2), dtype=np.int32)
        check(
            load().osmt_project(
                self._h, latlon.ctypes.data_as(C.POINTER(C.c_double)), len(latlon), zoom, tx, ty, float(scale),
                out.ctypes.data_as(C.POINTER(C.c_int32)),
            )
        )
        return out

    def composite_host(self, planes, canvas_rgba):
        planes = np.ascontiguousarray(planes, dtype=np.float64)
        n, L, H, W, four = planes.shape
        assert four == 4
        cv = np.ascontiguousarray(canvas_rgba, dtype=np.float64)
        out = np.empty((n, H, W, 4), dtype=np.uint8)
        check(
            load().osmt_composite(
                self._h, planes.ctypes.data_as(C.POINTER(C.c_double)), cv.ctypes.data_as(C.POINTER(C.c_double)), n, L,
                W, H, out.ctypes.data_as(C.POINTER(C.c_uint8)),
            )
        )
        return out

    def composite(self, planes, canvas_rgba, out=None, stream=None):
        """osmt_composite_device on a cuda float64 tensor [n, L, H, W, 4]."""
        torch = _torch()
        assert planes.is_cuda and planes.dtype == torch.float64 and planes.is_contiguous()
        n, L, H, W, four = planes.shape
        assert four == 4
        if out is None:
            out = torch.empty((n, H, W, 4), dtype=torch.uint8, device=planes.device)
        cv = (C.c_double * 4)(*[float(v) for v in canvas_rgba])
        check(
            load().osmt_composite_device(
                self._h, C.c_void_p(planes.data_ptr()), cv, n, L, W, H, C.c_void_p(out.data_ptr()), _stream_ptr(stream)
            )
        )
        return out


def encode_png(rgba, level=-1):
    """osmt_encode_png: RGB8 PNG bytes of one RGBA8 tile [H, W, 4] (png_writer.rs:4-21)."""
    img = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w, four = img.shape
    assert four == 4
    L = load()
    cap = L.osmt_png_bound(w, h)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t()
    check(L.osmt_encode_png(img.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, w * 4, level,
                            out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
    return out[: n.value].tobytes()
