"""Label lists: the flat form of what Drawer::draw_labels walks (drawer.rs:221-262).

One osmt_label == one Labeler::label_entity call (labeler.rs:16-38): an optional icon blit and an
optional text, the text given as the Rasterizer::draw_line calls (font/rasterizer.rs:27-88) the
reference's glyph walk makes.  Curves are flattened HERE (host side) exactly like
Rasterizer::draw_quad (font/rasterizer.rs:90-113) with libm's hypot, which is what f64::hypot is.

The second form, glyph runs (GlyphTable + GlyphLabelList), names glyph instances with the transform
TextPlacer::place passes to Glyph::rasterize; the library expands them on the GPU.
GlyphLabelList.to_label_list() is the same expansion on the host, with glyph_segments below.
"""
import math
import ctypes as C
import ctypes.util

import numpy as np

from . import abi

LABEL_DTYPE = np.dtype(
    [
        ("has_icon", "u1"),
        ("has_text", "u1"),
        ("text_color", "u1", (3,)),
        ("_pad", "u1", (3,)),
        ("image_id", "u4"),
        ("seg_off", "u4"),
        ("n_segs", "u4"),
        ("_reserved", "u4"),
        ("icon_center_x", "f8"),
        ("icon_center_y", "f8"),
    ]
)
assert LABEL_DTYPE.itemsize == 40

# osmt_label_request / osmt_label_position (label anchors, Context.label_positions)
LABEL_REQUEST_DTYPE = np.dtype([("ring_off", "<u4"), ("n_rings", "<u4"), ("scale", "<f8")])
LABEL_POSITION_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("status", "<u4"), ("_pad", "<u4")])
LABEL_TILE_REQUEST_DTYPE = np.dtype([("entity", "<u4"), ("tile", "<u4")])  # osmt_label_tile_request (Context.label_positions_tiles)
assert LABEL_REQUEST_DTYPE.itemsize == C.sizeof(abi.LabelRequest) == 16
assert LABEL_TILE_REQUEST_DTYPE.itemsize == C.sizeof(abi.LabelTileRequest) == 8
AREA_ANCHOR_DTYPE = np.dtype([("tile", "<u4"), ("entity", "<u4"), ("x", "<f8"), ("y", "<f8"), ("status", "<u4"), ("_pad", "<u4")])  # osmt_area_anchor
assert AREA_ANCHOR_DTYPE.itemsize == C.sizeof(abi.AreaAnchor) == 32
assert LABEL_POSITION_DTYPE.itemsize == C.sizeof(abi.LabelPosition) == 24

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = C.c_double
_libm.hypot.argtypes = [C.c_double, C.c_double]


def flatten_quad(x0, y0, x1, y1, x2, y2, out):
    """Rasterizer::draw_quad (font/rasterizer.rs:90-113): appends the draw_line calls to `out`."""
    d01 = _libm.hypot(abs(x0 - x1), abs(y0 - y1))
    d12 = _libm.hypot(abs(x1 - x2), abs(y1 - y2))
    d02 = _libm.hypot(abs(x0 - x2), abs(y0 - y2))
    if (d01 + d12) <= 1.0001 * d02:
        out.append((x0, y0, x2, y2))
        return
    m01x, m01y = (x0 + x1) / 2.0, (y0 + y1) / 2.0
    m12x, m12y = (x1 + x2) / 2.0, (y1 + y2) / 2.0
    mx, my = (m01x + m12x) / 2.0, (m01y + m12y) / 2.0
    flatten_quad(x0, y0, m01x, m01y, mx, my, out)
    flatten_quad(mx, my, m12x, m12y, x2, y2, out)


def glyph_segments(vertices, scale, tr, out):
    """Glyph::rasterize (font/text_placer.rs:232-259).  vertices: stb_truetype-style list of
    (type, x, y, cx, cy) in font units with type 'M' (MoveTo), 'L' (LineTo), 'Q' (CurveTo)."""
    frm = (0.0, 0.0)
    for t, x, y, cx, cy in vertices:
        to = (float(x) * scale, float(y) * scale)
        if t == "L":
            p1, p0 = tr(frm), tr(to)
            out.append((p0[0], p0[1], p1[0], p1[1]))
        elif t == "Q":
            mid = (float(cx) * scale, float(cy) * scale)
            p2, p1, p0 = tr(frm), tr(mid), tr(to)
            flatten_quad(p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], out)
        frm = to
    return out


class LabelList:
    """Labels of a batch of tiles (osmt_label_batch) backed by numpy arrays."""

    def __init__(self, labels, job_label_off, segs):
        self.labels = np.ascontiguousarray(labels, dtype=LABEL_DTYPE)
        self.job_label_off = np.ascontiguousarray(job_label_off, dtype=np.uint32)
        self.segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)

    @property
    def n_jobs(self):
        return len(self.job_label_off) - 1

    def as_batch(self):
        b = abi.LabelBatch()
        b.labels = self.labels.ctypes.data_as(C.POINTER(abi.Label))
        b.n_labels = len(self.labels)
        b.job_label_off = self.job_label_off.ctypes.data_as(C.POINTER(C.c_uint32))
        b.segs = self.segs.ctypes.data_as(C.POINTER(C.c_double)) if len(self.segs) else None
        b.n_segs = len(self.segs)
        return b

    def algorithmic_bytes(self):
        """bytes the label pass must read at least once: 40 per label + 32 per draw_line call."""
        return 40 * len(self.labels) + 32 * len(self.segs)

    def subset(self, idx):
        return concat_labels([self._single(i) for i in idx])

    def _single(self, i):
        a, b = int(self.job_label_off[i]), int(self.job_label_off[i + 1])
        lab = self.labels[a:b].copy()
        segs = []
        cur = 0
        for l in lab:
            n = int(l["n_segs"])
            segs.append(self.segs[int(l["seg_off"]) : int(l["seg_off"]) + n])
            l["seg_off"] = cur if n else 0
            cur += n
        segs = np.concatenate(segs) if segs else np.zeros((0, 4))
        return LabelList(lab, [0, len(lab)], segs)


def concat_labels(lists):
    labels, offs, segs = [], [0], []
    seg_cur = 0
    for ll in lists:
        lab = ll.labels.copy()
        lab["seg_off"][lab["n_segs"] > 0] += seg_cur
        labels.append(lab)
        segs.append(ll.segs)
        seg_cur += len(ll.segs)
        base = offs[-1]
        offs.extend((base + ll.job_label_off[1:].astype(np.int64)).tolist())
    return LabelList(
        np.concatenate(labels) if labels else np.zeros(0, LABEL_DTYPE),
        offs,
        np.concatenate(segs) if segs else np.zeros((0, 4)),
    )


class TileLabels:
    """Builder for the labels of ONE tile, in draw order."""

    def __init__(self):
        self._labels = []
        self._segs = []

    def label(self, icon=None, text=None):
        """icon: (image_id, center_x, center_y) or None; text: (color_rgb, segs[n][4]) or None.
        text with zero segments is a text that drew nothing (still `has_text`)."""
        l = np.zeros((), LABEL_DTYPE)
        if icon is not None:
            l["has_icon"] = 1
            l["image_id"] = icon[0]
            l["icon_center_x"], l["icon_center_y"] = float(icon[1]), float(icon[2])
        if text is not None:
            color, segs = text
            segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
            l["has_text"] = 1
            l["text_color"] = color
            l["seg_off"] = sum(len(s) for s in self._segs) if len(segs) else 0
            l["n_segs"] = len(segs)
            self._segs.append(segs)
        self._labels.append(l)
        return self

    def build(self):
        labels = np.array(self._labels, dtype=LABEL_DTYPE) if self._labels else np.zeros(0, LABEL_DTYPE)
        segs = np.concatenate(self._segs) if self._segs else np.zeros((0, 4))
        return LabelList(labels, [0, len(labels)], segs)


# ---- synthetic glyphs (TrueType-like quadratic outlines in a 1000-unit em) ----------------------
def _ring(cx, cy, rx, ry, ccw):
    """8 quadratic arcs approximating an ellipse, as (type, x, y, cx, cy) stb-style vertices."""
    k = 1.0 / np.cos(np.pi / 8)
    pts = []
    for i in range(9):
        a = 2 * np.pi * (i % 8) / 8 * (1 if ccw else -1)
        pts.append((cx + rx * np.cos(a), cy + ry * np.sin(a)))
    v = [("M", int(pts[0][0]), int(pts[0][1]), 0, 0)]
    for i in range(8):
        a = (2 * np.pi * (i + 0.5) / 8) * (1 if ccw else -1)
        c = (cx + k * rx * np.cos(a), cy + k * ry * np.sin(a))
        v.append(("Q", int(pts[i + 1][0]), int(pts[i + 1][1]), int(c[0]), int(c[1])))
    return v


def _poly(points):
    v = [("M", points[0][0], points[0][1], 0, 0)]
    for p in points[1:] + [points[0]]:
        v.append(("L", p[0], p[1], 0, 0))
    return v


SYNTH_GLYPHS = [
    # (advance, vertices)
    (620, _ring(310, 360, 250, 370, True) + _ring(310, 360, 150, 270, False)),  # "o"
    (280, _poly([(90, 0), (190, 0), (190, 720), (90, 720)])),  # "l"
    (560, _poly([(80, 0), (500, 0), (500, 90), (180, 90), (180, 720), (80, 720)])),  # "L"
    (600, _poly([(40, 0), (140, 0), (300, 560), (460, 0), (560, 0), (350, 720), (250, 720)])
     + _poly([(215, 200), (385, 200), (360, 290), (240, 290)][::-1])),  # "A"-like with a hole
    (260, []),  # space
]


def synth_text(rng, x, y, font_px, n_glyphs, angle=0.0):
    """Segments of a run of synthetic glyphs starting at (x, y) = left end of the baseline, rotated by `angle`."""
    scale = font_px / 1000.0
    out = []
    s, c = np.sin(angle), np.cos(angle)
    pen = 0.0
    for _ in range(n_glyphs):
        adv, verts = SYNTH_GLYPHS[int(rng.integers(0, len(SYNTH_GLYPHS)))]
        px = pen

        def tr(p, px=px):
            gx, gy = px + p[0], p[1]
            return (x + gx * c + gy * s, y + gx * s - gy * c)

        glyph_segments(verts, scale, tr, out)
        pen += adv * scale
    return np.array(out, dtype=np.float64).reshape(-1, 4), pen


def make_labels(n_tiles, labels_per_tile=24, scale=1, seed=7, n_images=0, image_sizes=None, text_frac=0.85,
                icon_frac=0.4, line_frac=0.3):
    """Synthetic label workload: per tile `labels_per_tile` labels scattered over the 3x3-tile label area
    (labels_bb, tile_pixels.rs:67-72) so that collisions happen both inside and outside the tile."""
    rng = np.random.default_rng(seed)
    W = 256 * scale
    out = []
    for _ in range(n_tiles):
        tl = TileLabels()
        for _ in range(labels_per_tile):
            cx = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 2)) * 0.5
            cy = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 4)) * 0.25
            icon = None
            y_off = 0.0
            if n_images and rng.random() < icon_frac:
                img = int(rng.integers(0, n_images))
                icon = (img, cx, cy)
                y_off = float(image_sizes[img][0] // 2)
            text = None
            if rng.random() < text_frac:
                font_px = float(rng.choice([9.0, 10.0, 11.0, 12.0, 14.0])) * scale
                n_gl = int(rng.integers(3, 13))
                color = tuple(int(v) for v in rng.integers(0, 256, size=3))
                if rng.random() < line_frac:
                    ang = float(rng.uniform(-1.2, 1.2))
                    segs, _ = synth_text(rng, cx, cy, font_px, n_gl, ang)
                else:
                    probe, width = synth_text(np.random.default_rng(0), 0.0, 0.0, font_px, 0)
                    st = rng.bit_generator.state
                    _, width = synth_text(rng, 0.0, 0.0, font_px, n_gl)
                    rng.bit_generator.state = st
                    segs, _ = synth_text(rng, cx - width / 2.0, cy + y_off + 0.8 * font_px, font_px, n_gl)
                text = (color, segs)
            tl.label(icon=icon, text=text)
        out.append(tl.build())
    return concat_labels(out)


# ---- glyph runs (osmt_glyph_label_batch) ---------------------------------------------------------
GLYPH_VERTEX_DTYPE = np.dtype([("x", "i2"), ("y", "i2"), ("cx", "i2"), ("cy", "i2"), ("type", "u1"), ("_pad", "u1")])
GLYPH_INSTANCE_DTYPE = np.dtype([("glyph_id", "u4"), ("form", "u4"), ("scale", "f8"), ("p", "f8", (6,))])
assert GLYPH_VERTEX_DTYPE.itemsize == 10 and GLYPH_INSTANCE_DTYPE.itemsize == 64
_VERTEX_TYPE = {"M": abi.GLYPH_MOVE_TO, "L": abi.GLYPH_LINE_TO, "Q": abi.GLYPH_CURVE_TO}


def center_tr(x_offset, baseline):
    """TextPlacer::place, TextPosition::Center (font/text_placer.rs:150-153)."""
    return lambda p: (x_offset + p[0], baseline - p[1])


def line_tr(glyph_center_x, glyph_center_y, angle_sin, angle_cos, way_x, way_y):
    """TextPlacer::place, TextPosition::Line (font/text_placer.rs:87-101); (angle_sin, angle_cos) = (-angle).sin_cos()."""

    def tr(p):
        translated_x = p[0] - glyph_center_x
        translated_y = p[1] - glyph_center_y
        rotated_x = translated_x * angle_cos - translated_y * angle_sin
        rotated_y = translated_y * angle_cos + translated_x * angle_sin
        return (way_x + rotated_x, way_y - rotated_y)

    return tr


class GlyphTable:
    """Glyph outlines as stb-style vertex lists [(type, x, y, cx, cy)] with type 'M' / 'L' / 'Q' in font units (an
    empty list is a glyph without shape).  Context.register_glyphs uploads them and sets `first_id`: glyph i of the
    table has id first_id + i."""

    def __init__(self, outlines):
        self.outlines = [list(o) if o else [] for o in outlines]
        self.first_id = 0

    def __len__(self):
        return len(self.outlines)

    def outline(self, glyph_id):
        return self.outlines[glyph_id - self.first_id]

    def arrays(self):
        """(vertices GLYPH_VERTEX_DTYPE, vertex_off uint32 [n + 1]) as osmt_register_glyphs takes them."""
        voff = np.zeros(len(self.outlines) + 1, dtype=np.uint32)
        verts = np.zeros(sum(len(o) for o in self.outlines), dtype=GLYPH_VERTEX_DTYPE)
        k = 0
        for i, o in enumerate(self.outlines):
            for t, x, y, cx, cy in o:
                verts[k] = (x, y, cx, cy, _VERTEX_TYPE[t], 0)
                k += 1
            voff[i + 1] = k
        return verts, voff


class GlyphLabelList:
    """Labels of a batch with glyph-run text (osmt_glyph_label_batch): `labels` are osmt_label records whose
    seg_off / n_segs name a range of `glyphs` (GLYPH_INSTANCE_DTYPE) instead of draw_line calls."""

    def __init__(self, labels, job_label_off, glyphs):
        self.labels = np.ascontiguousarray(labels, dtype=LABEL_DTYPE)
        self.job_label_off = np.ascontiguousarray(job_label_off, dtype=np.uint32)
        self.glyphs = np.ascontiguousarray(glyphs, dtype=GLYPH_INSTANCE_DTYPE)

    @property
    def n_jobs(self):
        return len(self.job_label_off) - 1

    def as_batch(self):
        b = abi.GlyphLabelBatch()
        b.labels = self.labels.ctypes.data_as(C.POINTER(abi.Label))
        b.n_labels = len(self.labels)
        b.job_label_off = self.job_label_off.ctypes.data_as(C.POINTER(C.c_uint32))
        b.glyphs = self.glyphs.ctypes.data_as(C.POINTER(abi.GlyphInstance)) if len(self.glyphs) else None
        b.n_glyphs = len(self.glyphs)
        return b

    def input_bytes(self):
        """bytes handed to the library: 40 per label + 64 per glyph instance + the job offsets."""
        return 40 * len(self.labels) + 64 * len(self.glyphs) + 4 * len(self.job_label_off)

    def subset(self, idx):
        """The labels of tiles idx (in that order) as a GlyphLabelList of their own, instances re-packed."""
        parts = []
        for i in idx:
            a, b = int(self.job_label_off[i]), int(self.job_label_off[i + 1])
            lab = self.labels[a:b].copy()
            gs, cur = [], 0
            for l in lab:
                n = int(l["n_segs"])
                gs.append(self.glyphs[int(l["seg_off"]) : int(l["seg_off"]) + n])
                l["seg_off"] = cur if n else 0
                cur += n
            parts.append(GlyphLabelList(lab, [0, len(lab)], np.concatenate(gs) if gs else np.zeros(0, GLYPH_INSTANCE_DTYPE)))
        return concat_glyph_labels(parts)

    def to_label_list(self, table):
        """The host expansion: every label's draw_line calls in label, glyph, vertex order (Glyph::rasterize with
        glyph_segments and the instance's `tr`), as the segment-form LabelList the GPU expansion must equal."""
        labels = self.labels.copy()
        segs = []
        n = 0
        for l in labels:
            if not l["has_text"]:
                l["seg_off"], l["n_segs"] = 0, 0
                continue
            out = []
            for g in self.glyphs[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])]:
                p = [float(v) for v in g["p"]]
                tr = center_tr(p[0], p[1]) if int(g["form"]) == abi.GLYPH_CENTER else line_tr(*p)
                glyph_segments(table.outline(int(g["glyph_id"])), float(g["scale"]), tr, out)
            l["seg_off"] = n if out else 0
            l["n_segs"] = len(out)
            n += len(out)
            segs.extend(out)
        return LabelList(labels, self.job_label_off.copy(), np.array(segs, dtype=np.float64).reshape(-1, 4))


def concat_glyph_labels(lists):
    labels, offs, glyphs = [], [0], []
    cur = 0
    for gl in lists:
        lab = gl.labels.copy()
        lab["seg_off"][lab["n_segs"] > 0] += cur
        labels.append(lab)
        glyphs.append(gl.glyphs)
        cur += len(gl.glyphs)
        offs.extend((offs[-1] + gl.job_label_off[1:].astype(np.int64)).tolist())
    return GlyphLabelList(np.concatenate(labels) if labels else np.zeros(0, LABEL_DTYPE), offs,
                          np.concatenate(glyphs) if glyphs else np.zeros(0, GLYPH_INSTANCE_DTYPE))


def synth_glyph_table():
    """SYNTH_GLYPHS as a GlyphTable (the last one, the space, has no shape)."""
    return GlyphTable([v for _, v in SYNTH_GLYPHS])


# vertical metrics of the synthetic 1000-unit em (ascent, descent, line_gap) and TextPlacer's MAX_TEXT_WIDTH-free one-row layout
_SYNTH_ASCENT, _SYNTH_DESCENT, _SYNTH_GAP = 800.0, -200.0, 0.0


def _instance(glyph_id, form, scale, p):
    g = np.zeros((), GLYPH_INSTANCE_DTYPE)
    g["glyph_id"], g["form"], g["scale"] = glyph_id, form, scale
    g["p"][: len(p)] = p
    return g


def synth_glyph_run(rng, table, cx, cy, font_px, n_glyphs, y_offset=0.0, angle=None):
    """Glyph instances of one synthetic text laid out as TextPlacer::place does: TextPosition::Center around (cx, cy)
    (one row; y_offset > 0 puts it below an icon, text_placer.rs:130-139), or, with `angle`, TextPosition::Line along
    a straight way through (cx, cy) at that angle (compute_way_position on one segment)."""
    scale = font_px / 1000.0
    ids = [int(rng.integers(0, len(SYNTH_GLYPHS))) for _ in range(n_glyphs)]
    widths = [float(SYNTH_GLYPHS[i][0]) * scale for i in ids]
    total = 0.0
    for w in widths:
        total += w
    asc, desc, gap = _SYNTH_ASCENT * scale, _SYNTH_DESCENT * scale, _SYNTH_GAP * scale
    out = []
    if angle is None:
        row_height = asc - desc + gap
        cur_y = cy + y_offset if y_offset > 0 else cy - row_height * 1.0 / 2.0
        cur_x = cx - total / 2.0
        for i, w in zip(ids, widths):
            out.append(_instance(table.first_id + i, abi.GLYPH_CENTER, scale, [cur_x, cur_y + asc]))
            cur_x += w
    else:
        s, c = math.sin(-angle), math.cos(-angle)
        ux, uy = math.cos(angle), math.sin(angle)
        length = total + float(rng.integers(0, 40))
        sx, sy = cx - ux * length / 2.0, cy - uy * length / 2.0
        cur = (length - total) / 2.0
        gcy = (desc + asc) / 2.0
        for i, w in zip(ids, widths):
            gcx = w / 2.0
            d = cur + gcx
            out.append(_instance(table.first_id + i, abi.GLYPH_LINE, scale, [gcx, gcy, s, c, sx + ux * d, sy + uy * d]))
            cur += w
    return np.array(out, dtype=GLYPH_INSTANCE_DTYPE) if out else np.zeros(0, GLYPH_INSTANCE_DTYPE)


def make_glyph_labels(n_tiles, table, labels_per_tile=24, scale=1, seed=7, n_images=0, image_sizes=None, text_frac=0.85,
                      icon_frac=0.4, line_frac=0.3, empty_frac=0.03):
    """The label workload of make_labels as glyph runs: center- and line-form texts over SYNTH_GLYPHS (spaces = empty
    glyphs included) scattered over the 3x3-tile label area so that labels collide inside and outside the tile, icons
    (n_images > 0), labels without text and texts of zero glyphs (empty_frac)."""
    rng = np.random.default_rng(seed)
    W = 256 * scale
    lists = []
    for _ in range(n_tiles):
        labs, glyphs = [], []
        for _ in range(labels_per_tile):
            l = np.zeros((), LABEL_DTYPE)
            cx = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 2)) * 0.5
            cy = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 4)) * 0.25
            y_off = 0.0
            if n_images and rng.random() < icon_frac:
                img = int(rng.integers(0, n_images))
                l["has_icon"], l["image_id"] = 1, img
                l["icon_center_x"], l["icon_center_y"] = cx, cy
                y_off = float(image_sizes[img][0] // 2)
            if rng.random() < text_frac:
                l["has_text"] = 1
                l["text_color"] = [int(v) for v in rng.integers(0, 256, size=3)]
                font_px = float(rng.choice([9.0, 10.0, 11.0, 12.0, 14.0])) * scale
                n_gl = 0 if rng.random() < empty_frac else int(rng.integers(3, 13))
                angle = float(rng.uniform(-1.2, 1.2)) if rng.random() < line_frac else None
                run = synth_glyph_run(rng, table, cx, cy, font_px, n_gl, y_offset=y_off, angle=angle)
                l["seg_off"] = sum(len(g) for g in glyphs) if len(run) else 0
                l["n_segs"] = len(run)
                glyphs.append(run)
            labs.append(l)
        lists.append(GlyphLabelList(np.array(labs, dtype=LABEL_DTYPE), [0, len(labs)],
                                    np.concatenate(glyphs) if glyphs else np.zeros(0, GLYPH_INSTANCE_DTYPE)))
    return concat_glyph_labels(lists)


# ---- text runs (osmt_text_label_batch) -----------------------------------------------------------
TEXT_GLYPH_DTYPE = np.dtype([("glyph_id", "<u4"), ("advance", "<i4"), ("kern", "<i4"), ("flags", "<u4")])
TEXT_RUN_DTYPE = np.dtype([("position", "<u4"), ("y_offset", "<u4"), ("pt_off", "<u4"), ("n_pts", "<u4"), ("scale", "<f8"),
                           ("ascent", "<i4"), ("descent", "<i4"), ("line_gap", "<i4"), ("_pad", "<i4"),
                           ("center_x", "<f8"), ("center_y", "<f8"), ("_reserved", "<f8")])
assert TEXT_GLYPH_DTYPE.itemsize == C.sizeof(abi.TextGlyph) == 16
assert TEXT_RUN_DTYPE.itemsize == C.sizeof(abi.TextRun) == 64


def way_sincos(points):
    """(-get_angle(points, e)).sin_cos() of every edge e -> e + 1 of a way (text_placer.rs:93, 256-262) with this
    process's libm, as osmt_text_label_batch.way_sincos wants it: float64 [n, 2], the last row unused (zero)."""
    out = np.zeros((len(points), 2), dtype=np.float64)
    for e in range(len(points) - 1):
        angle = math.atan2(float(int(points[e + 1][1]) - int(points[e][1])), float(int(points[e + 1][0]) - int(points[e][0])))
        out[e] = (math.sin(-angle), math.cos(-angle))
    return out


def walking_order(points):
    """The reversal of text_placer.rs:65-67: a way is walked from its end when points[0].x > last.x."""
    points = np.asarray(points, dtype=np.int32).reshape(-1, 2)
    if len(points) >= 2 and points[0][0] > points[-1][0]:
        points = points[::-1]
    return np.ascontiguousarray(points)


class TextLabelList:
    """Labels of a batch with text-run text (osmt_text_label_batch): `labels` are osmt_label records whose seg_off /
    n_segs name a range of `glyphs` (TEXT_GLYPH_DTYPE, the chars of the text), `runs` (TEXT_RUN_DTYPE) holds one
    TextPlacer::place call per label, `way_pts` (int32 [n, 2], in walking order) and `way_sincos` (float64 [n, 2]) the
    ways of the line-form runs."""

    def __init__(self, labels, job_label_off, runs, glyphs, way_pts, way_sincos):
        self.labels = np.ascontiguousarray(labels, dtype=LABEL_DTYPE)
        self.job_label_off = np.ascontiguousarray(job_label_off, dtype=np.uint32)
        self.runs = np.ascontiguousarray(runs, dtype=TEXT_RUN_DTYPE)
        self.glyphs = np.ascontiguousarray(glyphs, dtype=TEXT_GLYPH_DTYPE)
        self.way_pts = np.ascontiguousarray(way_pts, dtype=np.int32).reshape(-1, 2)
        self.way_sincos = np.ascontiguousarray(way_sincos, dtype=np.float64).reshape(-1, 2)
        assert len(self.runs) == len(self.labels) and len(self.way_pts) == len(self.way_sincos)

    @property
    def n_jobs(self):
        return len(self.job_label_off) - 1

    def as_batch(self):
        b = abi.TextLabelBatch()
        b.labels = self.labels.ctypes.data_as(C.POINTER(abi.Label))
        b.n_labels = len(self.labels)
        b.job_label_off = self.job_label_off.ctypes.data_as(C.POINTER(C.c_uint32))
        b.runs = self.runs.ctypes.data_as(C.POINTER(abi.TextRun))
        b.glyphs = self.glyphs.ctypes.data_as(C.POINTER(abi.TextGlyph)) if len(self.glyphs) else None
        b.n_glyphs = len(self.glyphs)
        b.way_pts = self.way_pts.ctypes.data_as(C.POINTER(C.c_int32)) if len(self.way_pts) else None
        b.way_sincos = self.way_sincos.ctypes.data_as(C.POINTER(C.c_double)) if len(self.way_pts) else None
        b.n_way_pts = len(self.way_pts)
        return b

    def input_bytes(self):
        """bytes handed to the library: 40 + 64 per label, 16 per glyph, 24 per way point + the job offsets."""
        return 104 * len(self.labels) + 16 * len(self.glyphs) + 24 * len(self.way_pts) + 4 * len(self.job_label_off)

    def subset(self, idx):
        """The labels of tiles idx (in that order) as a TextLabelList of their own, glyphs and ways re-packed."""
        parts = []
        for i in idx:
            a, b = int(self.job_label_off[i]), int(self.job_label_off[i + 1])
            lab, runs = self.labels[a:b].copy(), self.runs[a:b].copy()
            gs, ps, ss, cur, pcur = [], [], [], 0, 0
            for l, r in zip(lab, runs):
                n = int(l["n_segs"])
                gs.append(self.glyphs[int(l["seg_off"]) : int(l["seg_off"]) + n])
                l["seg_off"] = cur if n else 0
                cur += n
                m = int(r["n_pts"]) if int(r["position"]) == abi.TEXT_LINE else 0
                ps.append(self.way_pts[int(r["pt_off"]) : int(r["pt_off"]) + m])
                ss.append(self.way_sincos[int(r["pt_off"]) : int(r["pt_off"]) + m])
                r["pt_off"] = pcur if m else 0
                pcur += m
            parts.append(TextLabelList(lab, [0, len(lab)], runs, np.concatenate(gs) if gs else np.zeros(0, TEXT_GLYPH_DTYPE),
                                       np.concatenate(ps) if ps else np.zeros((0, 2), np.int32),
                                       np.concatenate(ss) if ss else np.zeros((0, 2))))
        return concat_text_labels(parts)


def concat_text_labels(lists):
    labels, offs, runs, glyphs, pts, scs = [], [0], [], [], [], []
    cur = pcur = 0
    for tl in lists:
        lab, run = tl.labels.copy(), tl.runs.copy()
        lab["seg_off"][lab["n_segs"] > 0] += cur
        run["pt_off"][(run["position"] == abi.TEXT_LINE) & (run["n_pts"] > 0)] += pcur
        labels.append(lab)
        runs.append(run)
        glyphs.append(tl.glyphs)
        pts.append(tl.way_pts)
        scs.append(tl.way_sincos)
        cur += len(tl.glyphs)
        pcur += len(tl.way_pts)
        offs.extend((offs[-1] + tl.job_label_off[1:].astype(np.int64)).tolist())
    return TextLabelList(np.concatenate(labels) if labels else np.zeros(0, LABEL_DTYPE), offs,
                         np.concatenate(runs) if runs else np.zeros(0, TEXT_RUN_DTYPE),
                         np.concatenate(glyphs) if glyphs else np.zeros(0, TEXT_GLYPH_DTYPE),
                         np.concatenate(pts) if pts else np.zeros((0, 2), np.int32), np.concatenate(scs) if scs else np.zeros((0, 2)))


def synth_text_glyphs(rng, table, n_words):
    """A synthetic text of n_words words over SYNTH_GLYPHS, single spaces (the shapeless last glyph, whitespace)
    between them; every glyph but the first gets a kern, non-zero for about a third of the pairs."""
    space = len(SYNTH_GLYPHS) - 1
    ids = []
    for w in range(n_words):
        if w:
            ids.append(space)
        ids.extend(int(rng.integers(0, space)) for _ in range(int(rng.integers(1, 6))))
    g = np.zeros(len(ids), TEXT_GLYPH_DTYPE)
    for k, i in enumerate(ids):
        kern = int(rng.integers(-60, 41)) if k and rng.random() < 0.35 else 0
        g[k] = (table.first_id + i, SYNTH_GLYPHS[i][0], kern, 1 if i == space else 0)
    return g


def synth_way(rng, cx, cy, n_pts, step):
    """A way of n_pts integer points through about (cx, cy): a heading that bends at every point, steps of about `step`
    pixels, now and then a repeated point (a zero-length edge)."""
    heading = float(rng.uniform(-math.pi, math.pi))
    x, y = float(cx), float(cy)
    pts = [(int(x), int(y))]
    for _ in range(n_pts - 1):
        if rng.random() < 0.05:
            pts.append(pts[-1])
            continue
        heading += float(rng.uniform(-0.6, 0.6))
        d = float(rng.uniform(0.3, 1.7)) * step
        x, y = x + d * math.cos(heading), y + d * math.sin(heading)
        pts.append((int(x), int(y)))
    pts = np.array(pts, dtype=np.int32).reshape(-1, 2)
    pts += np.array([int(cx), int(cy)], dtype=np.int32) - (pts[0] + pts[-1]) // 2  # about centred on (cx, cy)
    return pts


def make_text_labels(n_tiles, table, labels_per_tile=24, scale=1, seed=7, n_images=0, image_sizes=None, text_frac=0.85,
                     icon_frac=0.4, line_frac=0.3, empty_frac=0.03, f32_scale=False, _font_px=None):
    """The label workload of make_glyph_labels as text runs: what TextPlacer::place is GIVEN instead of what it
    computes.  Multi-word texts over SYNTH_GLYPHS with kerns (the centred ones wrap into rows at MAX_TEXT_WIDTH), ways
    of 2..40 points with bends (some too short for their text: place() skips those; now and then a way of one point
    or none), icons whose half height becomes y_offset, labels without text and texts of zero glyphs (empty_frac).
    f32_scale: the run's scale is the f32 quotient scale_for_pixel_height computes, widened (what the string form derives
    from a font size) instead of the f64 quotient; nothing else changes.  _font_px: a list that receives the font size
    of every label (0.0 without text), for make_string_labels."""
    rng = np.random.default_rng(seed)
    W = 256 * scale
    lists = []
    for _ in range(n_tiles):
        labs, runs, glyphs, pts = [], [], [], []
        n_gl = n_pt = 0
        for _ in range(labels_per_tile):
            l, r = np.zeros((), LABEL_DTYPE), np.zeros((), TEXT_RUN_DTYPE)
            cx = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 2)) * 0.5
            cy = float(rng.integers(-W // 2, W + W // 2)) + float(rng.integers(0, 4)) * 0.25
            y_off, font_px = 0, 0.0
            if n_images and rng.random() < icon_frac:
                img = int(rng.integers(0, n_images))
                l["has_icon"], l["image_id"] = 1, img
                l["icon_center_x"], l["icon_center_y"] = cx, cy
                y_off = int(image_sizes[img][0] // 2)
            if rng.random() < text_frac:
                l["has_text"] = 1
                l["text_color"] = [int(v) for v in rng.integers(0, 256, size=3)]
                font_px = float(rng.choice([9.0, 10.0, 11.0, 12.0, 14.0])) * scale
                r["scale"] = float(np.float32(font_px) / np.float32(1000.0)) if f32_scale else font_px / 1000.0
                r["ascent"], r["descent"], r["line_gap"] = int(_SYNTH_ASCENT), int(_SYNTH_DESCENT), int(_SYNTH_GAP)
                text = np.zeros(0, TEXT_GLYPH_DTYPE) if rng.random() < empty_frac else synth_text_glyphs(rng, table, int(rng.integers(1, 5)))
                if rng.random() < line_frac:
                    r["position"] = abi.TEXT_LINE
                    u = rng.random()
                    n = 0 if u < 0.02 else 1 if u < 0.04 else int(rng.integers(2, 41))
                    way = walking_order(synth_way(rng, cx, cy, n, 6.0 * scale)) if n else np.zeros((0, 2), np.int32)
                    r["pt_off"], r["n_pts"] = (n_pt if n else 0), n
                    pts.append(way)
                    n_pt += n
                else:
                    r["position"] = abi.TEXT_CENTER
                    r["y_offset"] = y_off
                    r["center_x"], r["center_y"] = cx, cy
                l["seg_off"], l["n_segs"] = (n_gl if len(text) else 0), len(text)
                glyphs.append(text)
                n_gl += len(text)
            if _font_px is not None:
                _font_px.append(font_px if l["has_text"] else 0.0)
            labs.append(l)
            runs.append(r)
        way_pts = np.concatenate(pts) if pts else np.zeros((0, 2), np.int32)
        sincos = np.concatenate([way_sincos(p) for p in pts]) if pts else np.zeros((0, 2))
        lists.append(TextLabelList(np.array(labs, dtype=LABEL_DTYPE), [0, len(labs)], np.array(runs, dtype=TEXT_RUN_DTYPE),
                                   np.concatenate(glyphs) if glyphs else np.zeros(0, TEXT_GLYPH_DTYPE), way_pts, sincos))
    return concat_text_labels(lists)


# ---- string labels (osmt_string_label_batch) -------------------------------------------------------
STRING_RUN_DTYPE = np.dtype([("position", "<u4"), ("y_offset", "<u4"), ("pt_off", "<u4"), ("n_pts", "<u4"), ("font_id", "<u4"),
                             ("_pad", "<u4"), ("font_size", "<f8"), ("center_x", "<f8"), ("center_y", "<f8"), ("_reserved", "<f8", (2,))])
CMAP_DTYPE = np.dtype([("code_point", "<u4"), ("glyph", "<u4")])
KERN_DTYPE = np.dtype([("left", "<u4"), ("right", "<u4"), ("value", "<i4")])
assert STRING_RUN_DTYPE.itemsize == C.sizeof(abi.StringRun) == 64
assert CMAP_DTYPE.itemsize == C.sizeof(abi.CmapEntry) == 8 and KERN_DTYPE.itemsize == C.sizeof(abi.KernPair) == 12

# char::is_whitespace of Rust: the Unicode White_Space set (not str.isspace: U+001C-001F are not in it)
WHITE_SPACE = frozenset(list(range(0x09, 0x0E)) + [0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])


class FontTable:
    """The flat tables of one font as osmt_register_font takes them (osmt_font_desc): `cmap` [(code point, glyph)] rising
    in code point, `advance` and `outline_id` per glyph index (outline ids as Context.register_glyphs assigned them),
    `kern` [(left, right, value)] rising in (left, right), and the v-metrics.  Context.register_font uploads it and sets
    `font_id`."""

    def __init__(self, cmap, advance, outline_id, kern=(), ascent=800, descent=-200, line_gap=0):
        def records(rows, dtype):
            if isinstance(rows, np.ndarray) and rows.dtype == dtype:
                return np.ascontiguousarray(rows)
            return np.array([tuple(int(v) for v in r) for r in rows], dtype=dtype) if len(rows) else np.zeros(0, dtype)

        self.cmap = records(cmap, CMAP_DTYPE)
        self.kern = records(kern, KERN_DTYPE)
        self.advance = np.ascontiguousarray(advance, dtype=np.int32)
        self.outline_id = np.ascontiguousarray(outline_id, dtype=np.uint32)
        assert len(self.advance) == len(self.outline_id)
        self.ascent, self.descent, self.line_gap = int(ascent), int(descent), int(line_gap)
        self.font_id = 0
        self._glyph_of = self._kern_of = None

    def as_desc(self):
        """(abi.FontDesc, the arrays it points into)."""
        d = abi.FontDesc()
        d.cmap = self.cmap.ctypes.data_as(C.POINTER(abi.CmapEntry)) if len(self.cmap) else None
        d.n_cmap = len(self.cmap)
        d.advance = self.advance.ctypes.data_as(C.POINTER(C.c_int32)) if len(self.advance) else None
        d.outline_id = self.outline_id.ctypes.data_as(C.POINTER(C.c_uint32)) if len(self.advance) else None
        d.n_glyphs = len(self.advance)
        d.kern = self.kern.ctypes.data_as(C.POINTER(abi.KernPair)) if len(self.kern) else None
        d.n_kern = len(self.kern)
        d.ascent, d.descent, d.line_gap = self.ascent, self.descent, self.line_gap
        return d, (self.cmap, self.advance, self.outline_id, self.kern)

    def scale(self, font_size):
        """f64::from(scale_for_pixel_height(font_size as f32)): one f32 division, widened."""
        return float(np.float32(font_size) / np.float32(self.ascent - self.descent))

    def shape(self, chars):
        """TextPlacer::text_to_glyphs (text_placer.rs:170-197) of one text given as code points: TEXT_GLYPH_DTYPE records
        with the outline id as glyph_id, kern 0 for the first char, Rust's is_whitespace as the flag."""
        if self._glyph_of is None:
            self._glyph_of = dict(zip(self.cmap["code_point"].tolist(), self.cmap["glyph"].tolist()))
            self._kern_of = {(l, r): v for l, r, v in self.kern.tolist()}
        out = np.zeros(len(chars), TEXT_GLYPH_DTYPE)
        prev = None
        for k, cp in enumerate(int(c) for c in chars):
            g = self._glyph_of.get(cp, 0)
            kern = self._kern_of.get((prev, g), 0) if prev is not None else 0
            out[k] = (int(self.outline_id[g]), int(self.advance[g]), kern, 1 if cp in WHITE_SPACE else 0)
            prev = g
        return out


class StringLabelList:
    """Labels of a batch with string text (osmt_string_label_batch): `labels` are osmt_label records whose seg_off /
    n_segs name a range of `chars` (uint32 code points, in text order), `runs` (STRING_RUN_DTYPE) holds the font id, the
    font size and the placement of every label, `way_pts` / `way_sincos` the ways of the line-form runs as in
    TextLabelList."""

    def __init__(self, labels, job_label_off, runs, chars, way_pts, way_sincos):
        self.labels = np.ascontiguousarray(labels, dtype=LABEL_DTYPE)
        self.job_label_off = np.ascontiguousarray(job_label_off, dtype=np.uint32)
        self.runs = np.ascontiguousarray(runs, dtype=STRING_RUN_DTYPE)
        self.chars = np.ascontiguousarray(chars, dtype=np.uint32).reshape(-1)
        self.way_pts = np.ascontiguousarray(way_pts, dtype=np.int32).reshape(-1, 2)
        self.way_sincos = np.ascontiguousarray(way_sincos, dtype=np.float64).reshape(-1, 2)
        assert len(self.runs) == len(self.labels) and len(self.way_pts) == len(self.way_sincos)

    @property
    def n_jobs(self):
        return len(self.job_label_off) - 1

    def as_batch(self):
        b = abi.StringLabelBatch()
        b.labels = self.labels.ctypes.data_as(C.POINTER(abi.Label))
        b.n_labels = len(self.labels)
        b.job_label_off = self.job_label_off.ctypes.data_as(C.POINTER(C.c_uint32))
        b.runs = self.runs.ctypes.data_as(C.POINTER(abi.StringRun))
        b.chars = self.chars.ctypes.data_as(C.POINTER(C.c_uint32)) if len(self.chars) else None
        b.n_chars = len(self.chars)
        b.way_pts = self.way_pts.ctypes.data_as(C.POINTER(C.c_int32)) if len(self.way_pts) else None
        b.way_sincos = self.way_sincos.ctypes.data_as(C.POINTER(C.c_double)) if len(self.way_pts) else None
        b.n_way_pts = len(self.way_pts)
        return b

    def input_bytes(self):
        """bytes handed to the library: 40 + 64 per label, 4 per char, 24 per way point + the job offsets."""
        return 104 * len(self.labels) + 4 * len(self.chars) + 24 * len(self.way_pts) + 4 * len(self.job_label_off)

    def with_font(self, font):
        """Names `font` (a registered FontTable, or a font id) in every run; returns self."""
        self.runs["font_id"] = font.font_id if isinstance(font, FontTable) else int(font)
        return self

    def subset(self, idx):
        """The labels of tiles idx (in that order) as a StringLabelList of their own, chars and ways re-packed."""
        parts = []
        for i in idx:
            a, b = int(self.job_label_off[i]), int(self.job_label_off[i + 1])
            lab, runs = self.labels[a:b].copy(), self.runs[a:b].copy()
            cs, ps, ss, cur, pcur = [], [], [], 0, 0
            for l, r in zip(lab, runs):
                n = int(l["n_segs"])
                cs.append(self.chars[int(l["seg_off"]) : int(l["seg_off"]) + n])
                l["seg_off"] = cur if n else 0
                cur += n
                m = int(r["n_pts"]) if int(r["position"]) == abi.TEXT_LINE else 0
                ps.append(self.way_pts[int(r["pt_off"]) : int(r["pt_off"]) + m])
                ss.append(self.way_sincos[int(r["pt_off"]) : int(r["pt_off"]) + m])
                r["pt_off"] = pcur if m else 0
                pcur += m
            parts.append(StringLabelList(lab, [0, len(lab)], runs, np.concatenate(cs) if cs else np.zeros(0, np.uint32),
                                         np.concatenate(ps) if ps else np.zeros((0, 2), np.int32),
                                         np.concatenate(ss) if ss else np.zeros((0, 2))))
        return concat_string_labels(parts)

    def to_text_label_list(self, font):
        """The same labels as text runs, shaped here (FontTable.shape): what a caller of osmt_scene_set_text_labels
        would upload.  `font`: a FontTable, or a sequence of them indexed by font id."""
        fonts = {font.font_id: font} if isinstance(font, FontTable) else {f.font_id: f for f in font}
        runs = np.zeros(len(self.runs), TEXT_RUN_DTYPE)
        for name in ("position", "y_offset", "pt_off", "n_pts", "center_x", "center_y"):
            runs[name] = self.runs[name]
        glyphs = np.zeros(len(self.chars), TEXT_GLYPH_DTYPE)
        for i, (l, s) in enumerate(zip(self.labels, self.runs)):
            if not l["has_text"]:
                continue
            f = fonts[int(s["font_id"])]
            runs[i]["scale"] = f.scale(float(s["font_size"]))
            runs[i]["ascent"], runs[i]["descent"], runs[i]["line_gap"] = f.ascent, f.descent, f.line_gap
            a, n = int(l["seg_off"]), int(l["n_segs"])
            glyphs[a : a + n] = f.shape(self.chars[a : a + n])
        return TextLabelList(self.labels.copy(), self.job_label_off.copy(), runs, glyphs, self.way_pts.copy(), self.way_sincos.copy())


def concat_string_labels(lists):
    labels, offs, runs, chars, pts, scs = [], [0], [], [], [], []
    cur = pcur = 0
    for sl in lists:
        lab, run = sl.labels.copy(), sl.runs.copy()
        lab["seg_off"][lab["n_segs"] > 0] += cur
        run["pt_off"][(run["position"] == abi.TEXT_LINE) & (run["n_pts"] > 0)] += pcur
        labels.append(lab)
        runs.append(run)
        chars.append(sl.chars)
        pts.append(sl.way_pts)
        scs.append(sl.way_sincos)
        cur += len(sl.chars)
        pcur += len(sl.way_pts)
        offs.extend((offs[-1] + sl.job_label_off[1:].astype(np.int64)).tolist())
    return StringLabelList(np.concatenate(labels) if labels else np.zeros(0, LABEL_DTYPE), offs,
                           np.concatenate(runs) if runs else np.zeros(0, STRING_RUN_DTYPE),
                           np.concatenate(chars) if chars else np.zeros(0, np.uint32),
                           np.concatenate(pts) if pts else np.zeros((0, 2), np.int32), np.concatenate(scs) if scs else np.zeros((0, 2)))


def splice_string_labels(area, node):
    """What osmt_scene_build_tile_labels attaches: per tile the labels of `area` in front of those of `node` (a batch
    without way points: node labels), the node chars behind the areas' and every node label's seg_off moved by them."""
    assert area.n_jobs == node.n_jobs and len(node.way_pts) == 0
    lab, runs, offs = [], [], [0]
    moved = node.labels.copy()
    moved["seg_off"] += len(area.chars)
    for t in range(area.n_jobs):
        a0, a1, n0, n1 = (int(v) for v in (*area.job_label_off[t : t + 2], *node.job_label_off[t : t + 2]))
        lab += [area.labels[a0:a1], moved[n0:n1]]
        runs += [area.runs[a0:a1], node.runs[n0:n1]]
        offs.append(offs[-1] + (a1 - a0) + (n1 - n0))
    return StringLabelList(np.concatenate(lab) if lab else np.zeros(0, LABEL_DTYPE), offs, np.concatenate(runs) if runs else np.zeros(0, STRING_RUN_DTYPE),
                           np.concatenate([area.chars, node.chars]), area.way_pts, area.way_sincos)


_SYNTH_CP_BASE = 0x4E00  # code point of synthetic glyph g (not a space): _SYNTH_CP_BASE + g


def make_string_labels(n_tiles, table, **kw):
    """The label workload of make_text_labels as strings: (StringLabelList, FontTable).  The labels are those of
    make_text_labels(n_tiles, table, f32_scale=True, **kw) — same seed, same texts, anchors, ways, icons — and the font
    is built so that shaping the strings gives exactly that workload's glyph records: make_text_labels draws a kern per
    OCCURRENCE of a pair, so every shape of SYNTH_GLYPHS gets as many glyph indices (variants with the same advance and
    outline, a code point each) as it takes for every (left, right) pair of glyph indices to carry one kern value.  A
    variant of the space must have a White_Space code point, of which there are 25; when they run out for a left glyph,
    the left char gets a variant of its own.  Glyph 0 is .notdef (no shape).  Register the font (Context.register_font)
    and name it with StringLabelList.with_font before use."""
    sizes = []
    tl = make_text_labels(n_tiles, table, f32_scale=True, _font_px=sizes, **kw)
    n_shapes, space = len(SYNTH_GLYPHS), len(SYNTH_GLYPHS) - 1
    ws = sorted(WHITE_SPACE)
    shape_of = [space]            # glyph index -> shape; glyph 0 = .notdef
    code_of = [None]              # glyph index -> code point
    variants = [[] for _ in range(n_shapes)]
    kern_of = {}                  # (left, right) -> value, zeros included (pinned as "not listed")
    by_value = {}                 # (left, shape, value) -> right
    used = {}                     # (left, shape) -> variants of shape already paired with left (in order)

    def new_variant(s):
        if s == space and len(variants[s]) == len(ws):
            return None
        g = len(shape_of)
        shape_of.append(s)
        code_of.append(ws[len(variants[s])] if s == space else _SYNTH_CP_BASE + g)
        variants[s].append(g)
        return g

    def right_for(left, s, value):
        """a glyph of shape s whose pair with `left` carries `value` (None: the space's code points are used up)"""
        g = by_value.get((left, s, value))
        if g is None:
            n = used.get((left, s), 0)
            while n < len(variants[s]) and (left, variants[s][n]) in kern_of:
                n += 1
            g = variants[s][n] if n < len(variants[s]) else new_variant(s)
            if g is None:
                return None
            used[(left, s)] = n + 1
            pin(left, g, value)
        return g

    def pin(left, g, value):
        kern_of[(left, g)] = value
        by_value.setdefault((left, shape_of[g], value), g)

    chars = np.zeros(len(tl.glyphs), np.uint32)
    for l in tl.labels:
        if not l["has_text"]:
            continue
        a, n = int(l["seg_off"]), int(l["n_segs"])
        gs = []
        for k in range(n):
            t = tl.glyphs[a + k]
            s, value = int(t["glyph_id"]) - table.first_id, int(t["kern"])
            if k == 0:
                g = variants[s][0] if variants[s] else new_variant(s)
            else:
                g = right_for(gs[-1], s, value)
                if g is None:  # the space's code points are used up for this left glyph: a fresh one pairs with anything
                    gs[-1] = new_variant(shape_of[gs[-1]])
                    if k >= 2:
                        pin(gs[-2], gs[-1], int(tl.glyphs[a + k - 1]["kern"]))
                    g = right_for(gs[-1], s, value)
            gs.append(g)
        chars[a : a + n] = [code_of[g] for g in gs]
    cmap = sorted((code_of[g], g) for g in range(1, len(shape_of)))
    kern = sorted((lft, r, v) for (lft, r), v in kern_of.items() if v)
    font = FontTable(cmap, [500] + [SYNTH_GLYPHS[s][0] for s in shape_of[1:]], [table.first_id + s for s in shape_of], kern,
                     int(_SYNTH_ASCENT), int(_SYNTH_DESCENT), int(_SYNTH_GAP))
    runs = np.zeros(len(tl.runs), STRING_RUN_DTYPE)
    for name in ("position", "y_offset", "pt_off", "n_pts", "center_x", "center_y"):
        runs[name] = tl.runs[name]
    runs["font_size"] = sizes
    return StringLabelList(tl.labels, tl.job_label_off, runs, chars, tl.way_pts, tl.way_sincos), font
