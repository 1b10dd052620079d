"""Text-run cases for the placer tests (tests/test_text_placer_cpu.py, tests/test_text_edge_cases_cpu.py on the host,
tests/test_gpu_text_edges.py on the device).

A case is a name, a builder and a check:

  * case.build(first_id) returns a labels.TextLabelList whose glyph ids are first_id + (a glyph of the synthetic table);
  * case.check(got, gl, first_id) holds the literal expectations on `got`, the instance array in slot order
    (osmt_scene_read_glyph_instances, the host mirror, or the model's .slots); `gl` is the model's GlyphLabelList of
    the same batch, for the expectations on its packed list.

The first group restates the directed cases the host tests always had.  The second group is shaped by k_text_place
(osmt_textplace.hip): 64 lanes, texts and ways worked through in chunks of 64 glyphs and 64 edges, a row scan that
restarts at any row_start, TEXT_WAVES = 4 labels per workgroup, MAX_TEXT_WIDTH = 32.0.  Those cases carry `claims`, one
per label, from which expected_slots() writes the whole instance array down WITHOUT walking the text the way
TextPlacer::place does: a centred text from its claimed row starts, a text along a way from cumulative edge lengths and
one bisection per glyph.  Everything is at scale 1/64 with integer edge lengths (axis-parallel and 3-4-5 edges), so
every sum of place() is exact and the expectation can be asked for bit by bit.  All distances of a way are kept in
half font units, "hu" = 1/128 px: widths are whole font units, a glyph's centre may lie half a unit off.

tests/test_text_edge_cases_cpu.py proves with the model alone that every case sits on the edge it names."""
import bisect
import functools
import math

import numpy as np

from osm_renderer_amd import abi, labels

S64 = 1.0 / 64.0  # a scale whose products with small integers are exact
A, B, SP = 0, 1, 4  # glyph ids of the synthetic table: two letters and the space
ASCENT, DESCENT, ROW_HEIGHT = 800 * S64, -200 * S64, 800 * S64 + 200 * S64  # of the default metrics (800, -200, 0)
LAST = "last"  # a glyph that compute_way_position puts on the way's last point
NONE = "none"  # a label place() returns from early: OSMT_GLYPH_NONE in all its slots


def text_labels(specs, n_jobs=1):
    """One tile of text labels from dicts: glyphs [(id, advance, kern, whitespace)], position, scale, metrics
    (ascent, descent, line_gap), y_offset, center, pts (already in walking order), has_text (default 1)."""
    labs, runs, glyphs, pts = [], [], [], []
    n_gl = n_pt = 0
    for s in specs:
        l, r = np.zeros((), labels.LABEL_DTYPE), np.zeros((), labels.TEXT_RUN_DTYPE)
        g = np.array([tuple(t) for t in s["glyphs"]], dtype=labels.TEXT_GLYPH_DTYPE) if s["glyphs"] else np.zeros(0, labels.TEXT_GLYPH_DTYPE)
        l["has_text"], l["text_color"] = s.get("has_text", 1), s.get("color", (10, 20, 30))
        if "icon" in s:
            l["has_icon"], l["image_id"], l["icon_center_x"], l["icon_center_y"] = 1, s["icon"], s["center"][0], s["center"][1]
        l["seg_off"], l["n_segs"] = (n_gl if len(g) else 0), len(g)
        r["position"], r["scale"] = s.get("position", abi.TEXT_CENTER), s.get("scale", S64)
        r["ascent"], r["descent"], r["line_gap"] = s.get("metrics", (800, -200, 0))
        if r["position"] == abi.TEXT_LINE:
            p = np.array(s.get("pts", []), dtype=np.int32).reshape(-1, 2)
            r["pt_off"], r["n_pts"] = (n_pt if len(p) else 0), len(p)
            pts.append(p)
            n_pt += len(p)
        else:
            r["y_offset"] = s.get("y_offset", 0)
            r["center_x"], r["center_y"] = s.get("center", (100.0, 100.0))
        labs.append(l)
        runs.append(r)
        glyphs.append(g)
        n_gl += len(g)
    way = np.concatenate(pts) if pts else np.zeros((0, 2), np.int32)
    sincos = np.concatenate([labels.way_sincos(p) for p in pts]) if pts else np.zeros((0, 2))
    offs = [0] + [len(labs)] * n_jobs
    return labels.TextLabelList(np.array(labs, dtype=labels.LABEL_DTYPE), offs, np.array(runs, dtype=labels.TEXT_RUN_DTYPE),
                                np.concatenate(glyphs) if glyphs else np.zeros(0, labels.TEXT_GLYPH_DTYPE), way, sincos)


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def reverse_pool(tl):
    """The same labels with their glyph ranges in reverse label order in the pool (ranges must not overlap; nothing asks
    for label order)."""
    lab, g, cur = tl.labels.copy(), np.zeros_like(tl.glyphs), 0
    for i in reversed(range(len(lab))):
        off, n = int(lab[i]["seg_off"]), int(lab[i]["n_segs"])
        if n:
            g[cur : cur + n] = tl.glyphs[off : off + n]
            lab[i]["seg_off"] = cur
            cur += n
    return labels.TextLabelList(lab, tl.job_label_off.copy(), tl.runs.copy(), g, tl.way_pts.copy(), tl.way_sincos.copy())


def merge(lists):
    """Several one-tile TextLabelLists as ONE tile: (TextLabelList, [(first slot, slots)] per list)."""
    lab, runs, glyphs, pts, scs, spans = [], [], [], [], [], []
    n_gl = n_pt = 0
    for tl in lists:
        l, r = tl.labels.copy(), tl.runs.copy()
        l["seg_off"][l["n_segs"] > 0] += n_gl
        r["pt_off"][(r["position"] == abi.TEXT_LINE) & (r["n_pts"] > 0)] += n_pt
        lab.append(l), runs.append(r), glyphs.append(tl.glyphs), pts.append(tl.way_pts), scs.append(tl.way_sincos)
        spans.append((n_gl, len(tl.glyphs)))
        n_gl += len(tl.glyphs)
        n_pt += len(tl.way_pts)
    lab = np.concatenate(lab)
    return labels.TextLabelList(lab, [0, len(lab)], np.concatenate(runs), np.concatenate(glyphs), np.concatenate(pts), np.concatenate(scs)), spans


# ---- the expectation, written down from claims ----------------------------------------------------------------------
def units(spec):
    """Glyph::width of every glyph in font units: the advance, plus the kern behind the first glyph."""
    return [g[1] + (g[2] if k else 0) for k, g in enumerate(spec["glyphs"])]


def way_lengths(pts):
    """The integer edge lengths of a way built from axis-parallel and 3-4-5 edges."""
    out = []
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        d2 = (x1 - x0) ** 2 + (y1 - y0) ** 2
        assert math.isqrt(d2) ** 2 == d2
        out.append(math.isqrt(d2))
    return out


def centres_hu(spec):
    """(distance along the way of every glyph centre in 1/128 px, total width in font units, way length in px) of a
    line-form text at scale 1/64: the text is centred on the way."""
    w, T = units(spec), sum(way_lengths(spec["pts"]))
    s = 64 * T - sum(w)  # cur_dist = (total_way_length - total_width) / 2
    out, pre = [], 0
    for wk in w:
        out.append(s + 2 * pre + wk)
        pre += wk
    return out, sum(w), T


def locate(spec):
    """Per glyph of a line-form text (edge, numerator, denominator) with ratio = numerator / denominator, or LAST: the
    first edge whose END lies at or beyond the centre (seg_dist >= to_travel), found by bisection of the cumulative
    lengths.  A centre at or before the way's start, or beyond its end, is the last point."""
    lens = way_lengths(spec["pts"])
    cum = [128 * int(v) for v in np.concatenate([[0], np.cumsum(lens)])]  # the way's points, in hu from its start
    out = []
    for c in centres_hu(spec)[0]:
        e = bisect.bisect_left(cum, c, 1) - 1 if c > 0 else len(lens)
        out.append(LAST if e >= len(lens) else (e, c - cum[e], 128 * lens[e]))
    return out


def expected_slots(tl, specs, claims, first_id=0):
    """The instance array of a batch from its claims: per label None (no slots are written), NONE, dict(rows=[...]) for a
    centred text, dict() for a text along a way (its hits are the bisection's)."""
    slots = np.zeros(len(tl.glyphs), labels.GLYPH_INSTANCE_DTYPE)
    for l, spec, claim in zip(tl.labels, specs, claims):
        off, n = int(l["seg_off"]), int(l["n_segs"])
        if claim is None:
            assert n == 0 or not l["has_text"]
            continue
        assert n == len(spec["glyphs"]) > 0
        out = slots[off : off + n]
        out["glyph_id"], out["scale"] = [g[0] for g in spec["glyphs"]], spec.get("scale", S64)
        if claim == NONE:
            out["form"] = abi.GLYPH_NONE
            continue
        assert spec.get("scale", S64) == S64 and spec.get("metrics", (800, -200, 0)) == (800, -200, 0)
        w = units(spec)
        if spec.get("position", abi.TEXT_CENTER) == abi.TEXT_CENTER:
            rows = claim["rows"]
            cx, cy = spec.get("center", (100.0, 100.0))
            top = cy + spec["y_offset"] if spec.get("y_offset", 0) > 0 else cy - ROW_HEIGHT * len(rows) / 2.0
            out["form"] = abi.GLYPH_CENTER
            for r, (a, b) in enumerate(zip(rows, rows[1:] + [n])):
                pre, row_width = 0, sum(w[a:b])
                for k in range(a, b):
                    out["p"][k, :2] = (cx - row_width / 128.0 + pre / 64.0, top + r * ROW_HEIGHT + ASCENT)
                    pre += w[k]
        else:
            pts = spec["pts"]
            sincos = labels.way_sincos(pts)
            out["form"] = abi.GLYPH_LINE
            for k, hit in enumerate(locate(spec)):
                if hit == LAST:
                    e, (x, y) = len(pts) - 2, (float(pts[-1][0]), float(pts[-1][1]))
                else:
                    e, ratio = hit[0], hit[1] / hit[2]
                    (fx, fy), (tx, ty) = pts[e], pts[e + 1]
                    x, y = float(fx) + (float(tx - fx) * ratio), float(fy) + (float(ty - fy) * ratio)
                out["p"][k] = (w[k] / 128.0, (DESCENT + ASCENT) / 2.0, sincos[e][0], sincos[e][1], x, y)
    return slots


class Case:
    """specs(first_id) -> the label dicts of text_labels(); claims: per label, see expected_slots(); named: what the case
    was built to hit, {label: ...}, proved by tests/test_text_edge_cases_cpu.py; literal(parts, gl, first_id): further
    literal expectations on the per-label slices of the instance array."""

    def __init__(self, name, specs, claims=None, named=None, literal=None, reverse=False):
        self.name, self.specs, self.claims, self.named, self.literal, self.reverse = name, specs, claims, named or {}, literal, reverse

    def __repr__(self):
        return f"Case({self.name})"

    def build(self, first_id=0):
        tl = text_labels(self.specs(first_id))
        return reverse_pool(tl) if self.reverse else tl

    def parts(self, got, first_id=0):
        tl = self.build(first_id)
        assert len(got) == len(tl.glyphs)
        return [got[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])] for l in tl.labels]

    def check(self, got, gl=None, first_id=0):
        if self.claims is not None:
            tl = self.build(first_id)
            want = expected_slots(tl, self.specs(first_id), self.claims, first_id)
            bad = np.nonzero((_u8(got).reshape(-1, 64) != _u8(want).reshape(-1, 64)).any(axis=1))[0]
            assert got.shape == want.shape and len(bad) == 0, f"{self.name}: {len(bad)} of {len(got)} slots differ from the written-down placement, first at slot {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
        if self.literal is not None:
            self.literal(self.parts(got, first_id), gl, first_id)


def rows_of(part):
    """Row starts of a centred text's instances."""
    y = part["p"][:, 1]
    return [0] + [k for k in range(1, len(y)) if y[k] != y[k - 1]]


# ---- the directed cases the host tests always had -------------------------------------------------------------------
def _break_threshold():
    def specs(f):
        # "A_B" at scale 1/64: A = 16.0, the space 8.0 -> current_row_width + w = 24 + 8 = 32.0, not > 32.0: one row
        on = dict(glyphs=[(f + A, 1024, 0, 0), (f + SP, 512, 0, 1), (f + B, 1024, 0, 0)])
        # one font unit more on the space: 24.015625 + 8.015625 > 32.0: the space closes its row and stays in it
        over = dict(glyphs=[(f + A, 1024, 0, 0), (f + SP, 513, 0, 1), (f + B, 1024, 0, 0)])
        # the same width reached through a kern; and a non-whitespace glyph never breaks
        kern = dict(glyphs=[(f + A, 1024, 0, 0), (f + SP, 500, 13, 1), (f + B, 1024, 0, 0)])
        wide = dict(glyphs=[(f + A, 4096, 0, 0), (f + B, 4096, 0, 0)])
        return [on, over, kern, wide]

    def literal(p, gl, f):
        on, over, kern, wide = p
        assert len(np.unique(on["p"][:, 1])) == 1
        assert over["p"][0, 1] == over["p"][1, 1] < over["p"][2, 1]
        assert over["p"][0, 0] == 100.0 - (16.0 + 8.015625) / 2.0 and over["p"][2, 0] == 100.0 - 8.0
        assert np.array_equal(kern["p"], over["p"])
        assert len(np.unique(wide["p"][:, 1])) == 1

    return Case("break-threshold", specs, claims=[dict(rows=[0]), dict(rows=[0, 2]), dict(rows=[0, 2]), dict(rows=[0])], literal=literal)


_G3 = lambda f: [(f + A, 1024, 0, 0), (f + SP, 2048, 0, 1), (f + B, 1024, 0, 0)]


def _whitespace_and_y_offset():
    def specs(f):
        trailing = dict(glyphs=[(f + A, 1024, 0, 0), (f + SP, 2048, 0, 1), (f + B, 1024, 0, 0), (f + SP, 2048, 0, 1)])
        only = dict(glyphs=[(f + SP, 2048, 0, 1)] * 3)
        return [trailing, only, dict(glyphs=_G3(f), y_offset=0), dict(glyphs=_G3(f), y_offset=8)]

    def literal(p, gl, f):
        trailing, only, a, b = p
        assert len(np.unique(trailing["p"][:, 1])) == 2  # the last space closes the second row, no empty third one
        assert len(np.unique(only["p"][:, 1])) == 3 and (only["form"] == abi.GLYPH_CENTER).all()
        row_height = 800 * S64 + 200 * S64
        assert a["p"][0, 1] == 100.0 - row_height * 2.0 / 2.0 + 800 * S64 and b["p"][0, 1] == 100.0 + 8.0 + 800 * S64
        assert np.array_equal(a["p"][:, 0], b["p"][:, 0])

    return Case("whitespace-and-y-offset", specs, claims=[dict(rows=[0, 2]), dict(rows=[0, 1, 2]), dict(rows=[0, 2]), dict(rows=[0, 2])], literal=literal)


def _empty_label_first():
    def literal(p, gl, f):
        assert sum(len(x) for x in p) == 3
        if gl is not None:
            assert gl.labels["n_segs"].tolist() == [0, 3]

    return Case("empty-label-first", lambda f: [dict(glyphs=[]), dict(glyphs=_G3(f))], claims=[None, dict(rows=[0, 2])], literal=literal)


def _widths_not_positive():
    def specs(f):
        # a kern larger than the advance: the width is negative, the pen moves back
        back = dict(glyphs=[(f + A, 1024, 0, 0), (f + B, 100, -300, 0), (f + A, 0, 0, 0), (f + B, 640, 0, 0)])
        # the kern of the FIRST glyph is ignored
        return [back, dict(glyphs=[(f + A, 1024, -999, 0)]), dict(glyphs=[(f + A, 1024, 0, 0)])]

    def literal(p, gl, f):
        got, a, b = p
        total = 16.0 + (100 * S64 + -300 * S64) + 0.0 + 10.0
        assert got["p"][0, 0] == 100.0 - total / 2.0 and got["p"][2, 0] < got["p"][1, 0] and got["p"][3, 0] == got["p"][2, 0]
        assert np.array_equal(_u8(a), _u8(b))

    return Case("widths-not-positive", specs, claims=[dict(rows=[0])] * 3, literal=literal)


def _line(glyphs, pts, **kw):
    return dict(glyphs=glyphs, position=abi.TEXT_LINE, pts=pts, **kw)


def _zero_length_edges_and_bends():
    pts = [(0, 0), (0, 0), (10, 0), (10, 0), (10, 0), (10, 20), (40, 60), (40, 60)]

    def literal(p, gl, f):
        (got,) = p
        assert (got["form"] == abi.GLYPH_LINE).all()
        # total way length 10 + 20 + 50 = 80: the glyph centres lie on the way, the first on the vertical edge
        assert got["p"][0, 4] == 10.0 and 0.0 < got["p"][0, 5] < 20.0
        assert got["p"][0, 2] == math.sin(-math.atan2(20.0, 0.0)) and got["p"][0, 3] == math.cos(-math.atan2(20.0, 0.0))
        assert (got["p"][:, 1] == (-200 * S64 + 800 * S64) / 2.0).all()

    return Case("line-zero-length-edges-and-bends", lambda f: [_line([(f + A, 640, 0, 0), (f + B, 640, 5, 0), (f + SP, 320, 0, 1), (f + A, 640, -7, 0)], pts)],
                claims=[dict()], literal=literal)


def _exactly_as_long_as_the_way():
    way = [(3, 7), (19, 7)]  # 16.0 long

    def literal(p, gl, f):
        (got,) = p
        assert got["form"].tolist() == [abi.GLYPH_LINE] and got["p"][0].tolist() == [8.0, 600 * S64 / 2.0, -0.0, 1.0, 11.0, 7.0]

    return Case("line-exactly-as-long-as-the-way", lambda f: [_line([(f + A, 1024, 0, 0)], way, scale=S64)], claims=[dict()], literal=literal)


LONGER = math.nextafter(S64, 1.0)  # 1024 * LONGER is the double after 16.0


def _one_ulp_longer_than_the_way():
    way = [(3, 7), (19, 7)]

    def literal(p, gl, f):
        (got,) = p
        assert 1024.0 * LONGER == math.nextafter(16.0, math.inf)
        assert got["form"].tolist() == [abi.GLYPH_NONE]
        if gl is not None:
            assert gl.labels["n_segs"].tolist() == [0] and gl.labels["has_text"].tolist() == [1] and len(gl.glyphs) == 0
        assert got["glyph_id"].tolist() == [f + A] and got["scale"][0] == LONGER and not got["p"].any()

    return Case("line-one-ulp-longer-than-the-way", lambda f: [_line([(f + A, 1024, 0, 0)], way, scale=LONGER)], claims=[NONE], literal=literal)


def _advance_not_positive():
    way = [(0, 0), (8, 0), (8, 24)]  # 32.0 long; the last edge points down

    def specs(f):
        # cur_dist = 0 and a first glyph of negative width: compute_way_position(-8) never enters its loop
        # exactly zero counts as "not positive" as well
        return [_line([(f + A, -1024, 0, 0), (f + B, 3072, 0, 0)], way), _line([(f + A, 0, 0, 0), (f + B, 640, 0, 0)], [(0, 0), (5, 0), (5, 5)])]

    def literal(p, gl, f):
        got, zero = p
        down = math.atan2(24.0, 0.0)
        assert got["p"][0].tolist() == [-8.0, 600 * S64 / 2.0, math.sin(-down), math.cos(-down), 8.0, 24.0]
        # the second glyph: cur_dist = -16, centre 24 -> advance 8.0 = the whole first edge (seg_dist >= to_travel)
        assert got["p"][1, 4:].tolist() == [8.0, 0.0] and got["p"][1, 2:4].tolist() == [math.sin(-0.0), math.cos(-0.0)]
        assert zero["p"][0, 4:].tolist() == [5.0, 5.0] and zero["p"][1, 4:].tolist() == [5.0, 0.0]

    return Case("line-advance-not-positive", specs, claims=[dict(), dict()], named={0: {0: LAST, 1: (0, 1.0)}, 1: {0: LAST, 1: (0, 1.0)}}, literal=literal)


def _running_off_the_end():
    # widths +40, -30: total 10 = the way's length, but the first glyph's centre (20) lies beyond the end
    way = [(0, 0), (6, 0), (6, 4)]

    def literal(p, gl, f):
        (got,) = p
        up = math.atan2(4.0, 0.0)
        assert got["p"][0, 2:].tolist() == [math.sin(-up), math.cos(-up), 6.0, 4.0]
        assert got["form"].tolist() == [abi.GLYPH_LINE] * 2

    return Case("line-running-off-the-end", lambda f: [_line([(f + A, 2560, 0, 0), (f + B, -1920, 0, 0)], way)], claims=[dict()],
                named={0: {0: LAST, 1: LAST}}, literal=literal)


def _ways_of_one_point_and_of_none():
    def specs(f):
        g = [(f + A, 64, 0, 0), (f + B, 64, 0, 0)]
        return [_line(g, []), _line(g, [(5, 5)]), _line(g, [(5, 5), (5, 5)]), _line(g, [(0, 0), (9, 0)])]

    def literal(p, gl, f):
        got = np.concatenate(p)
        assert got["form"].tolist() == [abi.GLYPH_NONE] * 6 + [abi.GLYPH_LINE] * 2  # two equal points: length 0 < width
        if gl is not None:
            assert gl.labels["n_segs"].tolist() == [0, 0, 0, 2] and gl.labels["seg_off"].tolist() == [0, 0, 0, 0]

    return Case("line-ways-of-one-point-and-of-none", specs, claims=[NONE, NONE, NONE, dict()], literal=literal)


# ---- cases shaped by the kernel ---------------------------------------------------------------------------------------
def _letter(f, k, advance, kern=0):
    return (f + k % 4, advance, kern, 0)


def _space(f, advance, kern=0):
    return (f + SP, advance, kern, 1)


def one_row_glyphs(f, n):
    """n small letters in one row; glyphs 64 and 128 (lane 0 of the second and third chunk) carry a kern, and so does
    glyph 0, whose kern does not count."""
    kern = {0: 9, 64: 3, 128: -2}
    return [_letter(f, k, 6 + k % 5, kern.get(k, 0)) for k in range(n)]


ONE_ROW_SIZES = (63, 64, 65, 127, 128, 129)


def _one_row():
    def literal(p, gl, f):
        for n, part in zip(ONE_ROW_SIZES, p):
            x = part["p"][:, 0]
            assert len(part) == n and rows_of(part) == [0]
            assert x[1] - x[0] == 6 * S64  # glyph 0: its advance alone
            if n > 65:
                assert x[65] - x[64] == (6 + 64 % 5 + 3) * S64

    return Case("center-one-row", lambda f: [dict(glyphs=one_row_glyphs(f, n), center=(100.0 + n, 80.0)) for n in ONE_ROW_SIZES],
                claims=[dict(rows=[0])] * len(ONE_ROW_SIZES), literal=literal)


def _closing_space(i):
    """Letters 0 .. i - 1 that sum to 16.0, a space of 8.0 at index i, three letters behind it: at the space
    current_row_width + w = 16 + 8 + 8 = 32.0, not > 32.0.  The second label has one font unit more on glyph i - 1."""
    def specs(f):
        base, rem = divmod(1024, i)
        head = [_letter(f, k, base + (1 if k < rem else 0)) for k in range(i)]
        tail = [_space(f, 512)] + [_letter(f, k, 40) for k in range(3)]
        over = head[:-1] + [_letter(f, i - 1, head[-1][1] + 1)]
        return [dict(glyphs=head + tail), dict(glyphs=over + tail, center=(120.0, 140.0))]

    return Case(f"center-space-closes-at-{i}", specs, claims=[dict(rows=[0]), dict(rows=[0, i + 1])],
                named={0: dict(edge_sum={i: 32.0}), 1: dict(edge_sum={i: 32.0 + S64})})


def _rows_mid_chunk():
    """200 glyphs, rows [0, 5), [5, 70), [70, 200): the row scan and the placing pass start at 5 and at 70 and cross a
    chunk border inside the row; spaces that do not break sit inside the rows; glyphs 70 (a row's first), 128 and 134 (lane
    0 of the second chunk counted from 0 and from 70) carry kerns."""
    def glyphs(f):
        g = []
        for k in range(200):
            if k < 4:
                g.append(_letter(f, k, 100))
            elif k == 4:
                g.append(_space(f, 2048))
            elif k < 69:
                g.append(_space(f, 16) if k == 20 else _letter(f, k, 16))
            elif k == 69:
                g.append(_space(f, 1024))  # 64 * 0.25 + 16 = 32.0 with it, + 16 > 32.0
            else:
                g.append(_space(f, 8) if k == 100 else _letter(f, k, 8, {70: 5, 128: -3, 134: 4}.get(k, 0)))
        return g

    return Case("center-rows-start-mid-chunk", lambda f: [dict(glyphs=glyphs(f), y_offset=0, center=(90.0, 120.0)), dict(glyphs=glyphs(f), y_offset=7, center=(150.5, 60.25))],
                claims=[dict(rows=[0, 5, 70])] * 2, named={0: dict(edge_sum={4: 6.25 + 32.0 + 32.0, 69: 48.0, 20: 4.0 + 0.25}), 1: dict()})


def _only_spaces():
    return Case("center-only-spaces", lambda f: [dict(glyphs=[_space(f, 2048)] * n, center=(100.0 + n, 100.0)) for n in (64, 65)],
                claims=[dict(rows=list(range(64))), dict(rows=list(range(65)))])


def _space_last():
    """A wide space as the last glyph, at index 63 and at 64: it closes the row it stands in, no empty row follows —
    with a break before it (rows [0, 11)) and without."""
    def specs(f):
        out = []
        for n in (64, 65):
            plain = [_letter(f, k, 8) for k in range(n - 1)] + [_space(f, 2048)]
            broken = list(plain)
            broken[10] = _space(f, 2048)
            out += [dict(glyphs=plain), dict(glyphs=broken)]
        return out

    return Case("center-space-is-the-last-glyph", specs, claims=[dict(rows=[0]), dict(rows=[0, 11])] * 2)


def _widths_not_positive_at_the_chunk_border():
    def specs(f):
        neg, zero = lambda k: _letter(f, k, 10, -300), lambda k: _letter(f, k, 0)
        out = []
        for at63, at64 in ((neg, zero), (zero, neg)):
            g = [_letter(f, k, 32) for k in range(70)]
            g[63], g[64] = at63(63), at64(64)
            out.append(dict(glyphs=g))
        return out

    def literal(p, gl, f):
        a, b = (part["p"][:, 0] for part in p)
        assert a[64] == a[63] - 290 * S64 and a[65] == a[64] and a[66] == a[65] + 32 * S64  # the pen moves back across the border
        assert b[64] == b[63] and b[65] == b[64] - 290 * S64

    return Case("center-widths-not-positive-at-lanes-63-64", specs, claims=[dict(rows=[0])] * 2, literal=literal)


def way(ne, zero=(), x0=0, y0=0):
    """A way of ne edges of integer length: even edges run along x (4 or 2 long), odd ones are 3-4-5 steps up or down,
    the last edge is 8 long along x; `zero`: indices of zero-length edges."""
    pts = [(x0, y0)]
    for e in range(ne):
        x, y = pts[-1]
        if e in zero:
            pts.append((x, y))
        elif e == ne - 1:
            pts.append((x + 8, y))
        elif e % 2 == 0:
            pts.append((x + (4 if e % 4 == 0 else 2), y))
        else:
            pts.append((x + 3, y + (4 if e % 4 == 1 else -4)))
    return pts


def _mid(lens, e):
    return 128 * sum(lens[:e]) + 64 * lens[e]


def _end(lens, e):
    return 128 * sum(lens[: e + 1])


TARGET_W = 16  # font units of a glyph that is aimed at a point of the way
MARGIN = 32  # hu between the way's ends and the text


def aimed_text(f, pts, targets, shift=0):
    """A text [front pad, glyph, spacer, glyph, ..., back pad] on the way `pts` whose glyphs of TARGET_W units have their
    centres at the distances `targets` (hu, rising, even) — plus `shift` hu when the front pad is made that many units
    wider.  Returns (glyphs, [index of the aimed glyph per target])."""
    lens = way_lengths(pts)
    start = targets[0] - TARGET_W
    assert (start - MARGIN) % 2 == 0 and start > MARGIN
    widths, aimed, pos = [(start - MARGIN) // 2 + shift], [], start
    for j, t in enumerate(targets):
        gap = t - TARGET_W - pos
        assert gap >= 0 and gap % 2 == 0
        if gap:
            widths.append(gap // 2)
            pos += gap
        aimed.append(len(widths))
        widths.append(TARGET_W)
        pos += 2 * TARGET_W
    back = 128 * sum(lens) - MARGIN - pos
    assert back > 0 and back % 2 == 0
    widths.append(back // 2)
    assert max(widths) + 7 <= 65535
    # behind the first glyph a part of every width comes from the kern
    return [_letter(f, k, w + (7 if k else 0), -7 if k else 0) for k, w in enumerate(widths)], aimed


def _way_targets(ne):
    """(targets in hu, what they are) for the way of ne edges."""
    lens = way_lengths(way(ne))
    if ne == 63:
        return [_mid(lens, 30), _mid(lens, 61), _mid(lens, 62)], [(30, 0.5), (61, 0.5), (62, 0.5)]
    if ne == 64:
        return [_mid(lens, 62), _mid(lens, 63)], [(62, 0.5), (63, 0.5)]
    t, what = [_mid(lens, 62), _mid(lens, 63), _end(lens, 63), _mid(lens, 64)], [(62, 0.5), (63, 0.5), (63, 1.0), (64, 0.5)]
    if ne - 1 > 64:
        t.append(_mid(lens, ne - 1))
        what.append((ne - 1, 0.5))
    return t, what


def _way_of(ne):
    """A way of ne edges with a text aimed at the middles of edges 62, 63, 64 and of the last edge, and at the END of edge
    63 exactly (seg_dist == to_travel: ratio 1.0 on edge 63).  The second label is the same text one hu further: what
    was the end of edge 63 is now on edge 64 with ratio (1 / 128) / its length."""
    pts = way(ne, x0=3, y0=40)
    targets, what = _way_targets(ne)
    lens = way_lengths(pts)

    def specs(f):
        return [_line(aimed_text(f, pts, targets, shift)[0], pts) for shift in ((0, 1) if ne >= 65 else (0,))]

    aimed = aimed_text(0, pts, targets)[1]
    named = {0: dict(zip(aimed, what))}
    if ne >= 65:
        named[1] = {aimed[2]: (64, (1.0 / 128.0) / lens[64])}
    return Case(f"line-way-of-{ne}-edges", specs, claims=[dict()] * (2 if ne >= 65 else 1), named=named)


def _long_text_on_a_long_way():
    """65 and 130 glyphs on a way of 130 edges: glyph 64's (and 128's) cur_dist comes from the serial carry across the
    chunk border, and its walk starts again at edge 0 while lane 63 of the chunk before ended beyond edge 64."""
    pts = way(130, x0=-100, y0=200)

    def glyphs(f, n):
        return [_letter(f, k, 24 + 8 * (k % 3), {0: 11, 64: -5, 128: 5}.get(k, 0)) for k in range(n)]

    return Case("line-glyph-64-starts-again-at-edge-0", lambda f: [_line(glyphs(f, 65), pts), _line(glyphs(f, 130), pts)], claims=[dict(), dict()],
                named={0: dict(beyond_edge_64=[63, 64]), 1: dict(beyond_edge_64=[63, 64, 65, 127, 128, 129])})


def _zero_length_edges_at_63_64():
    """Edges 63 and 64 of the way have no length.  A glyph aimed at the end of edge 62 stays there (ratio 1.0); one hu
    further it passes both (0 >= to_travel is false) and lands on edge 65."""
    pts = way(70, zero=(63, 64), x0=10, y0=90)
    lens = way_lengths(pts)
    targets = [_mid(lens, 62), _end(lens, 62), _mid(lens, 65), _mid(lens, 69)]
    aimed = aimed_text(0, pts, targets)[1]
    return Case("line-zero-length-edges-63-64", lambda f: [_line(aimed_text(f, pts, targets, shift)[0], pts) for shift in (0, 1)], claims=[dict(), dict()],
                named={0: dict(zip(aimed, [(62, 0.5), (62, 1.0), (65, 0.5), (69, 0.5)])), 1: {aimed[1]: (65, (1.0 / 128.0) / lens[65])}})


def _advance_not_positive_at_the_chunk_border():
    """cur_dist = 0 (the text is as long as the way) and a glyph 0 without width: its advance is 0.0.  Glyph 64, the first
    lane of the second chunk, has my_dist + w / 2 = 63 / 64 - 200 / 128 < 0.  Both get the last point and the last edge's
    angle, form LINE."""
    pts = way(66, x0=20, y0=150)
    T = sum(way_lengths(pts))

    def specs(f):
        g = [_letter(f, 0, 0)] + [_letter(f, k, 1) for k in range(1, 64)] + [_letter(f, 64, -200)]
        g += [_letter(f, 65, 64 * T - (63 - 200) - 120)] + [_letter(f, k, 40) for k in range(66, 69)]
        return [_line(g, pts)]

    return Case("line-advance-not-positive-at-glyphs-0-64", specs, claims=[dict()], named={0: {0: LAST, 1: (0, (1.0 / 128.0) / 4.0), 64: LAST}})


def _running_off_the_end_from_the_second_chunk():
    """Glyph 65 is twice as wide as the way is long, glyph 66 takes nearly all of it back: the text is shorter than the
    way, but the centres of both lie beyond its end; glyph 67 is back on it."""
    pts = way(70, x0=-30, y0=10)
    T = sum(way_lengths(pts))

    def specs(f):
        g = [_letter(f, k, 16) for k in range(65)] + [_letter(f, 65, 128 * T), _letter(f, 66, -(128 * T - 640)), _letter(f, 67, 16)]
        return [_line(g, pts)]

    return Case("line-running-off-the-end-from-glyph-65", specs, claims=[dict()], named={0: {64: "hit", 65: LAST, 66: LAST, 67: "hit"}})


def _as_long_as_a_way_of_65_edges():
    """A way of 65 edges, 128.0 long, and a text of two glyphs of 64.0: exactly as long.  At the next scale each glyph
    is 64 + 2^-46 and the text 128 + 2^-45, the double after 128.0: place() returns before it places anything."""
    lens = [5, 2, 2, 1, 1, 1] * 10 + [2, 2, 2, 1, 1]
    assert len(lens) == 65 and sum(lens) == 128
    pts = [(-20, 30)]
    for k, d in enumerate(lens):
        x, y = pts[-1]
        pts.append((x + 3, y + (4 if k % 12 == 0 else -4)) if d == 5 else (x + d, y))
    g = lambda f: [_letter(f, 0, 4096), _letter(f, 1, 4096)]
    return Case("line-as-long-as-a-way-of-65-edges", lambda f: [_line(g(f), pts), _line(g(f), pts, scale=LONGER)], claims=[dict(), NONE],
                named={0: dict(total=128.0), 1: dict(total=math.nextafter(128.0, math.inf))})


def _mixed_batch(reverse):
    """Nine labels, not a multiple of TEXT_WAVES: waves that return at once share a workgroup with waves that run long."""
    w70, w5 = way(70, x0=8, y0=180), [(30, 30), (60, 30), (63, 34), (90, 34), (90, 60)]

    def specs(f):
        short = [_letter(f, 0, 640), _letter(f, 1, 600, 5), _space(f, 300), _letter(f, 3, 620, -9)]
        return [_line(short, w5),
                dict(glyphs=[], has_text=0),
                dict(glyphs=[(f + A, 1024, 0, 0), (f + SP, 513, 0, 1), (f + B, 1024, 0, 0)], center=(60.0, 90.0)),
                dict(glyphs=[]),
                _line(short, [(5, 5)]),
                dict(glyphs=one_row_glyphs(f, 130), center=(128.0, 150.0)),
                _line([_letter(f, k, 100 + 8 * (k % 3), 3 if k == 64 else 0) for k in range(70)], w70),
                dict(glyphs=_G3(f), y_offset=8, center=(200.0, 80.0)),
                _line(short[:3], [(150, 20), (150, 60)])]

    claims = [dict(), None, dict(rows=[0, 2]), None, NONE, dict(rows=[0]), dict(), dict(rows=[0, 2]), dict()]
    return Case("batch-of-nine-reversed-pool" if reverse else "batch-of-nine", specs, claims=claims, reverse=reverse)


OLD = ("break-threshold", "whitespace-and-y-offset", "empty-label-first", "widths-not-positive", "line-zero-length-edges-and-bends",
       "line-exactly-as-long-as-the-way", "line-one-ulp-longer-than-the-way", "line-advance-not-positive", "line-running-off-the-end",
       "line-ways-of-one-point-and-of-none")


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order (tuple of Case): the directed cases of old (their names are in OLD), then the ones shaped
    by the kernel."""
    old = [_break_threshold(), _whitespace_and_y_offset(), _empty_label_first(), _widths_not_positive(), _zero_length_edges_and_bends(),
           _exactly_as_long_as_the_way(), _one_ulp_longer_than_the_way(), _advance_not_positive(), _running_off_the_end(),
           _ways_of_one_point_and_of_none()]
    assert tuple(c.name for c in old) == OLD
    new = [_one_row()] + [_closing_space(i) for i in (62, 63, 64, 65)] + [_rows_mid_chunk(), _only_spaces(), _space_last(),
                                                                          _widths_not_positive_at_the_chunk_border()]
    new += [_way_of(ne) for ne in (63, 64, 65, 128, 129)]
    new += [_long_text_on_a_long_way(), _zero_length_edges_at_63_64(), _advance_not_positive_at_the_chunk_border(),
            _running_off_the_end_from_the_second_chunk(), _as_long_as_a_way_of_65_edges(), _mixed_batch(False), _mixed_batch(True)]
    return tuple(old + new)


def case(name):
    return next(c for c in cases() if c.name == name)
