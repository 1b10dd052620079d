"""The cases of tests/_text_place_cases.py and tests/_text_shape_cases.py are what they claim (no GPU, the Python models
alone): a case that drifts off the edge it was built for fails here, on any machine.

Placer, per label of every case:

  * the model's instance array equals, byte for byte, the one written down from the case's claims (row starts; cumulative
    edge lengths and one bisection per glyph) — so the claims are the model's;
  * a centred text breaks where the claims say: the rows start there, every glyph in front of a row start is a
    whitespace whose current_row_width + w exceeds 32.0, and the sums named by the case have exactly the named value
    (32.0 and 32.015625 at the threshold);
  * a text along a way: compute_way_position is walked again for every glyph, keeping the edge and the ratio; they are
    the bisection's, the named glyphs hit the named edge with the named ratio, the named glyphs — and no others — get
    the last point;
  * a label place() returns early from is one the model returns None for.

Shaper: the pool slots the block-border case names, the reversed pool, and that the cases tell a correct kernel from one
with a 16-bit kern key, a kern carried across a label boundary or a White_Space member missing."""
import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from tests import _text_place_cases as pc
from tests import _text_placer_model as model
from tests import _text_shape_cases as sc
from tests import _text_shaper_model as shaper

PLACE = pc.cases()
SHAPE = sc.cases()


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def walk(points, advance_by):
    """compute_way_position (text_placer.rs:270-296) once more, returning where it stops: (edge, ratio) or pc.LAST."""
    to_travel = advance_by
    for e in range(len(points) - 1):
        if not to_travel > 0.0:
            break
        seg_dist = model._dist(points[e], points[e + 1])
        if seg_dist >= to_travel:
            return e, to_travel / seg_dist
        to_travel -= seg_dist
    return pc.LAST


def line_hits(run, glyphs, points):
    """(hits per glyph, total_width, total_way_length) of a text along a way, with the model's own sums."""
    gl, total_width = model.text_to_glyphs(glyphs, float(run["scale"]))
    total_way_length = 0.0
    for i in range(1, len(points)):
        total_way_length += model._dist(points[i - 1], points[i])
    cur_dist = (total_way_length - total_width) / 2.0
    hits = []
    for _, width, _ in gl:
        advance_by = cur_dist + width / 2.0
        hit = walk(points, advance_by)
        # the walk above is the model's: the same position, the same edge's angle
        x, y, angle = model.compute_way_position(points, advance_by)
        e = len(points) - 2 if hit == pc.LAST else hit[0]
        assert angle == model._get_angle(points, e)
        if hit == pc.LAST:
            assert (x, y) == (float(points[-1][0]), float(points[-1][1]))
        else:
            (fx, fy), (tx, ty) = (int(v) for v in points[e]), (int(v) for v in points[e + 1])
            assert (x, y) == (float(fx) + (float(tx - fx) * hit[1]), float(fy) + (float(ty - fy) * hit[1]))
        hits.append(hit)
        cur_dist += width
    return hits, total_width, total_way_length


@pytest.mark.parametrize("case", PLACE, ids=[c.name for c in PLACE])
def test_placer_case_is_what_it_claims(case):
    tl, specs = case.build(0), case.specs(0)
    gl = model.place_text_labels(tl)
    case.check(gl.slots, gl)  # the model's bytes are the ones written down from the claims
    assert len(case.claims) == len(specs) == len(tl.labels)
    for i, (l, r, spec, claim) in enumerate(zip(tl.labels, tl.runs, specs, case.claims)):
        named = case.named.get(i, {})
        glyphs = tl.glyphs[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])]
        if claim is None:
            assert not l["has_text"] or l["n_segs"] == 0
            continue
        line = int(r["position"]) == abi.TEXT_LINE
        points = tl.way_pts[int(r["pt_off"]) : int(r["pt_off"]) + int(r["n_pts"])] if line and int(r["n_pts"]) else []
        placed = model.place(r, glyphs, points)
        if claim == pc.NONE:
            assert placed is None
            if "total" in named:
                assert line_hits(r, glyphs, points)[1:] == (named["total"], 128.0) and named["total"] > 128.0
            continue
        assert placed is not None and len(placed) == len(glyphs)
        if not line:
            widths = [w for _, w, _ in model.text_to_glyphs(glyphs, float(r["scale"]))[0]]
            rows = [0] + [k for k in range(1, len(placed)) if placed[k][2][1] != placed[k - 1][2][1]]
            assert rows == claim["rows"] == model_rows(glyphs, widths)
            for start in rows[1:]:  # the breaking glyph: a whitespace over the threshold
                assert glyphs["flags"][start - 1] == 1 and row_sum(widths, rows, start - 1) > model.MAX_TEXT_WIDTH
            for k, value in named.get("edge_sum", {}).items():
                assert glyphs["flags"][k] == 1 and row_sum(widths, rows, k) == value, (k, row_sum(widths, rows, k))
        else:
            hits, total_width, total_way_length = line_hits(r, glyphs, points)
            assert total_width <= total_way_length
            located = pc.locate(spec)
            assert [h if h == pc.LAST else h[0] for h in hits] == [h if h == pc.LAST else h[0] for h in located]
            assert all(h == pc.LAST or h[1] == want[1] / want[2] for h, want in zip(hits, located))
            for k, want in named.items():
                if k == "beyond_edge_64":
                    assert all(hits[g] != pc.LAST and hits[g][0] > 64 for g in want)
                elif k == "total":
                    assert (total_width, total_way_length) == (want, 128.0) and len(points) == 66
                elif want == "hit":
                    assert hits[k] != pc.LAST
                else:
                    assert hits[k] == want, (k, hits[k], want)
            if any(v == pc.LAST for v in named.values() if isinstance(v, str)):  # the named glyphs, and no others, get the last point
                assert {k for k, h in enumerate(hits) if h == pc.LAST} == {k for k, v in named.items() if v == pc.LAST}


def model_rows(glyphs, widths):
    """text_placer.rs:119-133 on the widths: the row starts."""
    rows, cur, start = [], 0.0, 0
    for k, w in enumerate(widths):
        cur += w
        if (glyphs["flags"][k] & 1 and cur + w > model.MAX_TEXT_WIDTH) or k + 1 == len(widths):
            rows.append(start)
            start, cur = k + 1, 0.0
    return rows


def row_sum(widths, rows, k):
    """current_row_width + w as the break test of glyph k sees it."""
    start = max(s for s in rows if s <= k)
    cur = 0.0
    for w in widths[start : k + 1]:
        cur += w
    return cur + widths[k]


def test_the_placer_cases_cover_the_shapes_the_kernel_branches_on():
    by = {c.name: c for c in PLACE}
    # one row of 63 .. 129 glyphs with kerns on lane 0 of the second and the third chunk
    one = by["center-one-row"].specs(0)
    assert [len(s["glyphs"]) for s in one] == [63, 64, 65, 127, 128, 129]
    assert all(s["glyphs"][k][2] != 0 for s in one for k in (0, 64, 128) if k < len(s["glyphs"]))
    # a space that closes the row at 62 .. 65, from both sides of the threshold: the second row starts at 63 .. 66
    for i in (62, 63, 64, 65):
        c = by[f"center-space-closes-at-{i}"]
        on, over = c.specs(0)
        assert c.claims == [dict(rows=[0]), dict(rows=[0, i + 1])]
        assert [g[3] for g in on["glyphs"]] == [0] * i + [1] + [0] * 3 and sum(pc.units(over)) == sum(pc.units(on)) + 1
    mid = by["center-rows-start-mid-chunk"]
    assert mid.claims[0]["rows"] == [0, 5, 70] and len(mid.specs(0)[0]["glyphs"]) == 200
    assert [s.get("y_offset", 0) for s in mid.specs(0)] == [0, 7]
    assert [len(c["rows"]) for c in by["center-only-spaces"].claims] == [64, 65]
    assert [(len(s["glyphs"]), s["glyphs"][-1][3]) for s in by["center-space-is-the-last-glyph"].specs(0)] == [(64, 1), (64, 1), (65, 1), (65, 1)]
    a, b = (pc.units(s) for s in by["center-widths-not-positive-at-lanes-63-64"].specs(0))
    assert (a[63] < 0, a[64] == 0, b[63] == 0, b[64] < 0) == (True,) * 4
    # ways of 64 .. 130 points; every edge has an integer length, some are 3-4-5 edges
    for ne in (63, 64, 65, 128, 129):
        spec = by[f"line-way-of-{ne}-edges"].specs(0)[0]
        lens = pc.way_lengths(spec["pts"])
        assert len(spec["pts"]) == ne + 1 and len(lens) == ne and 5 in lens and min(lens) > 0
    long = by["line-glyph-64-starts-again-at-edge-0"].specs(0)
    assert [len(s["glyphs"]) for s in long] == [65, 130] and len(long[0]["pts"]) == 131
    z = pc.way_lengths(by["line-zero-length-edges-63-64"].specs(0)[0]["pts"])
    assert [k for k, d in enumerate(z) if d == 0] == [63, 64]
    assert len(by["line-running-off-the-end-from-glyph-65"].specs(0)[0]["pts"]) > 65
    # the batch of nine: its forms in the issue's order, and the reversed pool
    nine = by["batch-of-nine"].build(0)
    forms = ["none" if not l["has_text"] else "empty" if l["n_segs"] == 0 else ("line", "center")[int(r["position"]) == abi.TEXT_CENTER]
             for l, r in zip(nine.labels, nine.runs)]
    assert forms == ["line", "none", "center", "empty", "line", "center", "line", "center", "line"]
    assert nine.runs["n_pts"][4] == 1 and nine.labels["n_segs"][5] == 130
    rev = by["batch-of-nine-reversed-pool"].build(0)
    text = rev.labels["n_segs"] > 0
    assert (np.diff(rev.labels["seg_off"][text].astype(np.int64)) < 0).all() and (np.diff(nine.labels["seg_off"][text].astype(np.int64)) > 0).all()
    for i in np.nonzero(text)[0]:
        a, b, n = int(nine.labels["seg_off"][i]), int(rev.labels["seg_off"][i]), int(nine.labels["n_segs"][i])
        assert np.array_equal(_u8(nine.glyphs[a : a + n]), _u8(rev.glyphs[b : b + n]))


# ---- shaper -----------------------------------------------------------------------------------------------------------
def _shape(case, font_class=shaper.Font):
    sl, fonts = case.build()
    return sl, shaper.shape_labels(sl, [font_class(f) for f in fonts])


@pytest.mark.parametrize("case", SHAPE, ids=[c.name for c in SHAPE])
def test_shaper_case_holds_for_the_model(case):
    sl, got = _shape(case)
    case.check(got)


def _bisect(keys, key):
    """The kernel's bisection, on a list that may not be sorted."""
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if keys[mid] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


class Key16Font(shaper.Font):
    """A font whose kern key gives each glyph index 16 bits, computed in 64 bits (or in 32: Key16In32Font); the entry found is
    compared index by index, as the kernel does."""
    MASK = (1 << 64) - 1

    def kern_advance(self, left, right):
        pairs = list(zip(self.table.kern["left"].tolist(), self.table.kern["right"].tolist()))
        i = _bisect([((l << 16) | r) & self.MASK for l, r in pairs], ((left << 16) | right) & self.MASK)
        return self.values[i] if i < len(pairs) and pairs[i] == (left, right) else 0


class Key16In32Font(Key16Font):
    MASK = (1 << 32) - 1


def test_the_shaper_cases_tell_the_bugs_they_were_built_for():
    by = {c.name: c for c in SHAPE}
    # a 16-bit kern key: the big-index font's pairs are no longer in rising order, and its text shapes differently
    keys16 = [(l << 16) | r for l, r, _ in sc.BIG_KERN]
    assert keys16 != sorted(keys16) and [(l << 32) | r for l, r, _ in sc.BIG_KERN] == sorted((l << 32) | r for l, r, _ in sc.BIG_KERN)
    assert [k & 0xFFFFFFFF for k in keys16] != sorted(k & 0xFFFFFFFF for k in keys16)
    for broken in (Key16Font, Key16In32Font):
        with pytest.raises(AssertionError):
            by["kern-tables"].check(_shape(by["kern-tables"], broken)[1])
        by["kern-label-boundary"].check(_shape(by["kern-label-boundary"], broken)[1])  # small indices: such a key is as good
    # block borders: the pool slots the case names
    for name in ("kern-at-block-borders", "kern-at-block-borders-reversed-pool"):
        sl, got = _shape(by[name])
        assert sl.labels["has_text"].tolist() == [1, 0, 1, 1, 1, 1] and sl.labels["n_segs"].tolist() == [256, 0, 0, 1, 255, 600]
    sl, got = _shape(by["kern-at-block-borders"])
    assert sl.labels["seg_off"].tolist() == [0, 0, 0, 256, 257, 512]
    c3, c5 = sc.cp(3), sc.cp(5)
    assert sl.chars[[255, 256, 257]].tolist() == [c3, c5, c3]  # 3 | 5 across slots 255 | 256, 5 | 3 across 256 | 257: both are listed pairs
    assert sl.chars[[512 + 255, 512 + 256, 512 + 511, 512 + 512]].tolist() == [c3, c5, c3, c5] and (512 + 256) % 256 == 0
    # a kern carried across label boundaries (the pool shaped as one text) differs exactly at slots 256 and 257
    leaky = shaper.shape_text(shaper.Font(by["kern-at-block-borders"].build()[1][0]), sl.chars)
    assert leaky["kern"][[256, 257]].tolist() == [-40, 9] and got["kern"][[256, 257]].tolist() == [0, 0]
    rev = by["kern-at-block-borders-reversed-pool"].build()[0]
    text = rev.labels["n_segs"] > 0
    assert (np.diff(rev.labels["seg_off"][text].astype(np.int64)) < 0).all()
    # whitespace: all 25 members, both neighbours of each, the look-alikes
    probes = by["whitespace"].build()[0].chars.tolist()
    ws = sorted(labels.WHITE_SPACE)
    assert len(ws) == 25 and all(c + d in probes for c in ws for d in (-1, 0, 1)) and all(c in probes for c in (0x1C, 0x1D, 0x1E, 0x1F, 0x180E, 0x200B, 0x2060, 0xFEFF, 0x10FFFF))
    assert 0x205F in ws
    # the reference's texts: all twelve, in one batch
    sl = by["reference-texts"].build()[0]
    assert len(sl.labels) == 12 and sl.n_jobs == 1 and len({int(r["font_size"]) for r in sl.runs}) == 3
    # every cmap size, probed below, at and above both ends
    for n in sc.CMAP_SIZES:
        p = sc.cmap_probes(n)
        first, last = 0x30, 0x30 + 3 * (n - 1)
        assert {0, first - 1, first, first + 1, last - 1, last, last + 1, 0x10FFFF} <= set(p)
        assert by[f"cmap-{n}"].build()[0].labels["n_segs"].tolist() == [len(p), n]
