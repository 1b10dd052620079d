"""String labels on the host (no GPU): TextPlacer::text_to_glyphs as the library states it.

  * the ABI structs have the header's sizes in C, ctypes and numpy;
  * pinned to the reference's font: every text of ref_text_runs.json at sizes 9 / 11 / 14, given as code points and
    shaped against ref_font_tables.json by the host mirror (osm_renderer_amd/host/osmt_textshaper.hpp, built by
    tests/shape_shim.cpp), by the Python model (tests/_text_shaper_model.py) and by labels.FontTable.shape, gives exactly
    that fixture's [glyph, advance, kern, whitespace] per char, and the scale the validation derives from the font size
    has the fixture's bits;
  * mirror == model record for record on synthetic fonts: cmaps of 1, 2, 7, 8, 9, 1024 and 1025 entries probed below,
    above, in a gap and at both ends; kern tables that are empty, hold one pair, hold the wanted pair first or last,
    with both signs, and a pair present only in the other order; every White_Space code point and both neighbours of
    each range; a kern never crosses from one label into the next;
  * make_string_labels shapes to the records of make_text_labels at the same seed;
  * every refusal of osmt_register_font and osmt_validate_string_labels, with its status and the offender named.  A
    context needs a device, so here the refusals are checked on the code the library calls (the mirror's validate_font /
    validate_string_labels); tests/test_gpu_string_labels.py runs the same list through the C ABI and osmt_last_error()."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from tests import _shape_shim
from tests import _text_shaper_model as model

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEXTS = json.load(open(os.path.join(GOLD, "ref_text_runs.json")))
RUNS = json.load(open(os.path.join(GOLD, "ref_glyph_runs.json")))
PATCHES = json.load(open(os.path.join(GOLD, "ref_label_patches.json")))
FONT = json.load(open(os.path.join(GOLD, "ref_font_tables.json")))


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def ref_font(first_id=0, empty_id=None):
    """The reference's font as a FontTable: glyph g's outline is first_id + its position in ref_glyph_runs.json's
    glyphs; the glyphs the fixture has no outline for share the empty outline empty_id (default: right behind)."""
    empty_id = first_id + len(RUNS["glyphs"]) if empty_id is None else empty_id
    outline = [empty_id if o is None else first_id + o for o in FONT["outline"]]
    a, d, g = FONT["v_metrics"]
    return labels.FontTable(FONT["cmap"], FONT["advance"], outline, FONT["kern"], a, d, g)


def string_labels(specs, n_jobs=1):
    """One tile of string labels from dicts: chars (a str or code points), font (id), font_size, position, y_offset,
    center, pts (already in walking order), has_text (default 1)."""
    labs, runs, chars, pts = [], [], [], []
    n_ch = n_pt = 0
    for s in specs:
        l, r = np.zeros((), labels.LABEL_DTYPE), np.zeros((), labels.STRING_RUN_DTYPE)
        c = s.get("chars", [])
        c = np.array([ord(ch) for ch in c] if isinstance(c, str) else list(c), dtype=np.uint32)
        l["has_text"], l["text_color"] = s.get("has_text", 1), s.get("color", (10, 20, 30))
        if "icon" in s:
            l["has_icon"], l["image_id"], l["icon_center_x"], l["icon_center_y"] = 1, s["icon"], s["center"][0], s["center"][1]
        l["seg_off"], l["n_segs"] = (n_ch if len(c) else 0), len(c)
        r["position"], r["font_id"], r["font_size"] = s.get("position", abi.TEXT_CENTER), s.get("font", 0), s.get("font_size", 11.0)
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
        chars.append(c)
        n_ch += len(c)
    way = np.concatenate(pts) if pts else np.zeros((0, 2), np.int32)
    sincos = np.concatenate([labels.way_sincos(p) for p in pts]) if pts else np.zeros((0, 2))
    offs = [0] + [len(labs)] * n_jobs
    return labels.StringLabelList(np.array(labs, dtype=labels.LABEL_DTYPE), offs, np.array(runs, dtype=labels.STRING_RUN_DTYPE),
                                  np.concatenate(chars) if chars else np.zeros(0, np.uint32), way, sincos)


def station_string_labels(key, font_id=0, image_id=0):
    """The station label of ref_label_patches.json as a string: the text, the font size, the anchor, the icon's half height."""
    p = PATCHES[key]
    return string_labels([dict(chars="Арбатская", font=font_id, font_size=RUNS[key]["font_size"], center=tuple(float(v) for v in p["icon_center"]),
                               y_offset=len(p["icon_rgba"]) // 2, icon=image_id, color=tuple(p["text_color"]))])


def both(font, chars):
    """The records of one text from the mirror, asserted equal to the model's byte for byte."""
    got, want = _shape_shim.shape_text(font, chars), model.shape_text(model.Font(font), chars)
    assert got.shape == want.shape and np.array_equal(_u8(got), _u8(want)), (got.tolist(), want.tolist())
    return got


def test_struct_sizes_in_c_ctypes_and_numpy():
    s = _shape_shim.lib().shim_shape_abi_sizeof
    assert s(0) == C.sizeof(abi.CmapEntry) == labels.CMAP_DTYPE.itemsize == 8
    assert s(1) == C.sizeof(abi.KernPair) == labels.KERN_DTYPE.itemsize == 12
    assert s(2) == C.sizeof(abi.FontDesc)
    assert s(3) == C.sizeof(abi.StringRun) == labels.STRING_RUN_DTYPE.itemsize == 64
    assert s(4) == C.sizeof(abi.StringLabelBatch)
    assert s(10) == abi.FontDesc.advance.offset and s(11) == abi.FontDesc.outline_id.offset and s(12) == abi.FontDesc.kern.offset
    assert s(13) == abi.FontDesc.ascent.offset and s(14) == abi.FontDesc.line_gap.offset
    assert s(15) == abi.StringRun.font_id.offset == labels.STRING_RUN_DTYPE.fields["font_id"][1]
    assert s(16) == abi.StringRun.font_size.offset == labels.STRING_RUN_DTYPE.fields["font_size"][1]
    assert s(17) == abi.StringRun.center_x.offset == labels.STRING_RUN_DTYPE.fields["center_x"][1]
    assert s(18) == abi.StringLabelBatch.chars.offset and s(19) == abi.StringLabelBatch.n_way_pts.offset


def test_fixture_is_data_only_and_small():
    assert set(FONT) == {"_provenance", "v_metrics", "n_glyphs", "cmap", "advance", "kern", "outline"}
    assert FONT["v_metrics"] == TEXTS["v_metrics"] == [1069, -293, 0]
    assert len(FONT["advance"]) == len(FONT["outline"]) == FONT["n_glyphs"] and FONT["kern"] == []
    cps = [c for c, _ in FONT["cmap"]]
    assert cps == sorted(set(cps)) and len(cps) > 2000
    assert sorted(o for o in FONT["outline"] if o is not None) == list(range(len(RUNS["glyphs"])))
    assert os.path.getsize(os.path.join(GOLD, "ref_font_tables.json")) < 200 * 1024
    assert _shape_shim.validate_font(ref_font(), len(RUNS["glyphs"]) + 1) == (abi.OK, "")


def test_reference_texts_shape_to_the_fixture_records():
    font = ref_font()
    mfont = model.Font(font)
    assert len(TEXTS["texts"]) == 12
    for t in TEXTS["texts"]:
        chars = [ord(ch) for ch in t["text"]]
        want = np.array([tuple(c) for c in t["chars"]], dtype=labels.TEXT_GLYPH_DTYPE)
        got = both(font, chars)
        assert np.array_equal(_u8(got), _u8(want)), t["text"]
        assert np.array_equal(_u8(font.shape(chars)), _u8(want))
        # the scale: one f32 division, widened — the mirror's, the model's, FontTable's, and the run the validation builds
        size = t["font_size"]
        assert size in (9.0, 11.0, 14.0)
        bits = np.float64(t["scale"]).view(np.uint64)
        sl = string_labels([dict(chars=chars, font_size=size)])
        rc, why, runs = _shape_shim.validate(sl, [font], want_runs=True)
        assert (rc, why) == (abi.OK, "")
        for v in (_shape_shim.string_scale(font, size), mfont.scale(size), font.scale(size), runs["scale"][0]):
            assert np.float64(v).view(np.uint64) == bits
        assert (int(runs["ascent"][0]), int(runs["descent"][0]), int(runs["line_gap"][0])) == tuple(TEXTS["v_metrics"])
        # and the records of the whole batch sit in the label's slots
        assert np.array_equal(_u8(_shape_shim.shape_labels(sl, [font])), _u8(want))


def synth_font(n_cmap, kern=(), first_cp=0x30, step=3, n_glyphs=None):
    """n_cmap code points first_cp, first_cp + step, ... (gaps between them) -> glyphs 1, 2, ... cycling through n_glyphs
    - 1 glyphs; glyph g has advance 100 + 7 g and outline 1000 + g."""
    n_glyphs = n_glyphs or min(n_cmap + 1, 40)
    cmap = [(first_cp + step * i, 1 + i % (n_glyphs - 1)) for i in range(n_cmap)]
    return labels.FontTable(cmap, [100 + 7 * g for g in range(n_glyphs)], [1000 + g for g in range(n_glyphs)], kern)


@pytest.mark.parametrize("n_cmap", [1, 2, 7, 8, 9, 1024, 1025])
def test_cmap_bisection_at_every_size_and_position(n_cmap):
    font = synth_font(n_cmap)
    first, last = 0x30, 0x30 + 3 * (n_cmap - 1)
    probes = [0, first - 1, first, first + 1, last - 1, last, last + 1, last + 2, 0x10FFFF, 0xD7FF, 0xE000]
    probes += [first + 3 * i + d for i in range(0, n_cmap, max(1, n_cmap // 50)) for d in (0, 1, 2)]  # entries and the gaps behind them
    got = both(font, probes)
    listed = dict(font.cmap.tolist())
    assert got["glyph_id"].tolist() == [1000 + listed.get(p, 0) for p in probes]
    assert got["advance"].tolist() == [100 + 7 * listed.get(p, 0) for p in probes]
    assert got["glyph_id"][2] != 1000 and got["glyph_id"][5] != 1000 and got["glyph_id"][0] == got["glyph_id"][1] == got["glyph_id"][6] == 1000
    # every entry of the table, in one text
    all_cps = font.cmap["code_point"].tolist()
    assert both(font, all_cps)["glyph_id"].tolist() == [1000 + g for g in font.cmap["glyph"].tolist()]


def test_kern_tables_empty_one_pair_first_last_signs_and_order():
    cp = lambda g: 0x30 + 3 * (g - 1)  # the code point of glyph g in synth_font (g >= 1)
    text = [cp(3), cp(5), cp(3), cp(5), cp(9)]  # pairs (3, 5), (5, 3), (3, 5), (5, 9)
    assert both(synth_font(20), text)["kern"].tolist() == [0, 0, 0, 0, 0]  # no kern table
    assert both(synth_font(20, [(3, 5, -40)]), text)["kern"].tolist() == [0, -40, 0, -40, 0]  # one pair
    assert both(synth_font(20, [(5, 3, 25)]), text)["kern"].tolist() == [0, 0, 25, 0, 0]  # only the other order is listed
    many = [(l, r, 10 * l - r) for l in range(1, 20) for r in range(1, 20) if (l, r) not in ((3, 5), (5, 3), (5, 9))]
    assert both(synth_font(20, many), text)["kern"].tolist() == [0, 0, 0, 0, 0]  # everything but the wanted pairs
    firstp = [(3, 5, 33)] + [(l, r, 1) for l in range(4, 20) for r in range(1, 20)]
    assert both(synth_font(20, firstp), text)["kern"].tolist() == [0, 33, 1, 33, 1]  # the wanted pair is the first entry
    lastp = [(l, r, -1) for l in range(1, 3) for r in range(1, 20)] + [(3, 5, -65535)]
    assert both(synth_font(20, lastp), text)["kern"].tolist() == [0, -65535, 0, -65535, 0]  # ... the last entry
    # the first glyph has no kern even when (glyph 0, g) and (g, g) are listed; a missing code point is glyph 0 and pairs as such
    zero = [(0, 0, 7), (0, 3, 11), (3, 0, -13), (3, 3, 17)]
    got = both(synth_font(20, zero), [cp(3), cp(3), 0x10FFFF, 0x10FFFF, cp(3)])
    assert got["kern"].tolist() == [0, 17, -13, 7, 11] and got["glyph_id"].tolist() == [1003, 1003, 1000, 1000, 1003]
    # left and right glyph indices beyond 16 bits keep their order in the key
    big = labels.FontTable([(0x41, 70000), (0x42, 2), (0x43, 65536)], [5] * 70001, [9] * 70001, [(2, 70000, 4), (65536, 65536, 9), (70000, 2, -4)])
    assert _shape_shim.validate_font(big, 10) == (abi.OK, "")
    assert both(big, [0x41, 0x42, 0x41, 0x43, 0x43])["kern"].tolist() == [0, -4, 4, 0, 9]


def test_whitespace_is_rusts_not_isspace():
    ws = sorted(labels.WHITE_SPACE)
    assert len(ws) == 25 and ws == [cp for cp in range(0x3002) if model.is_whitespace(cp)]
    probes = sorted(set(ws) | {cp + d for cp in ws for d in (-1, 1)} | {0x1C, 0x1D, 0x1E, 0x1F, 0x180E, 0x200B, 0xFEFF, 0x2060, 0x10FFFF})
    font = synth_font(9)
    got = both(font, probes)
    assert got["flags"].tolist() == [1 if p in labels.WHITE_SPACE else 0 for p in probes]
    assert [p for p, f in zip(probes, got["flags"]) if f] == ws
    # Python's idea differs exactly where the issue says it does
    assert all(chr(c).isspace() for c in (0x1C, 0x1D, 0x1E, 0x1F)) and not any(c in labels.WHITE_SPACE for c in (0x1C, 0x1F, 0x180E, 0x200B, 0xFEFF))
    assert np.array_equal(_u8(font.shape(probes)), _u8(got))


def test_a_kern_never_crosses_from_one_label_into_the_next():
    cp = lambda g: 0x30 + 3 * (g - 1)
    fonts = [synth_font(20, [(3, 5, -40), (5, 3, 9)]), synth_font(20, [(3, 5, 77)], first_cp=0x30 - 3)]  # font 1: the same code point is another glyph
    fonts[1].font_id = 1
    sl = string_labels([dict(chars=[cp(3), cp(5), cp(3)]), dict(chars=[cp(5), cp(3)]), dict(has_text=0), dict(chars=[]),
                        dict(chars=[cp(5), cp(2), cp(4)], font=1), dict(chars=[cp(5)])])
    assert _shape_shim.validate(sl, fonts) == (abi.OK, "")
    got = _shape_shim.shape_labels(sl, fonts)
    want = model.shape_labels(sl, [model.Font(f) for f in fonts])
    assert np.array_equal(_u8(got), _u8(want))
    # the first char of label 1 sits behind a 3 | 5 boundary (-40 if the pool's neighbour leaked in); in font 1 the chars of
    # label 4 are glyphs 6, 3, 5
    assert got["kern"].tolist() == [0, -40, 9, 0, 9, 0, 0, 77, 0]
    assert got["glyph_id"][5] == 1006 and got["glyph_id"][3] == 1005  # cp(5) is glyph 6 in font 1
    tl = sl.to_text_label_list(fonts)
    assert np.array_equal(_u8(tl.glyphs), _u8(got))


def test_make_string_labels_is_make_text_labels():
    tab = labels.synth_glyph_table()
    tab.first_id = 130
    kw = dict(seed=11, n_images=3, image_sizes=[(16, 16), (12, 20), (5, 7)], line_frac=0.4, empty_frac=0.05)
    for scale in (1, 2):
        sl, font = labels.make_string_labels(40, tab, scale=scale, **kw)
        font.font_id = 3
        sl.with_font(font)
        fonts = [font] * 4
        assert _shape_shim.validate_font(font, 130 + len(labels.SYNTH_GLYPHS)) == (abi.OK, "")
        rc, why, runs = _shape_shim.validate(sl, fonts, want_runs=True)
        assert (rc, why) == (abi.OK, "")
        tl = labels.make_text_labels(40, tab, scale=scale, f32_scale=True, **kw)
        text = tl.labels["has_text"] == 1
        assert np.array_equal(_u8(sl.labels), _u8(tl.labels)) and np.array_equal(_u8(runs[text]), _u8(tl.runs[text]))
        got = _shape_shim.shape_labels(sl, fonts)
        assert np.array_equal(_u8(got), _u8(tl.glyphs)) and (got["kern"] != 0).sum() > 100 and (got["flags"] == 1).sum() > 100
        assert np.array_equal(_u8(model.shape_labels(sl, [model.Font(font)] * 4)), _u8(tl.glyphs))
        back = sl.to_text_label_list(font)
        for name in ("labels", "runs", "glyphs", "way_pts", "way_sincos", "job_label_off"):
            assert np.array_equal(_u8(getattr(back, name)), _u8(getattr(tl, name))), name
        # the plain workload differs from the f32_scale one in the scale only
        plain = labels.make_text_labels(40, tab, scale=scale, **kw)
        assert np.array_equal(_u8(plain.glyphs), _u8(tl.glyphs)) and not np.array_equal(plain.runs["scale"], tl.runs["scale"])
        sub = [7, 2, 30]
        assert np.array_equal(_u8(sl.subset(sub).to_text_label_list(font).glyphs), _u8(tl.subset(sub).glyphs))
        assert sl.input_bytes() == tl.input_bytes() - 12 * len(tl.glyphs)


# ---- refusals: (status, a word of the reason that names the offender, edit) --------------------------------------------
N_OUTLINES = 1040  # synth_font's outline ids are 1000 + g: a glyph table of at least 1020 outlines


def valid_font():
    return synth_font(20, [(1, 2, 5), (2, 1, -5), (7, 7, 1)], n_glyphs=20)


def _null(field):
    def edit(font, desc, n):
        setattr(desc, field, None)
    return edit


FONT_REFUSALS = [
    ("NULL", _null("cmap")),
    ("NULL", _null("advance")),
    ("NULL", _null("outline_id")),
    ("NULL", _null("kern")),
    ("n_glyphs == 0", lambda f, d, n: setattr(d, "n_glyphs", 0)),
    ("cmap entry 4: code points are not strictly increasing", lambda f, d, n: f.cmap["code_point"].__setitem__(4, f.cmap["code_point"][3])),
    ("cmap entry 5: code points are not strictly increasing", lambda f, d, n: f.cmap["code_point"].__setitem__(5, 1)),
    ("cmap entry 6: glyph 20 >= n_glyphs", lambda f, d, n: f.cmap["glyph"].__setitem__(6, 20)),
    ("cmap entry 19: U+110000", lambda f, d, n: f.cmap["code_point"].__setitem__(19, 0x110000)),
    ("cmap entry 19: U+D800", lambda f, d, n: f.cmap["code_point"].__setitem__(19, 0xD800)),
    ("cmap entry 19: U+DFFF", lambda f, d, n: f.cmap["code_point"].__setitem__(19, 0xDFFF)),
    ("glyph 3: |advance| > 65535", lambda f, d, n: f.advance.__setitem__(3, 65536)),
    ("glyph 0: |advance| > 65535", lambda f, d, n: f.advance.__setitem__(0, -65536)),
    ("glyph 9: outline id {n} is not in the glyph table ({n} glyphs)", lambda f, d, n: f.outline_id.__setitem__(9, n)),
    ("kern pair 1: (left, right) is not strictly increasing", lambda f, d, n: f.kern.__setitem__(1, (1, 2, 6))),
    ("kern pair 2: (left, right) is not strictly increasing", lambda f, d, n: f.kern.__setitem__(2, (2, 0, 6))),
    ("kern pair 2: glyph (20, 1)", lambda f, d, n: f.kern.__setitem__(2, (20, 1, 6))),
    ("kern pair 2: glyph (7, 20)", lambda f, d, n: f.kern.__setitem__(2, (7, 20, 6))),
    ("kern pair 0: |value| > 65535", lambda f, d, n: f.kern["value"].__setitem__(0, 65536)),
    ("kern pair 2: |value| > 65535", lambda f, d, n: f.kern["value"].__setitem__(2, -65536)),
    ("ascent - descent == 0", lambda f, d, n: setattr(d, "descent", d.ascent)),
]


def refused_font(edit, n_outlines=N_OUTLINES):
    """(FontTable, its abi.FontDesc) after `edit`; n_outlines: the size of the glyph table it will be checked against."""
    font = valid_font()
    desc, _ = font.as_desc()
    edit(font, desc, n_outlines)
    return font, desc


def valid_strings():
    way = [(0, 0), (60, 10), (90, 40)]
    return string_labels([dict(chars=[0x30, 0x33, 0x20, 0x36], font_size=11.0), dict(chars=[0x39, 0x3C], position=abi.TEXT_LINE, pts=way, font=1),
                          dict(has_text=0), dict(chars=[], font_size=9.0)])


LABEL_REFUSALS = [
    (abi.INVALID_ARG, "label 1: font id 2 is not registered (2 fonts)", lambda sl: sl.runs["font_id"].__setitem__(1, 2)),
    (abi.INVALID_ARG, "label 0, char 1: U+D800", lambda sl: sl.chars.__setitem__(1, 0xD800)),
    (abi.INVALID_ARG, "label 1, char 1: U+DFFF", lambda sl: sl.chars.__setitem__(5, 0xDFFF)),
    (abi.INVALID_ARG, "label 0, char 3: U+110000", lambda sl: sl.chars.__setitem__(3, 0x110000)),
    (abi.INVALID_ARG, "label 0: font_size is not finite", lambda sl: sl.runs["font_size"].__setitem__(0, np.nan)),
    (abi.INVALID_ARG, "label 3: font_size is not finite", lambda sl: sl.runs["font_size"].__setitem__(3, np.inf)),
    (abi.INVALID_ARG, "label 1: the scale of font_size 1e+300 is not finite", lambda sl: sl.runs["font_size"].__setitem__(1, 1e300)),
    # what osmt_validate_text_labels checks, on the string batch
    (abi.INVALID_ARG, "label 1: char range", lambda sl: sl.labels["n_segs"].__setitem__(1, 3)),
    (abi.INVALID_ARG, "overlap", lambda sl: sl.labels["seg_off"].__setitem__(1, 3)),
    (abi.INVALID_ARG, "label 1: way point range", lambda sl: sl.runs["n_pts"].__setitem__(1, 4)),
    (abi.INVALID_ARG, "label 0: unknown text position 7", lambda sl: sl.runs["position"].__setitem__(0, 7)),
    (abi.INVALID_ARG, "label 0: y_offset", lambda sl: sl.runs["y_offset"].__setitem__(0, 2**20 + 1)),
    (abi.INVALID_ARG, "label 0: centre", lambda sl: sl.runs["center_x"].__setitem__(0, np.nan)),
    (abi.INVALID_ARG, "label 3: centre", lambda sl: sl.runs["center_y"].__setitem__(3, 2.0**20 + 1)),
    (abi.INVALID_ARG, "label 1: way_sincos of edge 1", lambda sl: sl.way_sincos.__setitem__((1, 0), np.inf)),
    (abi.UNSUPPORTED, "label 1: way point 2 has |v| > 2^28", lambda sl: sl.way_pts.__setitem__((2, 1), 2**28 + 1)),
    (abi.INVALID_ARG, "job_label_off", lambda sl: sl.job_label_off.__setitem__(1, 3)),
]


def test_font_refusals_name_the_offender():
    assert _shape_shim.validate_font(valid_font(), N_OUTLINES) == (abi.OK, "")
    for word, edit in FONT_REFUSALS:
        font, desc = refused_font(edit)
        rc, why = _shape_shim.validate_font(desc, N_OUTLINES)
        assert rc == abi.INVALID_ARG and word.format(n=N_OUTLINES) in why, (word, rc, why)
    # legal: no kern pairs (NULL table), no cmap at all (every char is glyph 0), the limits themselves
    font, desc = refused_font(lambda f, d, n: (setattr(d, "kern", None), setattr(d, "n_kern", 0)))
    assert _shape_shim.validate_font(desc, N_OUTLINES)[0] == abi.OK
    font, desc = refused_font(lambda f, d, n: (setattr(d, "cmap", None), setattr(d, "n_cmap", 0)))
    assert _shape_shim.validate_font(desc, N_OUTLINES)[0] == abi.OK
    font, desc = refused_font(lambda f, d, n: (f.advance.__setitem__(3, -65535), f.kern["value"].__setitem__(0, 65535), f.cmap["code_point"].__setitem__(19, 0x10FFFF)))
    assert _shape_shim.validate_font(desc, N_OUTLINES)[0] == abi.OK


def test_string_label_refusals_name_the_offender():
    fonts = [valid_font(), valid_font()]
    assert _shape_shim.validate(valid_strings(), fonts) == (abi.OK, "")
    for code, word, edit in LABEL_REFUSALS:
        sl = valid_strings()
        edit(sl)
        rc, why = _shape_shim.validate(sl, fonts)
        assert rc == code and word in why, (word, rc, why)
    for field in ("labels", "job_label_off", "runs", "chars", "way_pts", "way_sincos"):
        sl = valid_strings()
        b = sl.as_batch()
        setattr(b, field, None)
        arr, _keep = _shape_shim._font_array(fonts)
        why = C.create_string_buffer(256)
        assert _shape_shim.lib().shim_string_validate(C.byref(b), 1, arr, 2, why, 256, None) == abi.INVALID_ARG and b"NULL" in why.value, field
    # not errors: a code point the font does not have, a label without text whose run is garbage, the last valid chars
    sl = valid_strings()
    sl.chars[:] = [0x10FFFF, 0xD7FF, 0xE000, 0x31, 0x0, 0x2FFFF]
    sl.runs["font_id"][2], sl.runs["font_size"][2], sl.runs["position"][2] = 99, np.nan, 9
    assert _shape_shim.validate(sl, fonts) == (abi.OK, "")
    assert _shape_shim.shape_labels(sl, fonts)["glyph_id"].tolist() == [1000] * 6
    # an empty batch is fine without fonts
    assert _shape_shim.validate(string_labels([]), []) == (abi.OK, "")
