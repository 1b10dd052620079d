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
from tests import _text_shape_cases as sc
from tests import _text_shaper_model as model
from tests._text_shape_cases import FONT, RUNS, TEXTS, ref_font, string_labels, synth_font  # noqa: F401  (other test files import them from here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PATCHES = json.load(open(os.path.join(GOLD, "ref_label_patches.json")))


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


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


def run_case(name):
    """One case of tests/_text_shape_cases.py: the batch is valid, the mirror equals the model byte for byte — on the whole
    batch and text by text —, FontTable.shape gives the same records, and they hold the case's literal expectations.
    Returns (records, StringLabelList, fonts)."""
    case = sc.case(name)
    sl, fonts = case.build()
    assert _shape_shim.validate(sl, fonts) == (abi.OK, "")
    got = _shape_shim.shape_labels(sl, fonts)
    want = model.shape_labels(sl, [model.Font(f) for f in fonts])
    assert got.shape == want.shape and np.array_equal(_u8(got), _u8(want))
    for l, r in zip(sl.labels, sl.runs):
        if l["has_text"] and l["n_segs"]:
            a, n = int(l["seg_off"]), int(l["n_segs"])
            assert np.array_equal(_u8(both(fonts[int(r["font_id"])], sl.chars[a : a + n])), _u8(got[a : a + n]))
    assert np.array_equal(_u8(sl.to_text_label_list(fonts).glyphs), _u8(got))
    case.check(got)
    case.check(want)
    return got, sl, fonts


@pytest.mark.parametrize("n_cmap", sc.CMAP_SIZES)
def test_cmap_bisection_at_every_size_and_position(n_cmap):
    assert sc.CMAP_SIZES == (1, 2, 7, 8, 9, 1024, 1025)
    run_case(f"cmap-{n_cmap}")


def test_kern_tables_empty_one_pair_first_last_signs_and_order():
    run_case("kern-tables")
    assert _shape_shim.validate_font(sc.big_font(9), 10) == (abi.OK, "")


def test_whitespace_is_rusts_not_isspace():
    ws = sorted(labels.WHITE_SPACE)
    assert len(ws) == 25 and ws == [cp for cp in range(0x3002) if model.is_whitespace(cp)]
    got, sl, fonts = run_case("whitespace")
    assert sl.chars.tolist() == sorted(set(ws) | {cp + d for cp in ws for d in (-1, 1)} | {0x1C, 0x1D, 0x1E, 0x1F, 0x180E, 0x200B, 0xFEFF, 0x2060, 0x10FFFF})
    # Python's idea differs exactly where the issue says it does
    assert all(chr(c).isspace() for c in (0x1C, 0x1D, 0x1E, 0x1F)) and not any(c in labels.WHITE_SPACE for c in (0x1C, 0x1F, 0x180E, 0x200B, 0xFEFF))
    assert np.array_equal(_u8(fonts[0].shape(sl.chars)), _u8(got))


def test_a_kern_never_crosses_from_one_label_into_the_next():
    run_case("kern-label-boundary")


NEW = ["kern-at-block-borders", "kern-at-block-borders-reversed-pool", "reference-texts"]


@pytest.mark.parametrize("name", NEW)
def test_cases_at_block_borders_and_the_reference_texts_in_one_batch(name):
    assert {c.name for c in sc.cases()} == {f"cmap-{n}" for n in sc.CMAP_SIZES} | {"kern-tables", "whitespace", "kern-label-boundary"} | set(NEW)
    run_case(name)


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
