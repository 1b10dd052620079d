"""Text-run labels on the host (no GPU): TextPlacer::place as the library states it.

  * the ABI structs have the header's sizes in C, ctypes and numpy;
  * the host mirror (osm_renderer_amd/host/osmt_textplacer.hpp, built by tests/text_shim.cpp) and the Python model
    (tests/_text_placer_model.py) lay the reference's station text out with x_offset / baseline equal AS BITS to
    tests/golden/ref_glyph_runs.json — the values whose expansion reproduces the reference's golden label pixels;
  * the row counts of the fixture's texts (checked with the reference's font when the fixture was made);
  * mirror == model bit for bit on > 20 000 seeded labels and on the directed cases of tests/_text_place_cases.py, which
    the device test (tests/test_gpu_text_edges.py) runs as well: the 32.0 threshold from both sides, trailing and only
    whitespace, y_offset, widths <= 0, zero-length edges, a text exactly as long as its way and one ulp longer, the
    advance <= 0 quirk, running off the end, ways of one point and none — and the same edges at lanes 63 / 64 and at
    the first lane of a later chunk of glyphs or edges; each case brings its literal expectations;
  * every refusal of osmt_validate_text_labels, with its status."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib
from tests import _text_place_cases as pc
from tests import _text_placer_model as model
from tests import _text_shim
from tests._text_place_cases import A, B, S64, SP, text_labels  # noqa: F401  (other test files import them from here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEXTS = json.load(open(os.path.join(GOLD, "ref_text_runs.json")))
RUNS = json.load(open(os.path.join(GOLD, "ref_glyph_runs.json")))
PATCHES = json.load(open(os.path.join(GOLD, "ref_label_patches.json")))


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def fixture_text(text, size):
    return next(t for t in TEXTS["texts"] if t["text"] == text and t["font_size"] == size)


def fixture_spec(text, size, first_id=0, **kw):
    t = fixture_text(text, size)
    return dict(glyphs=[(first_id + c[0], c[1], c[2], c[3]) for c in t["chars"]], scale=t["scale"], metrics=tuple(TEXTS["v_metrics"]), **kw)


def station_text_labels(key, first_id=0, image_id=0):
    """The station label of ref_label_patches.json as a text run: the text, the anchor, the icon's half height."""
    p = PATCHES[key]
    size = RUNS[key]["font_size"]
    return text_labels([fixture_spec("Арбатская", size, first_id, center=tuple(float(v) for v in p["icon_center"]),
                                     y_offset=len(p["icon_rgba"]) // 2, icon=image_id, color=tuple(p["text_color"]))])


def both(tl):
    """(mirror slots, model GlyphLabelList), asserted equal bit for bit."""
    assert _text_shim.validate(tl) == (abi.OK, "")
    got, gl = _text_shim.place(tl), model.place_text_labels(tl)
    assert got.shape == gl.slots.shape and np.array_equal(_u8(got), _u8(gl.slots))
    return got, gl


def test_struct_sizes_in_c_ctypes_and_numpy():
    s = _text_shim.lib().shim_text_abi_sizeof
    assert s(0) == C.sizeof(abi.TextGlyph) == labels.TEXT_GLYPH_DTYPE.itemsize == 16
    assert s(1) == C.sizeof(abi.TextRun) == labels.TEXT_RUN_DTYPE.itemsize == 64
    assert s(2) == C.sizeof(abi.TextLabelBatch)
    assert s(10) == abi.TextGlyph.kern.offset == labels.TEXT_GLYPH_DTYPE.fields["kern"][1]
    assert s(11) == abi.TextGlyph.flags.offset == labels.TEXT_GLYPH_DTYPE.fields["flags"][1]
    assert s(12) == abi.TextRun.scale.offset == labels.TEXT_RUN_DTYPE.fields["scale"][1]
    assert s(13) == abi.TextRun.ascent.offset == labels.TEXT_RUN_DTYPE.fields["ascent"][1]
    assert s(14) == abi.TextRun.center_x.offset == labels.TEXT_RUN_DTYPE.fields["center_x"][1]
    assert s(15) == abi.TextLabelBatch.runs.offset
    assert s(16) == abi.TextLabelBatch.way_pts.offset
    assert s(17) == abi.TextLabelBatch.n_way_pts.offset
    assert (s(20), s(21), s(22)) == (abi.TEXT_CENTER, abi.TEXT_LINE, abi.GLYPH_NONE)


@pytest.mark.parametrize("key", ["station", "station_z14_from_the_tile_above"])
def test_station_text_is_placed_where_the_reference_fixture_has_it(key):
    got, gl = both(station_text_labels(key))
    want = RUNS[key]
    assert len(got) == len(want["glyphs"]) == 9 and (got["form"] == abi.GLYPH_CENTER).all()
    assert np.array_equal(got["scale"].view(np.uint64), np.full(9, want["scale"]).view(np.uint64))
    assert got["glyph_id"].tolist() == [g["glyph"] for g in want["glyphs"]]
    for name, k in (("x_offset", 0), ("baseline", 1)):
        w = np.array([g[name] for g in want["glyphs"]], dtype=np.float64)
        assert np.array_equal(got["p"][:, k].view(np.uint64), w.view(np.uint64)), name
    assert np.array_equal(_u8(gl.glyphs), _u8(got)) and gl.labels["n_segs"].tolist() == [9]


def test_fixture_row_counts():
    assert TEXTS["v_metrics"] == [1069, -293, 0]
    want = {"Арбатская": (1, 1, 1), "Улица Новый Арбат": (2, 2, 3)}
    seen = 0
    for t in TEXTS["texts"]:
        tl = text_labels([fixture_spec(t["text"], t["font_size"])])
        got, gl = both(tl)
        rows = len(np.unique(got["p"][:, 1]))
        assert rows == t["rows"] == model.row_count(tl.runs[0], tl.glyphs)
        assert all(c[2] == 0 for c in t["chars"])  # this font has no kern pairs: non-zero kerns are synthetic only
        if t["text"] in want:
            assert rows == want[t["text"]][[9.0, 11.0, 14.0].index(t["font_size"])]
            seen += 1
    assert seen == 6 and len(TEXTS["texts"]) == 12
    assert os.path.getsize(os.path.join(GOLD, "ref_text_runs.json")) < 200 * 1024


def test_mirror_equals_model_on_twenty_thousand_seeded_labels():
    table = labels.synth_glyph_table()
    sizes = [(16, 16), (12, 20), (5, 7)]
    n = 0
    seen = set()
    for scale, seed, tiles in ((1, 11, 300), (2, 12, 300), (1, 13, 300)):
        tl = labels.make_text_labels(tiles, table, labels_per_tile=24, scale=scale, seed=seed, n_images=3, image_sizes=sizes, line_frac=0.4)
        got, gl = both(tl)
        n += len(tl.labels)
        seen |= set(np.unique(got["form"]).tolist())
        text = tl.labels["has_text"] == 1
        assert (tl.glyphs["kern"] != 0).any() and (tl.runs["y_offset"][text] > 0).any() and (tl.labels["n_segs"][text] == 0).any()
        center = text & (tl.runs["position"] == abi.TEXT_CENTER) & (tl.labels["n_segs"] > 0)
        rows = [len(np.unique(got["p"][int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"]), 1])) for l in tl.labels[center]]
        assert max(rows) >= 3 and min(rows) == 1  # texts that wrap
        line = text & (tl.runs["position"] == abi.TEXT_LINE)
        assert tl.runs["n_pts"][line].max() == 40 and (tl.runs["n_pts"][line] < 2).any()
        # the model's packed list drops exactly the skipped labels' instances
        assert len(gl.glyphs) == int((got["form"] != abi.GLYPH_NONE).sum())
    assert n >= 20_000 and seen == {abi.GLYPH_CENTER, abi.GLYPH_LINE, abi.GLYPH_NONE}


def run_case(name):
    """One case of tests/_text_place_cases.py: the mirror equals the model byte for byte, and both hold the case's
    literal expectations."""
    case = pc.case(name)
    got, gl = both(case.build(0))
    case.check(got, gl)
    case.check(gl.slots, gl)


def test_row_break_at_exactly_the_threshold_from_both_sides():
    run_case("break-threshold")


def test_whitespace_edge_cases_and_y_offset():
    run_case("whitespace-and-y-offset")
    run_case("empty-label-first")


def test_widths_that_are_not_positive():
    run_case("widths-not-positive")


def test_line_with_zero_length_edges_and_bends():
    run_case("line-zero-length-edges-and-bends")


def test_text_exactly_as_long_as_the_way_and_one_ulp_longer():
    run_case("line-exactly-as-long-as-the-way")
    run_case("line-one-ulp-longer-than-the-way")


def test_advance_not_positive_returns_the_last_point():
    run_case("line-advance-not-positive")


def test_running_off_the_end_returns_the_last_point():
    run_case("line-running-off-the-end")


def test_ways_of_one_point_and_of_none_place_nothing():
    run_case("line-ways-of-one-point-and-of-none")


NEW = [c.name for c in pc.cases() if c.name not in pc.OLD]


@pytest.mark.parametrize("name", NEW)
def test_cases_at_wave_and_chunk_edges(name):
    run_case(name)


def test_every_case_in_one_batch():
    """All cases as one tile (what the device test uploads in one call): the slots of every case hold what they held alone."""
    tl, spans = pc.merge([c.build(0) for c in pc.cases()])
    got, gl = both(tl)
    for c, (a, n) in zip(pc.cases(), spans):
        c.check(got[a : a + n])


def test_a_long_text_and_a_long_way():
    rng = np.random.default_rng(5)
    g = [(int(rng.integers(0, 4)), int(rng.integers(200, 700)), int(rng.integers(-50, 50)), 0) if k % 7 else (SP, 260, 0, 1) for k in range(1, 301)]
    got, _ = both(text_labels([dict(glyphs=g, scale=0.011)]))
    assert len(np.unique(got["p"][:, 1])) > 5
    pts = np.cumsum(rng.integers(-3, 8, size=(5000, 2)), axis=0).astype(np.int32)
    got, _ = both(text_labels([dict(glyphs=g, position=abi.TEXT_LINE, pts=labels.walking_order(pts).tolist(), scale=0.011)]))
    assert (got["form"] == abi.GLYPH_LINE).all() and len(np.unique(got["p"][:, 2])) > 50


def _c_validate(tl, n_jobs=None):
    L = lib.load()
    b = tl.as_batch()
    rc = L.osmt_validate_text_labels(C.byref(b), tl.n_jobs if n_jobs is None else n_jobs)
    return rc, L.osmt_last_error().decode()


def _valid():
    g = [(A, 640, 0, 0), (SP, 260, 3, 1), (B, 640, -4, 0)]
    return text_labels([dict(glyphs=g, y_offset=4), dict(glyphs=g, position=abi.TEXT_LINE, pts=[(0, 0), (10, 5), (90, 5)]), dict(glyphs=[])])


def test_validation_refuses_what_the_header_lists():
    table = labels.synth_glyph_table()
    for tl in (_valid(), labels.make_text_labels(4, table, seed=3)):
        assert _c_validate(tl) == (abi.OK, _c_validate(tl)[1]) and _text_shim.validate(tl)[0] == abi.OK

    def refuse(code, word, edit, n_jobs=None):
        tl = _valid()
        edit(tl)
        for rc, msg in (_c_validate(tl, n_jobs), _text_shim.validate(tl, n_jobs)):
            assert rc == code and word in msg, (rc, msg, word)

    for field in ("labels", "job_label_off", "runs", "glyphs", "way_pts", "way_sincos"):
        tl = _valid()
        L, b = lib.load(), tl.as_batch()
        setattr(b, field, None)
        assert L.osmt_validate_text_labels(C.byref(b), tl.n_jobs) == abi.INVALID_ARG and b"NULL" in L.osmt_last_error(), field
    refuse(abi.INVALID_ARG, "glyph range", lambda tl: tl.labels["n_segs"].__setitem__(1, 4))
    refuse(abi.INVALID_ARG, "glyph range", lambda tl: tl.labels["seg_off"].__setitem__(0, 4))
    refuse(abi.INVALID_ARG, "overlap", lambda tl: tl.labels["seg_off"].__setitem__(1, 2))
    refuse(abi.INVALID_ARG, "way point range", lambda tl: tl.runs["n_pts"].__setitem__(1, 4))
    refuse(abi.INVALID_ARG, "way point range", lambda tl: tl.runs["pt_off"].__setitem__(1, 1))
    refuse(abi.INVALID_ARG, "job_label_off", lambda tl: tl.job_label_off.__setitem__(1, 2))
    refuse(abi.INVALID_ARG, "job_label_off", lambda tl: None, n_jobs=2)
    refuse(abi.INVALID_ARG, "position", lambda tl: tl.runs["position"].__setitem__(0, 2))
    for bad in (np.nan, np.inf, -np.inf):
        refuse(abi.INVALID_ARG, "scale", lambda tl: tl.runs["scale"].__setitem__(1, bad))
        refuse(abi.INVALID_ARG, "centre", lambda tl: tl.runs["center_x"].__setitem__(0, bad))
        refuse(abi.INVALID_ARG, "centre", lambda tl: tl.runs["center_y"].__setitem__(0, bad))
        refuse(abi.INVALID_ARG, "way_sincos", lambda tl: tl.way_sincos.__setitem__((1, 0), bad))
        refuse(abi.INVALID_ARG, "way_sincos", lambda tl: tl.way_sincos.__setitem__((0, 1), bad))
    for v in (65536, -65536):
        refuse(abi.INVALID_ARG, "65535", lambda tl: tl.glyphs["advance"].__setitem__(4, v))
        refuse(abi.INVALID_ARG, "65535", lambda tl: tl.glyphs["kern"].__setitem__(0, v))
    refuse(abi.INVALID_ARG, "y_offset", lambda tl: tl.runs["y_offset"].__setitem__(0, 2**20 + 1))
    refuse(abi.INVALID_ARG, "centre", lambda tl: tl.runs["center_x"].__setitem__(0, 2.0**20 + 1))
    refuse(abi.INVALID_ARG, "centre", lambda tl: tl.runs["center_y"].__setitem__(0, -(2.0**20) - 1))
    for v in (2**28 + 1, -(2**28) - 1):
        refuse(abi.UNSUPPORTED, "2^28", lambda tl: tl.way_pts.__setitem__((2, 1), v))
    # at the limits, and where nothing is read: legal
    tl = _valid()
    tl.glyphs["advance"][0], tl.glyphs["kern"][1], tl.runs["y_offset"][0], tl.runs["center_x"][0] = 65535, -65535, 2**20, -(2.0**20)
    tl.way_pts[0] = (2**28, -(2**28))
    tl.way_sincos[2] = np.nan  # the last entry of a label's range is unused
    tl.runs["center_x"][1] = np.nan  # a LINE run's centre is not read
    assert _c_validate(tl)[0] == abi.OK and _text_shim.validate(tl)[0] == abi.OK
    tl = _valid()
    tl.labels["has_text"][1] = 0  # a label without text: its run is not looked at
    tl.runs["position"][1], tl.runs["scale"][1] = 9, np.nan
    assert _c_validate(tl)[0] == abi.OK
    assert lib.load().osmt_validate_text_labels(None, 0) == abi.INVALID_ARG
