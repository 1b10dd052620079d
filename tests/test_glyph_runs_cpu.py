"""Glyph-run labels on the host (no GPU): the new contract pinned to the reference-derived data, the host build of the
device walk against the host twin, and the ABI layouts.

  * GlyphLabelList.to_label_list() on the station label of tests/golden/ref_glyph_runs.json (the reference's font,
    TextPlacer::place's center layout) returns exactly the draw_line calls of ref_label_patches.json at z17 and z14;
  * osmt_glyph.h's walk (compiled for the host by tests/glyph_shim.cpp) produces the same calls in the same order for
    the station and for random center- and line-form runs;
  * the struct layouts agree between the header, ctypes and numpy."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from tests import _glyph_shim

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RUNS = json.load(open(os.path.join(GOLD, "ref_glyph_runs.json")))
PATCHES = json.load(open(os.path.join(GOLD, "ref_label_patches.json")))


def fixture_table():
    return labels.GlyphTable([[tuple(v) for v in g["vertices"]] for g in RUNS["glyphs"]])


def station_glyph_labels(key, table, image_id=0):
    """The station label of the fixture as a one-tile GlyphLabelList (icon + center-form glyph run)."""
    s = RUNS[key]
    l = np.zeros(1, labels.LABEL_DTYPE)
    l["has_icon"], l["image_id"] = 1, image_id
    l["icon_center_x"], l["icon_center_y"] = s["icon_center"]
    l["has_text"], l["text_color"] = 1, s["text_color"]
    g = np.zeros(len(s["glyphs"]), labels.GLYPH_INSTANCE_DTYPE)
    for i, e in enumerate(s["glyphs"]):
        g[i]["glyph_id"] = table.first_id + e["glyph"]
        g[i]["form"] = abi.GLYPH_CENTER
        g[i]["scale"] = s["scale"]
        g[i]["p"][:2] = [e["x_offset"], e["baseline"]]
    l["seg_off"], l["n_segs"] = 0, len(g)
    return labels.GlyphLabelList(l, [0, 1], g)


def shim_expand(table, glyphs):
    verts, voff = table.arrays()
    glyphs = glyphs.copy()
    glyphs["glyph_id"] -= table.first_id
    L = _glyph_shim.lib()
    n = L.shim_glyph_expand(verts.ctypes.data, voff.ctypes.data, glyphs.ctypes.data, len(glyphs), None, 0)
    assert n >= 0, f"device walk error {-n}"
    out = np.zeros((n, 4))
    L.shim_glyph_expand(verts.ctypes.data, voff.ctypes.data, glyphs.ctypes.data, len(glyphs), out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out


@pytest.mark.parametrize("key, n_calls", [("station", 3498), ("station_z14_from_the_tile_above", None)])
def test_station_runs_expand_to_the_reference_draw_line_calls(key, n_calls):
    table = fixture_table()
    ll = station_glyph_labels(key, table).to_label_list(table)
    want = np.array(PATCHES[key]["segs"], dtype=np.float64).reshape(-1, 4)
    assert n_calls is None or len(want) == n_calls
    assert ll.segs.shape == want.shape and np.array_equal(ll.segs.view(np.uint64), want.view(np.uint64))
    assert ll.labels["n_segs"].tolist() == [len(want)] and ll.labels["has_icon"].tolist() == [1]
    # the host build of the device walk: the same calls, bit for bit
    got = shim_expand(table, station_glyph_labels(key, table).glyphs)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_device_walk_equals_host_twin_on_random_runs():
    table = labels.synth_glyph_table()
    for scale, seed in ((1, 1), (2, 2)):
        gl = labels.make_glyph_labels(6, table, labels_per_tile=24, scale=scale, seed=seed, line_frac=0.5)
        ll = gl.to_label_list(table)
        assert (gl.glyphs["form"] == abi.GLYPH_LINE).any() and (gl.glyphs["form"] == abi.GLYPH_CENTER).any()
        # label order, glyph order: the walk of every text label's instances, concatenated
        parts = [shim_expand(table, gl.glyphs[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])]) for l in gl.labels if l["has_text"]]
        got = np.concatenate(parts)
        assert len(got) == len(ll.segs) > 1000
        assert np.array_equal(got.view(np.uint64), ll.segs.view(np.uint64))


def test_a_cusp_curve_hits_the_depth_cap_instead_of_truncating():
    """A control point collinear with and beyond the end points ((-1, 0) -> (2, 0) -> (-4, 0): x(t) = -(1 - 3t)^2)
    turns back at t = 1/3, on no dyadic split point: the piece holding the cusp stays folded at every level and its
    coordinates shrink towards 0 without losing relative precision.  The walk must report it, not stop early."""
    table = labels.GlyphTable([[("M", -4, 0, 0, 0), ("Q", -1, 0, 2, 0)]])
    g = np.zeros(1, labels.GLYPH_INSTANCE_DTYPE)
    g["scale"] = 1.0
    verts, voff = table.arrays()
    n = _glyph_shim.lib().shim_glyph_expand(verts.ctypes.data, voff.ctypes.data, g.ctypes.data, 1, None, 0)
    assert n == -2  # OSMT_GLYPH_ERR_DEPTH
    # the real outlines of the fixture stay far from the cap
    table = fixture_table()
    for key in ("station", "station_z14_from_the_tile_above"):
        assert len(shim_expand(table, station_glyph_labels(key, table).glyphs)) > 0


def test_glyph_struct_layouts_match_the_header():
    s = _glyph_shim.lib().shim_glyph_sizeof
    assert s(0) == C.sizeof(abi.GlyphVertex) == labels.GLYPH_VERTEX_DTYPE.itemsize == 10
    assert s(1) == C.sizeof(abi.GlyphInstance) == labels.GLYPH_INSTANCE_DTYPE.itemsize == 64
    assert s(2) == C.sizeof(abi.GlyphLabelBatch)
    assert s(10) == abi.GlyphVertex.type.offset == labels.GLYPH_VERTEX_DTYPE.fields["type"][1]
    assert s(11) == abi.GlyphInstance.scale.offset == labels.GLYPH_INSTANCE_DTYPE.fields["scale"][1]
    assert s(12) == abi.GlyphInstance.p.offset == labels.GLYPH_INSTANCE_DTYPE.fields["p"][1]
    assert s(13) == abi.GlyphLabelBatch.glyphs.offset
    assert s(14) == abi.GlyphLabelBatch.n_glyphs.offset
    assert (s(20), s(21)) == (abi.GLYPH_CENTER, abi.GLYPH_LINE)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLD, "ref_glyph_runs.json")) < 200 * 1024
    chars = {g["char"] for g in RUNS["glyphs"]}
    assert set("Арбатская") <= chars and len(chars) >= 40
    assert any(not g["vertices"] for g in RUNS["glyphs"])  # the space: no shape
