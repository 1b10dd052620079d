"""The coverage planes of the label pass (k_label_cover / k_label_cover_wide), bit for bit.

The label pass exists to reproduce the reference rasterizer's f64 sums in its call order (font/rasterizer.rs:77,80: the
per-key sums do not associate), and nothing else looked at those sums: after the blend into 8-bit pixels a permuted call
order is invisible.  Here every label's plane is read back (osmt_scene_read_label_cover) and compared with
oracle.rasterizer_pixels of its draw_line calls:

  * every oracle pixel whose row lies in [-W, 2W) is inside the window, and the plane holds the identical 64-bit
    pattern there; every other cell of the window is not > 0 (tests/_label_cover_cases.py: check_plane);
  * labels without a window report zero rows; a second render gives the same planes;
  * the glyph-run and the text-run form of a label give the planes of its segment form;
  * the `total > 0` bit k_label_resolve takes from the planes: a label whose cell is exactly 0 in call order — and
    2^-61 in the reversed order — lets the label behind it succeed, the reversed one makes it fail.

The cases (tests/_label_cover_cases.py) are proved order-sensitive on the CPU by tests/test_label_cover_cases_cpu.py.
The bar is bit equality everywhere."""
import json
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from osm_renderer_amd.display_list import TileBuilder
from osm_renderer_amd.lib import OsmtError
from tests import _label_cover_cases as lc
from tests import _text_placer_model as model
from tests.test_glyph_runs_cpu import fixture_table, station_glyph_labels

pytestmark = pytest.mark.gpu

PATCHES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_label_patches.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _tile(scale=1):
    return TileBuilder(zoom=17, scale=scale, canvas=(240, 240, 240)).build()


def _scene_labels(scale):
    """The generated cases of one scale as the labels of one tile, the window-less labels in between:
    (LabelList, [(name, segs)])."""
    tl, parts = labels.TileLabels(), []
    extra = lc.windowless_labels() if scale == 1 else lc.windowless_labels()[:2]
    for i, c in enumerate([c for c in lc.cases() if c.scale == scale]):
        if i % 6 == 2 and extra:
            has_text, segs = extra.pop()
            tl.label(text=((1, 2, 3), segs) if has_text else None)
            parts.append(("no window", segs))
        tl.label(text=((10, 20, 30), c.segs))
        parts.append((c.name, c.segs))
    for has_text, segs in extra:
        tl.label(text=((1, 2, 3), segs) if has_text else None)
        parts.append(("no window", segs))
    return tl.build(), parts


@pytest.mark.parametrize("scale", [1, 2])
def test_planes_hold_the_oracle_bits(gpu_ctx, oracle, scale):
    ll, parts = _scene_labels(scale)
    assert sum(1 for n, _ in parts if n == "no window") >= 2
    scene = gpu_ctx.upload(_tile(scale), ll)
    gpu_ctx.render(scene)
    W = lc.TILE * scale
    planes = [lc.check_plane(scene, oracle, i, segs, W, f"{name} (label {i}, scale {scale})") for i, (name, segs) in enumerate(parts)]
    gpu_ctx.render(scene)  # the planes are rebuilt by every render
    for i, (name, _) in enumerate(parts):
        again = scene.read_label_cover(i)[2]
        assert again.shape == planes[i].shape and np.array_equal(_bits(again), _bits(planes[i])), f"{name}: the second render differs"
    scene.free()


def test_reading_before_the_first_render_is_an_error_and_the_size_protocol(gpu_ctx):
    """Between osmt_scene_set_labels and the next render the planes have not been written (the allocator of the suite
    hands out poisoned memory): an error, never recycled memory.  out == NULL asks for the size; too small a cap and a
    label index beyond the batch are OSMT_INVALID_ARG."""
    import ctypes as C

    from osm_renderer_amd.lib import load

    tl = labels.TileLabels()
    tl.label(text=((0, 0, 0), lc.status_label_b()))
    tl.label()
    ll = tl.build()
    scene = gpu_ctx.upload(_tile())
    gpu_ctx.render(scene)  # a render without labels does not count
    scene.set_labels(ll)
    for i in (0, 1):
        with pytest.raises(OsmtError) as ei:
            scene.read_label_cover(i)
        assert ei.value.code == abi.INVALID_ARG and "render" in str(ei.value)
    gpu_ctx.render(scene)
    ry0, cx0, plane = scene.read_label_cover(0)
    assert (ry0, cx0) + plane.shape == (0, 38, 1, 6) and (plane > 0).sum() >= 1
    assert scene.read_label_cover(1)[2].shape[0] == 0
    L, n, win = load(), C.c_size_t(99), (C.c_int32 * 4)()
    assert L.osmt_scene_read_label_cover(gpu_ctx._h, scene._h, 0, win, None, 0, C.byref(n)) == abi.OK
    assert n.value == 6 and list(win) == [0, 0, 38, 6]
    buf = np.full(8, 7.0)
    assert L.osmt_scene_read_label_cover(gpu_ctx._h, scene._h, 0, win, buf.ctypes.data_as(C.POINTER(C.c_double)), 5, C.byref(n)) == abi.INVALID_ARG
    assert n.value == 6 and (buf == 7.0).all()
    assert L.osmt_scene_read_label_cover(gpu_ctx._h, scene._h, 0, win, buf.ctypes.data_as(C.POINTER(C.c_double)), 6, C.byref(n)) == abi.OK
    assert np.array_equal(_bits(buf[:6]), _bits(plane.ravel())) and (buf[6:] == 7.0).all()
    assert L.osmt_scene_read_label_cover(gpu_ctx._h, scene._h, 2, win, None, 0, C.byref(n)) == abi.INVALID_ARG
    scene.set_labels(ll)  # attached again: new buffers, nothing written yet
    with pytest.raises(OsmtError):
        scene.read_label_cover(0)
    scene.set_labels(None)
    with pytest.raises(OsmtError):
        scene.read_label_cover(0)  # no label 0
    scene.free()


def _planes_of_form(gpu_ctx, oracle, scene, ll, what):
    """Render, then every label's plane checked against the oracle on the calls the segment form `ll` gives it."""
    gpu_ctx.render(scene)
    out = []
    for i, l in enumerate(ll.labels):
        segs = ll.segs[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])] if l["has_text"] else np.zeros((0, 4))
        out.append(lc.check_plane(scene, oracle, i, segs, lc.TILE, f"{what}, label {i}"))
    return out


def _same_planes(a, b, what):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.shape == q.shape and np.array_equal(_bits(p), _bits(q)), f"{what}: label {i} differs between the forms"


def test_station_label_planes_in_segment_and_glyph_form(gpu_ctx, oracle):
    """The reference's own station label (tests/golden/ref_label_patches.json): real glyph outlines, 3498 calls."""
    ref = fixture_table()
    gpu_ctx.register_glyphs(ref)
    segs = np.array(PATCHES["station"]["segs"], dtype=np.float64).reshape(-1, 4)
    tl = labels.TileLabels()
    tl.label(text=((0, 0, 0), segs))
    ll = tl.build()
    scene = gpu_ctx.upload(_tile(), ll)
    a = _planes_of_form(gpu_ctx, oracle, scene, ll, "station, segments")
    assert len(segs) > 3000 and ((a[0] > 0.0) & (a[0] < 1.0)).sum() > 100
    gl = station_glyph_labels("station", ref)
    gl.labels["has_icon"] = 0
    scene.set_glyph_labels(gl)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(segs))
    _same_planes(a, _planes_of_form(gpu_ctx, oracle, scene, ll, "station, glyph run"), "station")
    scene.free()


def test_synthetic_glyph_and_text_runs_give_the_planes_of_their_segment_form(gpu_ctx, oracle):
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    dl = _tile()
    # glyph runs: centre- and line-form, texts of zero glyphs, labels without text
    gl = labels.make_glyph_labels(1, syn, labels_per_tile=40, seed=31, line_frac=0.4, empty_frac=0.08)
    ll = gl.to_label_list(syn)
    assert (ll.labels["n_segs"] > 0).sum() >= 24 and (gl.glyphs["form"] == abi.GLYPH_LINE).any()
    scene = gpu_ctx.upload(dl, ll)
    a = _planes_of_form(gpu_ctx, oracle, scene, ll, "glyph labels as segments")
    scene.set_glyph_labels(gl)
    _same_planes(a, _planes_of_form(gpu_ctx, oracle, scene, ll, "glyph labels"), "glyph runs")
    # text runs: placed on the device; the model's instances give the segment form
    tx = labels.make_text_labels(1, syn, labels_per_tile=30, seed=32, line_frac=0.4, empty_frac=0.08)
    tll = model.place_text_labels(tx).to_label_list(syn)
    assert (tll.labels["n_segs"] > 0).sum() >= 12
    scene.set_text_labels(tx)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(tll.segs))
    b = _planes_of_form(gpu_ctx, oracle, scene, tll, "text labels")
    scene.set_labels(tll)
    _same_planes(b, _planes_of_form(gpu_ctx, oracle, scene, tll, "text labels as segments"), "text runs")
    scene.free()


def test_a_zero_total_is_no_pixel_and_a_tiny_one_is(gpu_ctx, oracle):
    """k_label_resolve sees one bit per cell, total > 0.  Label A adds 2^-61, 0.25 and -0.25 to cell (40, 0): 0 in call
    order, 2^-61 in the reversed order (proved with the oracle in tests/test_label_cover_cases_cpu.py).  Label B covers
    that cell only: behind A it succeeds, behind the reversed A it collides."""
    a, b = lc.status_label_a(), lc.status_label_b()
    x, y = lc.STATUS_CELL
    dl = _tile()
    for a_calls, want_status, want_cell in [(a, [1, 1], 0.0), (a[::-1], [1, 0], 2.0 ** -61)]:
        tl = labels.TileLabels()
        tl.label(text=((200, 0, 0), a_calls))
        tl.label(text=((0, 0, 200), b))
        ll = tl.build()
        scene = gpu_ctx.upload(dl, ll)
        got = gpu_ctx.render(scene).cpu().numpy()
        lc.check_plane(scene, oracle, 0, a_calls, lc.TILE, "label A")
        ry0, cx0, plane = scene.read_label_cover(0)
        assert _bits(plane[y - ry0, x - cx0]) == _bits(np.float64(want_cell))
        lc.check_plane(scene, oracle, 1, b, lc.TILE, "label B")
        want, wst = oracle.render_batch(dl, labels=ll, want_status=True)
        assert wst.tolist() == want_status  # the oracle agrees that this is what the reference does
        assert scene.label_status().tolist() == want_status
        assert np.array_equal(got, want)
        scene.free()
