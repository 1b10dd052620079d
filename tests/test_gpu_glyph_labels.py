"""Glyph-run labels on the GPU (osmt_scene_set_glyph_labels: k_glyph_count -> read-back -> k_glyph_emit) through the C
ABI.  The expansion must write exactly the draw_line calls of the host twin (GlyphLabelList.to_label_list), so the
label kernels — unchanged — give the segment path's pixels and statuses:

  * the reference's station label given as glyph runs reproduces the golden window at z17 and z14;
  * > 10 000 random center- and line-form labels (icons, collisions, empty glyphs, labels without text) at scale 1 and
    2: the device arena equals the host expansion bit for bit, framebuffer and statuses equal the segment path's, and
    the one-piece osmt_render_batch_rgb_glyphs gives the same bytes as osmt_render_batch_rgb;
  * the device hypot equals libm on 10^7 pairs;
  * every error path is loud, and a scene's labels can be re-set between the forms and detached."""
import json
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, synth
from osm_renderer_amd.display_list import TileBuilder
from osm_renderer_amd.lib import OsmtError
from tests.test_glyph_runs_cpu import fixture_table, station_glyph_labels
from tests.test_reference_golden_labels import _check, _check_z14

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PATCHES = json.load(open(os.path.join(GOLD, "ref_label_patches.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def tables(gpu_ctx):
    ref = fixture_table()
    gpu_ctx.register_glyphs(ref)
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    rng = np.random.default_rng(17)
    sizes = [(16, 16), (12, 20), (5, 7)]
    ids = []
    for h, w in sizes:
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img[: h // 3, :, 3] = 255
        ids.append(gpu_ctx.register_image(img))
    return ref, syn, ids, sizes


@pytest.mark.parametrize("key", ["station", "station_z14_from_the_tile_above"])
def test_station_glyph_runs_reproduce_the_reference_golden(gpu_ctx, tables, key):
    ref = tables[0]
    p = PATCHES[key]
    icon_id = gpu_ctx.register_image(np.array(p["icon_rgba"], dtype=np.uint8))
    gl = station_glyph_labels(key, ref, image_id=icon_id)
    dl = TileBuilder(zoom=17, scale=1, canvas=tuple(p["canvas"])).build()
    scene = gpu_ctx.upload(dl)
    scene.set_glyph_labels(gl)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(np.array(p["segs"]).reshape(-1, 4)))
    out = gpu_ctx.render(scene).cpu().numpy()
    assert scene.label_status().tolist() == [1]
    (_check if key == "station" else _check_z14)(p, out[0, :, :, :3])
    scene.free()


def _random_case(tables, scale, n_tiles, per_tile, seed):
    _, syn, ids, sizes = tables
    gl = labels.make_glyph_labels(n_tiles, syn, labels_per_tile=per_tile, scale=scale, seed=seed, n_images=len(ids),
                                  image_sizes=sizes, line_frac=0.4, empty_frac=0.05)
    has_icon = gl.labels["has_icon"] == 1
    gl.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[gl.labels["image_id"][has_icon]]
    return synth.config2(n_tiles, scale=scale), gl, gl.to_label_list(syn)


@pytest.mark.parametrize("scale, n_tiles, per_tile, seed", [(1, 128, 80, 101), (2, 128, 80, 202)])
def test_random_glyph_runs_equal_the_host_expansion_and_the_segment_path(gpu_ctx, tables, scale, n_tiles, per_tile, seed):
    dl, gl, ll = _random_case(tables, scale, n_tiles, per_tile, seed)
    lab = gl.labels
    assert len(lab) >= 10_000 and (lab["has_icon"] == 1).any() and (lab["has_text"] == 0).any()
    assert ((lab["has_text"] == 1) & (lab["n_segs"] == 0)).any() and (gl.glyphs["form"] == abi.GLYPH_LINE).any()
    assert (gl.glyphs["glyph_id"] == tables[1].first_id + len(labels.SYNTH_GLYPHS) - 1).any()  # the empty glyph
    seg_scene = gpu_ctx.upload(dl, ll)
    want = gpu_ctx.render(seg_scene).cpu().numpy()
    want_st = seg_scene.label_status()
    seg_scene.free()
    assert 0 < want_st.sum() < len(lab)  # collisions happened
    scene = gpu_ctx.upload(dl)
    scene.set_glyph_labels(gl)
    got_segs = scene.read_label_segs()
    assert got_segs.shape == ll.segs.shape and np.array_equal(_bits(got_segs), _bits(ll.segs))
    got = gpu_ctx.render(scene).cpu().numpy()
    assert np.array_equal(scene.label_status(), want_st)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ from the segment path"
    scene.free()
    # the one-piece host-buffer call: the same bytes as osmt_render_batch_rgb with the expanded calls
    sub = list(range(0, n_tiles, 4))
    dls, gls, lls = dl.subset(sub), gl.subset(sub), ll.subset(sub)
    a = gpu_ctx.render_batch_rgb_glyphs(dls, gls)
    b = gpu_ctx.render_batch_rgb(dls, lls)
    assert np.array_equal(a, b)
    assert np.array_equal(a.reshape(len(sub), dl.dim, dl.dim, 3), want[sub, :, :, :3])


def _long_outline(n_arcs, n_lines, rx, ry, seed):
    """A closed outline of n_arcs quadratic arcs around a wobbly ellipse, then n_lines LineTo back along a zigzag: more
    than one wave's worth (64) of vertices in one glyph."""
    rng = np.random.default_rng(seed)
    v = [("M", 500 + rx, 500, 0, 0)]
    for i in range(1, n_arcs + 1):
        a, m = 2 * np.pi * i / n_arcs, 2 * np.pi * (i - 0.5) / n_arcs
        w = 1.0 + 0.15 * rng.random()
        v.append(("Q", int(500 + rx * np.cos(a)), int(500 + ry * np.sin(a)), int(500 + w * rx * np.cos(m)), int(500 + w * ry * np.sin(m))))
    for i in range(n_lines):
        v.append(("L", int(500 + rx * (1 - 2 * (i + 1) / n_lines)), int(500 + (40 if i % 2 else -40)), 0, 0))
    return v


def test_outlines_longer_than_a_wave(gpu_ctx, tables):
    """Glyphs of 65..250 vertices (CJK, '@', '&' have such outlines): the count pass's strided lanes and the emit pass's
    64-vertex chunks with the carried base.  Arena bit for bit against the host walk, pixels against the segment path."""
    long = labels.GlyphTable([_long_outline(60, 5, 420, 380, 1), _long_outline(100, 40, 300, 450, 2), _long_outline(180, 70, 450, 450, 3)])
    gpu_ctx.register_glyphs(long)
    verts, voff = long.arrays()
    assert np.diff(voff).tolist() == [66, 141, 251]
    rng = np.random.default_rng(31)
    n_tiles, parts = 4, []
    for _ in range(n_tiles):
        labs, gl = [], []
        for _ in range(6):
            l = np.zeros((), labels.LABEL_DTYPE)
            l["has_text"], l["text_color"] = 1, [int(c) for c in rng.integers(0, 256, 3)]
            ids = [long.first_id + int(k) for k in rng.integers(0, 3, int(rng.integers(1, 4)))]
            sc = float(rng.choice([0.011, 0.02, 0.035]))
            x, y = float(rng.integers(-100, 356)) + 0.25, float(rng.integers(-100, 356)) + 0.5
            run = []
            for k, g in enumerate(ids):
                if rng.random() < 0.5:
                    run.append(labels._instance(g, abi.GLYPH_CENTER, sc, [x + 1000 * sc * k, y]))
                else:
                    a = float(rng.uniform(-1, 1))
                    run.append(labels._instance(g, abi.GLYPH_LINE, sc, [500 * sc, 500 * sc, np.sin(-a), np.cos(-a), x + 1000 * sc * k, y]))
            l["seg_off"], l["n_segs"] = sum(len(r) for r in gl), len(run)
            gl.append(np.array(run, dtype=labels.GLYPH_INSTANCE_DTYPE))
            labs.append(l)
        parts.append(labels.GlyphLabelList(np.array(labs, dtype=labels.LABEL_DTYPE), [0, len(labs)], np.concatenate(gl)))
    gls = labels.concat_glyph_labels(parts)
    ll = gls.to_label_list(long)
    dl = synth.config2(n_tiles)
    seg_scene = gpu_ctx.upload(dl, ll)
    want = gpu_ctx.render(seg_scene).cpu().numpy()
    want_st = seg_scene.label_status()
    seg_scene.free()
    scene = gpu_ctx.upload(dl)
    scene.set_glyph_labels(gls)
    got_segs = scene.read_label_segs()
    assert len(got_segs) == len(ll.segs) > 20_000 and np.array_equal(_bits(got_segs), _bits(ll.segs))
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), want) and np.array_equal(scene.label_status(), want_st)
    scene.free()


def test_device_hypot_equals_libm_on_ten_million_pairs(gpu_ctx):
    rng = np.random.default_rng(99)
    n = 2_000_000
    xs = [rng.random(n) * 64.0, 10.0 ** (-8 + 12 * rng.random(n)), np.ldexp(rng.random(n), rng.integers(-1074, 1024, n)),
          np.floor(rng.random(n) * 4096) / 8.0]
    ys = [rng.random(n) * 64.0, 10.0 ** (-8 + 12 * rng.random(n)), np.ldexp(rng.random(n), rng.integers(-1074, 1024, n)),
          np.floor(rng.random(n) * 512) / 4.0]
    x, y = np.concatenate(xs + [xs[1]]), np.concatenate(ys + [xs[1]])  # + x == y
    assert len(x) >= 10_000_000
    got = gpu_ctx.debug_hypot(x, y)
    want = np.hypot(x, y)  # numpy's float64 hypot is libm's
    assert np.array_equal(want[:1000], np.array([labels._libm.hypot(a, b) for a, b in zip(x[:1000], y[:1000])]))
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, f"{bad} of {len(x)} device hypot values differ from libm"


def _one_label(glyph_id, form=abi.GLYPH_CENTER, scale=0.011, p=(100.0, 120.0), seg_off=0, n=1):
    l = np.zeros(1, labels.LABEL_DTYPE)
    l["has_text"], l["seg_off"], l["n_segs"] = 1, seg_off, n
    g = np.zeros(1, labels.GLYPH_INSTANCE_DTYPE)
    g["glyph_id"], g["form"], g["scale"] = glyph_id, form, scale
    g["p"][0, : len(p)] = p
    return labels.GlyphLabelList(l, [0, 1], g)


def test_error_paths_are_loud(gpu_ctx, tables):
    syn = tables[1]
    o = syn.first_id  # "o": curves
    dl = TileBuilder(zoom=17, scale=1, canvas=(240, 240, 240)).build()
    scene = gpu_ctx.upload(dl)
    cases = [
        (_one_label(0xFFFFFF), abi.INVALID_ARG),  # glyph id outside the table
        (_one_label(o, n=2), abi.INVALID_ARG),  # instance range out of bounds
        (_one_label(o, seg_off=1), abi.INVALID_ARG),
        (_one_label(o, form=7), abi.INVALID_ARG),  # unknown form
        (_one_label(o, scale=float("nan")), abi.INVALID_ARG),
        (_one_label(o, p=(float("inf"), 0.0)), abi.INVALID_ARG),
        (_one_label(o, p=(2.0e6, 10.0)), abi.UNSUPPORTED),  # calls beyond 2^20
        (_one_label(o, scale=3000.0), abi.UNSUPPORTED),  # outline scaled beyond 2^20
    ]
    cusp = labels.GlyphTable([[("M", -4, 0, 0, 0), ("Q", -1, 0, 2, 0)]])
    gpu_ctx.register_glyphs(cusp)
    cases.append((_one_label(cusp.first_id, scale=1.0, p=(0.0, 0.0)), abi.UNSUPPORTED))  # past the depth cap
    for gl, code in cases:
        with pytest.raises(OsmtError) as ei:
            scene.set_glyph_labels(gl)
        assert ei.value.code == code, str(ei.value)
        assert scene.read_label_segs().shape == (0, 4)  # nothing stays attached
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.render_batch_rgb_glyphs(dl, _one_label(0xFFFFFF))
    assert ei.value.code == abi.INVALID_ARG
    # a valid run afterwards works
    scene.set_glyph_labels(_one_label(o))
    assert len(scene.read_label_segs()) > 0
    scene.free()


def test_relabelling_between_forms_and_detaching(gpu_ctx, tables):
    dl, gl, ll = _random_case(tables, 1, 8, 24, 7)
    scene = gpu_ctx.upload(dl)
    plain = gpu_ctx.render(scene).cpu().numpy()
    scene.set_labels(ll)
    a = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    assert not np.array_equal(a, plain)
    scene.set_glyph_labels(gl)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), a) and np.array_equal(scene.label_status(), st)
    scene.set_glyph_labels(None)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), plain) and len(scene.label_status()) == 0
    scene.set_glyph_labels(gl)
    scene.set_labels(None)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), plain)
    scene.set_glyph_labels(gl)
    scene.set_labels(ll)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), a)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(ll.segs))
    scene.free()
