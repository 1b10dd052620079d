"""Text-run labels on the GPU (osmt_scene_set_text_labels: k_text_place -> k_glyph_count -> read-back -> k_glyph_emit)
through the C ABI.  The device must place every glyph where TextPlacer::place does:

  * on make_text_labels (1, 8 and 300 tiles, scale 1 and 2) osmt_scene_read_glyph_instances equals the Python model
    (tests/_text_placer_model.py) bit for bit, OSMT_GLYPH_NONE on the same labels; the draw_line arena, the rendered
    pixels and the label statuses equal those of the same scene with set_glyph_labels(model output) and the oracle's
    on to_label_list;
  * the reference's station label given as a text run reproduces the golden crops of ref_label_patches.json — the pin
    to real reference output.  LINE text has no golden crop: it is pinned to the model and this machine's libm only;
  * a 300-glyph text in several rows, a way of 5 000 points, a batch in which every label is skipped;
  * a scene can be switched between the three label forms and detached; the one-call entry equals scene + set + render;
  * an unregistered glyph id, a non-finite sincos entry and a placement beyond 2^20 are loud errors."""
import numpy as np
import pytest

from osm_renderer_amd import abi, labels, synth
from osm_renderer_amd.display_list import TileBuilder
from osm_renderer_amd.lib import OsmtError
from tests import _text_placer_model as model
from tests.test_glyph_runs_cpu import PATCHES, fixture_table
from tests.test_reference_golden_labels import _check, _check_z14
from tests.test_text_placer_cpu import A, B, SP, station_text_labels, text_labels

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (12, 20), (5, 7)]


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def tables(gpu_ctx):
    ref = fixture_table()
    gpu_ctx.register_glyphs(ref)
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    rng = np.random.default_rng(17)
    ids, imgs = [], []
    for h, w in SIZES:
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img[: h // 3, :, 3] = 255
        imgs.append(img)
        ids.append(gpu_ctx.register_image(img))
    return ref, syn, ids, imgs


def _case(tables, scale, n_tiles, seed, per_tile=24):
    _, syn, ids, _ = tables
    tl = labels.make_text_labels(n_tiles, syn, labels_per_tile=per_tile, scale=scale, seed=seed, n_images=len(ids), image_sizes=SIZES,
                                 line_frac=0.4, empty_frac=0.05)
    has_icon = tl.labels["has_icon"] == 1
    tl.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[tl.labels["image_id"][has_icon]]
    return synth.config2(n_tiles, scale=scale), tl


def _assert_instances(got, want):
    """Every field a form uses, bit for bit; OSMT_GLYPH_NONE on the same slots."""
    assert got.shape == want.shape
    assert np.array_equal(got["form"], want["form"]) and np.array_equal(got["glyph_id"], want["glyph_id"])
    assert np.array_equal(_bits(got["scale"]), _bits(want["scale"]))
    used = np.where(want["form"] == abi.GLYPH_LINE, 6, np.where(want["form"] == abi.GLYPH_CENTER, 2, 0))
    mask = np.arange(6)[None, :] < used[:, None]
    bad = (_bits(got["p"]).reshape(-1, 6) != _bits(want["p"]).reshape(-1, 6)) & mask
    assert not bad.any(), f"{int(bad.any(1).sum())} of {len(got)} instances differ from the model, first at slot {int(np.nonzero(bad.any(1))[0][0])}"
    assert np.array_equal(_u8(got), _u8(want))  # and the unused entries are zero, as documented


@pytest.mark.parametrize("n_tiles, seed, scale", [(1, 5, 1), (8, 6, 1), (300, 7, 1), (1, 5, 2), (8, 6, 2), (300, 7, 2),
                                                 (1, 5, 4), (8, 6, 4), (70, 7, 4)])  # (scale 4: 70 tiles, not 300 — 1.2 GB of pixels to read back)
def test_instances_equal_the_model_and_everything_downstream_follows(gpu_ctx, oracle, tables, scale, n_tiles, seed):
    syn = tables[1]
    dl, tl = _case(tables, scale, n_tiles, seed + 10 * scale)
    gl = model.place_text_labels(tl)
    scene = gpu_ctx.upload(dl)
    scene.set_text_labels(tl)
    got = scene.read_glyph_instances()
    _assert_instances(got, gl.slots)
    if n_tiles >= 8:
        assert {abi.GLYPH_CENTER, abi.GLYPH_LINE, abi.GLYPH_NONE} == set(np.unique(got["form"]).tolist())
        assert (tl.glyphs["kern"] != 0).any() and (tl.runs["y_offset"] > 0).any()
    segs = scene.read_label_segs()
    out = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    # the same scene with the model's instances as glyph runs
    scene.set_glyph_labels(gl)
    assert len(scene.read_glyph_instances()) == 0
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(segs))
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out) and np.array_equal(scene.label_status(), st)
    scene.free()
    # the host expansion and the oracle
    ll = gl.to_label_list(syn)
    assert segs.shape == ll.segs.shape and np.array_equal(_bits(segs), _bits(ll.segs))
    images = _images(tables)
    sub = list(range(n_tiles)) if n_tiles <= 8 else list(range(0, n_tiles, n_tiles // 12))
    want, wst = oracle.render_batch(dl.subset(sub), images=images, threads=min(8, len(sub)), labels=ll.subset(sub), want_status=True)
    lab_sub = np.concatenate([np.arange(int(tl.job_label_off[i]), int(tl.job_label_off[i + 1])) for i in sub])
    assert np.array_equal(st[lab_sub], wst)
    assert np.array_equal(out[sub], want)
    if n_tiles >= 300:
        assert 0 < st.sum() < len(st)  # collisions happened


def _images(tables):
    """The registered icons as the oracle takes them: a list indexed by image id (ids below the first are unused)."""
    return [np.zeros((1, 1, 4), np.uint8)] * tables[2][0] + list(tables[3])


@pytest.mark.parametrize("key", ["station", "station_z14_from_the_tile_above"])
def test_station_text_run_reproduces_the_reference_golden(gpu_ctx, tables, key):
    ref = tables[0]
    p = PATCHES[key]
    icon_id = gpu_ctx.register_image(np.array(p["icon_rgba"], dtype=np.uint8))
    tl = station_text_labels(key, first_id=ref.first_id, image_id=icon_id)
    dl = TileBuilder(zoom=17, scale=1, canvas=tuple(p["canvas"])).build()
    scene = gpu_ctx.upload(dl)
    scene.set_text_labels(tl)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(np.array(p["segs"]).reshape(-1, 4)))
    out = gpu_ctx.render(scene).cpu().numpy()
    assert scene.label_status().tolist() == [1]
    (_check if key == "station" else _check_z14)(p, out[0, :, :, :3])
    scene.free()


def _long_text(rng, first_id, n):
    return [(first_id + int(rng.integers(0, 4)), int(rng.integers(200, 700)), int(rng.integers(-50, 50)), 0) if k % 7
            else (first_id + SP, 260, 0, 1) for k in range(1, n + 1)]


def test_large_inputs_and_a_batch_of_skipped_labels(gpu_ctx, tables):
    syn = tables[1]
    f = syn.first_id
    rng = np.random.default_rng(5)
    g = _long_text(rng, f, 300)
    pts = labels.walking_order(np.cumsum(rng.integers(-1, 3, size=(5000, 2)), axis=0).astype(np.int32) - 1120).tolist()
    short = [(f + A, 640, 0, 0)] * 70  # more than one chunk of glyphs on a way of more than one chunk of edges
    bends = labels.walking_order(np.cumsum(rng.integers(-2, 6, size=(200, 2)), axis=0).astype(np.int32)).tolist()
    tl = text_labels([dict(glyphs=g, scale=0.011, center=(128.0, 100.0)),
                      dict(glyphs=g, scale=0.004, position=abi.TEXT_LINE, pts=pts),
                      dict(glyphs=short, scale=0.004, position=abi.TEXT_LINE, pts=bends),
                      dict(glyphs=g[:130], scale=0.012, center=(90.5, 300.25), y_offset=6)])
    gl = model.place_text_labels(tl)
    assert len(np.unique(gl.slots["p"][:300, 1])) > 5 and (gl.slots["form"][300:670] == abi.GLYPH_LINE).all()
    dl = synth.config2(1)
    scene = gpu_ctx.upload(dl)
    scene.set_text_labels(tl)
    _assert_instances(scene.read_glyph_instances(), gl.slots)
    ll = gl.to_label_list(syn)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(ll.segs))
    out = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    scene.set_labels(ll)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out) and np.array_equal(scene.label_status(), st)
    # every label skipped: ways too short, of one point, of none
    g = [(f + A, 640, 0, 0), (f + B, 640, 0, 0)]
    skipped = text_labels([dict(glyphs=g, position=abi.TEXT_LINE, pts=p) for p in ([], [(5, 5)], [(0, 0), (3, 4)], [(9, 9), (9, 9), (9, 9)])] * 40)
    scene.set_text_labels(skipped)
    got = scene.read_glyph_instances()
    assert len(got) == 320 and (got["form"] == abi.GLYPH_NONE).all()
    _assert_instances(got, model.place_text_labels(skipped).slots)
    assert scene.read_label_segs().shape == (0, 4)
    plain = gpu_ctx.render(scene).cpu().numpy()
    assert scene.label_status().tolist() == [1] * 160  # place() returned true
    scene.set_text_labels(None)
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), plain)
    scene.free()


def test_switching_between_the_three_forms_and_detaching(gpu_ctx, tables):
    syn = tables[1]
    dl, tl = _case(tables, 1, 8, 77)
    gl = model.place_text_labels(tl)
    ll = gl.to_label_list(syn)
    scene = gpu_ctx.upload(dl)
    plain = gpu_ctx.render(scene).cpu().numpy()
    scene.set_labels(ll)
    a = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    assert not np.array_equal(a, plain) and len(scene.read_glyph_instances()) == 0
    for step in ("text", "glyph", "text", "segs", "text", None, "text"):
        if step == "text":
            scene.set_text_labels(tl)
            _assert_instances(scene.read_glyph_instances(), gl.slots)
        elif step == "glyph":
            scene.set_glyph_labels(gl)
        elif step == "segs":
            scene.set_labels(ll)
        else:
            scene.set_text_labels(None)
            assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), plain) and len(scene.label_status()) == 0
            assert len(scene.read_glyph_instances()) == 0
            continue
        assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), a) and np.array_equal(scene.label_status(), st)
        assert np.array_equal(_bits(scene.read_label_segs()), _bits(ll.segs))
    scene.free()


def test_one_call_entry_equals_scene_set_render(gpu_ctx, tables):
    syn = tables[1]
    for scale in (1, 2):
        dl, tl = _case(tables, scale, 12, 90 + scale)
        scene = gpu_ctx.upload(dl)
        scene.set_text_labels(tl)
        want = gpu_ctx.render(scene).cpu().numpy()
        scene.free()
        got = gpu_ctx.render_batch_rgb_text(dl, tl)
        assert np.array_equal(got.reshape(12, dl.dim, dl.dim, 3), want[..., :3])
        assert np.array_equal(got, gpu_ctx.render_batch_rgb(dl, model.place_text_labels(tl).to_label_list(syn)))
        sub = [7, 2, 3]
        assert np.array_equal(gpu_ctx.render_batch_rgb_text(dl.subset(sub), tl.subset(sub)), got[sub])
    assert np.array_equal(gpu_ctx.render_batch_rgb_text(dl, None), gpu_ctx.render_batch_rgb(dl, None))


def test_error_paths_are_loud(gpu_ctx, tables):
    syn = tables[1]
    f = syn.first_id
    dl = TileBuilder(zoom=17, scale=1, canvas=(240, 240, 240)).build()
    scene = gpu_ctx.upload(dl)
    g = [(f + A, 640, 0, 0), (f + B, 640, 0, 0)]
    way = [(0, 0), (50, 10), (90, 10)]

    def nan_sincos():
        tl = text_labels([dict(glyphs=g, position=abi.TEXT_LINE, pts=way)])
        tl.way_sincos[1, 0] = np.nan
        return tl

    cases = [
        (text_labels([dict(glyphs=[(f + A, 640, 0, 0), (0xFFFFFF, 640, 0, 0)])]), abi.INVALID_ARG, "glyph table"),  # unregistered glyph id
        (nan_sincos(), abi.INVALID_ARG, "way_sincos"),
        # centred at the edge of what is admitted, a row 60 000 px wide: the first glyphs lie beyond 2^20
        (text_labels([dict(glyphs=[(f + A, 60000, 0, 0)] * 64, scale=1.0 / 64.0, center=(2.0**20, 0.0))]), abi.UNSUPPORTED, "2^20"),
        (text_labels([dict(glyphs=g, position=abi.TEXT_LINE, scale=1.0 / 64.0, pts=[(2**22, 0), (2**22 + 100, 0)])]), abi.UNSUPPORTED, "2^20"),
        (text_labels([dict(glyphs=g, position=abi.TEXT_LINE, pts=[(2**28 + 1, 0), (2**28 + 100, 0)])]), abi.UNSUPPORTED, "2^28"),
    ]
    for tl, code, word in cases:
        with pytest.raises(OsmtError) as ei:
            scene.set_text_labels(tl)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        assert scene.read_label_segs().shape == (0, 4) and len(scene.read_glyph_instances()) == 0  # nothing stays attached
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.render_batch_rgb_text(dl, cases[0][0])
    assert ei.value.code == abi.INVALID_ARG
    # a valid run afterwards works
    scene.set_text_labels(text_labels([dict(glyphs=g, position=abi.TEXT_LINE, pts=way)]))
    assert len(scene.read_label_segs()) > 0 and (scene.read_glyph_instances()["form"] == abi.GLYPH_LINE).all()
    scene.free()
