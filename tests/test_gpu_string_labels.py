"""String labels on the GPU (osmt_scene_set_string_labels: k_text_shape -> k_text_place -> k_glyph_count -> read-back ->
k_glyph_emit) through the C ABI.  The device must shape every char as TextPlacer::text_to_glyphs does:

  * osmt_scene_read_text_glyphs equals the Python model (tests/_text_shaper_model.py) and the host mirror bit for bit on
    one batch of texts of 0 .. 300 chars with kern pairs across the 64- and 128-char marks, across a label boundary
    (where none may be applied), labels without text in between, a code point the font does not have and two fonts that
    map one code point to different glyphs;
  * make_string_labels against make_text_labels at the same seed: glyph instances, draw_line arena, label statuses and
    pixels are identical at scale 1 and 2, and through osmt_render_batch_rgb_strings into a padded stride;
  * the reference's station label given as the string "Арбатская" with the reference's font tables reproduces the golden
    crops of ref_label_patches.json;
  * a surrogate, an unknown font and a non-finite font size are loud and leave nothing attached; every refusal of
    osmt_register_font and osmt_validate_string_labels names its offender in osmt_last_error(); a font registered after a
    scene was set does not disturb that scene."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, synth
from osm_renderer_amd.display_list import TileBuilder
from osm_renderer_amd.lib import OsmtError, load
from tests import _shape_shim
from tests import _text_placer_model as placer
from tests import _text_shaper_model as model
from tests.test_glyph_runs_cpu import PATCHES, fixture_table
from tests.test_gpu_text_labels import _assert_instances
from tests.test_reference_golden_labels import _check, _check_z14
from tests.test_text_shaper_cpu import (FONT_REFUSALS, LABEL_REFUSALS, N_OUTLINES, ref_font, refused_font, station_string_labels,
                                        string_labels, valid_font, valid_strings)

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (12, 20), (5, 7)]
NS = len(labels.SYNTH_GLYPHS)
SPACE = NS - 1


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def tables(gpu_ctx):
    ref = fixture_table()
    gpu_ctx.register_glyphs(ref)
    empty = labels.GlyphTable([[]])
    gpu_ctx.register_glyphs(empty)
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    rng = np.random.default_rng(17)
    ids = []
    for h, w in SIZES:
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img[: h // 3, :, 3] = 255
        ids.append(gpu_ctx.register_image(img))
    return ref, empty, syn, ids


def _letter_font(syn, shift, kern):
    """'A' + i -> glyph 1 + (i + shift) % 12, ' ' -> glyph 13; glyph g draws shape (g - 1) % (NS - 1) of SYNTH_GLYPHS."""
    shapes = [SPACE] + [(g - 1) % (NS - 1) for g in range(1, 13)] + [SPACE]
    cmap = [(0x20, 13)] + [(0x41 + i, 1 + (i + shift) % 12) for i in range(12)]
    return labels.FontTable(cmap, [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]], [syn.first_id + s for s in shapes], kern)


def _text(n, seed):
    """n chars of 'A'..'L' with a space now and then, and the pair "CE" across chars 63 | 64 and 127 | 128."""
    rng = np.random.default_rng(seed)
    t = [0x20 if k % 9 == 8 else 0x41 + int(rng.integers(0, 12)) for k in range(n)]
    for k in (63, 127):
        if k + 1 < n:
            t[k], t[k + 1] = 0x43, 0x45
    return t


def test_shaped_records_equal_the_model_bit_for_bit(gpu_ctx, tables):
    syn = tables[2]
    # font 0: C = glyph 3, E = glyph 5; font 1 shifts every letter by one glyph: C = 4, E = 6
    fonts = [_letter_font(syn, 0, [(3, 5, -45), (5, 3, 20), (7, 13, 12)]), _letter_font(syn, 1, [(3, 5, 31), (4, 6, -17), (6, 4, 8)])]
    base = gpu_ctx.register_font(fonts[0])
    assert gpu_ctx.register_font(fonts[1]) == base + 1
    specs = []
    for i, n in enumerate([0, 1, 2, 63, 64, 65, 128, 129, 300]):
        specs.append(dict(chars=_text(n, 40 + i), font=base + i % 2, font_size=9.0 + i % 3, center=(20.0 + 25 * i, 30.0 + 20 * i)))
        if i % 3 == 1:
            specs.append(dict(has_text=0))
    way = labels.walking_order(np.cumsum(np.random.default_rng(3).integers(0, 9, size=(300, 2)), axis=0).astype(np.int32)).tolist()
    specs += [dict(chars="ABC", font=base, center=(60.0, 200.0)),  # ... C | E ...: the next label starts with the right half of a pair
              dict(chars="EC", font=base, center=(160.0, 200.0)),
              dict(has_text=0),
              dict(chars="EAC", font=base + 1, center=(60.0, 230.0)),
              dict(chars=[0x45, 0x416, 0x10FFFF, 0x43, 0x45], font=base + 1, center=(160.0, 230.0)),  # two code points the font does not have
              dict(chars=_text(129, 77), font=base + 1, font_size=10.0, position=abi.TEXT_LINE, pts=way)]
    sl = string_labels(specs)
    by_id = {base: fonts[0], base + 1: fonts[1]}
    want = model.shape_labels(sl, {k: model.Font(f) for k, f in by_id.items()})
    scene = gpu_ctx.upload(synth.config2(1))
    scene.set_string_labels(sl)
    got = scene.read_text_glyphs()
    assert got.shape == want.shape and np.array_equal(_u8(got), _u8(want)), np.nonzero(_u8(got).reshape(-1, 16) != _u8(want).reshape(-1, 16))[0][:8]
    mirror = _shape_shim.shape_labels(sl, [fonts[0]] * (base + 1) + [fonts[1]])
    assert np.array_equal(_u8(mirror), _u8(want))
    # the properties themselves, not only agreement
    text_labels_ = [l for l in sl.labels if l["has_text"]]
    for l, r in zip(sl.labels, sl.runs):
        if not l["has_text"] or l["n_segs"] == 0:
            continue
        a, n = int(l["seg_off"]), int(l["n_segs"])
        assert got["kern"][a] == 0  # no kern for the first glyph, whatever stands in front of it in the pool
        pair = -45 if r["font_id"] == base else -17
        for k in (64, 128):
            if k < n:  # "CE" across the 64- and the 128-char mark
                assert got["kern"][a + k] == pair, (n, k)
    ec = int(text_labels_[-4]["seg_off"])  # "EC" behind "ABC": E is a first char, C follows E
    assert sl.chars[ec - 1] == 0x43 and got["kern"][ec : ec + 2].tolist() == [0, 20]
    miss = int(text_labels_[-2]["seg_off"])
    assert got["glyph_id"][miss + 1] == got["glyph_id"][miss + 2] == syn.first_id + SPACE and got["advance"][miss + 1] == 300
    assert got["kern"][miss + 4] == -17  # C | E in font 1 is (4, 6)
    c0, c1 = int(text_labels_[-5]["seg_off"]) + 2, int(text_labels_[-3]["seg_off"]) + 2  # 'C' in font 0 and in font 1
    assert sl.chars[c0] == sl.chars[c1] == 0x43 and got["glyph_id"][c0] != got["glyph_id"][c1]
    assert (got["flags"] == (sl.chars == 0x20)).all() and (got["flags"] == 1).sum() > 50
    # and the placement behind it is the text form's on these records
    tl = sl.to_text_label_list(fonts)
    assert np.array_equal(_u8(tl.glyphs), _u8(got))
    _assert_instances(scene.read_glyph_instances(), placer.place_text_labels(tl).slots)
    segs = scene.read_label_segs()
    out = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    scene.set_text_labels(tl)
    assert len(scene.read_text_glyphs()) == 0
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(segs)) and len(segs) > 1000
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out) and np.array_equal(scene.label_status(), st)
    scene.set_string_labels(None)
    assert len(scene.read_text_glyphs()) == 0 and len(scene.read_glyph_instances()) == 0 and scene.read_label_segs().shape == (0, 4)
    scene.free()


@pytest.mark.parametrize("scale", [1, 2, 4])
def test_string_form_equals_text_form(gpu_ctx, tables, scale):
    syn, ids = tables[2], tables[3]
    kw = dict(labels_per_tile=24, scale=scale, seed=60 + scale, n_images=len(ids), image_sizes=SIZES, line_frac=0.4, empty_frac=0.05)
    sl, font = labels.make_string_labels(8, syn, **kw)
    tl = labels.make_text_labels(8, syn, f32_scale=True, **kw)
    for x in (sl, tl):
        has_icon = x.labels["has_icon"] == 1
        x.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[x.labels["image_id"][has_icon]]
    gpu_ctx.register_font(font)
    sl.with_font(font)
    assert {abi.TEXT_CENTER, abi.TEXT_LINE} == set(sl.runs["position"][sl.labels["has_text"] == 1].tolist())
    assert (sl.labels["has_icon"] == 1).any() and (sl.runs["y_offset"] > 0).any() and (tl.glyphs["kern"] != 0).any()
    dl = synth.config2(8, scale=scale)
    scene = gpu_ctx.upload(dl)
    scene.set_text_labels(tl)
    inst, segs = scene.read_glyph_instances(), scene.read_label_segs()
    out = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    scene.set_string_labels(sl)
    assert np.array_equal(_u8(scene.read_text_glyphs()), _u8(tl.glyphs))
    got = scene.read_glyph_instances()
    assert np.array_equal(_u8(got), _u8(inst)) and {abi.GLYPH_CENTER, abi.GLYPH_LINE, abi.GLYPH_NONE} == set(np.unique(got["form"]).tolist())
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(segs)) and len(segs) > 0
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out)
    assert np.array_equal(scene.label_status(), st) and 0 < st.sum()
    scene.free()
    if scale == 1:  # the one-call entry, into a padded stride
        tight = dl.dim * dl.dim * 3
        stride = tight + 64
        buf = np.full((8, stride), 0x5A, dtype=np.uint8)
        gpu_ctx.render_batch_rgb_strings(dl, sl, out=buf, stride=stride)
        assert np.array_equal(buf[:, :tight].reshape(8, dl.dim, dl.dim, 3), out[..., :3]) and (buf[:, tight:] == 0x5A).all()
        sub = [7, 2, 3]
        assert np.array_equal(gpu_ctx.render_batch_rgb_strings(dl.subset(sub), sl.subset(sub)), buf[sub, :tight])
        assert np.array_equal(gpu_ctx.render_batch_rgb_strings(dl, None), gpu_ctx.render_batch_rgb(dl, None))


@pytest.mark.parametrize("key", ["station", "station_z14_from_the_tile_above"])
def test_station_string_reproduces_the_reference_golden(gpu_ctx, tables, key):
    ref, empty = tables[0], tables[1]
    font = ref_font(first_id=ref.first_id, empty_id=empty.first_id)
    gpu_ctx.register_font(font)
    p = PATCHES[key]
    icon_id = gpu_ctx.register_image(np.array(p["icon_rgba"], dtype=np.uint8))
    sl = station_string_labels(key, font_id=font.font_id, image_id=icon_id)
    dl = TileBuilder(zoom=17, scale=1, canvas=tuple(p["canvas"])).build()
    scene = gpu_ctx.upload(dl)
    scene.set_string_labels(sl)
    assert np.array_equal(_bits(scene.read_label_segs()), _bits(np.array(p["segs"]).reshape(-1, 4)))
    out = gpu_ctx.render(scene).cpu().numpy()
    assert scene.label_status().tolist() == [1]
    (_check if key == "station" else _check_z14)(p, out[0, :, :, :3])
    scene.free()


def test_errors_are_loud_and_a_later_font_leaves_a_set_scene_alone(gpu_ctx, tables):
    syn = tables[2]
    font = _letter_font(syn, 0, [(3, 5, -45)])
    fid = gpu_ctx.register_font(font)
    dl = TileBuilder(zoom=17, scale=1, canvas=(240, 240, 240)).build()
    scene = gpu_ctx.upload(dl)
    good = string_labels([dict(chars="ABC DE", font=fid, font_size=12.0, center=(100.0, 90.0)),
                          dict(chars="CE", font=fid, position=abi.TEXT_LINE, pts=[(10, 10), (60, 20), (120, 20)])])
    cases = [
        (string_labels([dict(chars=[0x41, 0xD800], font=fid)]), "U+D800"),
        (string_labels([dict(chars=[0x41, 0xDFFF], font=fid)]), "U+DFFF"),
        (string_labels([dict(chars="AB", font=0xFFFFFF)]), "font id 16777215"),
        (string_labels([dict(chars="AB", font=fid, font_size=float("nan"))]), "font_size"),
        (string_labels([dict(chars="AB", font=fid, font_size=float("inf"))]), "font_size"),
    ]
    for sl, word in cases:
        scene.set_string_labels(good)
        assert len(scene.read_label_segs()) > 0 and len(scene.read_text_glyphs()) == 8
        with pytest.raises(OsmtError) as ei:
            scene.set_string_labels(sl)
        assert ei.value.code == abi.INVALID_ARG and word in str(ei.value), str(ei.value)
        # the previous labels are gone, nothing stays attached
        assert scene.read_label_segs().shape == (0, 4) and len(scene.read_glyph_instances()) == 0 and len(scene.read_text_glyphs()) == 0
        with pytest.raises(OsmtError) as ei:
            gpu_ctx.validate_string_labels(sl)
        assert ei.value.code == abi.INVALID_ARG and word in str(ei.value)
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.render_batch_rgb_strings(dl, cases[0][0])
    assert ei.value.code == abi.INVALID_ARG
    # a font that names an outline nobody registered
    bad = _letter_font(syn, 0, [])
    bad.outline_id[4] = 0xFFFFFF
    with pytest.raises(OsmtError) as ei:
        gpu_ctx.register_font(bad)
    assert ei.value.code == abi.INVALID_ARG and "glyph 4: outline id 16777215" in str(ei.value)
    # the snapshot rule: fonts registered after the scene was set — its render does not change, and the new ones work
    scene.set_string_labels(good)
    before = gpu_ctx.render(scene).cpu().numpy()
    recs = scene.read_text_glyphs()
    later = [_letter_font(syn, 3 + i, [(3, 5, 60)]) for i in range(3)]
    for f in later:
        gpu_ctx.register_font(f)
    other = gpu_ctx.upload(dl)
    other.set_string_labels(string_labels([dict(chars="ABC DE", font=later[-1].font_id, font_size=12.0, center=(100.0, 90.0))]))
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), before) and np.array_equal(_u8(scene.read_text_glyphs()), _u8(recs))
    assert not np.array_equal(gpu_ctx.render(other).cpu().numpy(), before)
    assert np.array_equal(_u8(other.read_text_glyphs()), _u8(model.shape_text(model.Font(later[-1]), [ord(c) for c in "ABC DE"])))
    other.free()
    scene.free()


def test_every_refusal_through_the_c_abi_names_its_offender():
    """The lists of tests/test_text_shaper_cpu.py on a context of its own (the messages count its fonts and outlines)."""
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)
    L = load()
    try:
        ctx.register_glyphs(labels.GlyphTable([[]] * N_OUTLINES))
        out = C.c_uint32(77)
        for word, edit in FONT_REFUSALS:
            font, desc = refused_font(edit, N_OUTLINES)
            rc = L.osmt_register_font(ctx._h, C.byref(desc), C.byref(out))
            msg = L.osmt_last_error().decode()
            assert rc == abi.INVALID_ARG and word.format(n=N_OUTLINES) in msg, (word, rc, msg)
        assert L.osmt_register_font(ctx._h, None, C.byref(out)) == abi.INVALID_ARG and out.value == 77
        assert [ctx.register_font(valid_font()), ctx.register_font(valid_font())] == [0, 1]  # the refused ones took no id
        ok = valid_strings().as_batch()
        assert L.osmt_validate_string_labels(C.byref(ok), 1, ctx._h) == abi.OK
        assert L.osmt_validate_string_labels(C.byref(ok), 1, None) == abi.INVALID_ARG
        assert L.osmt_validate_string_labels(None, 1, ctx._h) == abi.INVALID_ARG
        for code, word, edit in LABEL_REFUSALS:
            sl = valid_strings()
            edit(sl)
            b = sl.as_batch()
            rc = L.osmt_validate_string_labels(C.byref(b), 1, ctx._h)
            msg = L.osmt_last_error().decode()
            assert rc == code and word in msg, (word, rc, msg)
    finally:
        ctx.close()
