"""k_text_place and k_text_shape at wave, chunk, block and table edges, on the GPU through the C ABI.

The cases are those of tests/_text_place_cases.py and tests/_text_shape_cases.py, which the host tests run against the
host mirrors (tests/test_text_placer_cpu.py, tests/test_text_shaper_cpu.py) and tests/test_text_edge_cases_cpu.py proves
to sit on the edges they name: a row break, a hit edge, seg_dist == to_travel and an advance <= 0 at lane 63, lane 64
and the first lane of a later chunk; cmap tables of 1 .. 1025 entries, glyph indices beyond 16 bits, all 25 White_Space
code points, kern pairs across the borders of a block of 256 chars and across label boundaries there.

  * placer: every case alone and all of them as one batch — osmt_scene_read_glyph_instances equals the Python model bit for
    bit, unused entries zero, and holds the case's literal expectations;
  * shaper: osmt_scene_read_text_glyphs equals the Python model byte for byte and holds the case's literal expectations;
    the instances behind it are the placer model's on those records;
  * the batch of nine labels, set on a scene that held a larger batch before: draw_line arena, pixels and statuses equal
    those of the same scene with the model's instances as glyph runs.

No tolerances: every comparison is on bytes or bits."""
import numpy as np
import pytest

from osm_renderer_amd import labels, synth
from tests import _text_place_cases as pc
from tests import _text_placer_model as placer
from tests import _text_shape_cases as sc
from tests import _text_shaper_model as shaper
from tests.test_glyph_runs_cpu import fixture_table
from tests.test_gpu_text_labels import _assert_instances

pytestmark = pytest.mark.gpu

PLACE = pc.cases()
SHAPE = sc.cases()


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def syn(gpu_ctx):
    table = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(table)
    return table


@pytest.fixture(scope="module")
def outlines(gpu_ctx):
    """Registered outline ids for the shaper cases: the reference fixture's glyphs, and 1040 outlines without a shape."""
    ref = fixture_table()
    gpu_ctx.register_glyphs(ref)
    blank = labels.GlyphTable([[]] * 1040)
    gpu_ctx.register_glyphs(blank)
    return sc.Outlines(base=blank.first_id, one=blank.first_id + 9, ref_first=ref.first_id, ref_empty=blank.first_id)


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    s = gpu_ctx.upload(synth.config2(1))
    yield s
    s.free()


# ---- k_text_place -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PLACE, ids=[c.name for c in PLACE])
def test_placer_case_alone(syn, scene, case):
    tl = case.build(syn.first_id)
    gl = placer.place_text_labels(tl)
    scene.set_text_labels(tl)
    got = scene.read_glyph_instances()
    _assert_instances(got, gl.slots)
    case.check(got, gl, syn.first_id)


def test_every_placer_case_in_one_batch(syn, scene):
    tl, spans = pc.merge([c.build(syn.first_id) for c in PLACE])
    gl = placer.place_text_labels(tl)
    scene.set_text_labels(tl)
    got = scene.read_glyph_instances()
    _assert_instances(got, gl.slots)
    for c, (a, n) in zip(PLACE, spans):
        c.check(got[a : a + n], None, syn.first_id)


@pytest.mark.parametrize("name", ["batch-of-nine", "batch-of-nine-reversed-pool"])
def test_mixed_batch_renders_as_the_models_glyph_runs(gpu_ctx, syn, name):
    """Waves that return at once (no text, no glyphs, a way of one point) beside waves that run long: no slot keeps what
    the batch before left in it, and everything downstream of the instances follows."""
    scene = gpu_ctx.upload(synth.config2(1))
    before, _ = pc.merge([c.build(syn.first_id) for c in PLACE])
    scene.set_text_labels(before)
    assert len(scene.read_glyph_instances()) == len(before.glyphs)
    case = pc.case(name)
    tl = case.build(syn.first_id)
    gl = placer.place_text_labels(tl)
    scene.set_text_labels(tl)
    got = scene.read_glyph_instances()
    _assert_instances(got, gl.slots)
    case.check(got, gl, syn.first_id)
    segs = scene.read_label_segs()
    out = gpu_ctx.render(scene).cpu().numpy()
    st = scene.label_status()
    scene.set_glyph_labels(gl)
    assert len(scene.read_glyph_instances()) == 0
    assert len(segs) > 1000 and np.array_equal(_bits(scene.read_label_segs()), _bits(segs))
    assert np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out) and np.array_equal(scene.label_status(), st)
    assert len(st) == 9
    ll = gl.to_label_list(syn)  # the host expansion of the model's instances
    assert segs.shape == ll.segs.shape and np.array_equal(_bits(segs), _bits(ll.segs))
    scene.set_text_labels(None)
    assert not np.array_equal(gpu_ctx.render(scene).cpu().numpy(), out)  # the labels drew something
    scene.free()


# ---- k_text_shape -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPE, ids=[c.name for c in SHAPE])
def test_shaper_case(gpu_ctx, outlines, scene, case):
    sl, fonts = case.build(outlines)
    for f in fonts:
        gpu_ctx.register_font(f)
    sc.bind_fonts(sl, fonts)
    want = shaper.shape_labels(sl, {f.font_id: shaper.Font(f) for f in fonts})
    scene.set_string_labels(sl)
    got = scene.read_text_glyphs()
    assert got.shape == want.shape
    bad = np.nonzero((_u8(got).reshape(-1, 16) != _u8(want).reshape(-1, 16)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(got)} records differ from the model, first at slot {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    case.check(got, outlines)
    # and the placement behind it is the text form's on these records
    tl = sl.to_text_label_list(fonts)
    assert np.array_equal(_u8(tl.glyphs), _u8(got))
    _assert_instances(scene.read_glyph_instances(), placer.place_text_labels(tl).slots)
