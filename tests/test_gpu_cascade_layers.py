"""The cascade with layer numbers local to a class (osmt_register_rules_ex with OSMT_RULES_CLASS_LAYERS; k_cs_class_layers,
k_cs_count<true>, k_cs_fold<16, true> in osm_renderer_amd/csrc/osmt_cascade.hip): sheets of up to 255 layer names, classes of
up to 16 layers.

As in tests/test_gpu_cascade.py every array of osmt_cascade_read is compared byte for byte with the host mirror
osmt::cascade_host over the classes the device match produced, and selector i of a sheet tests the tag "s<i>".  The sheets and
classes are those of tests/_cascade_layers.py, which tests/test_cascade_layers_cpu.py holds against the Python restatement.
Nothing outside the repository is read."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch, styled
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _cascade as cs
from tests import _cascade_layers as cl
from tests import _labelbind as lb
from tests import _selmatch as sm
from tests import _tilelabels as tl
from tests import _tilequery as tq
from tests._cascade import nums
from tests._styled_feed import geodata_of
from tests.test_gpu_cascade import GPU_SHEET, Case, entity, icons, rule_world, tagged  # noqa: F401  (icons: a fixture)
from tests.test_gpu_label_bindings_matched import tables  # noqa: F401  (a fixture: the font and two icons)

pytestmark = pytest.mark.gpu
A = abi
NODE, WAY, AREA = A.SEL_NODE, A.SEL_WAY, A.SEL_AREA
E = A.TEST_EXISTS
CX, CY = tq.center_z18()


class LCase(Case):
    """tests/test_gpu_cascade.Case with the rules registered with OSMT_RULES_CLASS_LAYERS"""

    def __init__(self, ctx, path, w, sheet, icons=None, font_id=0, casing=2.0, font_mult=None, index=False):
        self.ctx, self.w, self.sheet = ctx, w, sheet
        self.r = w.write(path, tq.max_zoom_tile if index else None)
        self.gid = ctx.register_geodata(geodata_of(self.r))
        t = sm.TagsOf(self.r)
        self.tags = lb.tags_of(t)
        t.close()
        ctx.register_tags(self.gid, self.tags)
        self.sels = cs.selector_set(sheet)
        self.sid = ctx.register_selectors(self.sels)
        self.rules = cs.rule_set(sheet, self.sid, icons, casing, font_mult, font_id)
        self.rid = ctx.register_rules(self.rules, class_layers=True)
        self.m = ctx.match_selectors(self.gid, self.sid)
        self.ent, self.cls, self.pooled = self.m.read()

    def py_classes(self):
        return [(int(c["slot"]), int(c["layer"]) if c["has_layer"] else None, self.pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]].tolist()) for c in self.cls]

    def layer_counts(self):
        return [cl.layer_count(self.sheet, sels) for _, _, sels in self.py_classes()]


def world_of(classes):
    w = sm.World()
    for slot, layer, sels in classes:
        entity(w, slot, layer, sels)
    return w


def case_of(ctx, path, sheet, classes, font):
    return LCase(ctx, path, world_of(classes), tagged(sheet), font_id=font)


@pytest.mark.parametrize("n", [9, 26, 255])
def test_sheets_of_many_names(gpu_ctx, tmp_path, tables, n):
    """classes whose layers have the set-wide numbers 0, 7, 8, 31, 32, 63, 64, 127, 128 and 254 (those the sheet has); in the sheet
    of 255 names "*" carries the highest number"""
    font = tables[0].font_id
    sheet, classes = cl.names_case(n)
    case = case_of(gpu_ctx, tmp_path / "w.bin", sheet, classes, font)
    assert len({s[4] or "default" for ss, _ in case.sheet for s in ss}) == n and max(case.layer_counts()) == min(n, 16)
    for labels_all in (True, False):
        got = case.check(labels_all)
        cs.same_as_py(got, cs.py_cascade(case.sheet, case.py_classes()), labels_all, font)
    assert len(got.styles) > len(classes) // 4
    case.close()


def test_layers_per_class(gpu_ctx, tmp_path, tables):
    """classes of 1 .. 16 layers; "*" absent, first, in the middle, last, at some zooms only; "default" spelled out and implied; a
    layer created after "*"; two classes with the same layers met in opposite order; labels_all 0 and 1; two runs and the hash cut
    down give identical bytes"""
    font = tables[0].font_id
    sheet, classes = cl.layers_case()
    case = case_of(gpu_ctx, tmp_path / "w.bin", sheet, classes, font)
    assert sorted(set(case.layer_counts())) == list(range(17))
    for labels_all in (True, False):
        got = case.check(labels_all)
        py = cs.py_cascade(case.sheet, case.py_classes())
        cs.same_as_py(got, py, labels_all, font)
        assert max(len(x) for per_zoom in py for x in per_zoom) == 16
        for bits in (0, 1, 8, 32):
            gpu_ctx.debug_match_hash_bits(bits)
            try:
                cs.same_bytes(case.device(labels_all), got)
            finally:
                gpu_ctx.debug_match_hash_bits(32)
    assert len(got.zoom_lo) > 3
    case.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_class_counts_at_the_wave_edges_of_the_per_class_kernel(gpu_ctx, tmp_path, n):
    """n classes over the sheet of 26 names: one of untagged nodes, the others ways that differ in their layer tag"""
    sheet, _ = cl.names_case(26)
    w = sm.World()
    if n == 1:
        w.node()
    for k in range(n - 1):
        entity(w, 2, k - 7, sorted({0, 1, 2 + k % 24, 2 + (k // 24) % 24, 2 + (k // 576) % 24}))
    case = LCase(gpu_ctx, tmp_path / "w.bin", w, tagged(sheet))
    assert len(case.cls) == n
    got = case.check()
    if n > 1:
        assert len(got.styles) >= n - 1
    else:
        assert len(got.styles) == 0 and got.zoom_lo.tolist() == [0] and got.zoom_hi.tolist() == [18]
    case.close()


def test_a_long_class(gpu_ctx, tmp_path, tables):
    """300 selectors cycling over 16 of 255 names"""
    sheet, classes = cl.long_case()
    case = case_of(gpu_ctx, tmp_path / "w.bin", sheet, classes, tables[0].font_id)
    assert max(int(c["n_sels"]) for c in case.cls) == 300 and max(case.layer_counts()) == 16
    case.check(True)
    case.check(False)
    case.close()


@pytest.mark.parametrize("labels_all", [True, False])
def test_eight_names_give_the_same_bytes_with_and_without_the_flag(gpu_ctx, tmp_path, icons, tables, labels_all):
    case = Case(gpu_ctx, tmp_path / "w.bin", rule_world(), tagged(GPU_SHEET), icons, tables[0].font_id, 2.0, 1.5)
    flagged = gpu_ctx.register_rules(case.rules, class_layers=True)
    assert flagged != case.rid
    plain = case.device(labels_all)
    c = case.m.cascade(flagged, labels_all)
    try:
        cs.same_bytes(c.read(), plain)
    finally:
        c.close()
    cs.same_bytes(plain, case.mirror(labels_all))
    case.close()


def test_a_class_of_17_layers_is_refused_and_named(gpu_ctx, tmp_path):
    L = lib.load()
    sheet, classes = cl.layers_case()
    for bad_sels in ([cl.PLAIN[:17]], [cl.PLAIN[:20], cl.PLAIN[2:19]]):
        world = classes[:20] + [(2, 5, s) for s in bad_sels] + classes[20:]
        case = LCase(gpu_ctx, tmp_path / f"w{len(bad_sels)}.bin", world_of(world), tagged(sheet))
        counts = case.layer_counts()
        over = [i for i, k in enumerate(counts) if k > 16]
        assert sorted(counts[i] for i in over) == ([17] if len(bad_sels) == 1 else [17, 20]) and len(counts) > 30  # among good ones
        before = gpu_ctx.register_styles(np.zeros(1, styled.STYLE_REC_DTYPE))
        h = C.c_void_p(1)
        assert L.osmt_cascade_classes(gpu_ctx._h, case.m._h, case.rid, 1, C.byref(h)) == A.UNSUPPORTED
        msg = L.osmt_last_error().decode()
        assert not h.value
        # the lowest offending class, with its exact count
        assert f"class {over[0]} name {counts[over[0]]} distinct layers (> OSMT_CASCADE_MAX_CLASS_LAYERS = 16)" in msg, msg
        with pytest.raises(OsmtError) as e:
            case.m.cascade(case.rid, False)
        assert e.value.code == A.UNSUPPORTED and f"class {over[0]} " in str(e.value)
        assert gpu_ctx.register_styles(np.zeros(1, styled.STYLE_REC_DTYPE)) == before + 1  # nothing was registered
        case.close()
        # a good cascade on the same context follows
        case = LCase(gpu_ctx, tmp_path / f"v{len(bad_sels)}.bin", world_of(classes[:24]), tagged(sheet))
        case.check()
        case.close()


def test_nine_names_need_the_flag(gpu_ctx):
    sheet = tagged(cl.names_case(9)[0])
    sid = gpu_ctx.register_selectors(cs.selector_set(sheet))
    with pytest.raises(OsmtError, match=r"9 distinct layer names \(> OSMT_CASCADE_MAX_LAYERS = 8\)") as e:
        gpu_ctx.register_rules(cs.rule_set(sheet, sid))
    assert e.value.code == A.UNSUPPORTED
    gpu_ctx.validate_rules(cs.rule_set(sheet, sid), class_layers=True)
    rid = gpu_ctx.register_rules(cs.rule_set(sheet, sid), class_layers=True)
    assert gpu_ctx.register_rules(cs.rule_set(sheet, sid), class_layers=True) == rid + 1
    # what needs the context is checked by the _ex forms as by the old ones; an unknown flag is refused before anything else
    rules = cs.rule_set(sheet, 10 ** 6)
    with pytest.raises(OsmtError, match="selectors id 1000000 is not registered"):
        gpu_ctx.validate_rules(rules, class_layers=True)
    out = C.c_uint32()
    d = rules.as_desc()
    assert lib.load().osmt_register_rules_ex(gpu_ctx._h, C.byref(d), 2, C.byref(out)) == A.INVALID_ARG and b"flags = 0x2" in lib.load().osmt_last_error()


def test_scene_from_a_sheet_of_26_names_equals_the_scene_from_the_mirrors_arrays(gpu_ctx, tmp_path, tables):
    """the world of tests/test_gpu_cascade.test_scenes_from_rules_equal_scenes_from_the_mirrors_arrays at one zoom, its sheet
    written over the 26 names of the reference's sheet: once through osmt_cascade_register, once through the mirror's arrays handed
    to the existing registrations; styled areas, display list, both label batches and the pixels agree"""
    font, icon_ids = tables
    f = font.font_id
    words = ["CAFE", "BAKED", "A", "HIGH GLADE", "", "LAKE", "BIG FIELD"]
    w = sm.World()
    node_fn = lambda la, lo: w.node(None, la, lo)
    for k in range(40):
        ids = tq.square(node_fn, k)
        t = {"name": words[k % len(words)]} if k % 4 else {}
        if k % 3 == 0:
            t["highway" if k % 2 else "building"] = "yes"
        if k % 5 == 0:
            t["ref"] = "A" * (1 + k % 3)
        w.way(ids if k % 2 else ids[:3], t)
        if k % 6 == 0:
            w.nodes[ids[0]][3].update({"name": words[(k + 2) % len(words)], "shop": "yes"} if k % 12 else {"shop": "yes"})
    for m in range(8):
        w.polygons.append(tq.square(node_fn, 3 * m + 1, size=0.0007))
        w.mps.append((9000 + m, [len(w.polygons) - 1], {"name": words[(m + 3) % len(words)], "building": "yes"} if m % 3 else {"building": "yes"}))
    # every name of the reference's sheet is named once by a selector nothing matches, in the sheet's order, so the layers below
    # carry their set-wide numbers: "*" 1, "casing1" 15, "access" 17, "tram" 22, "ele" 25
    sheet = [([(WAY, [(E, f"nothing{k}")], None, None, nm)], [("width", nums(1.0))]) for k, nm in enumerate(cl.REF_NAMES)] + [
        ([(WAY, [], None, None, "*")], [("linecap", ("id", "round")), ("text-color", ("color", (150, 20, 60)))]),
        ([(AREA, [(A.TEST_EQUAL, "building", "yes")], None, None, None)], [("fill-color", ("color", (170, 200, 150))), ("z-index", nums(2.0))]),
        ([(AREA, [(A.TEST_EQUAL, "building", "yes")], 17, None, "ele")], [("text", ("id", "name")), ("font-size", nums(9.0)), ("text-position", ("id", "center"))]),
        ([(WAY, [(E, "highway")], None, None, "casing1")], [("color", ("id", "red")), ("width", nums(3.0)), ("casing-width", nums(1.0)), ("casing-color", ("id", "navy"))]),
        ([(WAY, [(E, "highway")], None, 17, "access")], [("text", ("id", "name")), ("font-size", nums(11.0))]),
        ([(WAY, [(E, "ref")], 17, None, "tram")], [("text", ("str", "ref")), ("font-size", nums(13.0)), ("dashes", nums(4, 2)), ("width", nums(1.0)), ("color", ("id", "white"))]),
        ([(NODE, [(E, "shop")], None, None, None)], [("icon-image", ("str", "shop.png")), ("text", ("id", "name")), ("font-size", nums(9.0))]),
        ([(NODE, [(E, "shop")], 17, 17, "tram_under3")], [("icon-image", ("str", "dot.png"))]),
    ]
    icons_of = {"shop.png": icon_ids[0], "dot.png": icon_ids[1]}
    case = LCase(gpu_ctx, tmp_path / "w.bin", w, sheet, icons_of, f, 2.0, None, index=True)
    gpu_ctx.register_tile_index(case.gid, tq.index_of(w.refs))
    gpu_ctx.register_node_mercator(case.gid, an.mercator_factors(case.r.node_table()))
    gpu_ctx.register_node_index(case.gid, tl.node_index_of(case.r, w.refs))
    zoom = 17
    # 1. the device's way
    c = case.m.cascade(case.rid, False)
    got = c.read()
    want = case.mirror(False)
    cs.same_bytes(got, want)
    d_bind, d_node, d_area = c.register(A.CASCADE_AREA_STYLES | A.CASCADE_NODE_LABELS | A.CASCADE_AREA_LABELS)
    c.close()
    assert (d_bind != A.BINDINGS_NONE).all()
    # 2. the mirror's arrays through the existing calls
    s0 = gpu_ctx.register_styles(want.styles, want.dashes)
    l0 = gpu_ctx.register_label_styles(want.label_styles)
    r = want.range_of(zoom)
    h_bind = case.m.register_style_bindings(zoom, zoom, [[s0 + i for i in row] for row in want.class_styles_of(r)])
    b = selmatch.ClassLabelBindings(zoom, zoom, [[(l0 + i, k) for i, k in row] for row in want.class_bindings_of(r)], want.keys())
    h_node = case.m.register_label_bindings(zoom, zoom, b)
    h_area = case.m.register_area_label_bindings(zoom, zoom, b)
    sh = 18 - zoom
    tiles = [(zoom, CX >> sh, CY >> sh), (zoom, (CX >> sh) + 1, CY >> sh)]
    out = []
    for bind, node, area in (({zoom: int(d_bind[zoom])}, {zoom: int(d_node[zoom])}, {zoom: int(d_area[zoom])}), ({zoom: h_bind}, {zoom: h_node}, {zoom: h_area})):
        sc = gpu_ctx.build_tiles(styled.TileBatch(case.gid, tiles, bind))
        st_tiles, st_areas = sc.read_styled_areas()
        dl = sc.read_display_list()
        a, n = sc.build_tile_labels_all(area, node)
        out.append((st_tiles, st_areas, dl, n, a, gpu_ctx.render(sc).cpu().numpy()))
        sc.free()
    x, y = out
    assert x[0].tobytes() == y[0].tobytes() and len(x[1]) == len(y[1]) > 10
    assert x[1]["entity"].tobytes() == y[1]["entity"].tobytes()
    for name in ("jobs", "ops", "rings", "coords", "dashes"):
        assert np.asarray(getattr(x[2], name)).tobytes() == np.asarray(getattr(y[2], name)).tobytes(), name
    assert len(x[3].labels) > 0 and len(x[4].labels) > 5 and x[4].labels["has_text"].any()
    for g, h in ((x[3], y[3]), (x[4], y[4])):
        assert g.job_label_off.tobytes() == h.job_label_off.tobytes()
        for name in ("labels", "runs", "chars", "way_pts", "way_sincos"):
            assert getattr(g, name).tobytes() == getattr(h, name).tobytes(), name
    assert np.array_equal(x[5], y[5]) and len(np.unique(x[5].reshape(-1, x[5].shape[-1]), axis=0)) > 3
    case.close()
