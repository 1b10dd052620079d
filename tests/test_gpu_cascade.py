"""The cascade on the device (osmt_register_rules, osmt_cascade_classes, osmt_cascade_read, osmt_cascade_register;
osm_renderer_amd/csrc/osmt_cascade.hip).

Every array of osmt_cascade_read is compared byte for byte with the host mirror osmt::cascade_host
(host/osmt_cascade.hpp, through tests/cascade_shim.cpp) over the classes the device match produced; tests/test_cascade_cpu.py
holds that mirror against a Python restatement of the reference's styler.  Worlds are written with tests/_geodata.write_geodata:
selector i of a sheet tests the tag "s<i>", so an entity's tags choose the selectors it matches.  Nothing outside the
repository is read."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch, styled
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _cascade as cs
from tests import _labelbind as lb
from tests import _selmatch as sm
from tests import _tilelabels as tl
from tests import _tilequery as tq
from tests._styled_feed import geodata_of
from tests._cascade import CLASSES, SHEET, fma_triple, nums, sel
from tests.test_gpu_label_bindings_matched import tables  # noqa: F401  (a fixture: the font and two icons)

pytestmark = pytest.mark.gpu
A = abi
NODE, WAY, AREA = A.SEL_NODE, A.SEL_WAY, A.SEL_AREA
E = A.TEST_EXISTS
CX, CY = tq.center_z18()


def tagged(sheet):
    """the sheet with selector i testing [s<i>], once for ways and multipolygons and once more for nodes (same rule, layer, zooms)"""
    out, i = [], 0
    for sels, props in sheet:
        both = []
        for s in sels:
            both.append((WAY, [(E, f"s{i}")], s[2], s[3], s[4]))
            i += 1
        both += [(NODE, t, lo, hi, layer) for _, t, lo, hi, layer in both]
        out.append((both, props))
    return out


def entity(w, slot, layer, sels):
    tags = {f"s{i}": "1" for i in sels}
    if layer is not None:
        tags["layer"] = str(layer)
    (w.node, w.closed_way, w.open_way, w.mp)[slot](tags)


@pytest.fixture(scope="module")
def icons(gpu_ctx):
    ids = [gpu_ctx.register_image(np.full((4, 4, 4), 40 * k + 15, np.uint8)) for k in range(2)]
    return {"pin.png": ids[0], "grass": ids[1]}


class Case:
    """a world registered with its tags, a tagged sheet registered as selectors and rules, the match"""

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
        self.rid = ctx.register_rules(self.rules)
        self.m = ctx.match_selectors(self.gid, self.sid)
        self.ent, self.cls, self.pooled = self.m.read()

    def mirror(self, labels_all=True):
        return cs.mirror(self.rules, self.sels, self.cls, self.pooled, labels_all)

    def device(self, labels_all=True):
        c = self.m.cascade(self.rid, labels_all)
        try:
            return c.read()
        finally:
            c.close()

    def check(self, labels_all=True):
        got, want = self.device(labels_all), self.mirror(labels_all)
        cs.same_bytes(got, want)
        cs.canonical(got)
        return got

    def close(self):
        self.m.close()
        self.r.close()


# osmt_validate_styles refuses Some([]) as a dash list, so the produced-record check would refuse the whole cascade: the device
# world leaves that one property out (tests/test_cascade_cpu.py keeps it for the mirror)
GPU_SHEET = [(sels, [p for p in props if p != ("casing-dashes", ("nums", []))]) for sels, props in SHEET]


def rule_world():
    w = sm.World()
    for slot, layer, sels in CLASSES:
        entity(w, slot, layer, sels)
        entity(w, slot, layer, sels)  # a second member changes nothing
    return w


@pytest.mark.parametrize("labels_all", [True, False])
def test_the_cases_of_the_rule_in_one_world(gpu_ctx, tmp_path, icons, tables, labels_all):
    font = tables[0].font_id
    case = Case(gpu_ctx, tmp_path / "w.bin", rule_world(), tagged(GPU_SHEET), icons, font, 2.0, 1.5)
    got = case.check(labels_all)
    # the device's classes are those of the CPU test (plus the untagged nodes of the ways): the same styles come out
    py = cs.py_cascade(case.sheet, [(int(c["slot"]), int(c["layer"]) if c["has_layer"] else None, case.pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]].tolist())
                                    for c in case.cls], icons, 2.0, 1.5)
    cs.same_as_py(got, py, labels_all, font)
    assert max(len(x) for per_zoom in py for x in per_zoom) == 7 and len(got.zoom_lo) == 5
    # Numbers of length 0 / 1 / 2 for every numeric name, and the casing number over default's width: classes 12, 14 and 20 .. 23 of CLASSES,
    # found among the device's classes by their slot and selectors, come to what tests/_cascade.numeric_cases states
    sel_id, pos = {}, 0
    for sels, _ in GPU_SHEET:
        for k in range(len(sels)):
            sel_id[len(sel_id)] = pos + k
        pos += 2 * len(sels)  # the way copies, then the node copies
    found = {(int(c["slot"]), tuple(case.pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]].tolist())): i for i, c in enumerate(case.cls)}
    cs.numeric_cases({k: py[found[(CLASSES[k][0], tuple(sorted(sel_id[x] for x in CLASSES[k][2])))]] for k in (12, 14, 20, 21, 22, 23)}, 2.0, 1.5)
    # two runs, and the hash cut down: identical bytes
    for bits in (0, 1, 8, 32):
        gpu_ctx.debug_match_hash_bits(bits)
        try:
            cs.same_bytes(case.device(labels_all), got)
        finally:
            gpu_ctx.debug_match_hash_bits(32)
    case.close()


def test_unfused_casing_width_on_the_device(gpu_ctx, tmp_path):
    base, wv = fma_triple(3.0)
    assert cs.fma(3.0, wv, base) != base + 3.0 * wv
    sheet = tagged([([sel()], [("width", nums(base)), ("casing-width", nums(wv))])])
    w = sm.World()
    entity(w, 2, None, [0])
    case = Case(gpu_ctx, tmp_path / "w.bin", w, sheet, casing=3.0)
    got = case.check()
    cw = [float(x) for x in got.styles["casing_width"][got.styles["has_casing_width"] == 1]]
    assert [cs.bits(x) for x in cw] == [cs.bits(base + 3.0 * wv)]
    case.close()


LAYERS = [None, "*", "a", "b", "c", "d", "e", "f"]  # eight names with "default"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_class_counts(gpu_ctx, tmp_path, n):
    """n classes: one of untagged nodes, the others ways that differ in their layer tag, so every class has records of its own"""
    sheet = tagged([([sel(L, lo, None)], [("width", nums(1.0 + k)), ("text", ("id", "name"))]) for k, (L, lo) in enumerate(zip(LAYERS, [None, 3, None, 9, 9, 12, None, 15]))])
    w = sm.World()
    if n == 1:
        w.node()
    for k in range(n - 1):
        entity(w, 2, k - 7, [0, 1, 2 + k % 6, 2 + (k // 6) % 6])
    case = Case(gpu_ctx, tmp_path / "w.bin", w, sheet)
    assert len(case.cls) == n
    got = case.check()
    if n > 1:
        assert len(got.styles) >= n - 1 and len(got.zoom_lo) >= 4
    else:
        assert len(got.styles) == 0 and got.zoom_lo.tolist() == [0] and got.zoom_hi.tolist() == [18]
    case.close()


def test_selector_counts_and_layers_per_class(gpu_ctx, tmp_path, tables):
    """classes with 0, 1, 2, 16 and 300 selectors, and with 1 .. 8 layers"""
    rules = [([sel(LAYERS[k % 8], k % 5 if k % 3 == 0 else None, 18 - k % 7 if k % 4 == 0 else None)],
              [(A.PROP_NAMES[(k + j) % 20], [nums(float(k)), ("id", "round"), ("color", (k % 256, 1, 2)), ("delta", 0.5), nums(1, k)][(k + j) % 5]) for j in range(k % 4)])
             for k in range(300)]
    w = sm.World()
    for k in (0, 1, 2, 16, 300):
        entity(w, 2, None, range(k))
        entity(w, 3, 2, range(300 - k, 300))
    for k in range(1, 9):
        entity(w, 1, None, [0] + [j for j in range(1, 8) if j < k])  # "default", then "*", "a", ...
    case = Case(gpu_ctx, tmp_path / "w.bin", w, tagged(rules), font_id=tables[0].font_id)
    assert sorted({int(c["n_sels"]) for c in case.cls if c["slot"] == 2}) == [0, 1, 2, 16, 300]
    case.check(True)
    case.check(False)
    case.close()


def zoom_world():
    w = sm.World()
    for k in range(5):
        entity(w, 2, k, [0, 1])
    return w


def test_zoom_ranges(gpu_ctx, tmp_path, tables):
    font = tables[0].font_id
    # all 19 zooms identical
    case = Case(gpu_ctx, tmp_path / "a.bin", zoom_world(), tagged([([sel()], [("width", nums(2.0))]), ([sel("x")], [("color", ("color", (1, 2, 3)))])]))
    assert case.check().zoom_lo.tolist() == [0]
    case.close()
    # all 19 different
    sheet = [([sel(None, z, z)], [("width", nums(1.0 + z))]) for z in range(19)]
    w = sm.World()
    entity(w, 2, None, range(19))
    entity(w, 1, None, [3])
    case = Case(gpu_ctx, tmp_path / "b.bin", w, tagged(sheet))
    assert case.check().zoom_lo.tolist() == list(range(19))
    case.close()
    # a split only because of a label style: the area records of both zoom halves are the same
    sheet = [([sel()], [("width", nums(2.0)), ("text", ("id", "name"))]), ([sel(None, 12)], [("font-size", nums(9.0))])]
    case = Case(gpu_ctx, tmp_path / "c.bin", zoom_world(), tagged(sheet), font_id=font)
    got = case.check()
    assert got.zoom_lo.tolist() == [0, 12] and len(got.styles) == 5 and len(got.label_styles) == 10
    assert got.class_styles_of(0) == got.class_styles_of(1)
    # ... and without labels for styles that draw nothing the key still splits them; a sheet without text does not split at all
    case.close()
    sheet = [([sel()], [("width", nums(2.0))]), ([sel(None, 12)], [("font-size", nums(9.0))])]
    case = Case(gpu_ctx, tmp_path / "d.bin", zoom_world(), tagged(sheet))
    assert case.check(True).zoom_lo.tolist() == [0] and case.check(False).zoom_lo.tolist() == [0]
    assert len(case.device(False).bindings) == 0
    case.close()


def test_4097_users_of_one_record_and_records_one_byte_apart(gpu_ctx, tmp_path):
    # 256 classes (subsets of eight selectors whose rule sets nothing that is read) x 19 zooms use one record
    sheet = [([sel()], [("width", nums(2.0))])] + [([sel()], [("linejoin", ("id", "round"))]) for _ in range(8)]
    w = sm.World()
    for k in range(256):
        entity(w, 2, None, [0] + [1 + j for j in range(8) if k >> j & 1])
    case = Case(gpu_ctx, tmp_path / "a.bin", w, tagged(sheet))
    got = case.check()
    assert len(case.cls) == 257 and len(got.styles) == 1 and len(got.label_styles) == 1 and len(got.class_styles) == 256 and 256 * 19 >= 4097
    case.close()
    # records that differ in one byte of one field, or in the last bit of a number, or in one dash
    one = np.nextafter(1.0, 2.0)
    variants = [[("color", ("color", (1, 2, 3)))], [("color", ("color", (1, 2, 4)))], [("width", nums(1.0))], [("width", nums(one))], [("dashes", nums(4, 2))],
                [("dashes", nums(4, one))], [("casing-dashes", nums(4, 2))], [("linecap", ("id", "round"))], [("linecap", ("id", "square"))],
                [("fill-position", ("id", "background"))], [("dashes", nums(4, 2)), ("opacity", nums(1.0))], [("dashes", nums(2, 2, 2)), ("dashes", nums(4, 2))]]
    w = sm.World()
    for k in range(len(variants)):
        entity(w, 2, None, [k])
    case = Case(gpu_ctx, tmp_path / "b.bin", w, tagged([([sel()], v) for v in variants]))
    got = case.check()
    assert len(got.styles) == len(variants) - 1  # the last is the fifth written twice: equal dashes in another place of the pool
    case.close()


def test_4097_distinct_records(gpu_ctx, tmp_path):
    w = sm.World()
    for k in range(4097):
        entity(w, 2, k, [0])
    case = Case(gpu_ctx, tmp_path / "w.bin", w, tagged([([sel()], [("width", nums(2.0)), ("text", ("str", "name"))])]))
    got = case.check()
    assert len(got.styles) == 4097 and len(got.label_styles) == 4097 and got.styles["layer"].tolist() == list(range(4097))
    case.close()


def test_a_refused_style_names_its_lowest_user_and_registers_nothing(gpu_ctx, tmp_path):
    sheet = [([sel()], [("width", nums(2.0))]), ([sel("x", 7)], [("opacity", nums(5e15))])]  # opacity beyond 2^52: osmt_validate_styles refuses
    w = sm.World()
    entity(w, 2, None, [0])
    entity(w, 2, None, [0, 1])
    entity(w, 1, None, [0, 1])
    case = Case(gpu_ctx, tmp_path / "w.bin", w, tagged(sheet))
    before = gpu_ctx.register_styles(np.zeros(1, styled.STYLE_REC_DTYPE))
    with pytest.raises(OsmtError) as e:
        case.m.cascade(case.rid)
    bad_class = min(i for i, c in enumerate(case.cls) if c["n_sels"] == 2)
    assert e.value.code == A.INVALID_ARG and "opacity must be in [0, 2^52]" in str(e.value)
    assert f"class {bad_class} at zoom 7, layer position 1" in str(e.value)
    assert gpu_ctx.register_styles(np.zeros(1, styled.STYLE_REC_DTYPE)) == before + 1
    case.close()
    # a good cascade follows
    case = Case(gpu_ctx, tmp_path / "v.bin", zoom_world(), tagged([([sel()], [("width", nums(2.0))])]))
    case.check()
    case.close()


def test_refusals_of_the_calls(gpu_ctx, tmp_path):
    from osm_renderer_amd.renderer import Context

    L = lib.load()
    case = Case(gpu_ctx, tmp_path / "w.bin", zoom_world(), tagged([([sel()], [("width", nums(2.0))])]))

    def refused(word, ctx_h=None, match_h=None, rid=None, labels_all=1):
        h = C.c_void_p(1)
        assert L.osmt_cascade_classes(ctx_h or gpu_ctx._h, match_h or case.m._h, case.rid if rid is None else rid, labels_all, C.byref(h)) == A.INVALID_ARG
        assert word in L.osmt_last_error().decode(), L.osmt_last_error()
        assert not h.value

    stranger = Context(0)
    refused("another context", ctx_h=stranger._h)
    stranger.close()
    refused("is not registered", rid=10 ** 6)
    refused("labels_all = 2", labels_all=2)
    other = gpu_ctx.match_selectors(case.gid, gpu_ctx.register_selectors(case.sels))  # equal selectors, another set
    refused("the rules are over set", match_h=other._h)
    w = sm.World()
    w.open_way({"lanes": "1e23"})
    r = w.write(tmp_path / "d.bin")
    gid = gpu_ctx.register_geodata(geodata_of(r))
    t = sm.TagsOf(r)
    gpu_ctx.register_tags(gid, t.desc())
    sid = gpu_ctx.register_selectors(selmatch.SelectorSet([(WAY, [(A.TEST_GREATER, "lanes", 2.0)])]))
    h = C.c_void_p()
    assert L.osmt_match_selectors(gpu_ctx._h, gid, sid, None, 0, C.byref(h)) == A.UNSUPPORTED and h.value
    refused("declined state", match_h=h)
    L.osmt_match_free(h)
    t.close()
    r.close()
    # registration: what needs the context
    for edit, word in ((lambda r: setattr(r, "selectors_id", 10 ** 6), "selectors id"), (lambda r: setattr(r, "font_id", 10 ** 6), None)):
        rules = cs.rule_set(case.sheet, case.sid)
        edit(rules)
        if word:
            with pytest.raises(OsmtError, match=word):
                gpu_ctx.register_rules(rules)
        else:
            gpu_ctx.register_rules(rules)  # no rule writes font-size: the font is not asked for
    with pytest.raises(OsmtError, match="selectors, the selector set"):
        gpu_ctx.register_rules(cs.rule_set(case.sheet[:0], case.sid))
    with pytest.raises(OsmtError, match="font_id 1000000 is not registered"):
        gpu_ctx.register_rules(cs.rule_set(tagged([([sel()], [("font-size", nums(2.0))])]), case.sid, font_id=10 ** 6))
    with pytest.raises(OsmtError, match="image 1000000 is not registered"):
        gpu_ctx.register_rules(cs.rule_set(tagged([([sel()], [("icon-image", ("str", "x"))])]), case.sid, {"x": 10 ** 6}))
    # read: a short cap; register: no table asked for, unknown bits, a match the cascade was not made from, another context
    c = case.m.cascade(case.rid)
    counts, caps = (C.c_size_t * 9)(), (C.c_size_t * 8)()
    st = np.zeros(8, styled.STYLE_REC_DTYPE)
    assert L.osmt_cascade_read(c._h, C.c_void_p(st.ctypes.data), *([None] * 12), caps, counts) == A.INVALID_ARG and counts[0] == 5
    ids = np.zeros(19, np.uint32)
    p = C.c_void_p(ids.ctypes.data)
    assert L.osmt_cascade_register(gpu_ctx._h, c._h, case.m._h, 0, p, p, p) == A.INVALID_ARG
    assert L.osmt_cascade_register(gpu_ctx._h, c._h, case.m._h, 8, p, p, p) == A.INVALID_ARG and b"OSMT_CASCADE_* bits" in L.osmt_last_error()
    assert L.osmt_cascade_register(gpu_ctx._h, c._h, other._h, A.CASCADE_AREA_STYLES, p, p, p) == A.INVALID_ARG
    assert b"not the one the cascade was made from" in L.osmt_last_error()
    stranger = Context(0)
    assert L.osmt_cascade_register(stranger._h, c._h, case.m._h, A.CASCADE_AREA_STYLES, p, p, p) == A.INVALID_ARG and b"another context" in L.osmt_last_error()
    stranger.close()
    assert (ids == 0).all()  # a refused call fills nothing
    assert L.osmt_cascade_register(gpu_ctx._h, c._h, case.m._h, A.CASCADE_AREA_STYLES, None, None, None) == A.INVALID_ARG
    c.close()
    other.close()
    case.close()


def test_scenes_from_rules_equal_scenes_from_the_mirrors_arrays(gpu_ctx, tmp_path, tables):
    """the small world of the label-bindings scene test, three zooms: once through osmt_cascade_register, once through the
    mirror's arrays handed to the existing registrations; styled areas, display list, both label batches and the pixels agree"""
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
    sheet = [
        ([(WAY, [], None, None, "*")], [("linecap", ("id", "round")), ("text-color", ("color", (150, 20, 60)))]),
        ([(AREA, [(A.TEST_EQUAL, "building", "yes")], None, None, None)], [("fill-color", ("color", (170, 200, 150))), ("z-index", nums(2.0))]),
        ([(AREA, [(A.TEST_EQUAL, "building", "yes")], 17, None, None)], [("text", ("id", "name")), ("font-size", nums(9.0)), ("text-position", ("id", "center"))]),
        ([(WAY, [(E, "highway")], None, None, None)], [("color", ("id", "red")), ("width", nums(3.0)), ("casing-width", nums(1.0)), ("casing-color", ("id", "navy"))]),
        ([(WAY, [(E, "highway")], None, 17, "names")], [("text", ("id", "name")), ("font-size", nums(11.0))]),
        ([(WAY, [(E, "ref")], 18, None, "refs")], [("text", ("str", "ref")), ("font-size", nums(13.0)), ("dashes", nums(4, 2)), ("width", nums(1.0)), ("color", ("id", "white"))]),
        ([(NODE, [(E, "shop")], None, None, None)], [("icon-image", ("str", "shop.png")), ("text", ("id", "name")), ("font-size", nums(9.0))]),
        ([(NODE, [(E, "shop")], 17, 17, "dot")], [("icon-image", ("str", "dot.png"))]),
    ]
    icons = {"shop.png": icon_ids[0], "dot.png": icon_ids[1]}
    case = Case(gpu_ctx, tmp_path / "w.bin", w, sheet, icons, f, 2.0, None, index=True)
    gpu_ctx.register_tile_index(case.gid, tq.index_of(w.refs))
    gpu_ctx.register_node_mercator(case.gid, an.mercator_factors(case.r.node_table()))
    gpu_ctx.register_node_index(case.gid, tl.node_index_of(case.r, w.refs))
    zooms = (16, 17, 18)
    # 1. the device's way
    c = case.m.cascade(case.rid, False)
    got = c.read()
    cs.same_bytes(got, case.mirror(False))
    d_bind, d_node, d_area = c.register(A.CASCADE_AREA_STYLES | A.CASCADE_NODE_LABELS | A.CASCADE_AREA_LABELS)
    c.close()
    assert (d_bind != A.BINDINGS_NONE).all() and len(set(d_bind[list(zooms)].tolist())) == 3
    # 2. the mirror's arrays through the existing calls
    want = case.mirror(False)
    s0 = gpu_ctx.register_styles(want.styles, want.dashes)
    l0 = gpu_ctx.register_label_styles(want.label_styles)
    h_bind, h_node, h_area = {}, {}, {}
    for z in zooms:
        r = want.range_of(z)
        h_bind[z] = case.m.register_style_bindings(z, z, [[s0 + i for i in row] for row in want.class_styles_of(r)])
        rows = [[(l0 + i, k) for i, k in row] for row in want.class_bindings_of(r)]
        b = selmatch.ClassLabelBindings(z, z, rows, want.keys())
        h_node[z] = case.m.register_label_bindings(z, z, b)
        h_area[z] = case.m.register_area_label_bindings(z, z, b)
    tiles = []
    for zoom in zooms:
        sh = 18 - zoom
        tiles += [(zoom, CX >> sh, CY >> sh), (zoom, (CX >> sh) + 1, CY >> sh)]
    out = []
    for bind, node, area in (({z: int(d_bind[z]) for z in zooms}, {z: int(d_node[z]) for z in zooms}, {z: int(d_area[z]) for z in zooms}), (h_bind, h_node, h_area)):
        sc = gpu_ctx.build_tiles(styled.TileBatch(case.gid, tiles, bind))
        st_tiles, st_areas = sc.read_styled_areas()
        dl = sc.read_display_list()
        a, n = sc.build_tile_labels_all(area, node)
        out.append((st_tiles, st_areas, dl, n, a, gpu_ctx.render(sc).cpu().numpy()))
        sc.free()
    x, y = out
    assert x[0].tobytes() == y[0].tobytes() and len(x[1]) == len(y[1]) > 10
    # the two registrations gave the same styles different ids: the areas agree entity by entity, the lists in every byte
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


def test_cpp_program_over_the_c_abi(gpu_ctx, tmp_path):
    """tests/cascade_host_demo.cpp: register -> match -> cascade -> register -> build tiles in C++, in a process of its own"""
    w = sm.World()
    node_fn = lambda la, lo: w.node(None, la, lo)
    for k in range(12):
        ids = tq.square(node_fn, k)
        w.way(ids if k % 2 else ids[:3], {"highway": "yes"} if k % 3 == 0 else {"building": "yes"} if k % 3 == 1 else {"layer": str(k)})
    r = w.write(tmp_path / "w.bin", tq.max_zoom_tile)
    r.close()
    out = subprocess.run([cs.build_demo(), str(tmp_path / "w.bin"), "18", str(CX), str(CY)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    word, n_classes, n_styles, n_ranges, n_areas = out.stdout.split()
    assert word == "OK" and int(n_classes) >= 4 and int(n_styles) >= 3 and int(n_ranges) == 2 and int(n_areas) > 0
