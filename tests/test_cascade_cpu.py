"""The cascade on the host: osmt::cascade_host (osm_renderer_amd/host/osmt_cascade.hpp, through tests/cascade_shim.cpp) against a
Python restatement of Styler::style_area and property_map_to_style over real dicts (tests/_cascade.py), osmt_validate_rules
without a device, and builder + mirror in a program of their own under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch
from tests import _cascade as cs
from tests._cascade import CLASSES, ICONS, SHEET, fma_triple, nums, sel

A = abi
WAY, NODE, AREA = A.SEL_WAY, A.SEL_NODE, A.SEL_AREA
REFERENCE_SHEET = "/root/reference/tests/mapcss/mapnik.parsed.canonical"


def run(sheet, classes, labels_all=True, **kw):
    sels = cs.selector_set(sheet)
    rules = cs.rule_set(sheet, icons=ICONS, **kw)
    d = rules.as_desc()
    assert lib.load().osmt_validate_rules(C.byref(d), None) == A.OK, lib.load().osmt_last_error()
    cls, pooled = cs.classes_array(classes)
    res = cs.mirror(rules, sels, cls, pooled, labels_all)
    py = cs.py_cascade(sheet, classes, ICONS, kw.get("casing", 2.0), kw.get("font_mult"))
    cs.same_as_py(res, py, labels_all, kw.get("font_id", 0))
    return res, py


def test_struct_layouts_match_the_header():
    L = cs.shim()
    assert L.cs_sizeof(0) == C.sizeof(A.RuleProp) == selmatch.RULE_PROP_DTYPE.itemsize == 40
    assert L.cs_sizeof(1) == C.sizeof(A.RulesDesc)
    assert L.cs_sizeof(2) == 32
    assert L.cs_sizeof(10) == A.RuleProp.image.offset and L.cs_sizeof(11) == A.RuleProp.delta.offset
    assert L.cs_sizeof(12) == A.RulesDesc.layer_off.offset and L.cs_sizeof(13) == A.RulesDesc.numbers.offset
    assert L.cs_sizeof(14) == A.RulesDesc.casing_width_multiplier.offset and L.cs_sizeof(15) == A.RulesDesc.has_font_size_multiplier.offset
    assert selmatch.RULE_PROP_DTYPE.fields["image"][1] == A.RuleProp.image.offset and selmatch.RULE_PROP_DTYPE.fields["delta"][1] == A.RuleProp.delta.offset


@pytest.mark.parametrize("labels_all", [True, False])
@pytest.mark.parametrize("casing,font_mult", [(2.0, None), (1.0, 1.5)])
def test_mirror_equals_the_restatement_on_the_cases_of_the_rule(labels_all, casing, font_mult):
    res, py = run(SHEET, CLASSES, labels_all, casing=casing, font_mult=font_mult, font_id=2)
    assert py[0] == [[] for _ in range(cs.ZOOMS)]                       # "*" alone
    assert len(py[18][0]) == 7                                          # eight layers, seven styles
    assert py[3][0][0]["line_cap"] == "round" and py[3][0][-1]["text_style"]["text"] == "name"  # "*" reaches old layers, new ones copy it
    assert py[5][0][1]["casing_width"] == 3.0 + casing * 3.5 and py[6][0][0]["casing_width"] == casing * 0.5
    assert [s["z_index"] for c in (10, 11, 12, 13) for s in py[c][0]] == [4.0, 1.0, 3.0, 1.0]
    assert py[15][0][0]["icon_image"] is None and py[15][0][0]["fill_image"] is None
    assert [len(py[9][z]) for z in (0, 4, 5, 7, 8, 9, 10, 18)] == [1, 1, 2, 2, 1, 2, 1, 1]
    assert res.zoom_lo.tolist() == [0, 5, 8, 9, 10]                     # class 9's zoom bounds alone split the zooms
    cs.numeric_cases(py, casing, font_mult)                             # Numbers of length 0 / 1 / 2 for every numeric name


def test_casing_width_and_font_size_are_unfused():
    mult = 3.0  # 1.0 and 2.0, the reference's two multipliers, make the product exact: nothing to tell apart
    base, w = fma_triple(mult)
    unfused = base + mult * w
    assert cs.fma(mult, w, base) != unfused  # the operands tell a fused multiply-add apart
    fs, fm = 0.1, 1.1
    sheet = [([sel()], [("width", nums(base)), ("casing-width", nums(w)), ("text", ("id", "name")), ("font-size", nums(fs))])]
    res, _ = run(sheet, [(2, None, [0])], casing=mult, font_mult=fm)
    assert cs.bits(float(res.styles[0]["casing_width"])) == cs.bits(unfused)
    assert cs.bits(float(res.label_styles[0]["font_size"])) == cs.bits(fs * fm)
    # and through a delta: base + mult * (base + d)
    for skip in range(50):
        base, inner = fma_triple(mult, skip)
        d = inner - base
        if base + d == inner:
            break
    sheet = [([sel()], [("width", nums(base)), ("casing-width", ("delta", d))])]
    res, _ = run(sheet, [(2, None, [0])], casing=mult)
    assert cs.fma(mult, inner, base) != base + mult * inner
    assert cs.bits(float(res.styles[0]["casing_width"])) == cs.bits(base + mult * inner)


def seeded_sheet(rng, n_rules, layers):
    names = list(A.PROP_NAMES) + ["linejoin"]
    values = [("id", "red"), ("id", "none"), ("id", "round"), ("id", "line"), ("id", "center"), ("id", "background"), ("id", "name"), ("str", "pin.png"),
              ("str", "ref"), ("color", (10, 20, 30)), nums(), nums(1.0), nums(2.5), nums(1, 2), ("delta", 1.0), ("delta", -0.5), ("id", "grass")]
    sheet = []
    for _ in range(n_rules):
        sels = []
        for _ in range(rng.randint(1, 3)):
            lo = rng.choice([None, None, 0, 5, 12])
            hi = rng.choice([None, None, 4, 12, 18])
            sels.append(sel(rng.choice(layers), lo, hi, rng.choice([WAY, NODE])))
        sheet.append((sels, [(rng.choice(names), rng.choice(values)) for _ in range(rng.randint(0, 6))]))
    return sheet


@pytest.mark.parametrize("seed", range(6))
def test_mirror_equals_the_restatement_on_seeded_rules(seed):
    rng = random.Random(seed)
    layers = [None, None, "default", "*", "a", "b", "c", "d", "e"][: rng.randint(2, 9)]
    sheet = seeded_sheet(rng, 30, layers)
    n_sel = sum(len(s) for s, _ in sheet)
    classes = [(rng.randrange(4), rng.choice([None, 0, -3]), sorted(rng.sample(range(n_sel), rng.randint(0, min(12, n_sel))))) for _ in range(40)]
    run(sheet, classes, labels_all=bool(seed & 1), casing=rng.choice([1.0, 2.0]), font_mult=rng.choice([None, 1.25]))


def test_validate_rules_refusals():
    """osmt_validate_rules without a context: every refusal that needs no registry"""
    L = lib.load()
    good = cs.rule_set(SHEET, icons=ICONS)

    def rc_of(edit, rules=None):
        r = rules or cs.rule_set(SHEET, icons=ICONS)
        d = r.as_desc()
        edit(d, r)
        rc = L.osmt_validate_rules(C.byref(d), None)
        return rc, L.osmt_last_error().decode()

    d = good.as_desc()
    assert L.osmt_validate_rules(C.byref(d), None) == A.OK
    assert L.osmt_validate_rules(None, None) == A.INVALID_ARG
    u32 = C.POINTER(C.c_uint32)

    def null(field):
        def e(d, r):
            setattr(d, field, C.cast(None, type(getattr(d, field))))
        return e

    for field in ("selector_rule", "selector_layer", "layer_off", "layer_bytes", "rule_prop_off", "props", "numbers", "strings"):
        rc, msg = rc_of(null(field))
        assert rc == A.INVALID_ARG and "NULL" in msg, field

    def poke(arr, i, v):
        def e(d, r):
            getattr(r, arr)[i] = v
        return e

    cases = [
        (poke("layer_off", 0, 1), "layer_off"), (poke("rule_prop_off", 2, 0), "rule_prop_off"), (poke("rule_prop_off", -1, 1), "rule_prop_off"),
        (poke("selector_rule", 3, 99), "selector_rule[3]"), (poke("selector_rule", 5, 0), "decreases"), (poke("selector_layer", 0, 77), "selector_layer[0]"),
    ]
    for edit, word in cases:
        rc, msg = rc_of(edit)
        assert rc == A.INVALID_ARG and word in msg, (word, msg)

    def prop(i, field, v):
        def e(d, r):
            r.props[field][i] = v
        return e

    for edit, word in [(prop(0, "name", 22), "name 22"), (prop(0, "kind", 5), "kind 5"), (prop(0, "has_color", 2), "flag"), (prop(0, "has_image", 2), "flag"),
                       (prop(0, "str_off", 10 ** 6), "string"), (prop(1, "num_off", 10 ** 6), "numbers"), (prop(1, "n_nums", 10 ** 6), "numbers")]:
        rc, msg = rc_of(edit)
        assert rc == A.INVALID_ARG and word in msg, (word, msg)

    def color_without_flag(d, r):
        i = int(np.nonzero(r.props["kind"] == A.PV_COLOR)[0][0])
        r.props["has_color"][i] = 0

    def flag_on(kind, name):
        def e(d, r):
            i = int(np.nonzero(r.props["kind"] == kind)[0][0])
            r.props[name][i] = 1
        return e

    def image_on_text(d, r):
        i = int(np.nonzero((r.props["kind"] == A.PV_IDENTIFIER) & (r.props["name"] == A.PROP_NAMES.index("text")))[0][0])
        r.props["has_image"][i] = 1

    for edit, word in [(color_without_flag, "a COLOR value has has_color = 1"), (flag_on(A.PV_NUMBERS, "has_color"), "neither COLOR nor IDENTIFIER"),
                       (flag_on(A.PV_WIDTH_DELTA, "has_color"), "neither COLOR nor IDENTIFIER"), (flag_on(A.PV_NUMBERS, "has_image"), "has_image on a property"),
                       (image_on_text, "has_image on a property")]:
        rc, msg = rc_of(edit)
        assert rc == A.INVALID_ARG and word in msg, (word, msg)

    def field(name, v):
        def e(d, r):
            setattr(d, name, v)
        return e

    for edit, word in [(field("casing_width_multiplier", float("nan")), "casing_width_multiplier is NaN"), (field("has_font_size_multiplier", 2), "0 or 1")]:
        rc, msg = rc_of(edit)
        assert rc == A.INVALID_ARG and word in msg, (word, msg)
    rc, msg = rc_of(field("font_size_multiplier", float("nan")), cs.rule_set(SHEET, icons=ICONS, font_mult=1.0))
    assert rc == A.INVALID_ARG and "font_size_multiplier is NaN" in msg
    # nine layer names; the ninth need not be used by a selector
    nine = SHEET + [([sel("l9")], [])]
    rc, msg = rc_of(lambda d, r: None, cs.rule_set(nine))
    assert rc == A.UNSUPPORTED and "9 distinct layer names" in msg
    # 256 text strings pass, 257 do not; identifier and string of the same bytes are one key
    many = lambda n: [([sel()], [("text", ("id" if i & 1 else "str", f"k{i}")) for i in range(n)] + [("text", ("str", "k1"))])]
    assert rc_of(lambda d, r: None, cs.rule_set(many(256)))[0] == A.OK
    rc, msg = rc_of(lambda d, r: None, cs.rule_set(many(257)))
    assert rc == A.UNSUPPORTED and "257 distinct text strings" in msg
    # an empty rule set is fine
    assert rc_of(lambda d, r: None, cs.rule_set([]))[0] == A.OK


def test_host_program_under_sanitizers():
    out = subprocess.run([cs.build_host_main()], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out == ["labels_all 0: 3 styles 2 dashes 2 label styles 1 keys 6 class styles 6 bindings, ranges 0-9 10-13 14-18",
                   "labels_all 1: 3 styles 2 dashes 2 label styles 1 keys 6 class styles 6 bindings, ranges 0-9 10-13 14-18"]


@pytest.mark.skipif(not os.path.exists(REFERENCE_SHEET), reason="the reference's stylesheet dump is not on this machine")
def test_reference_stylesheet_at_its_real_size():
    sheet = cs.read_canonical(REFERENCE_SHEET)
    flat = [s for sels, _ in sheet for s in sels]
    assert len(sheet) > 300 and len(flat) > 600
    rng = random.Random(7)
    # classes: random ascending subsets of the selectors of one object type (what one entity can match), all four slots
    by_type = {t: [i for i, s in enumerate(flat) if s[0] == t] for t in (NODE, WAY, AREA)}
    classes = []
    for i in range(64):
        slot = i % 4
        cand = by_type[NODE] if slot == 0 else by_type[WAY] + (by_type[AREA] if slot != 2 else [])
        classes.append((slot, rng.choice([None, 1, -1]), sorted(rng.sample(cand, rng.randint(0, min(10, len(cand)))))))
    icons = {v: i for i, v in enumerate(sorted({v for _, ps in sheet for n, (k, v) in ps if n in ("icon-image", "fill-image") and k in ("id", "str")})) if i % 5}
    sels, rules = cs.selector_set(sheet), cs.rule_set(sheet, icons=icons)
    d = rules.as_desc()
    # The stylesheet names 26 layers ("default" included), so the library refuses it with the figure: OSMT_CASCADE_MAX_LAYERS
    # bounds the names of a rule set, not the layers of one entity.  The mirror has no such bound and is held at full size.
    n_names = len({s[4] or "default" for s in flat})
    assert n_names == 26
    assert lib.load().osmt_validate_rules(C.byref(d), None) == A.UNSUPPORTED
    assert b"26 distinct layer names" in lib.load().osmt_last_error()
    cls, pooled = cs.classes_array(classes)
    for labels_all in (True, False):
        res = cs.mirror(rules, sels, cls, pooled, labels_all)
        cs.same_as_py(res, cs.py_cascade(sheet, classes, icons), labels_all)
