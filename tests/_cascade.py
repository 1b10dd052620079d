"""Shared helpers of the cascade tests (tests/test_cascade_cpu.py, tests/test_gpu_cascade.py): the shim over
osm_renderer_amd/host/osmt_cascade.hpp (the host mirror osmt::cascade_host), a Python restatement of the rule written from
mapcss/styler.rs:128-160,205-242,277-429 over real dicts keyed by strings, rule sets as plain Python data that feed both, and a
reader of the reference's canonical stylesheet dumps.

A stylesheet here is a list of rules; a rule is (selectors, properties); a selector is (object type, tests, min zoom or None,
max zoom or None, layer name or None); a property is (name, value) with value one of ("id", str), ("str", str), ("color", (r,
g, b)), ("nums", [floats]), ("delta", float).  COLORS plays from_color_name, `icons` the icon cache."""
import ctypes as C
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np

from osm_renderer_amd import abi, selmatch
from osm_renderer_amd.styled import LABEL_STYLE_REC_DTYPE, STYLE_REC_DTYPE
from tests._geodata import ROOT
from tests._selmatch import _stale

SHIM = os.path.join(ROOT, "tests", "_build", "libcascade_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "cascade_host_main")
DEMO = os.path.join(ROOT, "tests", "_build", "cascade_host_demo")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_cascade.hpp", "osmt_selmatch.hpp", "osmt_geodata.hpp")]
_HDRS += [os.path.join(ROOT, "osm_renderer_amd", "csrc", h) for h in ("osmt_cascade_rule.h", "osmt_cascade_tables.h", "osmt_numparse.h", "osmt_utf8.h")]
_HDRS += [os.path.join(ROOT, "include", "osmtile.h")]
_lib = None
NONE = abi.TEXT_NONE
ZOOMS = abi.MAX_ZOOM + 1
COLORS = {"red": (255, 0, 0), "white": (255, 255, 255), "navy": (0, 0, 128)}  # the caller's from_color_name
KIND_OF = {"id": abi.PV_IDENTIFIER, "str": abi.PV_STRING, "color": abi.PV_COLOR, "nums": abi.PV_NUMBERS, "delta": abi.PV_WIDTH_DELTA}


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "cascade_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz = C.c_void_p, C.c_size_t
        L.cs_host_new.restype = vp
        L.cs_host_new.argtypes = [C.POINTER(abi.RulesDesc), C.POINTER(abi.SelectorsDesc), vp, sz, vp, C.c_int]
        L.cs_host_free.argtypes = [vp]
        L.cs_host_counts.argtypes = [vp, C.POINTER(sz)]
        L.cs_host_copy.argtypes = [vp, C.POINTER(vp)]
        L.cs_sizeof.restype = sz
        L.cs_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def build_host_main():
    """tests/cascade_host_main.cpp: builder + mirror in a program of its own, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "cascade_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def build_demo():
    """tests/cascade_host_demo.cpp against the built library: register -> match -> cascade -> register -> build tiles in C++"""
    src = os.path.join(ROOT, "tests", "cascade_host_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    if _stale(DEMO, [src, os.path.join(libdir, "libosmtile.so")] + _HDRS):
        os.makedirs(os.path.dirname(DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", DEMO, src, "-L" + libdir, "-losmtile", "-Wl,-rpath," + libdir])
    return DEMO


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- a stylesheet as Python data -> the library's descriptors -------------------------------------------------------
def selector_set(sheet):
    return selmatch.SelectorSet([(s[0], s[1], s[2], s[3]) for sels, _ in sheet for s in sels])


def rule_set(sheet, selectors_id=0, icons=None, casing=2.0, font_mult=None, font_id=0):
    icons = icons or {}
    rules = []
    for sels, props in sheet:
        ps = []
        for name, (kind, value) in props:
            extra = {}
            if kind in ("id", "str"):
                extra["image"] = icons.get(value)
            if kind == "id":
                extra["color"] = COLORS.get(value)
            ps.append((name, KIND_OF[kind], value, extra))
        rules.append(([s[4] for s in sels], ps))
    return selmatch.RuleSet(selectors_id, rules, casing, font_mult, font_id)


def classes_array(classes):
    """[(slot, layer or None, [selector ids])] -> (MATCH_CLASS_DTYPE, pooled ids)"""
    cls, pooled = np.zeros(len(classes), selmatch.MATCH_CLASS_DTYPE), []
    for c, (slot, layer, sels) in zip(cls, classes):
        c["slot"], c["has_layer"], c["layer"] = slot, layer is not None, layer or 0
        c["sel_off"], c["n_sels"] = len(pooled), len(sels)
        pooled += list(sels)
    return cls, np.array(pooled, dtype=np.uint32)


def mirror(rules, selectors, cls, pooled, labels_all=True):
    """osmt::cascade_host: a selmatch.CascadeResult"""
    L = shim()
    rd, sd = rules.as_desc(), selectors.as_desc()
    cls = np.ascontiguousarray(cls, dtype=selmatch.MATCH_CLASS_DTYPE)
    pooled = np.ascontiguousarray(pooled, dtype=np.uint32)
    h = L.cs_host_new(C.byref(rd), C.byref(sd), C.c_void_p(cls.ctypes.data), len(cls), C.c_void_p(pooled.ctypes.data), int(labels_all))
    try:
        n = (C.c_size_t * 8)()
        L.cs_host_counts(h, n)
        out = selmatch.CascadeResult(list(n) + [len(cls)])
        L.cs_host_copy(h, (C.c_void_p * 13)(*out.pointers()))
        return out
    finally:
        L.cs_host_free(h)


def same_bytes(got, want):
    """two CascadeResults, array by array, byte for byte"""
    for name, a, b in zip(got.FIELDS, got.arrays(), want.arrays()):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


# ---- the restatement ---------------------------------------------------------------------------------------------
def py_style_area(sheet_selectors, class_sels, zoom):
    """Styler::style_area (styler.rs:205-242) for an entity that matches the selectors `class_sels` up to zoom.
    sheet_selectors: per selector (rule properties, min zoom, max zoom, layer)."""
    result = {}  # IndexMap<&str, PropertyMap>
    for s in class_sels:  # ascending = rule by rule, selector by selector
        props, lo, hi, layer = sheet_selectors[s]
        if lo is not None and zoom < lo:
            continue
        if hi is not None and zoom > hi:
            continue
        layer_id = layer if layer is not None else "default"

        def update_layer(m):
            for name, value in props:
                m[name] = value

        if layer_id not in result:
            result[layer_id] = dict(result["*"]) if "*" in result else {}
        update_layer(result[layer_id])
        if layer_id == "*":
            for k, v in result.items():
                if k != "*":
                    update_layer(v)
    return result


def py_property_map_to_style(cur, base, default_z, casing_mult, font_mult, layer, icons):
    """property_map_to_style (styler.rs:277-429): a dict of the Style's fields, Options as None"""
    def get_color(name):
        v = cur.get(name)
        if v is None:
            return None
        if v[0] == "color":
            return tuple(v[1])
        if v[0] == "id":
            return COLORS.get(v[1])
        return None

    def get_num(m, name):
        v = m.get(name)
        return v[1][0] if v is not None and v[0] == "nums" and len(v[1]) == 1 else None

    def get_id(name):
        v = cur.get(name)
        return v[1] if v is not None and v[0] == "id" else None

    def get_string(name):
        v = cur.get(name)
        return v[1] if v is not None and v[0] in ("id", "str") else None

    def get_line_cap(name):
        return {"none": "butt", "butt": "butt", "round": "round", "square": "square"}.get(get_id(name))

    def get_dashes(name):
        v = cur.get(name)
        return tuple(v[1]) if v is not None and v[0] == "nums" else None

    z = get_num(cur, "z-index")
    z_index = z if z is not None else default_z
    fp = cur.get("fill-position")
    is_foreground_fill = not (fp is not None and fp[0] == "id" and fp[1] == "background")
    width = get_num(cur, "width")
    base_width = width
    if base_width is None and base is not None:
        base_width = get_num(base, "width")
    if base_width is None:
        base_width = 0.0
    cw = cur.get("casing-width")
    if cw is not None and cw[0] == "nums" and len(cw[1]) == 1:
        casing_only = cw[1][0]
    elif cw is not None and cw[0] == "delta":
        casing_only = base_width + cw[1]
    else:
        casing_only = None
    full_casing = None if casing_only is None else base_width + casing_mult * casing_only  # Python floats: a product, then a sum
    text = get_string("text")
    fs = get_num(cur, "font-size")
    font_size = None if fs is None else fs * (font_mult if font_mult is not None else 1.0)
    text_style = None
    if text is not None:
        text_style = {"text": text, "text_color": get_color("text-color"), "text_position": {"center": "center", "line": "line"}.get(get_id("text-position")),
                      "font_size": font_size}
    return {"layer": layer, "z_index": z_index, "color": get_color("color"), "fill_color": get_color("fill-color"),
            "is_foreground_fill": is_foreground_fill, "background_color": get_color("background-color"), "opacity": get_num(cur, "opacity"),
            "fill_opacity": get_num(cur, "fill-opacity"), "width": width, "dashes": get_dashes("dashes"), "line_cap": get_line_cap("linecap"),
            "casing_color": get_color("casing-color"), "casing_width": full_casing, "casing_dashes": get_dashes("casing-dashes"),
            "casing_line_cap": get_line_cap("casing-linecap"), "icon_image": icons.get(get_string("icon-image")),
            "fill_image": icons.get(get_string("fill-image")), "text_style": text_style}


DEFAULT_Z = {0: 4.0, 1: 1.0, 2: 3.0, 3: 1.0}


def py_cascade(sheet, classes, icons=None, casing=2.0, font_mult=None):
    """per class, per zoom the list of Styles (dicts), as Styler::style_entities makes them for a cache miss (128-160)"""
    icons = icons or {}
    flat = [(props, s[2], s[3], s[4]) for sels, props in sheet for s in sels]
    out = []
    for slot, layer, sels in classes:
        per_zoom = []
        for zoom in range(ZOOMS):
            maps = py_style_area(flat, sels, zoom)
            base = maps.get("default")
            per_zoom.append([py_property_map_to_style(m, base, DEFAULT_Z[slot], casing, font_mult, layer, icons) for k, m in maps.items() if k != "*"])
        out.append(per_zoom)
    return out


# ---- records back into the restatement's terms -------------------------------------------------------------------------
_CAP = {0: None, 1: "butt", 2: "round", 3: "square"}
_POS = {0: None, 1: "center", 2: "line"}


def _f(x):
    return None if x is None else bits(float(x))


def area_key_of_style(s):
    d = lambda v: None if v is None else tuple(bits(x) for x in v)
    return (s["layer"], bits(s["z_index"]), s["color"], s["fill_color"], s["is_foreground_fill"], s["background_color"], _f(s["opacity"]),
            _f(s["fill_opacity"]), _f(s["width"]), d(s["dashes"]), s["line_cap"], s["casing_color"], _f(s["casing_width"]), d(s["casing_dashes"]),
            s["casing_line_cap"], s["fill_image"])


def label_key_of_style(s, font_id):
    t = s["text_style"]
    ts = None if t is None else (t["text_color"], t["text_position"], _f(t["font_size"]), font_id if t["font_size"] is not None else None)
    return (s["layer"], bits(s["z_index"]), s["icon_image"], ts)


def area_key_of_rec(r, dashes):
    opt = lambda has, v: v if has else None
    col = lambda has, v: tuple(int(x) for x in v) if has else None
    dl = lambda has, off, n: tuple(bits(x) for x in dashes[off:off + n]) if has else None
    return (opt(r["has_layer"], int(r["layer"])), bits(float(r["z_index"])), col(r["has_color"], r["color"]), col(r["has_fill_color"], r["fill_color"]),
            bool(r["is_foreground_fill"]), col(r["has_background_color"], r["background_color"]), opt(r["has_opacity"], bits(float(r["opacity"]))),
            opt(r["has_fill_opacity"], bits(float(r["fill_opacity"]))), opt(r["has_width"], bits(float(r["width"]))),
            dl(r["has_dashes"], int(r["dashes_off"]), int(r["n_dashes"])), _CAP[int(r["line_cap"])], col(r["has_casing_color"], r["casing_color"]),
            opt(r["has_casing_width"], bits(float(r["casing_width"]))), dl(r["has_casing_dashes"], int(r["casing_dashes_off"]), int(r["n_casing_dashes"])),
            _CAP[int(r["casing_line_cap"])], opt(r["has_fill_image"], int(r["fill_image"])))


def label_key_of_rec(r):
    ts = None
    if r["has_text_style"]:
        ts = (tuple(int(x) for x in r["text_color"]) if r["has_text_color"] else None, _POS[int(r["text_position"])],
              bits(float(r["font_size"])) if r["has_font_size"] else None, int(r["font_id"]) if r["has_font_size"] else None)
    return (int(r["layer"]) if r["has_layer"] else None, bits(float(r["z_index"])), int(r["icon_image"]) if r["has_icon"] else None, ts)


def canonical(res):
    """every byte a has_* flag does not vouch for is zero"""
    for r in res.styles:
        z = np.zeros((), STYLE_REC_DTYPE)
        for has, fields in (("has_layer", ["layer"]), ("has_color", ["color"]), ("has_fill_color", ["fill_color"]), ("has_opacity", ["opacity"]),
                            ("has_fill_opacity", ["fill_opacity"]), ("has_width", ["width"]), ("has_dashes", ["dashes_off", "n_dashes"]),
                            ("has_casing_color", ["casing_color"]), ("has_casing_width", ["casing_width"]),
                            ("has_casing_dashes", ["casing_dashes_off", "n_casing_dashes"]), ("has_fill_image", ["fill_image"]),
                            ("has_background_color", ["background_color"])):
            assert r[has] in (0, 1)
            if not r[has]:
                for f in fields:
                    assert r[f].tobytes() == z[f].tobytes(), (has, f)
        assert r["_pad"] == 0
    for r in res.label_styles:
        assert bytes(r["_pad"]) == bytes(7)
        if not r["has_text_style"]:
            assert not r["has_font_size"] and not r["has_text_color"] and r["text_position"] == 0 and r["font_size"] == 0
        if not r["has_font_size"]:
            assert r["font_id"] == 0 and bits(float(r["font_size"])) == 0
        if not r["has_icon"]:
            assert r["icon_image"] == 0


def same_as_py(res, py, labels_all=True, font_id=0):
    """a CascadeResult against py_cascade's lists: the expanded styles per (class, zoom), ids in order of first use, no two
    distinct records equal, ranges the maximal runs"""
    canonical(res)
    keys = res.keys()
    akeys = [area_key_of_rec(r, res.dashes) for r in res.styles]
    lkeys = [label_key_of_rec(r) for r in res.label_styles]
    assert len(set(akeys)) == len(akeys) and len(set(lkeys)) == len(lkeys)
    assert np.array_equal(res.key_off, np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32))
    n_classes = len(py)
    assert res.n_classes == n_classes
    assert res.zoom_lo[0] == 0 and res.zoom_hi[-1] == ZOOMS - 1 and np.array_equal(res.zoom_lo[1:], res.zoom_hi[:-1] + 1)
    lists = {}
    for r in range(len(res.zoom_lo)):
        st, bd = res.class_styles_of(r), res.class_bindings_of(r)
        lists[r] = (st, bd)
        for zoom in range(int(res.zoom_lo[r]), int(res.zoom_hi[r]) + 1):
            for c in range(n_classes):
                want = py[c][zoom]
                assert [akeys[i] for i in st[c]] == [area_key_of_style(s) for s in want], (c, zoom)
                binds = [s for s in want if labels_all or s["icon_image"] is not None or s["text_style"] is not None]
                got = [(lkeys[i], None if k is None else keys[k]) for i, k in bd[c]]
                assert got == [(label_key_of_style(s, font_id), None if s["text_style"] is None else s["text_style"]["text"].encode()) for s in binds], (c, zoom)
        if r:
            assert lists[r] != lists[r - 1]  # maximal runs
    # ids in order of first use over (class, zoom, position)
    for which in (0, 1):
        seen = []
        for c in range(n_classes):
            for zoom in range(ZOOMS):
                row = lists[res.range_of(zoom)][which][c]
                for i in row:
                    i = i if which == 0 else i[0]
                    if i not in seen:
                        seen.append(i)
        assert seen == list(range(len(seen))), which
        assert len(seen) == (len(akeys) if which == 0 else len(lkeys))


def fma(a, b, c):
    """a * b + c rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---- the sheet of the cases of the rule, shared by the CPU and the GPU tests ----------------------------------------------
def sel(layer=None, lo=None, hi=None, typ=abi.SEL_WAY):
    return (typ, [], lo, hi, layer)


def nums(*v):
    return ("nums", list(v))


NUMERIC = ("z-index", "width", "casing-width", "font-size", "opacity", "fill-opacity")  # every name get_num (or its twin in casing-width) reads
NUMERIC_VALUES = (5.0, 2.5, 0.5, 12.0, 0.75, 0.5)
# One sheet for the cases of the rule.  A class lists its selectors ascending, as a match does: the order of the rules is the
# order of the writers.  Selector ids are in the comments.
SHEET = [
    ([sel("*")], [("linecap", ("id", "none")), ("width", nums(1.5)), ("opacity", nums(0.5))]),                         # 0: "*" first
    ([sel()], [("color", ("id", "red")), ("width", nums(3.0)), ("casing-width", ("delta", 1.0))]),                     # 1: default, implicit
    ([sel("default")], [("fill-color", ("color", (1, 2, 3))), ("z-index", nums(7.0))]),                                # 2: ::default spelled out
    ([sel("over"), sel("under")], [("casing-width", nums(0.75)), ("dashes", nums(4, 2)), ("casing-dashes", nums())]),  # 3, 4: one rule, two layers
    ([sel("*")], [("linecap", ("id", "round")), ("casing-linecap", ("id", "square")), ("text", ("id", "name"))]),      # 5: "*" after other layers
    ([sel("late")], [("font-size", nums(11.0)), ("text-color", ("id", "navy")), ("text-position", ("id", "line"))]),   # 6: created after "*" has content
    ([sel()], [("width", nums(2.0)), ("width", ("id", "thin"))]),                                                      # 7: a name twice; good shadowed by wrong type
    ([sel("w")], [("casing-width", ("delta", 0.5))]),                                                                  # 8: delta, width only in default
    ([sel("n")], [("casing-width", ("delta", 0.25)), ("width", nums(1, 2))]),                                          # 9: Numbers of length 2 is no width
    ([sel(lo=5), sel("over", hi=7), sel("under", 9, 9), sel("w", 12, 3)], [("fill-opacity", nums(0.25))]),             # 10-13: zoom bounds
    ([sel()], [("color", ("color", (9, 8, 7))), ("fill-color", ("id", "white")), ("background-color", ("id", "navy")), ("casing-color", ("id", "red")),   # 14: good values
               ("opacity", nums(1.0)), ("fill-opacity", nums(0.5)), ("z-index", nums(-1.0)), ("font-size", nums(10.0)), ("dashes", nums(1, 2, 3)),
               ("casing-dashes", nums(5.0)), ("linecap", ("id", "butt")), ("casing-linecap", ("id", "round")), ("text-position", ("id", "center")),
               ("text", ("str", "ref")), ("icon-image", ("str", "pin.png")), ("fill-image", ("id", "grass")), ("fill-position", ("id", "background")),
               ("casing-width", nums(1.0)), ("text-color", ("color", (4, 5, 6))), ("unknown-name", ("id", "x"))]),
    ([sel()], [("color", ("id", "nocolour")), ("fill-color", nums(1.0)), ("background-color", ("str", "red")),          # 15: every getter shadowed
               ("casing-color", ("delta", 1.0)), ("text-color", nums(1.0)), ("opacity", nums()), ("fill-opacity", nums(1, 2)),
               ("z-index", ("id", "top")), ("font-size", ("color", (0, 0, 0))), ("dashes", ("id", "none")), ("casing-dashes", ("str", "1,2")),
               ("linecap", ("str", "round")), ("casing-linecap", ("id", "bevel")), ("text-position", ("str", "center")), ("text", nums(1.0)),
               ("icon-image", nums(1.0)), ("fill-image", ("color", (9, 9, 9))), ("fill-position", ("str", "background")),
               ("casing-width", ("id", "wide"))]),
    ([sel()], [("icon-image", ("str", "missing.png")), ("fill-image", ("str", "missing.png"))]),                        # 16: not in the icon cache
    ([sel(typ=abi.SEL_NODE)], [("icon-image", ("str", "pin.png"))]),                                                           # 17
    ([sel("l3")], [("width", nums(1.0))]),                                                                             # 18: eight names in all
    ([sel()], [(n, nums(v)) for n, v in zip(NUMERIC, NUMERIC_VALUES)] + [("text", ("id", "name"))]),                   # 19: Numbers of length 1
    ([sel()], [(n, nums()) for n in NUMERIC]),                                                                         # 20: of length 0
    ([sel()], [(n, nums(v)) for n, v in zip(NUMERIC, NUMERIC_VALUES)]),                                                # 21: of length 1 again
    ([sel()], [(n, nums(v, 1.0)) for n, v in zip(NUMERIC, NUMERIC_VALUES)]),                                           # 22: of length 2
    ([sel("w")], [("casing-width", nums(0.5))]),                                                                       # 23: casing as a number
]
ICONS = {"pin.png": 3, "grass": 5}
CLASSES = [
    (2, None, [0]),                      # "*" as the only layer: no style
    (2, None, [0, 1]),
    (1, 3, [1, 2]),
    (3, -1, [0, 1, 3, 4, 5, 6]),
    (2, None, [1, 7]),
    (2, None, [1, 8]),                   # width only in default
    (2, None, [8]),                      # width in neither
    (2, None, [0, 9]),                   # "*" gives the width of the current layer
    (2, None, [1, 9]),
    (1, None, [10, 11, 12, 13]),
    (0, None, [14, 15]), (1, None, [14, 15]), (2, None, [14, 15]), (3, None, [14, 15]),  # shadowed: z-index absent for the four slots
    (2, 0, [14]),                        # the good values alone
    (2, None, [14, 16]),
    (0, None, [17]),
    (0, None, []),
    (2, None, [0, 1, 3, 4, 6, 8, 9, 18]),  # eight layers
    (2, None, [5, 6]),
    (2, None, [19, 20]),                 # 20: every numeric name, length 0 last, over a good value
    (2, None, [19, 20, 21]),             # 21: length 1 last, over length 0
    (2, None, [19, 21, 22]),             # 22: length 2 last, over a good value
    (1, None, [1, 23]),                  # 23: casing-width as a number, width only in default
]


def numeric_cases(py, casing, font_mult):
    """what classes 12, 14 and 20 .. 23 of CLASSES must come to, at any zoom"""
    (good,), (shadowed,) = py[14][0], py[12][0]
    for f in ("color", "fill_color", "background_color", "casing_color", "opacity", "fill_opacity", "dashes", "casing_dashes", "line_cap", "casing_line_cap",
              "text_style", "icon_image", "fill_image", "casing_width"):
        assert good[f] is not None and shadowed[f] is None, f  # a last writer of the wrong type shadows the good value, for every getter
    assert (good["z_index"], shadowed["z_index"]) == (-1.0, 3.0) and (good["is_foreground_fill"], shadowed["is_foreground_fill"]) == (False, True)
    for c, default_z in ((20, 3.0), (22, 3.0)):
        (s,) = py[c][0]
        assert s["z_index"] == default_z and s["width"] is None and s["casing_width"] is None and s["opacity"] is None and s["fill_opacity"] is None
        assert s["text_style"] is not None and s["text_style"]["font_size"] is None
    (s,) = py[21][0]
    assert (s["z_index"], s["width"], s["opacity"], s["fill_opacity"]) == (5.0, 2.5, 0.75, 0.5) and s["casing_width"] == 2.5 + casing * 0.5
    assert s["text_style"]["font_size"] == 12.0 * (font_mult if font_mult is not None else 1.0)
    base, w = py[23][0]
    assert base["width"] == 3.0 and w["width"] is None and w["casing_width"] == 3.0 + casing * 0.5



def fma_triple(mult, skip=0):
    """(base, w) with base + mult * w different when fused, found by a seeded search"""
    rng = random.Random(11)
    while True:
        base, w = rng.uniform(0.1, 9.0), rng.uniform(0.1, 9.0)
        if fma(mult, w, base) != base + mult * w:
            if not skip:
                return base, w
            skip -= 1



# ---- the reference's canonical stylesheet dump -----------------------------------------------------------------------
def read_canonical(path):
    """A `*.parsed.canonical` file of the reference's parser tests: the stylesheet printed back in canonical MapCSS, one
    rule per block.  Returns a stylesheet (see the module docstring) with object types as abi.SEL_* and tests as SelectorSet
    takes them; a value is classified as the parser classifies it (parser.rs: colour, numbers, eval, string, identifier)."""
    import re

    text = open(path, encoding="utf-8").read()
    sheet = []
    types = {"node": abi.SEL_NODE, "way": abi.SEL_WAY, "area": abi.SEL_AREA}
    for head, body in re.findall(r"([^{}]+)\{([^{}]*)\}", text):
        sels = []
        for one in [x.strip() for x in head.strip().split(",\n")] if ",\n" in head else [x.strip() for x in head.strip().split(",")]:
            if not one:
                continue
            m = re.match(r"^([a-z*]+)(\|z(\d*)(-?)(\d*))?((?:\[[^\]]*\])*)(::([\w*-]+))?$", one)
            if not m:
                raise ValueError(f"selector {one!r}")
            lo = hi = None
            if m.group(2):
                lo = int(m.group(3)) if m.group(3) else None
                hi = int(m.group(5)) if m.group(5) else (lo if not m.group(4) else None)
            tests = []
            for t in re.findall(r"\[([^\]]*)\]", m.group(6)):
                mm = re.match(r'^(!?)([\w:.-]+|"[^"]*")(\?)?(?:(=|!=|<=|>=|<|>)(.*))?$', t)
                if not mm:
                    raise ValueError(f"test {t!r}")
                neg, key, truth, op, val = mm.groups()
                key = key.strip('"')
                if op is None:
                    kind = (abi.TEST_FALSE if neg else abi.TEST_TRUE) if truth else (abi.TEST_NOT_EXISTS if neg else abi.TEST_EXISTS)
                    tests.append((kind, key))
                elif op in ("=", "!="):
                    tests.append((abi.TEST_EQUAL if op == "=" else abi.TEST_NOT_EQUAL, key, val.strip('"')))
                else:
                    kind = {"<": abi.TEST_LESS, "<=": abi.TEST_LESS_OR_EQUAL, ">": abi.TEST_GREATER, ">=": abi.TEST_GREATER_OR_EQUAL}[op]
                    tests.append((kind, key, float(val)))
            sels.append((types.get(m.group(1), abi.SEL_OTHER), tests, lo, hi, m.group(8)))
        props = []
        for line in body.split(";"):
            if ":" not in line:
                continue
            name, value = [x.strip() for x in line.split(":", 1)]
            if re.match(r"^#[0-9a-fA-F]{6}$", value):
                v = ("color", tuple(int(value[i:i + 2], 16) for i in (1, 3, 5)))
            elif re.match(r"^#[0-9a-fA-F]{3}$", value):
                v = ("color", tuple(int(value[i] * 2, 16) for i in (1, 2, 3)))
            elif value.startswith("eval("):
                mm = re.search(r"[+-]?\d+(\.\d+)?", value[5:])
                v = ("delta", float(mm.group(0)))
            elif value.startswith('"'):
                v = ("str", value.strip('"'))
            else:
                try:
                    v = ("nums", [float(x) for x in value.split(",")])
                except ValueError:
                    v = ("id", value)
            props.append((name, v))
        if sels:
            sheet.append((sels, props))
    return sheet
