"""Selector matching: the inputs and the result of osmt_match_selectors, backed by numpy arrays.

Rule matching (Styler::style_area -> area_matches -> matches_by_tags, reference: src/mapcss/styler.rs:205-242,450-520) for
every entity of a registered geodata file, and the entities' classes (cache slot, layer, matched selectors).  The dtypes
mirror include/osmtile.h.
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import OsmtError, check, load

SELECTOR_REC_DTYPE = np.dtype([("object_type", "u1"), ("has_min_zoom", "u1"), ("min_zoom", "u1"), ("has_max_zoom", "u1"), ("max_zoom", "u1"),
                               ("_pad", "u1", (3,)), ("test_off", "<u4"), ("n_tests", "<u4")])
SELECTOR_TEST_DTYPE = np.dtype([("kind", "<u4"), ("key_off", "<u4"), ("key_len", "<u4"), ("value_off", "<u4"), ("value_len", "<u4"), ("_pad", "<u4"),
                                ("value", "<f8")])
NUMBER_OVERRIDE_DTYPE = np.dtype([("v_off", "<u4"), ("v_len", "<u4"), ("has_value", "<u4"), ("_pad", "<u4"), ("value", "<f8")])
DECLINED_NUMBER_DTYPE = np.dtype([("v_off", "<u4"), ("v_len", "<u4")])
MATCH_CLASS_DTYPE = np.dtype([("layer", "<i8"), ("sel_off", "<u4"), ("n_sels", "<u4"), ("first_entity", "<u4"), ("slot", "u1"), ("has_layer", "u1"),
                              ("_pad", "u1", (2,))])
assert SELECTOR_REC_DTYPE.itemsize == 16 and SELECTOR_TEST_DTYPE.itemsize == 32 and NUMBER_OVERRIDE_DTYPE.itemsize == 24
CLASS_LABEL_BINDING_DTYPE = np.dtype([("style", "<u4"), ("text_key", "<u4")])
assert DECLINED_NUMBER_DTYPE.itemsize == 8 and MATCH_CLASS_DTYPE.itemsize == 24 and CLASS_LABEL_BINDING_DTYPE.itemsize == 8

_STRING_KINDS = (abi.TEST_EQUAL, abi.TEST_NOT_EQUAL)


def _bytes(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


class SelectorSet:
    """osmt_selectors_desc.  selectors: [(object type, [test, ...])] or [(object type, [test, ...], min zoom or None, max zoom
    or None)] in stylesheet order; a test is (kind, key), (kind, key, value str / bytes) for EQUAL / NOT_EQUAL, or (kind, key,
    float) for the numeric kinds."""

    def __init__(self, selectors):
        recs, tests, pool = [], [], bytearray()

        def put(b):
            off = len(pool)
            pool.extend(b)
            return off, len(b)

        for sel in selectors:
            typ, ts = sel[0], sel[1]
            lo = sel[2] if len(sel) > 2 else None
            hi = sel[3] if len(sel) > 3 else None
            recs.append((typ, lo is not None, lo or 0, hi is not None, hi or 0, (0, 0, 0), len(tests), len(ts)))
            for t in ts:
                kind, (koff, klen) = t[0], put(_bytes(t[1]))
                voff = vlen = 0
                num = 0.0
                if kind in _STRING_KINDS:
                    voff, vlen = put(_bytes(t[2]))
                elif len(t) > 2:
                    num = float(t[2])
                tests.append((kind, koff, klen, voff, vlen, 0, num))
        self.selectors = np.array(recs, dtype=SELECTOR_REC_DTYPE).reshape(-1)
        self.tests = np.array(tests, dtype=SELECTOR_TEST_DTYPE).reshape(-1)
        self.strings = np.frombuffer(bytes(pool), dtype=np.uint8).copy()

    def as_desc(self):
        """ctypes osmt_selectors_desc pointing into this object's arrays (keep `self` alive)."""
        d = abi.SelectorsDesc()
        d.selectors, d.n_selectors = self.selectors.ctypes.data_as(C.POINTER(abi.SelectorRec)), len(self.selectors)
        d.tests, d.n_tests = self.tests.ctypes.data_as(C.POINTER(abi.SelectorTest)), len(self.tests)
        d.strings, d.n_string_bytes = self.strings.ctypes.data_as(C.POINTER(C.c_uint8)), len(self.strings)
        return d

    def at_zoom(self, class_selectors, zoom):
        """osmt::selectors_at_zoom: the zoom filter of area_matches over a class's selector ids."""
        s = self.selectors[np.asarray(class_selectors, dtype=np.int64)]
        keep = ~((s["has_min_zoom"] != 0) & (zoom < s["min_zoom"])) & ~((s["has_max_zoom"] != 0) & (zoom > s["max_zoom"]))
        return np.asarray(class_selectors)[keep]


class Tags:
    """osmt_tags_desc over per-kind arrays: *_tag_off [n + 1] uint32, *_tags [n_tags, 4] uint32, strings uint8."""

    def __init__(self, node_tag_off, node_tags, way_tag_off, way_tags, multipolygon_tag_off, multipolygon_tags, strings):
        u32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint32).reshape(shape)
        self.node_tag_off, self.node_tags = u32(node_tag_off, -1), u32(node_tags, (-1, 4))
        self.way_tag_off, self.way_tags = u32(way_tag_off, -1), u32(way_tags, (-1, 4))
        self.multipolygon_tag_off, self.multipolygon_tags = u32(multipolygon_tag_off, -1), u32(multipolygon_tags, (-1, 4))
        self.strings = np.ascontiguousarray(strings, dtype=np.uint8).reshape(-1)

    def as_desc(self):
        u32 = C.POINTER(C.c_uint32)
        d = abi.TagsDesc()
        d.node_tag_off, d.node_tags = self.node_tag_off.ctypes.data_as(u32), self.node_tags.ctypes.data_as(u32)
        d.n_nodes, d.n_node_tags = len(self.node_tag_off) - 1, len(self.node_tags)
        d.way_tag_off, d.way_tags = self.way_tag_off.ctypes.data_as(u32), self.way_tags.ctypes.data_as(u32)
        d.n_ways, d.n_way_tags = len(self.way_tag_off) - 1, len(self.way_tags)
        d.multipolygon_tag_off, d.multipolygon_tags = self.multipolygon_tag_off.ctypes.data_as(u32), self.multipolygon_tags.ctypes.data_as(u32)
        d.n_multipolygons, d.n_multipolygon_tags = len(self.multipolygon_tag_off) - 1, len(self.multipolygon_tags)
        d.strings, d.n_string_bytes = self.strings.ctypes.data_as(C.POINTER(C.c_uint8)), len(self.strings)
        return d

    def value(self, v_off, v_len):
        return self.strings[v_off:v_off + v_len].tobytes()


class ClassLabelBindings:
    """osmt_class_label_bindings_desc.  class_bindings: per class one list of (label style id, index into `keys` or None), in
    push order; keys: the tag names text_style.text may name (str or bytes; neither sorted nor distinct)."""

    def __init__(self, zoom_lo, zoom_hi, class_bindings, keys=()):
        self.zoom_lo, self.zoom_hi = int(zoom_lo), int(zoom_hi)
        self.class_off = np.zeros(len(class_bindings) + 1, dtype=np.uint32)
        if len(class_bindings):
            self.class_off[1:] = np.cumsum([len(v) for v in class_bindings])
        flat = [(int(s), abi.TEXT_NONE if k is None else int(k)) for v in class_bindings for s, k in v]
        self.bindings = np.array(flat, dtype=CLASS_LABEL_BINDING_DTYPE).reshape(-1)
        raw = [_bytes(k) for k in keys]
        self.key_off = np.zeros(len(raw) + 1, dtype=np.uint32)
        if raw:
            self.key_off[1:] = np.cumsum([len(k) for k in raw])
        self.key_bytes = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()

    def as_desc(self):
        """ctypes osmt_class_label_bindings_desc pointing into this object's arrays (keep `self` alive)."""
        u32 = C.POINTER(C.c_uint32)
        d = abi.ClassLabelBindingsDesc()
        d.zoom_lo, d.zoom_hi = self.zoom_lo, self.zoom_hi
        d.class_off, d.bindings = self.class_off.ctypes.data_as(u32), self.bindings.ctypes.data_as(C.POINTER(abi.ClassLabelBinding))
        d.n_classes, d.n_bindings = len(self.class_off) - 1, len(self.bindings)
        d.key_off, d.key_bytes = self.key_off.ctypes.data_as(u32), self.key_bytes.ctypes.data_as(C.POINTER(C.c_uint8))
        d.n_keys, d.n_key_bytes = len(self.key_off) - 1, len(self.key_bytes)
        return d


RULE_PROP_DTYPE = np.dtype([("name", "u1"), ("kind", "u1"), ("has_color", "u1"), ("rgb", "u1", (3,)), ("has_image", "u1"), ("_pad", "u1"), ("image", "<u4"),
                            ("str_off", "<u4"), ("str_len", "<u4"), ("num_off", "<u4"), ("n_nums", "<u4"), ("_pad2", "<u4"), ("delta", "<f8")])
assert RULE_PROP_DTYPE.itemsize == 40
_PROP_OF = {n: i for i, n in enumerate(abi.PROP_NAMES)}


class RuleSet:
    """osmt_rules_desc over a registered selector set.  rules: [(selector layers, properties)] in stylesheet order; the
    selector layers are one entry per selector of the rule (None: no `::layer`; str / bytes: its name), the selectors being
    those of the SelectorSet in the same order; a property is (name, kind, value[, extra]):
      (name, PV_IDENTIFIER, id[, {"color": (r, g, b), "image": id}])   the caller's from_color_name / icon lookup, if any
      (name, PV_STRING, s[, {"image": id}])
      (name, PV_COLOR, (r, g, b))
      (name, PV_NUMBERS, [floats])
      (name, PV_WIDTH_DELTA, float)"""

    def __init__(self, selectors_id, rules, casing_width_multiplier=2.0, font_size_multiplier=None, font_id=0):
        self.selectors_id, self.font_id = int(selectors_id), int(font_id)
        self.casing_width_multiplier, self.font_size_multiplier = float(casing_width_multiplier), font_size_multiplier
        sel_rule, sel_layer, layer_off, layer_bytes = [], [], [0], bytearray()
        rule_off, props, numbers, pool = [0], [], [], bytearray()
        for r, (layers, ps) in enumerate(rules):
            for layer in layers:
                sel_rule.append(r)
                if layer is None:
                    sel_layer.append(abi.LAYER_DEFAULT)
                else:
                    sel_layer.append(len(layer_off) - 1)
                    layer_bytes.extend(_bytes(layer))
                    layer_off.append(len(layer_bytes))
            for p in ps:
                name, kind, value = p[0], p[1], p[2]
                extra = p[3] if len(p) > 3 else {}
                rec = np.zeros((), RULE_PROP_DTYPE)
                rec["name"], rec["kind"] = _PROP_OF.get(name, abi.PROP_OTHER), kind
                if kind in (abi.PV_IDENTIFIER, abi.PV_STRING):
                    b = _bytes(value)
                    rec["str_off"], rec["str_len"] = len(pool), len(b)
                    pool.extend(b)
                    if extra.get("image") is not None and name in ("icon-image", "fill-image"):
                        rec["has_image"], rec["image"] = 1, extra["image"]
                    if kind == abi.PV_IDENTIFIER and extra.get("color") is not None:
                        rec["has_color"], rec["rgb"] = 1, extra["color"]
                elif kind == abi.PV_COLOR:
                    rec["has_color"], rec["rgb"] = 1, value
                elif kind == abi.PV_NUMBERS:
                    rec["num_off"], rec["n_nums"] = len(numbers), len(value)
                    numbers.extend(float(v) for v in value)
                else:
                    rec["delta"] = float(value)
                props.append(rec)
            rule_off.append(len(props))
        u32 = lambda a: np.array(a, dtype=np.uint32).reshape(-1)
        self.selector_rule, self.selector_layer, self.layer_off, self.rule_prop_off = u32(sel_rule), u32(sel_layer), u32(layer_off), u32(rule_off)
        self.layer_bytes = np.frombuffer(bytes(layer_bytes), dtype=np.uint8).copy()
        self.props = np.array(props, dtype=RULE_PROP_DTYPE).reshape(-1)
        self.numbers = np.array(numbers, dtype=np.float64).reshape(-1)
        self.strings = np.frombuffer(bytes(pool), dtype=np.uint8).copy()

    def as_desc(self):
        """ctypes osmt_rules_desc pointing into this object's arrays (keep `self` alive)."""
        u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        d = abi.RulesDesc()
        d.selectors_id, d.font_id = self.selectors_id, self.font_id
        d.selector_rule, d.selector_layer, d.n_selectors = self.selector_rule.ctypes.data_as(u32), self.selector_layer.ctypes.data_as(u32), len(self.selector_rule)
        d.layer_off, d.layer_bytes = self.layer_off.ctypes.data_as(u32), self.layer_bytes.ctypes.data_as(u8)
        d.n_layers, d.n_layer_bytes = len(self.layer_off) - 1, len(self.layer_bytes)
        d.rule_prop_off, d.props = self.rule_prop_off.ctypes.data_as(u32), self.props.ctypes.data_as(C.POINTER(abi.RuleProp))
        d.n_rules, d.n_props = len(self.rule_prop_off) - 1, len(self.props)
        d.numbers, d.n_numbers = self.numbers.ctypes.data_as(C.POINTER(C.c_double)), len(self.numbers)
        d.strings, d.n_string_bytes = self.strings.ctypes.data_as(u8), len(self.strings)
        d.casing_width_multiplier = self.casing_width_multiplier
        d.has_font_size_multiplier = self.font_size_multiplier is not None
        d.font_size_multiplier = 0.0 if self.font_size_multiplier is None else float(self.font_size_multiplier)
        return d


def validate_rules(rules, class_layers=False, ctx=None):
    """osmt_validate_rules_ex over a RuleSet: the checks of Context.register_rules(rules, class_layers) without a device
    (ctx None: the lookups of ids are skipped).  Raises OsmtError with the refusal."""
    d = rules.as_desc()
    check(load().osmt_validate_rules_ex(C.byref(d), abi.RULES_CLASS_LAYERS if class_layers else 0, ctx._h if ctx is not None else None))


class CascadeResult:
    """The arrays of osmt_cascade_read (or of the host mirror).  Range r covers zooms zoom_lo[r] .. zoom_hi[r]; its class lists
    are class_style_off[r] / class_styles[range_style_base[r]:range_style_base[r + 1]] and class_off[r] / bindings[...]."""
    FIELDS = ("styles", "dashes", "label_styles", "key_bytes", "key_off", "zoom_lo", "zoom_hi", "class_style_off", "class_styles", "range_style_base",
              "class_off", "bindings", "range_binding_base")

    def __init__(self, counts):
        from .styled import LABEL_STYLE_REC_DTYPE, STYLE_REC_DTYPE

        n_st, n_d, n_ls, n_kb, n_k, n_r, n_cs, n_b, n_c = [int(c) for c in counts]
        self.n_classes = n_c
        self.styles, self.dashes, self.label_styles = np.zeros(n_st, STYLE_REC_DTYPE), np.zeros(n_d, np.float64), np.zeros(n_ls, LABEL_STYLE_REC_DTYPE)
        self.key_bytes, self.key_off = np.zeros(n_kb, np.uint8), np.zeros(n_k + 1, np.uint32)
        self.zoom_lo, self.zoom_hi = np.zeros(n_r, np.uint8), np.zeros(n_r, np.uint8)
        self.class_style_off, self.class_styles, self.range_style_base = np.zeros((n_r, n_c + 1), np.uint32), np.zeros(n_cs, np.uint32), np.zeros(n_r + 1, np.uint32)
        self.class_off, self.bindings, self.range_binding_base = np.zeros((n_r, n_c + 1), np.uint32), np.zeros(n_b, CLASS_LABEL_BINDING_DTYPE), np.zeros(n_r + 1, np.uint32)

    def arrays(self):
        return [getattr(self, f) for f in self.FIELDS]

    def pointers(self):
        return [C.c_void_p(a.ctypes.data) for a in self.arrays()]

    def keys(self):
        return [self.key_bytes[self.key_off[i]:self.key_off[i + 1]].tobytes() for i in range(len(self.key_off) - 1)]

    def range_of(self, zoom):
        return int(np.nonzero((self.zoom_lo <= zoom) & (zoom <= self.zoom_hi))[0][0])

    def class_styles_of(self, r):
        """per class the distinct style indices of range r"""
        pool, off = self.class_styles[self.range_style_base[r]:self.range_style_base[r + 1]], self.class_style_off[r]
        return [pool[off[c]:off[c + 1]].tolist() for c in range(self.n_classes)]

    def class_bindings_of(self, r):
        """per class the (distinct label style index, key index or None) pairs of range r"""
        pool, off = self.bindings[self.range_binding_base[r]:self.range_binding_base[r + 1]], self.class_off[r]
        return [[(int(s), None if k == abi.TEXT_NONE else int(k)) for s, k in pool[off[c]:off[c + 1]].tolist()] for c in range(self.n_classes)]


class Cascade:
    """An osmt_cascade.  Free with close()."""

    def __init__(self, match, handle):
        self.match, self._h = match, handle

    def read(self):
        L, counts = load(), (C.c_size_t * 9)()
        check(L.osmt_cascade_read(self._h, *([None] * 13), None, counts))
        out = CascadeResult(counts)
        caps = (C.c_size_t * 8)(*list(counts)[:8])
        check(L.osmt_cascade_read(self._h, *out.pointers(), caps, counts))
        return out

    def register(self, what):
        """osmt_cascade_register: (bindings_of_zoom, label_bindings_of_zoom, area_label_bindings_of_zoom), each uint32 [19]"""
        ids = [np.full(abi.MAX_ZOOM + 1, abi.BINDINGS_NONE, np.uint32) for _ in range(3)]
        check(load().osmt_cascade_register(self.match.ctx._h, self._h, self.match._h, what, *[C.c_void_p(a.ctypes.data) for a in ids]))
        return tuple(ids)

    def close(self):
        if self._h:
            load().osmt_cascade_free(self._h)
            self._h = None


class Declined(OsmtError):
    """osmt_match_selectors declined tag values: `declined` (DECLINED_NUMBER_DTYPE) lists them; compute their f64 and call again."""

    def __init__(self, code, msg, declined):
        super().__init__(code, msg)
        self.declined = declined


class Match:
    """An osmt_match: entity_class [n_entities], classes (MATCH_CLASS_DTYPE), class_selectors (pooled ids).  Free with close()."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        self._result = None

    def read(self):
        if self._result is None:
            L, counts = load(), (C.c_size_t * 3)()
            check(L.osmt_match_read(self._h, None, None, None, None, counts))
            ent = np.zeros(counts[0], np.uint32)
            cls = np.zeros(counts[1], MATCH_CLASS_DTYPE)
            sels = np.zeros(counts[2], np.uint32)
            caps = (C.c_size_t * 3)(*counts)
            ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
            check(L.osmt_match_read(self._h, ptr(ent), ptr(cls), ptr(sels), caps, counts))
            self._result = ent, cls, sels
        return self._result

    def declined(self):
        L, n = load(), C.c_size_t()
        check(L.osmt_match_read_declined_numbers(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, DECLINED_NUMBER_DTYPE)
        if n.value:
            check(L.osmt_match_read_declined_numbers(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def register_style_bindings(self, zoom_lo, zoom_hi, class_styles):
        """osmt_register_style_bindings_matched: class_styles is one list of style ids per class, in push order."""
        off = np.zeros(len(class_styles) + 1, dtype=np.uint32)
        if len(class_styles):
            off[1:] = np.cumsum([len(v) for v in class_styles])
        flat = np.array([s for v in class_styles for s in v], dtype=np.uint32)
        out = C.c_uint32()
        check(load().osmt_register_style_bindings_matched(self.ctx._h, self._h, zoom_lo, zoom_hi, C.c_void_p(off.ctypes.data),
                                                          C.c_void_p(flat.ctypes.data) if flat.size else None, len(class_styles), C.byref(out)))
        return out.value

    def _register_labels(self, call, zoom_lo, zoom_hi, class_bindings, keys):
        b = class_bindings if isinstance(class_bindings, ClassLabelBindings) else ClassLabelBindings(zoom_lo, zoom_hi, class_bindings, keys)
        d, out = b.as_desc(), C.c_uint32()
        check(call(self.ctx._h, self._h, C.byref(d), C.byref(out)))
        return out.value

    def register_label_bindings(self, zoom_lo, zoom_hi, class_bindings, keys=()):
        """osmt_register_label_bindings_matched: the node table.  class_bindings: per class one list of (label style id, index
        into `keys` or None); returns an id of the kind Context.register_label_bindings returns."""
        return self._register_labels(load().osmt_register_label_bindings_matched, zoom_lo, zoom_hi, class_bindings, keys)

    def register_area_label_bindings(self, zoom_lo, zoom_hi, class_bindings, keys=()):
        """osmt_register_area_label_bindings_matched: the table of ways and multipolygons; returns an id of the kind
        Context.register_area_label_bindings returns."""
        return self._register_labels(load().osmt_register_area_label_bindings_matched, zoom_lo, zoom_hi, class_bindings, keys)

    def cascade(self, rules_id, labels_all=True):
        """osmt_cascade_classes over the rule set `rules_id` (Context.register_rules): a Cascade."""
        h = C.c_void_p()
        check(load().osmt_cascade_classes(self.ctx._h, self._h, rules_id, 1 if labels_all else 0, C.byref(h)))
        return Cascade(self, h)

    def close(self):
        if self._h:
            load().osmt_match_free(self._h)
            self._h = None


def overrides(values):
    """NUMBER_OVERRIDE_DTYPE from [(v_off, v_len, float or None)], sorted by (v_off, v_len)."""
    out = np.zeros(len(values), NUMBER_OVERRIDE_DTYPE)
    for o, (off, ln, v) in zip(out, sorted(values, key=lambda t: (t[0], t[1]))):
        o["v_off"], o["v_len"], o["has_value"], o["value"] = off, ln, v is not None, 0.0 if v is None else v
    return out


def match(ctx, geodata_id, selectors_id, ov=None):
    """osmt_match_selectors.  Raises Declined (with the declined values) when the exact number parse declines tag values."""
    L, h = load(), C.c_void_p()
    n = 0 if ov is None else len(ov)
    rc = L.osmt_match_selectors(ctx._h, geodata_id, selectors_id, C.c_void_p(ov.ctypes.data) if n else None, n, C.byref(h))
    if rc == abi.OK:
        return Match(ctx, h)
    msg = L.osmt_last_error().decode("utf-8", "replace")
    if h.value:
        m = Match(ctx, h)
        d = m.declined()
        m.close()
        raise Declined(rc, msg, d)
    raise OsmtError(rc, msg)
