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
