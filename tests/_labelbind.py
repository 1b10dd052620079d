"""Shared helpers of the tests of label bindings per class (tests/test_label_bindings_matched_cpu.py,
tests/test_gpu_label_bindings_matched.py): the shim over osm_renderer_amd/host/osmt_selmatch.hpp (the host mirrors
osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host, osmt::ClassLabelBindings) and
osm_renderer_amd/csrc/osmt_utf8.h, a Python restatement of the rule, and tags as numpy arrays a test can edit."""
import ctypes as C
import os
import subprocess

import numpy as np

from osm_renderer_amd import abi, selmatch
from osm_renderer_amd.styled import LABEL_BINDING_DTYPE
from tests._geodata import ROOT
from tests._selmatch import _stale

SHIM = os.path.join(ROOT, "tests", "_build", "liblabelbind_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "labelbind_host_main")
TABLE_MAIN = os.path.join(ROOT, "tests", "_build", "labelbind_utf8_table")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_selmatch.hpp", "osmt_geodata.hpp")]
_HDRS += [os.path.join(ROOT, "osm_renderer_amd", "csrc", h) for h in ("osmt_numparse.h", "osmt_utf8.h")] + [os.path.join(ROOT, "include", "osmtile.h")]
_lib = None
NONE = abi.TEXT_NONE


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "labelbind_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
        L.lb_table_new.restype = vp
        L.lb_table_new.argtypes = [C.POINTER(abi.TagsDesc), vp, C.POINTER(abi.ClassLabelBindingsDesc), C.c_int]
        L.lb_table_free.argtypes = [vp]
        L.lb_table_counts.argtypes = [vp, C.POINTER(sz)]
        L.lb_table_copy.restype = None
        L.lb_table_copy.argtypes = [vp] * 7
        L.lb_table_bad.restype = C.c_char_p
        L.lb_table_bad.argtypes = [vp, C.POINTER(sz)]
        L.lb_builder_new.restype = vp
        L.lb_builder_new.argtypes = [C.c_uint8, C.c_uint8]
        L.lb_builder_add_class.argtypes = [vp]
        L.lb_builder_bind.argtypes = [vp, u32, C.c_char_p, sz, C.c_int]
        L.lb_builder_get.restype = C.POINTER(abi.ClassLabelBindingsDesc)
        L.lb_builder_get.argtypes = [vp]
        L.lb_builder_free.argtypes = [vp]
        L.lb_utf8.restype = u32
        L.lb_utf8.argtypes = [C.c_char_p, u32, vp, C.POINTER(u32)]
        L.lb_utf8_many.restype = None
        L.lb_utf8_many.argtypes = [vp, u32, sz, vp, vp, vp]
        L.lb_sizeof.restype = sz
        L.lb_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def _build_program(out, name, flags):
    src = os.path.join(ROOT, "tests", name)
    if _stale(out, [src] + _HDRS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off"] + flags + ["-o", out, src])
    return out


def build_host_main():
    """tests/labelbind_host_main.cpp: mirror + decoder in a program of its own, under AddressSanitizer and UBSan"""
    return _build_program(HOST_MAIN, "labelbind_host_main.cpp", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def build_table_main():
    """tests/labelbind_utf8_table.cpp: every 3-byte string against a literal statement of Table 3-7"""
    return _build_program(TABLE_MAIN, "labelbind_utf8_table.cpp", ["-O2"])


def utf8(b):
    """csrc/osmt_utf8.h over bytes: (index of the first bad byte or None, the scalars or None)"""
    out, n = np.zeros(max(len(b), 1), np.uint32), C.c_uint32()
    bad = shim().lb_utf8(bytes(b), len(b), C.c_void_p(out.ctypes.data), C.byref(n))
    return (None, out[:n.value].tolist()) if bad == len(b) else (int(bad), None)


def py_utf8(b):
    """Python's strict decoder: the same pair"""
    try:
        return None, [ord(c) for c in bytes(b).decode("utf-8")]
    except UnicodeDecodeError as e:
        return e.start, None


def tags_of(t):
    """an editable selmatch.Tags (numpy copies) of a tests._selmatch.TagsOf"""
    d = t.desc()

    def arr(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    return selmatch.Tags(arr(d.node_tag_off, d.n_nodes + 1), arr(d.node_tags, 4 * d.n_node_tags), arr(d.way_tag_off, d.n_ways + 1),
                         arr(d.way_tags, 4 * d.n_way_tags), arr(d.multipolygon_tag_off, d.n_multipolygons + 1),
                         arr(d.multipolygon_tags, 4 * d.n_multipolygon_tags),
                         np.frombuffer(t.strings(), np.uint8).copy())


class Table:
    """the arrays of a label bindings table, as the read calls and the mirror return them"""

    def __init__(self, off0, bind0, off1, bind1, text_off, chars):
        self.off, self.bind, self.text_off, self.chars = (off0, off1), (bind0, bind1), text_off, chars

    def arrays(self):
        return [self.off[0], self.bind[0], self.off[1], self.bind[1], self.text_off, self.chars]

    def text(self, i):
        """text i as a str"""
        return "".join(chr(c) for c in self.chars[self.text_off[i]:self.text_off[i + 1]])

    def texts_of(self, kind, entity):
        """per binding of the entity (style, its text as a str or None)"""
        b = self.bind[kind][self.off[kind][entity]:self.off[kind][entity + 1]]
        return [(int(x["style"]), None if x["text"] == NONE else self.text(int(x["text"]))) for x in b]


class Refused(Exception):
    """the mirror found a used value that is not well-formed UTF-8"""

    def __init__(self, kind, entity, tag, v_off, v_len):
        super().__init__(f"{kind} {entity} tag {tag} v_off {v_off}")
        self.kind, self.entity, self.tag, self.v_off, self.v_len = kind, entity, tag, v_off, v_len


def mirror(tags, entity_class, bindings, area):
    """osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host over selmatch.Tags (or a ctypes osmt_tags_desc),
    the entity classes of a match and a selmatch.ClassLabelBindings: a Table, or raises Refused"""
    L = shim()
    td = tags.as_desc() if hasattr(tags, "as_desc") else tags
    bd = bindings.as_desc()
    ent = np.ascontiguousarray(entity_class, dtype=np.uint32)
    h = L.lb_table_new(C.byref(td), C.c_void_p(ent.ctypes.data), C.byref(bd), int(area))
    try:
        n = (C.c_size_t * 6)()
        if not L.lb_table_counts(h, n):
            out = (C.c_size_t * 4)()
            kind = L.lb_table_bad(h, out).decode()
            raise Refused(kind, *[int(x) for x in out])
        a = [np.zeros(n[0], np.uint32), np.zeros(n[1], LABEL_BINDING_DTYPE), np.zeros(n[2], np.uint32), np.zeros(n[3], LABEL_BINDING_DTYPE),
             np.zeros(n[4], np.uint32), np.zeros(n[5], np.uint32)]
        L.lb_table_copy(h, *[C.c_void_p(x.ctypes.data) for x in a])
        if not area:  # the node table has one kind
            a[2], a[3] = np.zeros(0, np.uint32), np.zeros(0, LABEL_BINDING_DTYPE)
        return Table(*a)
    finally:
        L.lb_table_free(h)


def py_table(tags, entity_class, bindings, area):
    """The rule restated in Python over selmatch.Tags: a dict lookup by key bytes, bytes.decode("utf-8"), texts numbered by
    first use in tag order of (v_off, v_len).  Returns (per kind [per entity [(style, (v_off, v_len) or None)]], the used ranges
    in text order, their decoded strings); raises UnicodeDecodeError for an ill-formed used value."""
    pool = tags.strings.tobytes()
    n_nodes, n_ways = len(tags.node_tag_off) - 1, len(tags.way_tag_off) - 1
    kinds = [(tags.way_tag_off, tags.way_tags, n_nodes), (tags.multipolygon_tag_off, tags.multipolygon_tags, n_nodes + n_ways)] if area else \
        [(tags.node_tag_off, tags.node_tags, 0)]
    keys = [bindings.key_bytes[bindings.key_off[k]:bindings.key_off[k + 1]].tobytes() for k in range(len(bindings.key_off) - 1)]
    per_kind, used = [], {}  # used: range -> the lowest tag number that uses it
    number = 0
    for off, quads, first in kinds:
        rows = []
        for i in range(len(off) - 1):
            q = quads[off[i]:off[i + 1]]
            by_key = {pool[a:a + b]: (number + j, (int(c), int(d))) for j, (a, b, c, d) in enumerate(q.tolist())}
            c = int(entity_class[first + i])
            row = []
            for style, k in bindings.bindings[bindings.class_off[c]:bindings.class_off[c + 1]].tolist():
                hit = by_key.get(keys[k]) if k != NONE else None
                if hit is not None:
                    used[hit[1]] = min(used.get(hit[1], hit[0]), hit[0])
                row.append((style, None if hit is None else hit[1]))
            rows.append(row)
            number += len(q)
        per_kind.append(rows)
    order = sorted(used, key=used.get)
    return per_kind, order, [pool[a:a + b].decode("utf-8") for a, b in order]


def same_as_py(table, py):
    """a Table against py_table's result, array by array"""
    per_kind, order, strings = py
    ids = {r: i for i, r in enumerate(order)}
    assert [table.text(i) for i in range(len(table.text_off) - 1)] == strings
    assert table.text_off.tolist() == [0] + np.cumsum([len(s) for s in strings]).tolist()
    for k, rows in enumerate(per_kind):
        assert table.off[k].tolist() == [0] + np.cumsum([len(r) for r in rows]).tolist()
        flat = [(s, NONE if r is None else ids[r]) for row in rows for s, r in row]
        assert [tuple(x) for x in table.bind[k].tolist()] == flat
