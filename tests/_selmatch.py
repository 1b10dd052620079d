"""Shared helpers of the selector-match tests (tests/test_selector_match_cpu.py, tests/test_gpu_selector_match.py): the shim
over osm_renderer_amd/host/osmt_selmatch.hpp (osmt::TagsDesc, osmt::SelectorSet, the host mirror osmt::match_selectors_host,
the parsers), a Python restatement of matches_by_tags written from mapcss/styler.rs, and small tagged worlds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from osm_renderer_amd import abi, selmatch
from tests._geodata import ROOT, Reader, write_geodata

SHIM = os.path.join(ROOT, "tests", "_build", "libselmatch_shim.so")
HOST_MAIN = os.path.join(ROOT, "tests", "_build", "selmatch_host_main")
HOST_DEMO = os.path.join(ROOT, "tests", "_build", "selmatch_host_demo")
_HDRS = [os.path.join(ROOT, "osm_renderer_amd", "host", h) for h in ("osmt_selmatch.hpp", "osmt_geodata.hpp")]
_HDRS += [os.path.join(ROOT, "osm_renderer_amd", "csrc", "osmt_numparse.h"), os.path.join(ROOT, "include", "osmtile.h")]
_lib = None

NUM_ERROR, NUM_OK, NUM_DECLINED = 0, 1, 2
# str::parse::<f64>, as a regular expression
F64_RE = re.compile(r"[+-]?(inf|infinity|nan|(\d+\.?\d*|\.\d+)(e[+-]?\d+)?)", re.I | re.A)
I64_RE = re.compile(r"[+-]?\d+", re.A)


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)


def shim():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "selmatch_shim.cpp")
        if _stale(SHIM, [src] + _HDRS):
            os.makedirs(os.path.dirname(SHIM), exist_ok=True)
            tmp = f"{SHIM}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-o", tmp, src])
            os.replace(tmp, SHIM)
        L = C.CDLL(SHIM)
        vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
        L.sm_tags_new.restype = vp
        L.sm_tags_new.argtypes = [vp]
        L.sm_tags_get.restype = C.POINTER(abi.TagsDesc)
        L.sm_tags_get.argtypes = [vp]
        L.sm_tags_free.argtypes = [vp]
        L.sm_set_new.restype = vp
        L.sm_set_add.argtypes = [vp, C.c_uint8, C.c_int, C.c_int]
        L.sm_set_test.argtypes = [vp, C.c_uint32, cp, sz, cp, sz, C.c_double]
        L.sm_set_get.restype = C.POINTER(abi.SelectorsDesc)
        L.sm_set_get.argtypes = [vp]
        L.sm_set_free.argtypes = [vp]
        L.sm_match_host.restype = None
        L.sm_match_host.argtypes = [vp, C.POINTER(abi.SelectorsDesc), vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
        for f in (L.sm_parse_f64, L.sm_fast_path):
            f.argtypes = [cp, sz, C.POINTER(C.c_double)]
        for f in (L.sm_parse_i64, L.sm_device_i64):
            f.argtypes = [cp, sz, C.POINTER(C.c_int64)]
        L.sm_host_numbers.restype = None
        L.sm_host_numbers.argtypes = [vp, vp, sz, vp]
        L.sm_at_zoom.restype = sz
        L.sm_at_zoom.argtypes = [C.POINTER(abi.SelectorsDesc), vp, sz, C.c_uint8, vp]
        L.sm_sizeof.restype = sz
        L.sm_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def build_host_main():
    """the stand-alone host program over osmt_selmatch.hpp, under AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "selmatch_host_main.cpp")
    if _stale(HOST_MAIN, [src] + _HDRS):
        os.makedirs(os.path.dirname(HOST_MAIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", HOST_MAIN, src])
    return HOST_MAIN


def build_demo():
    """tests/selmatch_host_demo.cpp: the declined-and-retry loop over the C ABI, linked to libosmtile.so"""
    src = os.path.join(ROOT, "tests", "selmatch_host_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    lib = os.path.join(libdir, "libosmtile.so")
    if _stale(HOST_DEMO, [src, lib] + _HDRS):
        os.makedirs(os.path.dirname(HOST_DEMO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", HOST_DEMO, src, "-L" + libdir, "-losmtile",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    return HOST_DEMO


def fast_path(s):
    """(status, value) of the device's number rule over bytes or str"""
    b, v = selmatch._bytes(s), C.c_double()
    rc = shim().sm_fast_path(b, len(b), C.byref(v))
    return rc, v.value


def parse_f64(s):
    """the mirror's str::parse::<f64>: a float, or None for an error"""
    b, v = selmatch._bytes(s), C.c_double()
    return v.value if shim().sm_parse_f64(b, len(b), C.byref(v)) else None


def parse_i64(s, device=False):
    b, v = selmatch._bytes(s), C.c_int64()
    f = shim().sm_device_i64 if device else shim().sm_parse_i64
    return v.value if f(b, len(b), C.byref(v)) else None


def py_f64(s):
    """str::parse::<f64> restated with Python: the grammar as a regular expression, then float() (correctly rounded)"""
    try:
        t = selmatch._bytes(s).decode("ascii")
    except UnicodeDecodeError:
        return None
    return float(t) if F64_RE.fullmatch(t) else None


def py_i64(s):
    try:
        t = selmatch._bytes(s).decode("ascii")
    except UnicodeDecodeError:
        return None
    if not I64_RE.fullmatch(t):
        return None
    v = int(t)
    return v if -(1 << 63) <= v < (1 << 63) else None


def bits(x):
    return np.float64(x).view(np.uint64)


class TagsOf:
    """osmt::TagsDesc over a tests._geodata.Reader"""

    def __init__(self, r):
        self.r = r
        self.h = shim().sm_tags_new(r.h)

    def desc(self):
        return shim().sm_tags_get(self.h).contents

    def way_tag(self, i, j):
        """tag j of way i: (k_off, k_len, v_off, v_len)"""
        d = self.desc()
        q = 4 * (d.way_tag_off[i] + j)
        return tuple(int(d.way_tags[q + k]) for k in range(4))

    def strings(self):
        d = self.desc()
        return C.string_at(d.strings, d.n_string_bytes) if d.n_string_bytes else b""

    def close(self):
        if self.h:
            shim().sm_tags_free(self.h)
            self.h = None


def mirror(r, sel):
    """osmt::match_selectors_host over a Reader and a selmatch.SelectorSet: (entity_class, classes, class_selectors)"""
    L, d = shim(), sel.as_desc()
    counts, caps = (C.c_size_t * 3)(), (C.c_size_t * 3)()
    L.sm_match_host(r.h, C.byref(d), None, None, None, caps, counts)
    ent, cls, sels = np.zeros(counts[0], np.uint32), np.zeros(counts[1], selmatch.MATCH_CLASS_DTYPE), np.zeros(counts[2], np.uint32)
    caps = (C.c_size_t * 3)(*counts)
    L.sm_match_host(r.h, C.byref(d), ent.ctypes.data, cls.ctypes.data, sels.ctypes.data, caps, counts)
    return ent, cls, sels


def host_numbers(strings, declined):
    """osmt::HostNumbers: NUMBER_OVERRIDE_DTYPE for DECLINED_NUMBER_DTYPE entries"""
    out = np.zeros(len(declined), selmatch.NUMBER_OVERRIDE_DTYPE)
    buf = C.create_string_buffer(strings, len(strings))
    d = np.ascontiguousarray(declined)
    shim().sm_host_numbers(C.addressof(buf), d.ctypes.data, len(d), out.ctypes.data)
    return out


# ---- the restatement, written from mapcss/styler.rs:450-557 -----------------------------------------------------------------
def py_test(tags, t):
    """matches_by_tags: tags is {bytes: bytes}, t a test tuple of selmatch.SelectorSet"""
    kind, v = t[0], tags.get(selmatch._bytes(t[1]))
    true = v in (b"yes", b"true", b"1")
    if kind == abi.TEST_EXISTS:
        return v is not None
    if kind == abi.TEST_NOT_EXISTS:
        return v is None
    if kind == abi.TEST_TRUE:
        return true
    if kind == abi.TEST_FALSE:
        return not true
    if kind == abi.TEST_EQUAL:
        return v == selmatch._bytes(t[2])
    if kind == abi.TEST_NOT_EQUAL:
        return v != selmatch._bytes(t[2])
    x = None if v is None else py_f64(v)
    if x is None:
        return False
    rhs = float(t[2])
    return {abi.TEST_LESS: x < rhs, abi.TEST_LESS_OR_EQUAL: x <= rhs, abi.TEST_GREATER: x > rhs, abi.TEST_GREATER_OR_EQUAL: x >= rhs}[kind]


def py_match(entities, selectors):
    """entities: [(slot, {bytes: bytes})] in entity order; selectors as selmatch.SelectorSet takes them.  Returns (entity
    classes, [(slot, has_layer, layer, first entity, [selector ids])]) with classes numbered by their lowest member."""
    seen, classes, ent = {}, [], []
    for e, (slot, tags) in enumerate(entities):
        ids = []
        for s, sel in enumerate(selectors):
            typ = sel[0]
            good = typ == abi.SEL_NODE if slot == 0 else (typ == abi.SEL_WAY or (typ == abi.SEL_AREA and slot != 2))
            if good and all(py_test(tags, t) for t in sel[1]):
                ids.append(s)
        layer = py_i64(tags[b"layer"]) if b"layer" in tags else None
        key = (slot, layer is not None, layer or 0, tuple(ids))
        if key not in seen:
            seen[key] = len(classes)
            classes.append((slot, int(layer is not None), layer or 0, e, ids))
        ent.append(seen[key])
    return ent, classes


def classes_as_tuples(cls, sels):
    return [(int(c["slot"]), int(c["has_layer"]), int(c["layer"]), int(c["first_entity"]), sels[c["sel_off"]:c["sel_off"] + c["n_sels"]].tolist())
            for c in cls]


# ---- worlds -----------------------------------------------------------------------------------------------------------------
LAT0, LON0 = 55.75, 37.61


class World:
    """nodes, ways and multipolygons with tags ({str: str}); write() makes the file and a Reader"""

    def __init__(self):
        self.nodes, self.ways, self.polygons, self.mps = [], [], [], []

    def node(self, tags=None, lat=None, lon=None):
        k = len(self.nodes)
        self.nodes.append((1000 + k, LAT0 + 1e-5 * (k % 97) if lat is None else lat, LON0 + 1e-5 * (k // 97) if lon is None else lon, dict(tags or {})))
        return k

    def way(self, node_ids, tags=None):
        self.ways.append((5000 + len(self.ways), list(node_ids), dict(tags or {})))
        return len(self.ways) - 1

    def open_way(self, tags=None):
        return self.way([self.node(), self.node()], tags)

    def closed_way(self, tags=None):
        a = self.node()
        return self.way([a, self.node(), self.node(), a], tags)

    def mp(self, tags=None, n_polygons=1):
        ids = []
        for _ in range(n_polygons):
            a = self.node()
            self.polygons.append([a, self.node(), self.node(), a])
            ids.append(len(self.polygons) - 1)
        self.mps.append((9000 + len(self.mps), ids, dict(tags or {})))
        return len(self.mps) - 1

    def write(self, path, max_zoom_tile=None):
        """max_zoom_tile(lat, lon) -> (x, y): the file gets the tile references of saver.rs (kept in self.refs), else none"""
        self.refs = write_geodata(str(path), self.nodes, self.ways, self.polygons, self.mps, tile_refs=None if max_zoom_tile else {},
                                  max_zoom_tile=max_zoom_tile)
        return Reader(str(path))

    def entities(self, r):
        """[(slot, {bytes: bytes})] in entity order, the slots from the Reader's own is_closed"""
        b = lambda t: {selmatch._bytes(k): selmatch._bytes(v) for k, v in t.items()}
        out = [(0, b(t)) for _, _, _, t in self.nodes]
        out += [(1 if r.way_is_closed(i) else 2, b(t)) for i, (_, _, t) in enumerate(self.ways)]
        return out + [(3, b(t)) for _, _, t in self.mps]
