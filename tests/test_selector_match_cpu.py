"""Selector matching on the host (osm_renderer_amd/host/osmt_selmatch.hpp through tests/selmatch_shim.cpp): the mirror
osmt::match_selectors_host against a Python restatement written from mapcss/styler.rs, the number parsers against Python's
float() and int() behind Rust's grammar, the device's fast-path rule (csrc/osmt_numparse.h, compiled for the host), the
validators' refusals that need no device, and the mirror under ASan + UBSan as a stand-alone program."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch
from tests import _selmatch as sm

A = abi
CORPUS_VALID = ["5", "-0", "+3.5", ".5", "5.", "1e3", "1E-2", "0.1", "4.35", "inf", "-Infinity", "NaN", "-nan", str(2**53), str(2**53 + 1),
                "123456789012345678901234567890", "0" * 40 + "1", "1e22", "1e23", "1e99999999999", "0." + "0" * 30 + "1"]
CORPUS_ERRORS = ["", ".", "e5", "1e", " 1", "1 ", "0x10", "1_0", "١"]  # the last: ARABIC-INDIC DIGIT ONE
LAYERS = ["1", "-1", "+2", "", "-", "1.0", " 1", "9223372036854775807", "9223372036854775808", "-9223372036854775808", "0" * 21 + "1", "0", "+", "-0", "1e3",
          "99999999999999999999", "-9223372036854775809"]

KEYS = ["building", "highway", "lanes", "layer", "nam", "name", "name:en", "naïve", "oneway", "width", "имя"]
VALUES = ["yes", "true", "1", "Yes", "yes ", "", "no", "residential", "residentia", "residential_", "primary", "primarz", "2", "2.0", "3.5", "-1", "1e1",
          "abc", "nan", "inf", "07", ".", "4.35"]


def _random_selectors(rng, n):
    out = []
    for _ in range(n):
        tests = []
        for _ in range(int(rng.integers(0, 4))):
            kind, key = int(rng.integers(0, A.TEST_LESS + 4)), KEYS[int(rng.integers(0, len(KEYS)))]
            if kind in (A.TEST_EQUAL, A.TEST_NOT_EQUAL):
                tests.append((kind, key, VALUES[int(rng.integers(0, len(VALUES)))]))
            elif kind >= A.TEST_LESS:
                tests.append((kind, key, float(rng.choice([2.0, 3.5, -1.0, 10.0, 0.0, float("nan"), float("inf"), 4.35]))))
            else:
                tests.append((kind, key))
        lo = int(rng.integers(0, 19)) if rng.random() < 0.3 else None
        hi = int(rng.integers(0, 19)) if rng.random() < 0.3 else None
        out.append((int(rng.integers(0, 4)), tests, lo, hi))
    return out


def _random_tags(rng):
    keys = rng.choice(len(KEYS), int(rng.integers(0, 5)), replace=False)
    return {KEYS[k]: VALUES[int(rng.integers(0, len(VALUES)))] for k in keys}


def random_world(rng, n_nodes, n_ways, n_mps):
    w = sm.World()
    for _ in range(n_nodes):
        w.node(_random_tags(rng))
    for i in range(n_ways):
        (w.closed_way if i % 3 else w.open_way)(_random_tags(rng))
    for _ in range(n_mps):
        w.mp(_random_tags(rng))
    return w


def test_struct_layouts_match_the_header():
    s = sm.shim().sm_sizeof
    assert s(0) == C.sizeof(A.TagsDesc)
    assert s(1) == C.sizeof(A.SelectorTest) == selmatch.SELECTOR_TEST_DTYPE.itemsize == 32
    assert s(2) == C.sizeof(A.SelectorRec) == selmatch.SELECTOR_REC_DTYPE.itemsize == 16
    assert s(3) == C.sizeof(A.SelectorsDesc)
    assert s(4) == C.sizeof(A.NumberOverride) == selmatch.NUMBER_OVERRIDE_DTYPE.itemsize == 24
    assert s(5) == C.sizeof(A.DeclinedNumber) == selmatch.DECLINED_NUMBER_DTYPE.itemsize == 8
    assert s(6) == C.sizeof(A.MatchClass) == selmatch.MATCH_CLASS_DTYPE.itemsize == 24
    assert s(10) == A.TagsDesc.strings.offset
    assert s(11) == A.SelectorTest.value.offset == selmatch.SELECTOR_TEST_DTYPE.fields["value"][1]
    assert s(12) == A.SelectorRec.test_off.offset == selmatch.SELECTOR_REC_DTYPE.fields["test_off"][1]
    assert s(13) == A.NumberOverride.value.offset == selmatch.NUMBER_OVERRIDE_DTYPE.fields["value"][1]
    assert s(14) == A.MatchClass.first_entity.offset == selmatch.MATCH_CLASS_DTYPE.fields["first_entity"][1]
    assert s(15) == A.MatchClass.has_layer.offset == selmatch.MATCH_CLASS_DTYPE.fields["has_layer"][1]


def test_mirror_equals_the_restatement(tmp_path):
    """8 seeded worlds x 40 selectors x 300 entities: every (entity, selector) decision, the slots, the layers and the class
    numbering; the value pool makes every test kind hold and fail"""
    rng = np.random.default_rng(5)
    kinds_true, kinds_false = set(), set()
    for k in range(8):
        w = random_world(rng, 100, 150, 50)
        r = w.write(tmp_path / f"w{k}.bin")
        sels = _random_selectors(rng, 40)
        ent, cls, pooled = sm.mirror(r, selmatch.SelectorSet(sels))
        entities = w.entities(r)
        want_ent, want_cls = sm.py_match(entities, sels)
        assert ent.tolist() == want_ent
        assert sm.classes_as_tuples(cls, pooled) == want_cls
        for _, tags in entities:
            for sel in sels:
                for t in sel[1]:
                    (kinds_true if sm.py_test(tags, t) else kinds_false).add(t[0])
        r.close()
    assert kinds_true == kinds_false == set(range(10))


def test_number_parsers_against_float():
    """the mirror's parse and the device's fast path against float() behind Rust's grammar: equal bits, or declined — never
    different; a grammar error is an error in all three"""
    rng = np.random.default_rng(11)
    strings = list(CORPUS_VALID) + list(CORPUS_ERRORS) + ["+", "-", "1.e5", ".e5", "1e+", "infinit", "INF", "nAn", "+.5e-3", "00.100e+02", "1e-22", "1e-23",
                                                          "9007199254740992e22", "9007199254740993e-22", "0e99999999999", "-0.0e-9999", "1" + "0" * 22,
                                                          "1" + "0" * 23, "0." + "0" * 21 + "1", "0." + "0" * 22 + "1"]
    alphabet = "0123456789" * 3 + ".eE+-" + "x _"
    for _ in range(6000):
        n = int(rng.integers(1, 24))
        strings.append("".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n)))
    for _ in range(3000):  # well-formed decimals around the fast path's edges
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, int(rng.integers(1, 20))))
        point = int(rng.integers(0, len(digits) + 1))
        s = digits[:point] + "." + digits[point:] if rng.random() < 0.6 else digits
        if rng.random() < 0.5:
            s += "e" + str(int(rng.integers(-30, 31)))
        strings.append(("-" if rng.random() < 0.2 else "") + s)
    n_ok = n_declined = n_err = 0
    for s in strings:
        want = sm.py_f64(s)
        got = sm.parse_f64(s)
        rc, fast = sm.fast_path(s)
        if want is None:
            assert got is None and rc == sm.NUM_ERROR, s
            n_err += 1
            continue
        assert got is not None and sm.bits(got) == sm.bits(want) or (got != got and want != want), s
        assert rc != sm.NUM_ERROR, s
        if rc == sm.NUM_OK:
            assert sm.bits(fast) == sm.bits(want) or (fast != fast and want != want), (s, fast, want)
            n_ok += 1
        else:
            n_declined += 1
    assert n_ok > 2000 and n_declined > 200 and n_err > 2000, (n_ok, n_declined, n_err)
    # the corpus of the GPU test: at least half of its valid numbers take the fast path
    rcs = [sm.fast_path(s)[0] for s in CORPUS_VALID]
    assert all(rc != sm.NUM_ERROR for rc in rcs) and 2 * sum(rc == sm.NUM_OK for rc in rcs) >= len(rcs)
    assert [s for s, rc in zip(CORPUS_VALID, rcs) if rc == sm.NUM_DECLINED] == [str(2**53 + 1), "123456789012345678901234567890", "1e23", "1e99999999999",
                                                                               "0." + "0" * 30 + "1"]


def test_i64_parsers_against_int():
    rng = np.random.default_rng(13)
    strings = list(LAYERS)
    for _ in range(3000):
        n = int(rng.integers(1, 22))
        strings.append(("", "+", "-")[int(rng.integers(0, 3))] + "".join(str(int(d)) for d in rng.integers(0, 10, n)))
    for _ in range(500):
        strings.append("".join("0123456789+- ."[int(i)] for i in rng.integers(0, 14, int(rng.integers(0, 6)))))
    for s in strings:
        want = sm.py_i64(s)
        assert sm.parse_i64(s) == want, s
        assert sm.parse_i64(s, device=True) == want, s
    assert sm.py_i64("9223372036854775807") == 2**63 - 1 and sm.py_i64("9223372036854775808") is None and sm.py_i64("-9223372036854775808") == -(2**63)


def test_selector_set_builder_and_zoom_filter():
    """osmt::SelectorSet fills the descriptor selmatch.SelectorSet fills; osmt::selectors_at_zoom is the filter of area_matches"""
    rng = np.random.default_rng(17)
    sels = _random_selectors(rng, 60)
    py = selmatch.SelectorSet(sels)
    L = sm.shim()
    h = L.sm_set_new()
    for typ, tests, lo, hi in sels:
        L.sm_set_add(h, typ, -1 if lo is None else lo, -1 if hi is None else hi)
        for t in tests:
            key = selmatch._bytes(t[1])
            val = selmatch._bytes(t[2]) if t[0] in (A.TEST_EQUAL, A.TEST_NOT_EQUAL) else b""
            num = float(t[2]) if t[0] >= A.TEST_LESS else 0.0
            L.sm_set_test(h, t[0], key, len(key), val, len(val), num)
    d = L.sm_set_get(h).contents
    assert d.n_selectors == len(py.selectors) and d.n_tests == len(py.tests) and d.n_string_bytes == len(py.strings)
    assert C.string_at(d.selectors, 16 * d.n_selectors) == py.selectors.tobytes()
    assert C.string_at(d.tests, 32 * d.n_tests) == py.tests.tobytes()
    assert C.string_at(d.strings, d.n_string_bytes) == py.strings.tobytes()
    ids = np.arange(len(sels), dtype=np.uint32)
    for zoom in (0, 7, 12, 18):
        out = np.zeros(len(sels), np.uint32)
        n = L.sm_at_zoom(C.byref(py.as_desc()), ids.ctypes.data, len(ids), zoom, out.ctypes.data)
        want = [i for i, (_, _, lo, hi) in enumerate(sels) if not (lo is not None and zoom < lo) and not (hi is not None and zoom > hi)]
        assert out[:n].tolist() == want == py.at_zoom(ids, zoom).tolist()
    L.sm_set_free(h)


def _tags(node_tags=(), way_tags=(), mp_tags=(), strings=b"abcdefgh"):
    """selmatch.Tags from per-entity lists of (k_off, k_len, v_off, v_len)"""
    def csr(rows):
        off = np.zeros(len(rows) + 1, np.uint32)
        if len(rows):
            off[1:] = np.cumsum([len(v) for v in rows])
        return off, np.array([q for v in rows for q in v], dtype=np.uint32).reshape(-1, 4)

    return selmatch.Tags(*csr(node_tags), *csr(way_tags), *csr(mp_tags), np.frombuffer(strings, np.uint8))


def _tags_rc(t, mutate=None):
    d = t.as_desc()
    if mutate:
        mutate(d)
    L = lib.load()
    return L.osmt_validate_tags(C.byref(d), 0, None), L.osmt_last_error().decode()


def test_validate_tags_refusals():
    ok = _tags([[(0, 1, 1, 1), (1, 2, 0, 0)]], [[], [(2, 1, 3, 5)]], [[(7, 1, 8, 0)]])
    assert _tags_rc(ok)[0] == A.OK
    assert _tags_rc(_tags())[0] == A.OK  # nothing at all
    assert lib.load().osmt_validate_tags(None, 0, None) == A.INVALID_ARG

    def null(name):
        def f(d):
            setattr(d, name, None)
        return f

    for name in ("node_tags", "way_tag_off", "multipolygon_tags", "strings"):
        rc, msg = _tags_rc(ok, null(name))
        assert rc == A.INVALID_ARG and "NULL" in msg, (name, msg)
    # offsets: the house rules
    t = _tags([[(0, 1, 1, 1)]])
    t.node_tag_off[0] = 1
    assert "node_tag_off[0] is 1" in _tags_rc(t)[1]
    t = _tags([[(0, 1, 1, 1)], []])
    t.node_tag_off[:] = (0, 1, 0)
    rc, msg = _tags_rc(t)
    assert rc == A.INVALID_ARG and "less than the entry before" in msg
    t = _tags([], [[(0, 1, 1, 1), (1, 1, 1, 1)]])
    t.way_tag_off[1] = 1
    rc, msg = _tags_rc(t)
    assert rc == A.INVALID_ARG and "way_tag_off" in msg and "does not end at the 2 entries" in msg
    # a string range outside the pool: key and value
    for q in ((7, 2, 0, 1), (0, 1, 8, 1), (0xFFFFFFFF, 2, 0, 0)):
        rc, msg = _tags_rc(_tags([], [], [[q]]))
        assert rc == A.INVALID_ARG and "multipolygon 0" in msg and "8 string bytes" in msg, msg
    # keys: strictly ascending, as UNSIGNED bytes
    rc, msg = _tags_rc(_tags([[(1, 1, 0, 0), (0, 1, 0, 0)]]))
    assert rc == A.INVALID_ARG and "node 0" in msg and "strictly ascending" in msg
    rc, msg = _tags_rc(_tags([], [[], [(0, 2, 0, 0), (0, 2, 0, 0)]]))  # equal keys
    assert rc == A.INVALID_ARG and "way 1" in msg
    assert "strictly ascending" in _tags_rc(_tags([[(0, 2, 0, 0), (0, 1, 0, 0)]]))[1]  # "ab" then its prefix "a"
    hi = "zé".encode()  # 7A C3 A9
    assert _tags_rc(_tags([[(0, 1, 0, 0), (1, 2, 0, 0)]], strings=hi))[0] == A.OK  # 'z' < 'é' as unsigned bytes
    assert _tags_rc(_tags([[(1, 2, 0, 0), (0, 1, 0, 0)]], strings=hi))[0] == A.INVALID_ARG


def _sel_rc(s, mutate=None):
    d = s.as_desc()
    if mutate:
        mutate(d)
    L = lib.load()
    return L.osmt_validate_selectors(C.byref(d)), L.osmt_last_error().decode()


def test_validate_selectors_refusals():
    good = selmatch.SelectorSet([(A.SEL_WAY, [(A.TEST_EQUAL, "highway", "primary"), (A.TEST_LESS, "lanes", 3.0)], 10, None), (A.SEL_OTHER, [])])
    assert _sel_rc(good)[0] == A.OK
    assert _sel_rc(selmatch.SelectorSet([]))[0] == A.OK
    assert lib.load().osmt_validate_selectors(None) == A.INVALID_ARG
    for name in ("selectors", "tests", "strings"):
        def f(d, name=name):
            setattr(d, name, None)
        rc, msg = _sel_rc(good, f)
        assert rc == A.INVALID_ARG and "NULL" in msg
    # the limits, with the figure
    assert _sel_rc(selmatch.SelectorSet([(A.SEL_NODE, [])] * A.MATCH_MAX_SELECTORS))[0] == A.OK
    rc, msg = _sel_rc(selmatch.SelectorSet([(A.SEL_NODE, [])] * (A.MATCH_MAX_SELECTORS + 1)))
    assert rc == A.UNSUPPORTED and f"{A.MATCH_MAX_SELECTORS + 1} selectors" in msg and f"OSMT_MATCH_MAX_SELECTORS = {A.MATCH_MAX_SELECTORS}" in msg
    assert _sel_rc(selmatch.SelectorSet([(A.SEL_WAY, [(A.TEST_EXISTS, "k")] * A.MATCH_MAX_SELECTOR_TESTS)]))[0] == A.OK
    rc, msg = _sel_rc(selmatch.SelectorSet([(A.SEL_WAY, []), (A.SEL_WAY, [(A.TEST_EXISTS, "k")] * (A.MATCH_MAX_SELECTOR_TESTS + 1))]))
    assert rc == A.UNSUPPORTED and f"selector 1 has {A.MATCH_MAX_SELECTOR_TESTS + 1} tests" in msg and f"= {A.MATCH_MAX_SELECTOR_TESTS}" in msg
    # fields
    def bad(field_of, value, word, tests=False):
        s = selmatch.SelectorSet([(A.SEL_WAY, [(A.TEST_EQUAL, "highway", "primary")], 10, None)])
        (s.tests if tests else s.selectors)[field_of][0] = value
        rc, msg = _sel_rc(s)
        assert rc == A.INVALID_ARG and word in msg, (field_of, msg)

    bad("object_type", 4, "object type 4")
    bad("has_min_zoom", 2, "zoom flag")
    bad("test_off", 1, "leave the 1 tests")
    bad("kind", 10, "kind 10", tests=True)
    bad("key_len", 100, "string range", tests=True)
    bad("value_off", 0xFFFFFFF0, "string range", tests=True)


def test_host_program_under_sanitizers(tmp_path):
    """tests/selmatch_host_main.cpp under ASan + UBSan: its classes equal the restatement's over the same fixed selector set"""
    rng = np.random.default_rng(19)
    w = sm.World()
    pool = [{"highway": "primary", "bridge": "yes", "lanes": "2"}, {"building": "yes", "layer": "1"}, {"building": "yes"}, {"place": "town", "population": "5000"},
            {"place": "hamlet", "population": "1e4"}, {"tunnel": "1", "name:en": "x", "highway": "path"}, {}, {"layer": "-1", "highway": "x", "lanes": "2.5"},
            {"population": "many"}, {"layer": "1.0"}]
    for _ in range(60):
        w.node(pool[int(rng.integers(0, len(pool)))])
    for i in range(90):
        (w.closed_way if i % 2 else w.open_way)(pool[int(rng.integers(0, len(pool)))])
    for _ in range(20):
        w.mp(pool[int(rng.integers(0, len(pool)))])
    r = w.write(tmp_path / "w.bin")
    sels = [(A.SEL_WAY, [(A.TEST_EXISTS, "highway")]), (A.SEL_AREA, [(A.TEST_EQUAL, "building", "yes")], 12, None),
            (A.SEL_NODE, [(A.TEST_GREATER_OR_EQUAL, "population", 1000.0), (A.TEST_NOT_EQUAL, "place", "hamlet")], None, 15),
            (A.SEL_WAY, [(A.TEST_TRUE, "bridge"), (A.TEST_LESS, "lanes", 3.0)]), (A.SEL_OTHER, []),
            (A.SEL_WAY, [(A.TEST_FALSE, "tunnel"), (A.TEST_NOT_EXISTS, "name:en")])]
    out = subprocess.run([sm.build_host_main(), str(tmp_path / "w.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    _, want = sm.py_match(w.entities(r), sels)
    assert lines[0].split()[:2] == ["classes", str(len(want))]
    at14 = lambda ids: [s for s in ids if not (s == 2 and 14 > 15) and not (s == 1 and 14 < 12)]
    for line, (slot, has_layer, layer, first, ids) in zip(lines[1:], want):
        assert [int(v) for v in line.split()] == [slot, has_layer, first, layer] + at14(ids)
    assert lines[len(want) + 1].startswith("numbers ")
    r.close()
