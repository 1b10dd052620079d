"""Label bindings per class on the host: the mirrors osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host
(osm_renderer_amd/host/osmt_selmatch.hpp through tests/labelbind_shim.cpp) against a Python restatement of the rule, the UTF-8
decoder and validator of osm_renderer_amd/csrc/osmt_utf8.h (compiled for the host) against Python's strict decoder and, in a
program of its own, against a literal statement of Table 3-7, the validator's refusals that need no device, and mirror and
decoder under ASan + UBSan as a stand-alone program."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch
from tests import _labelbind as lb
from tests import _selmatch as sm

A = abi
KEYS = ["name", "nam", "name:en", "ref", "имя", "", "brand", "zzz"]
VALUES = ["Main Street", "Main Street", "", "é", "Москва", "京都", "A1", "a", "😀 park", "x" * 70, "Main", "\x00", "\x7f\u0080߿ࠀ￿\U00010000\U0010ffff"]


def _world(rng, n_nodes, n_ways, n_mps):
    """tags drawn from few keys and few values: ties (one value under several keys and on several entities) are the rule"""
    def tags():
        ks = rng.choice(len(KEYS), int(rng.integers(0, 5)), replace=False)
        t = {KEYS[k]: VALUES[int(rng.integers(0, len(VALUES)))] for k in ks}
        if rng.random() < 0.2:
            t["layer"] = str(int(rng.integers(-1, 2)))
        if rng.random() < 0.5:
            t["highway"] = ("primary", "path")[int(rng.integers(0, 2))]
        return t

    w = sm.World()
    for _ in range(n_nodes):
        w.node(tags())
    for i in range(n_ways):
        (w.closed_way if i % 3 else w.open_way)(tags())
    for _ in range(n_mps):
        w.mp(tags())
    return w


def _class_bindings(rng, n_classes, n_keys):
    """0 .. 3 bindings per class; keys drawn with repeats, some bindings without a key"""
    out = []
    for _ in range(n_classes):
        out.append([(int(rng.integers(0, 50)), None if rng.random() < 0.25 else int(rng.integers(0, n_keys))) for _ in range(int(rng.integers(0, 4)))])
    return out


def test_struct_layouts_match_the_header():
    s = lb.shim().lb_sizeof
    assert s(0) == C.sizeof(A.ClassLabelBinding) == selmatch.CLASS_LABEL_BINDING_DTYPE.itemsize == 8
    assert s(1) == C.sizeof(A.ClassLabelBindingsDesc) == 72
    assert s(10) == A.ClassLabelBindingsDesc.class_off.offset == 8
    assert s(11) == A.ClassLabelBindingsDesc.n_classes.offset
    assert s(12) == A.ClassLabelBindingsDesc.key_off.offset
    assert s(13) == A.ClassLabelBindingsDesc.n_key_bytes.offset
    assert A.LABEL_TEXT_KEYS_MAX == 256


def test_mirror_equals_the_restatement(tmp_path):
    """6 seeded worlds, both tables: offsets, bindings, the numbering of the texts and their scalars; the worlds make one value
    serve several keys and entities, the empty value, the empty key, classes without bindings and bindings without a key"""
    rng = np.random.default_rng(11)
    seen_shared = seen_empty_value = seen_none = 0
    for k in range(6):
        w = _world(rng, 120, 90, 40)
        r = w.write(tmp_path / f"w{k}.bin")
        t = sm.TagsOf(r)
        tags = lb.tags_of(t)
        ent, cls, _ = sm.mirror(r, selmatch.SelectorSet([(A.SEL_WAY, [(A.TEST_EXISTS, "highway")]), (A.SEL_NODE, [(A.TEST_EQUAL, "highway", "path")])]))
        keys = KEYS + ["name", "nobody has this"]  # a duplicate and a key that is never found
        b = selmatch.ClassLabelBindings(3, 17, _class_bindings(rng, len(cls), len(keys)), keys)
        for area in (False, True):
            got, want = lb.mirror(tags, ent, b, area), lb.py_table(tags, ent, b, area)
            lb.same_as_py(got, want)
            per_kind, order, strings = want
            flat = [x for rows in per_kind for row in rows for _, x in row]
            seen_none += sum(x is None for x in flat)
            seen_shared += len([x for x in flat if x is not None]) - len(order)
            seen_empty_value += sum(s == "" for s in strings)
            assert len(set(strings)) == len(strings)  # the writer interns: equal strings are equal ranges
        t.close()
        r.close()
    assert seen_shared > 100 and seen_empty_value and seen_none


def test_text_numbering_follows_tags_not_bindings(tmp_path):
    """one entity whose first binding reads its LAST tag: the texts are numbered by the tags' order, and a value whose
    lowest-numbered tag belongs to an entity without bindings is numbered by its lowest USED tag"""
    w = sm.World()
    w.node({"layer": "5", "name": "shared"})  # its class gets no bindings: this tag uses nothing
    w.node({"a": "first tag", "z": "last tag"})
    w.node({"name": "shared"})
    r = w.write(tmp_path / "w.bin")
    t = sm.TagsOf(r)
    tags = lb.tags_of(t)
    ent, cls, _ = sm.mirror(r, selmatch.SelectorSet([]))
    assert len(cls) == 2 and ent.tolist() == [0, 1, 1]
    b = selmatch.ClassLabelBindings(0, 18, [[], [(1, 0), (2, 1), (3, 2)]], ["z", "a", "name"])
    got = lb.mirror(tags, ent, b, False)
    lb.same_as_py(got, lb.py_table(tags, ent, b, False))
    assert [got.text(i) for i in range(3)] == ["first tag", "last tag", "shared"]
    assert got.texts_of(0, 0) == [] and got.texts_of(0, 1) == [(1, "last tag"), (2, "first tag"), (3, None)]
    assert got.texts_of(0, 2) == [(1, None), (2, None), (3, "shared")]
    t.close()
    r.close()


def test_mirror_refuses_ill_formed_used_values(tmp_path):
    """the pool edited in place: an ill-formed value is refused naming the lowest-numbered USED tag; the same bytes under a tag no
    binding reads are accepted"""
    w = sm.World()
    w.node({"name": "AAAA", "note": "BBBB"})
    w.node({"name": "CCCC"})
    r = w.write(tmp_path / "w.bin")
    t = sm.TagsOf(r)
    tags = lb.tags_of(t)
    ent = sm.mirror(r, selmatch.SelectorSet([]))[0]
    pool = tags.strings.tobytes()
    for word, bad in ((b"BBBB", b"\xed\xa0\x80B"), (b"CCCC", b"C\xc0\x80C"), (b"AAAA", b"AAA\xff")):
        at = pool.index(word)
        tags.strings[at:at + 4] = np.frombuffer(bad, np.uint8)
    b = selmatch.ClassLabelBindings(0, 18, [[(0, 0)]], ["name"])
    with pytest.raises(lb.Refused) as e:
        lb.mirror(tags, ent, b, False)
    assert (e.value.kind, e.value.entity, e.value.v_off, e.value.v_len) == ("node", 0, pool.index(b"AAAA"), 4)
    with pytest.raises(UnicodeDecodeError):
        lb.py_table(tags, ent, b, False)
    at = pool.index(b"AAAA")
    tags.strings[at:at + 4] = np.frombuffer(b"good", np.uint8)
    with pytest.raises(lb.Refused) as e:
        lb.mirror(tags, ent, b, False)
    assert (e.value.kind, e.value.entity, e.value.tag) == ("node", 1, 0)
    at = pool.index(b"CCCC")
    tags.strings[at:at + 4] = np.frombuffer(b"fine", np.uint8)
    got = lb.mirror(tags, ent, b, False)  # "note" still holds a surrogate: nobody reads it
    assert [got.text(i) for i in range(2)] == ["good", "fine"]
    t.close()
    r.close()


def _many(strings, length):
    """csrc/osmt_utf8.h over equally long strings at once: (first bad byte or `length`, scalar count, scalars)"""
    n = len(strings)
    buf = np.frombuffer(b"".join(strings), np.uint8).copy() if length else np.zeros(1, np.uint8)
    bad, count, scalars = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(max(n * length, 1), np.uint32)
    lb.shim().lb_utf8_many(C.c_void_p(buf.ctypes.data), length, n, C.c_void_p(bad.ctypes.data), C.c_void_p(count.ctypes.data), C.c_void_p(scalars.ctypes.data))
    return bad, count, scalars.reshape(-1, max(length, 1)) if length else scalars


def test_decoder_on_every_string_of_one_and_two_bytes():
    """accept / reject, the scalars and the index of the first bad byte against bytes.decode("utf-8")"""
    assert lb.utf8(b"") == lb.py_utf8(b"") == (None, [])
    for length in (1, 2):
        strings = [v.to_bytes(length, "big") for v in range(256 ** length)]
        bad, count, scalars = _many(strings, length)
        accepted = 0
        for i, s in enumerate(strings):
            stop, want = lb.py_utf8(s)
            if stop is None:
                assert bad[i] == length and scalars[i, :count[i]].tolist() == want, s
                accepted += 1
            else:
                assert bad[i] == stop, s
        assert accepted == (128 if length == 1 else 128 * 128 + 30 * 64)


def _seeded_strings(rng, n):
    """valid sequences of every length class, then seeded corruptions: a byte replaced, dropped, inserted, or the string cut"""
    edges = [0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF]
    out = []
    for _ in range(n):
        cps = []
        for _ in range(int(rng.integers(0, 9))):
            kind = int(rng.integers(0, 6))
            hi = (0x80, 0x800, 0x10000, 0x110000)[min(kind, 3)]
            cp = edges[int(rng.integers(0, len(edges)))] if kind >= 4 else int(rng.integers(0, hi))
            if 0xD800 <= cp < 0xE000:
                cp = 0xD7FF
            cps.append(cp)
        s = bytearray("".join(chr(c) for c in cps).encode("utf-8"))
        how = int(rng.integers(0, 6))
        if s and how == 1:
            s[int(rng.integers(0, len(s)))] = int(rng.choice([0x80, 0xBF, 0xC0, 0xC1, 0xE0, 0xED, 0xF0, 0xF4, 0xF5, 0xFF, 0xA0, 0x9F, 0x90, 0x8F, 0x7F]))
        elif s and how == 2:
            del s[int(rng.integers(0, len(s)))]
        elif how == 3:
            s.insert(int(rng.integers(0, len(s) + 1)), int(rng.integers(0x80, 0x100)))
        elif s and how == 4:
            del s[int(rng.integers(0, len(s))):]
        out.append(bytes(s))
    return out


def test_decoder_on_seeded_strings():
    rng = np.random.default_rng(17)
    strings = _seeded_strings(rng, 20000)
    good = bad = 0
    for s in strings:
        got, want = lb.utf8(s), lb.py_utf8(s)
        assert got == want, s
        good += want[0] is None
        bad += want[0] is not None
    assert good > 5000 and bad > 5000


def test_decoder_against_table_3_7_in_a_program_of_its_own():
    """tests/labelbind_utf8_table.cpp: every string of 1, 2 and 3 bytes and the corners of the 4-byte rows"""
    out = subprocess.run([lb.build_table_main()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["OK", str(256 + 256 ** 2 + 256 ** 3 + 14)], (out.stdout[-500:], out.stderr[-500:])


def test_builder_pools_keys():
    """osmt::ClassLabelBindings: equal keys share an entry, the empty key is a key, a binding without text has OSMT_TEXT_NONE"""
    L = lb.shim()
    h = L.lb_builder_new(2, 9)
    for rows in ([(5, b"name"), (6, None)], [], [(7, b""), (8, b"name"), (9, "имя".encode())]):
        L.lb_builder_add_class(h)
        for style, key in rows:
            L.lb_builder_bind(h, style, key or b"", len(key or b""), key is not None)
    d = L.lb_builder_get(h).contents
    assert (d.zoom_lo, d.zoom_hi, d.n_classes, d.n_bindings, d.n_keys) == (2, 9, 3, 5, 3)
    assert [d.class_off[i] for i in range(4)] == [0, 2, 2, 5]
    assert [(d.bindings[i].style, d.bindings[i].text_key) for i in range(5)] == [(5, 0), (6, A.TEXT_NONE), (7, 1), (8, 0), (9, 2)]
    assert [d.key_off[i] for i in range(4)] == [0, 4, 4, 10] and C.string_at(d.key_bytes, 10) == b"name" + "имя".encode()
    assert lib.load().osmt_validate_class_label_bindings(C.byref(d), None, None) == A.OK
    L.lb_builder_free(h)


def test_validate_class_label_bindings_refusals():
    """osmt_validate_class_label_bindings without a match and without a context: what can be checked is checked"""
    L = lib.load()

    def rc_of(b, edit=None):
        d = b.as_desc()
        if edit:
            edit(d)
        rc = L.osmt_validate_class_label_bindings(C.byref(d), None, None)
        return rc, L.osmt_last_error().decode()

    good = lambda: selmatch.ClassLabelBindings(0, 18, [[(0, 0), (1, None)], [], [(2, 1)]], ["name", ""])
    assert rc_of(good())[0] == A.OK
    assert rc_of(selmatch.ClassLabelBindings(0, 18, [], []))[0] == A.OK
    assert L.osmt_validate_class_label_bindings(None, None, None) == A.INVALID_ARG
    for lo, hi in ((5, 19), (7, 6)):
        rc, msg = rc_of(selmatch.ClassLabelBindings(lo, hi, [[]], []))
        assert rc == A.INVALID_ARG and "zoom range" in msg
    b = good()
    b.class_off[0] = 1
    rc, msg = rc_of(b)
    assert rc == A.INVALID_ARG and "class_off[0] is 1" in msg
    b = good()
    b.class_off[2] = 1
    rc, msg = rc_of(b)
    assert rc == A.INVALID_ARG and "less than the entry before" in msg
    b = good()
    b.class_off[3] = 2
    rc, msg = rc_of(b)
    assert rc == A.INVALID_ARG and "does not end at" in msg
    b = good()
    b.key_off[1] = 9
    rc, msg = rc_of(b)
    assert rc == A.INVALID_ARG and "key_off" in msg
    b = good()
    b.bindings["text_key"][0] = 2
    rc, msg = rc_of(b)
    assert rc == A.INVALID_ARG and "text_key = 2" in msg
    b = good()
    b.bindings["text_key"][0] = A.TEXT_NONE - 1
    assert rc_of(b)[0] == A.INVALID_ARG

    def null_bindings(d):
        d.bindings = None

    rc, msg = rc_of(good(), null_bindings)
    assert rc == A.INVALID_ARG and "NULL array" in msg
    rc, msg = rc_of(selmatch.ClassLabelBindings(0, 18, [[]], [f"k{i}" for i in range(A.LABEL_TEXT_KEYS_MAX)]))
    assert rc == A.OK
    rc, msg = rc_of(selmatch.ClassLabelBindings(0, 18, [[]], [f"k{i}" for i in range(A.LABEL_TEXT_KEYS_MAX + 1)]))
    assert rc == A.UNSUPPORTED and "257 keys" in msg and "= 256" in msg


def test_host_program_under_sanitizers(tmp_path):
    """tests/labelbind_host_main.cpp under ASan + UBSan: both mirrors over a written world, the decoder over strings that end
    where their heap block ends; its figures equal the restatement's"""
    rng = np.random.default_rng(23)
    w = _world(rng, 80, 70, 30)
    for i in range(10):
        w.node({"place": "town", "name": VALUES[i % len(VALUES)], "ref": f"R{i % 3}"})
    r = w.write(tmp_path / "w.bin")
    t = sm.TagsOf(r)
    tags = lb.tags_of(t)
    sels = [(A.SEL_WAY, [(A.TEST_EXISTS, "highway")]), (A.SEL_NODE, [(A.TEST_EXISTS, "place")])]
    ent, cls, _ = sm.mirror(r, selmatch.SelectorSet(sels))
    b = selmatch.ClassLabelBindings(0, 18, [[(7, 0), (8, None), (9, 1), (7, 0)] if c["n_sels"] else [] for c in cls], ["name", "ref"])
    node, area = lb.py_table(tags, ent, b, False), lb.py_table(tags, ent, b, True)
    out = subprocess.run([lb.build_host_main(), str(tmp_path / "w.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    count = lambda py: [sum(len(row) for row in rows) for rows in py[0]] + [len(py[1]), sum(len(s) for s in py[2])]
    assert lines[0].split() == ["node"] + [str(x) for x in count(node)] and count(node)[0] > 0 and count(node)[1] > 3
    assert lines[1].split() == ["area"] + [str(x) for x in count(area)] and count(area)[2] > 3
    texts = lines[2:2 + len(area[1])]
    assert texts == [" ".join(f"U+{ord(c):04X}" for c in s) for s in area[2]]
    assert lines[-1].split() == ["utf8", "12", "17"]
    t.close()
    r.close()
