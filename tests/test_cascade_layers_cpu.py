"""OSMT_RULES_CLASS_LAYERS without a device: osmt_validate_rules_ex (flags 0 is osmt_validate_rules; with the flag the bound on
the names is 255), and the host mirror osmt::cascade_host against the Python restatement on the wide sheets of
tests/_cascade_layers.py — the oracle tests/test_gpu_cascade_layers.py leans on.  The change adds no host code beyond the flag
check (the per-class numbering is a kernel), so there is no new program under a sanitizer.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch
from osm_renderer_amd.lib import OsmtError
from tests import _cascade as cs
from tests import _cascade_layers as cl
from tests._cascade import SHEET, sel

A = abi
REFERENCE_SHEET = "/root/reference/tests/mapcss/mapnik.parsed.canonical"


def validate(rules, flags):
    d = rules.as_desc()
    L = lib.load()
    rc = L.osmt_validate_rules_ex(C.byref(d), flags, None)
    return rc, L.osmt_last_error().decode()


def test_flags_zero_is_the_existing_validator():
    L = lib.load()
    nine = cs.rule_set(SHEET + [([sel("l9")], [])])
    d = nine.as_desc()
    assert L.osmt_validate_rules(C.byref(d), None) == A.UNSUPPORTED
    old = L.osmt_last_error().decode()
    rc, msg = validate(nine, 0)
    assert rc == A.UNSUPPORTED and msg == old and "9 distinct layer names (> OSMT_CASCADE_MAX_LAYERS = 8)" in msg
    assert validate(cs.rule_set(SHEET), 0)[0] == A.OK and validate(cs.rule_set(SHEET), A.RULES_CLASS_LAYERS)[0] == A.OK
    assert L.osmt_validate_rules_ex(None, 0, None) == A.INVALID_ARG


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFE])
def test_an_unknown_flag_bit_is_refused_with_its_value(flags):
    rc, msg = validate(cs.rule_set(SHEET), flags)
    assert rc == A.INVALID_ARG and f"flags = 0x{flags:x}" in msg


def named(n):
    return cs.rule_set([([sel(f"n{k}")], []) for k in range(n - 2)] + [([sel("*"), sel()], [])])


def test_names_up_to_255_pass_with_the_flag():
    assert A.CASCADE_MAX_LAYER_NAMES == 255 and A.CASCADE_MAX_CLASS_LAYERS == 16 and A.RULES_CLASS_LAYERS == 1
    for n in (9, 26, 255):
        assert validate(named(n), A.RULES_CLASS_LAYERS)[0] == A.OK, n
        rc, msg = validate(named(n), 0)
        assert rc == A.UNSUPPORTED and f"{n} distinct layer names (> OSMT_CASCADE_MAX_LAYERS = 8)" in msg
    rc, msg = validate(named(256), A.RULES_CLASS_LAYERS)
    assert rc == A.UNSUPPORTED and "256 distinct layer names (> OSMT_CASCADE_MAX_LAYER_NAMES = 255)" in msg
    # a name no selector uses counts, as without the flag
    r = named(255)
    d = r.as_desc()
    pool = bytes(r.layer_bytes) + b"unused"
    off = np.concatenate([r.layer_off, [len(pool)]]).astype(np.uint32)
    buf = np.frombuffer(pool, np.uint8).copy()
    d.layer_off, d.layer_bytes = off.ctypes.data_as(C.POINTER(C.c_uint32)), buf.ctypes.data_as(C.POINTER(C.c_uint8))
    d.n_layers, d.n_layer_bytes = len(off) - 1, len(buf)
    assert lib.load().osmt_validate_rules_ex(C.byref(d), A.RULES_CLASS_LAYERS, None) == A.UNSUPPORTED
    assert b"256 distinct layer names" in lib.load().osmt_last_error()
    # the Python helper raises the same refusals
    selmatch.validate_rules(named(255), class_layers=True)
    with pytest.raises(OsmtError, match="255 distinct layer names"):
        selmatch.validate_rules(named(255))
    with pytest.raises(OsmtError, match="256 distinct layer names") as e:
        selmatch.validate_rules(named(256), class_layers=True)
    assert e.value.code == A.UNSUPPORTED


def test_the_text_key_refusal_is_unchanged():
    many = lambda n: cs.rule_set([([sel()], [("text", ("id" if i & 1 else "str", f"k{i}")) for i in range(n)] + [("text", ("str", "k1"))])])
    for flags in (0, A.RULES_CLASS_LAYERS):
        assert validate(many(256), flags)[0] == A.OK
        rc, msg = validate(many(257), flags)
        assert rc == A.UNSUPPORTED and "257 distinct text strings (> OSMT_LABEL_TEXT_KEYS_MAX = 256)" in msg


def against_py(sheet, classes, labels_all):
    sels, rules = cs.selector_set(sheet), cs.rule_set(sheet)
    cls, pooled = cs.classes_array(classes)
    py = cs.py_cascade(sheet, classes)
    cs.same_as_py(cs.mirror(rules, sels, cls, pooled, labels_all), py, labels_all)
    return py


def test_the_wide_sheets_pass_the_flagged_validator():
    for sheet, _ in [cl.names_case(n) for n in (9, 26, 255)] + [cl.layers_case(), cl.long_case()]:
        assert validate(cs.rule_set(sheet), A.RULES_CLASS_LAYERS)[0] == A.OK
        assert validate(cs.rule_set(sheet), 0)[0] == A.UNSUPPORTED


@pytest.mark.parametrize("n", [9, 26, 255])
def test_mirror_equals_the_restatement_on_wide_sheets(n):
    sheet, classes = cl.names_case(n)
    assert len({s[4] or "default" for ss, _ in sheet for s in ss}) == n
    assert max(cl.layer_count(sheet, sels) for _, _, sels in classes) == min(n, 16)
    py = against_py(sheet, classes, True)
    # the longest list is the class of the 16 highest numbers; "*", where it is among them (not in the sheet of 26), makes no style
    assert max(len(x) for per_zoom in py for x in per_zoom) == {9: 8, 26: 16, 255: 15}[n]
    against_py(sheet, classes, False)


def test_mirror_equals_the_restatement_on_the_layers_of_a_class():
    sheet, classes = cl.layers_case()
    assert [cl.layer_count(sheet, sels) for _, _, sels in classes[:16]] == list(range(1, 17))
    for labels_all in (True, False):
        py = against_py(sheet, classes, labels_all)
    assert [len(py[k][0]) for k in range(16)] == list(range(1, 17))
    by_sels = {tuple(sels): py[i] for i, (_, _, sels) in enumerate(classes)}
    assert by_sels[(27,)] == [[] for _ in range(cs.ZOOMS)] and by_sels[(1,)] == [[] for _ in range(cs.ZOOMS)]  # "*" alone
    # "*" at zooms 8 .. 12 only: its writes show there and nowhere else
    z = by_sels[(0, 2, 27)]
    assert len(z[7]) == len(z[8]) == 2 and z[7] != z[8] and z[8] == z[12] and z[13] == z[7] and z[8][1]["opacity"] == 1.0
    # a layer created after "*" starts as its copy
    assert by_sels[(14, 20)][0][0]["color"] == (14, 2, 3) and by_sels[(14, 20)][0][0]["opacity"] == 0.75
    # the same two layers met in opposite order
    assert [len(by_sels[k][18]) for k in ((2, 4), (29, 30), (4, 30), (1, 2, 4, 29, 30))] == [2, 2, 2, 2]
    sheet, classes = cl.long_case()
    assert [cl.layer_count(sheet, sels) for _, _, sels in classes] == [16, 16, 16]
    against_py(sheet, classes, True)


@pytest.mark.skipif(not os.path.exists(REFERENCE_SHEET), reason="the reference's stylesheet dump is not on this machine")
def test_reference_stylesheet_is_accepted_with_the_flag():
    sheet = cs.read_canonical(REFERENCE_SHEET)
    rules = cs.rule_set(sheet)
    names = {s[4] or "default" for sels, _ in sheet for s in sels}
    assert names == {nm or "default" for nm in cl.REF_NAMES}  # the list the GPU tests type in is the sheet's
    rc, msg = validate(rules, A.RULES_CLASS_LAYERS)
    assert rc == A.OK, msg
    rc, msg = validate(rules, 0)
    assert rc == A.UNSUPPORTED and "26 distinct layer names" in msg
