"""Selector matching on the device (osmt_match_selectors, osm_renderer_amd/csrc/osmt_selmatch.hip) and bindings per class
(osmt_register_style_bindings_matched).

Every comparison is element by element against the host mirror osmt::match_selectors_host (host/osmt_selmatch.hpp, through
tests/selmatch_shim.cpp), which tests/test_selector_match_cpu.py holds against a restatement of mapcss/styler.rs: entity
classes, class records, pooled selector ids.  Where a case is about one decision (a key, a test kind, a number), the decision
is also asserted directly.  The worlds are written with tests/_geodata.write_geodata; nothing outside the repository is read."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, selmatch, styled
from osm_renderer_amd.lib import OsmtError
from tests import _selmatch as sm
from tests import _tilequery as tq
from tests._styled_feed import fill_only_styles, geodata_of, recs_of
from tests.test_selector_match_cpu import CORPUS_ERRORS, CORPUS_VALID, LAYERS

pytestmark = pytest.mark.gpu
A = abi
E, NE, T, F, EQ, NEQ, LT, LE, GT, GE = range(10)
NODE, WAY, AREA, OTHER = A.SEL_NODE, A.SEL_WAY, A.SEL_AREA, A.SEL_OTHER


class Run:
    """a world registered with its tags, a selector set registered, the match made (a decline answered with
    osmt::HostNumbers) and compared with the mirror"""

    def __init__(self, ctx, path, w, sels, max_zoom_tile=None, compare=True):
        self.ctx, self.w, self.sels = ctx, w, sels
        self.r = w.write(path, max_zoom_tile)
        self.gid = ctx.register_geodata(geodata_of(self.r))
        self.tags = sm.TagsOf(self.r)
        ctx.register_tags(self.gid, self.tags.desc())
        self.set = selmatch.SelectorSet(sels)
        self.sid = ctx.register_selectors(self.set)
        self.declined, self.declined_msg, self.ov = None, None, None
        try:
            self.m = ctx.match_selectors(self.gid, self.sid)
        except selmatch.Declined as e:
            assert e.code == A.UNSUPPORTED
            self.declined, self.declined_msg = e.declined, str(e)
            self.ov = sm.host_numbers(self.tags.strings(), e.declined)
            self.m = ctx.match_selectors(self.gid, self.sid, self.ov)
        self.ent, self.cls, self.pooled = self.m.read()
        self.want = sm.mirror(self.r, self.set)
        if compare:
            same(self.m.read(), self.want)

    def rematch(self):
        m = self.ctx.match_selectors(self.gid, self.sid, self.ov)
        out = m.read()
        m.close()
        return out

    def of(self, e):
        """the selector ids of entity e"""
        c = self.cls[self.ent[e]]
        return self.pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]].tolist()

    def way(self, i):
        return self.of(len(self.w.nodes) + i)

    def mp(self, i):
        return self.of(len(self.w.nodes) + len(self.w.ways) + i)

    def close(self):
        self.m.close()
        self.tags.close()
        self.r.close()


def same(got, want):
    ent, cls, pooled = got
    went, wcls, wpooled = want
    assert ent.shape == went.shape and np.array_equal(ent, went), np.flatnonzero(ent != went)[:8] if ent.shape == went.shape else (ent.shape, went.shape)
    assert sm.classes_as_tuples(cls, pooled) == sm.classes_as_tuples(wcls, wpooled)
    assert cls.tobytes() == wcls.tobytes() and pooled.tobytes() == wpooled.tobytes()


BASIC = [(WAY, [(E, "highway")]), (AREA, [(EQ, "building", "yes")]), (NODE, [(T, "shop")]), (WAY, []), (NODE, [(NE, "highway")]), (OTHER, [])]
TAGSETS = [{}, {"highway": "primary"}, {"building": "yes"}, {"shop": "yes", "highway": "x"}, {"building": "no", "layer": "1"}, {"layer": "-1"}]


def _fill(w, n_nodes, n_ways, n_mps, tagsets=TAGSETS):
    for i in range(n_nodes):
        w.node(tagsets[i % len(tagsets)])
    anchor = [w.node(), w.node(), w.node()] if n_ways else []
    for i in range(n_ways):  # shared nodes: only the tags matter
        w.way(anchor + [anchor[0]] if i % 2 else anchor[:2], tagsets[(i // 2) % len(tagsets)])
    for i in range(n_mps):
        w.mp(tagsets[i % len(tagsets)], n_polygons=0)
    return w


@pytest.mark.parametrize("counts", [(0, 0, 0), (5, 0, 0), (0, 0, 5), (3, 0, 4), (63, 64, 65), (65, 63, 64), (64, 65, 63)])
def test_entity_counts(gpu_ctx, tmp_path, counts):
    """0 entities of one, two and all kinds (ways need nodes: without nodes there are none); 63, 64, 65 of each kind"""
    n, wy, m = counts
    if n == 0 and wy == 0:
        w = sm.World()
        for i in range(m):
            w.mps.append((9000 + i, [], TAGSETS[i % len(TAGSETS)]))
    else:
        w = _fill(sm.World(), n, wy, m)
    run = Run(gpu_ctx, tmp_path / "w.bin", w, BASIC)
    assert len(run.ent) == len(w.nodes) + len(w.ways) + len(w.mps)
    run.close()


def test_4097_entities_of_each_kind(gpu_ctx, tmp_path):
    w = _fill(sm.World(), 4097, 4097, 4097)
    run = Run(gpu_ctx, tmp_path / "w.bin", w, BASIC)
    assert len(run.cls) > 12
    run.close()


def test_tag_counts_and_key_positions(gpu_ctx, tmp_path):
    """entities with 0, 1, 2, 3, 64, 65 tags; the looked-up key first, last, absent before the first, behind the last and
    between; nam / name / name:en side by side; a key with bytes >= 0x80 next to ASCII ones; a test key nobody has"""
    w = sm.World()
    keys = [f"k{i:02d}" for i in range(65)]
    for n in (0, 1, 2, 3, 64, 65):
        w.node({k: "v" for k in keys[:n]})
    first, last = w.node({"k00": "v", "m": "v", "z": "v"}), w.node({"a": "v", "k00": "v"})
    before, after, between = w.node({"l": "v", "m": "v"}), w.node({"a": "v", "b": "v"}), w.node({"a": "v", "z": "v"})
    names = [w.node(t) for t in ({"nam": "1"}, {"name": "1"}, {"name:en": "1"}, {"nam": "1", "name": "1", "name:en": "1"}, {"nam": "1", "name:en": "1"})]
    high = [w.node(t) for t in ({"z": "1", "é": "1"}, {"é": "1"}, {"z": "1"}, {"zz": "1", "é": "1", "имя": "1"})]
    sels = [(NODE, [(E, k)]) for k in ("k00", "k01", "k02", "k63", "k64")]
    sels += [(NODE, [(E, "nam")]), (NODE, [(E, "name")]), (NODE, [(E, "name:en")]), (NODE, [(E, "z")]), (NODE, [(E, "é")]), (NODE, [(E, "имя")]),
             (NODE, [(E, "nobody")]), (NODE, [(NE, "nobody"), (NE, "k64")])]
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    assert [run.of(i) for i in range(6)] == [[12], [0, 12], [0, 1, 12], [0, 1, 2, 12], [0, 1, 2, 3, 12], [0, 1, 2, 3, 4]]
    assert run.of(first) == [0, 8, 12] and run.of(last) == [0, 12]
    assert run.of(before) == run.of(after) == [12] and run.of(between) == [8, 12]
    assert [run.of(i) for i in names] == [[5, 12], [6, 12], [7, 12], [5, 6, 7, 12], [5, 7, 12]]
    assert [run.of(i) for i in high] == [[8, 9, 12], [9, 12], [8, 12], [9, 10, 12]]
    run.close()


def test_more_than_64_test_keys(gpu_ctx, tmp_path):
    """130 distinct test keys, entities that have 0, 1, 4, 10 and all of them: key ids beyond one 64-bit word"""
    keys = [f"q{i:03d}" for i in range(130)]
    w = sm.World()
    picks = [[0, 63, 64, 129], [63], [64], [], list(range(130)), [1, 62, 65, 128], list(range(60, 70))]
    for p in picks:
        w.node({keys[i]: "v" if i % 2 else "u" for i in p})
    sels = [(NODE, [(E, k)]) for k in keys] + [(NODE, [(EQ, keys[63], "v"), (EQ, keys[64], "u")]), (NODE, [(NE, keys[64]), (E, keys[63])])]
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    for n, p in enumerate(picks):
        assert run.of(n) == p + ([130] if 63 in p and 64 in p else []) + ([131] if 63 in p and 64 not in p else []), n
    run.close()


def test_selector_counts_and_limits(gpu_ctx, tmp_path):
    """0 selectors; a selector without tests for each object type; 1, 31, 32, 33, 64, 65 selectors; the most tests a selector
    may have; one selector and one test past the limits, refused with the figure"""
    def world():
        return _fill(sm.World(), 7, 8, 3)

    run = Run(gpu_ctx, tmp_path / "w0.bin", world(), [])
    assert len(run.pooled) == 0 and not run.cls["n_sels"].any() and len(run.cls) == 6  # (slot, layer) alone: 3 of nodes, 2 of ways, 1
    run.close()
    run = Run(gpu_ctx, tmp_path / "w1.bin", world(), [(NODE, []), (WAY, []), (AREA, []), (OTHER, [])])
    assert run.of(0) == [0] and run.way(0) == [1] and run.way(1) == [1, 2] and run.mp(0) == [1, 2]
    run.close()
    pool = [(WAY, [(E, "highway")]), (NODE, [(EQ, "layer", "1")]), (AREA, [(NEQ, "building", "no")]), (WAY, [(NE, "layer")]), (NODE, [])]
    for k, n in enumerate((1, 31, 32, 33, 64, 65)):
        run = Run(gpu_ctx, tmp_path / f"n{k}.bin", world(), [pool[(3 * i) % len(pool)] for i in range(n)])
        assert max(len(run.of(e)) for e in range(len(run.ent))) >= n // 5
        run.close()
    many = [(E, "building"), (NE, "shop")] * (A.MATCH_MAX_SELECTOR_TESTS // 2)
    run = Run(gpu_ctx, tmp_path / "t.bin", world(), [(WAY, many), (WAY, many[:-1] + [(E, "shop")])])
    assert run.way(4) == [0] and run.way(0) == []  # way 4 has a building and no shop
    run.close()
    with pytest.raises(OsmtError, match=f"has {A.MATCH_MAX_SELECTOR_TESTS + 1} tests") as e:
        gpu_ctx.register_selectors(selmatch.SelectorSet([(WAY, many + [(E, "x")])]))
    assert e.value.code == A.UNSUPPORTED and str(A.MATCH_MAX_SELECTOR_TESTS) in str(e.value)
    gpu_ctx.register_selectors(selmatch.SelectorSet([(NODE, [])] * A.MATCH_MAX_SELECTORS))
    with pytest.raises(OsmtError, match=f"{A.MATCH_MAX_SELECTORS + 1} selectors") as e:
        gpu_ctx.register_selectors(selmatch.SelectorSet([(NODE, [])] * (A.MATCH_MAX_SELECTORS + 1)))
    assert e.value.code == A.UNSUPPORTED and f"= {A.MATCH_MAX_SELECTORS}" in str(e.value)


def test_every_test_kind(gpu_ctx, tmp_path):
    """every kind with the tag present and absent; True / False against yes, true, 1, Yes, "yes " and the empty value; Equal /
    NotEqual against the equal value, a proper prefix, an extension, the empty value, and two selectors whose values differ
    in the last byte"""
    w = sm.World()
    vals = ["yes", "true", "1", "Yes", "yes ", "", None]
    tf = [w.node({} if v is None else {"k": v}) for v in vals]
    eqv = ["primary", "primar", "primary_", "", "primarz", None]
    eq = [w.node({} if v is None else {"h": v}) for v in eqv]
    sels = [(NODE, [(E, "k")]), (NODE, [(NE, "k")]), (NODE, [(T, "k")]), (NODE, [(F, "k")]),  # 0..3
            (NODE, [(EQ, "h", "primary")]), (NODE, [(NEQ, "h", "primary")]), (NODE, [(EQ, "h", "primarz")]), (NODE, [(EQ, "h", "")]),  # 4..7
            (NODE, [(NEQ, "h", "")]), (NODE, [(LT, "k", 2.0)]), (NODE, [(LE, "k", 1.0)]), (NODE, [(GT, "k", 0.5)]), (NODE, [(GE, "k", 1.0)])]  # 8..12
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    k_of = lambda i: [s for s in run.of(i) if s in (0, 1, 2, 3, 9, 10, 11, 12)]
    assert [k_of(i) for i in tf] == [[0, 2], [0, 2], [0, 2, 9, 10, 11, 12], [0, 3], [0, 3], [0, 3], [1, 3]]
    h_of = lambda i: [s for s in run.of(i) if 4 <= s <= 8]
    assert [h_of(i) for i in eq] == [[4, 8], [5, 8], [5, 8], [5, 7], [5, 6, 8], [5, 8]]
    run.close()


def test_object_types(gpu_ctx, tmp_path):
    """a node against every object type; ways of 0 nodes, of 2 nodes with first == last (not closed), of 3 nodes closed by one
    node id, closed by two node ids with equal coordinates, with lon -0.0 against +0.0, and open; a multipolygon"""
    w = sm.World()
    n = w.node({"x": "1"})
    a, b, c = w.node(lat=10.0, lon=20.0), w.node(lat=10.001, lon=20.0), w.node(lat=10.0, lon=20.0)
    z0, z1 = w.node(lat=5.0, lon=0.0), w.node(lat=5.0, lon=-0.0)
    d = w.node(lat=10.0, lon=20.001)
    ways = [w.way(ids) for ids in ([], [a, a], [a, b, a], [a, b, c], [z0, b, z1], [a, b, d], [a, b, d, a], [a, d])]
    m = w.mp({}, n_polygons=1)
    sels = [(NODE, []), (WAY, []), (AREA, []), (OTHER, [])]  # All, Canvas and Meta arrive as OTHER
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    assert run.of(n) == [0]
    assert [run.way(i) for i in ways] == [[1], [1], [1, 2], [1, 2], [1, 2], [1], [1, 2], [1]]
    assert run.mp(m) == [1, 2]
    slots = [int(run.cls[run.ent[len(w.nodes) + i]]["slot"]) for i in ways]
    assert slots == [2, 2, 1, 1, 1, 2, 1, 2] and int(run.cls[run.ent[len(w.nodes) + len(w.ways) + m]]["slot"]) == 3
    run.close()


def _number_world():
    w = sm.World()
    strings = CORPUS_VALID + CORPUS_ERRORS
    for s in strings:
        w.open_way({"n": s, "ref": "1e24"})  # "1e24" sits under a key no numeric test names: never parsed, never declined
    w.open_way({"ref": "7"})
    values = sorted({float(s) for s in CORPUS_VALID if float(s) == float(s)})
    sels = []
    for v in values:
        sels += [(WAY, [(GE, "n", v)]), (WAY, [(LE, "n", v)]), (WAY, [(LT, "n", v)]), (WAY, [(GT, "n", v)])]
    nan_first = len(sels)
    sels += [(WAY, [(k, "n", float("nan"))]) for k in (LT, LE, GT, GE)]
    return w, strings, values, sels, nan_first


def test_numbers_exact_or_declined(gpu_ctx, tmp_path):
    """the corpus as tag values: each converts to the bits of float() — x >= v and x <= v hold together only for x == v — or is
    declined and supplied by osmt::HostNumbers; errors make every comparison false; a NaN on either side is false; < against
    <= at equality; the declined set is the fast-path rule's, a condition stated in csrc/osmt_numparse.h"""
    w, strings, values, sels, nan_first = _number_world()
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    pool = run.tags.strings()
    got_declined = sorted(pool[d["v_off"]:d["v_off"] + d["v_len"]].decode() for d in run.declined)
    want_declined = sorted(s for s in CORPUS_VALID if sm.fast_path(s)[0] == sm.NUM_DECLINED)
    assert got_declined == want_declined and 2 * len(want_declined) <= len(CORPUS_VALID)
    first = run.declined[0]
    assert f"{len(want_declined)} distinct" in run.declined_msg
    assert '"' + pool[first["v_off"]:first["v_off"] + min(first["v_len"], 48)].decode() in run.declined_msg
    assert np.all(np.diff(run.declined["v_off"].astype(np.int64)) >= 0) and len({(int(d["v_off"]), int(d["v_len"])) for d in run.declined}) == len(run.declined)
    for i, s in enumerate(strings):
        ids = run.way(i)
        assert not any(x >= nan_first for x in ids), s
        if s in CORPUS_ERRORS or float(s) != float(s):
            assert ids == [], s
            continue
        v = float(s)
        k = values.index(v)
        want = []
        for j, u in enumerate(values):
            want += [4 * j + q for q, holds in enumerate((v >= u, v <= u, v < u, v > u)) if holds]
        assert ids == want, s
        assert 4 * k in ids and 4 * k + 1 in ids and 4 * k + 2 not in ids and 4 * k + 3 not in ids, s
    assert run.way(len(strings)) == []
    run.close()


def test_declined_flow_and_override_refusals(gpu_ctx, tmp_path):
    w, strings, values, sels, _ = _number_world()
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    L = lib.load()
    h = C.c_void_p()
    rc = L.osmt_match_selectors(gpu_ctx._h, run.gid, run.sid, None, 0, C.byref(h))
    assert rc == A.UNSUPPORTED and h.value
    counts = (C.c_size_t * 3)()
    assert L.osmt_match_read(h, None, None, None, None, counts) == A.INVALID_ARG and b"declined state" in L.osmt_last_error()
    out = C.c_uint32()
    off = np.zeros(2, np.uint32)
    assert L.osmt_register_style_bindings_matched(gpu_ctx._h, h, 0, 18, C.c_void_p(off.ctypes.data), None, 1, C.byref(out)) == A.INVALID_ARG
    assert b"declined state" in L.osmt_last_error()
    n = C.c_size_t()
    assert L.osmt_match_read_declined_numbers(h, None, 0, C.byref(n)) == A.OK and n.value == len(run.declined)
    small = np.zeros(1, selmatch.DECLINED_NUMBER_DTYPE)
    assert L.osmt_match_read_declined_numbers(h, C.c_void_p(small.ctypes.data), 1, C.byref(n)) == A.INVALID_ARG
    L.osmt_match_free(h)
    # a partial list: the rest is declined again
    with pytest.raises(selmatch.Declined) as e:
        gpu_ctx.match_selectors(run.gid, run.sid, run.ov[:2].copy())
    assert e.value.declined.tobytes() == run.declined[2:].tobytes()
    # an override wins over the device's own parse, with and without a value
    pool = run.tags.strings()
    _, _, off5, len5 = run.tags.way_tag(strings.index("5"), 0)  # its tags in key order: n, ref
    assert pool[off5:off5 + len5] == b"5"
    forced = np.concatenate([run.ov, selmatch.overrides([(off5, len5, None)])])
    forced = forced[np.lexsort((forced["v_len"], forced["v_off"]))]
    m = gpu_ctx.match_selectors(run.gid, run.sid, forced)
    ent, cls, pooled = m.read()
    c = cls[ent[len(w.nodes) + strings.index("5")]]
    assert c["n_sels"] == 0  # "5" is an error now; every other way as before
    m.close()

    def refused(ov, word):
        with pytest.raises(OsmtError, match=word) as e:
            gpu_ctx.match_selectors(run.gid, run.sid, ov)
        assert e.value.code == A.INVALID_ARG and not isinstance(e.value, selmatch.Declined)

    refused(run.ov[::-1].copy(), "strictly ascending")
    refused(np.concatenate([run.ov[:1], run.ov[:1], run.ov[1:]]), "strictly ascending")
    bad = run.ov.copy()
    bad["v_off"][-1] = len(pool)
    bad["v_len"][-1] = 1
    refused(bad, "leaves the")
    bad = run.ov.copy()
    bad["has_value"][0] = 2
    refused(bad, "has_value")
    run.close()


def test_layer(gpu_ctx, tmp_path):
    """tags["layer"].parse::<i64>() in full on the device: signs, leading zeros, the i64 edges, errors; no layer tag and
    layer=0 are two classes"""
    w = sm.World()
    for s in LAYERS:
        w.node({"layer": s})
    none = w.node({})
    w.node({"layer": "0", "lay": "x", "layers": "y"})
    run = Run(gpu_ctx, tmp_path / "w.bin", w, [(NODE, [(E, "layer")])])
    for i, s in enumerate(LAYERS):
        c, want = run.cls[run.ent[i]], sm.py_i64(s)
        assert (int(c["has_layer"]), int(c["layer"])) == (int(want is not None), want or 0), s
    assert run.ent[none] != run.ent[LAYERS.index("0")] and run.ent[none + 1] == run.ent[LAYERS.index("0")] == run.ent[LAYERS.index("-0")]
    assert run.ent[LAYERS.index("0" * 21 + "1")] == run.ent[LAYERS.index("1")]
    assert int(run.cls[run.ent[none]]["has_layer"]) == 0
    run.close()


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_one_class(gpu_ctx, tmp_path, n):
    w = sm.World()
    for _ in range(n):
        w.node({"shop": "yes", "layer": "2"})
    run = Run(gpu_ctx, tmp_path / "w.bin", w, BASIC)
    assert len(run.cls) == 1 and not run.ent.any() and run.of(0) == [2, 4] and int(run.cls[0]["first_entity"]) == 0
    run.close()


def test_every_entity_its_own_class(gpu_ctx, tmp_path):
    w = sm.World()
    for i in range(4097):
        w.node({"layer": str(i - 2000)})
    run = Run(gpu_ctx, tmp_path / "w.bin", w, BASIC)
    assert np.array_equal(run.ent, np.arange(4097)) and np.array_equal(run.cls["first_entity"], np.arange(4097))
    run.close()


def test_class_keys_and_hash_bits(gpu_ctx, tmp_path):
    """two entities that differ only in slot, only in layer, only in the last selector id; the same input with the class
    table's hash cut to 0, 1 and 8 bits gives identical bytes (a collision costs probes, never a merge); so do two runs"""
    rng = np.random.default_rng(29)
    w = sm.World()
    shared = [w.node(), w.node(), w.node()]
    closed, opened = w.way(shared + [shared[0]], {"highway": "x"}), w.way(shared, {"highway": "x"})
    l1, l2 = w.way(shared, {"highway": "x", "layer": "1"}), w.way(shared, {"highway": "x", "layer": "2"})
    last_a, last_b = w.way(shared, {"highway": "x", "a": "0"}), w.way(shared, {"highway": "x", "b": "0"})
    keys = ["highway", "building", "shop", "a", "b", "c", "d"]
    for i in range(700):
        t = {k: ("yes", "no", "1")[int(rng.integers(0, 3))] for k in rng.choice(keys, int(rng.integers(0, 4)), replace=False)}
        if i % 5 == 0:
            t["layer"] = str(int(rng.integers(-2, 3)))
        (w.node, lambda t: w.way(shared + [shared[0]], t), lambda t: w.way(shared[:2], t), lambda t: w.mp(t, 0))[i % 4](t)
    sels = [(WAY, [(E, "highway")]), (WAY, [(E, "a")]), (WAY, [(E, "b")])] + [(typ, [(T, k)]) for k in keys for typ in (NODE, WAY, AREA)]
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels)
    cls_of = lambda i: int(run.ent[len(w.nodes) + i])
    assert len({cls_of(i) for i in (closed, opened, l1, l2, last_a, last_b)}) == 6
    assert run.way(last_a) == [0, 1] and run.way(last_b) == [0, 2] and run.way(closed) == run.way(opened) == [0]
    assert len(run.cls) > 60
    base = [a.tobytes() for a in run.m.read()]
    try:
        for bits in (0, 1, 8, 32, 32):
            gpu_ctx.debug_match_hash_bits(bits)
            assert [a.tobytes() for a in run.rematch()] == base, bits
    finally:
        gpu_ctx.debug_match_hash_bits(32)
    with pytest.raises(OsmtError):
        gpu_ctx.debug_match_hash_bits(33)
    run.close()


def test_registration_refusals(gpu_ctx, tmp_path):
    """the rules that compare with the context's tables: one tags table per file, the file's counts, known ids"""
    run = Run(gpu_ctx, tmp_path / "w.bin", _fill(sm.World(), 4, 4, 2), BASIC)
    other = _fill(sm.World(), 5, 4, 2).write(tmp_path / "o.bin")
    gid2 = gpu_ctx.register_geodata(geodata_of(other))

    def refused(word, f, *args):
        with pytest.raises(OsmtError, match=word) as e:
            f(*args)
        assert e.value.code == A.INVALID_ARG

    refused("has tags already", gpu_ctx.register_tags, run.gid, run.tags.desc())
    refused("but geodata id", gpu_ctx.register_tags, gid2, run.tags.desc())
    refused("is not registered", gpu_ctx.register_tags, 10**6, run.tags.desc())
    refused("has no tags", gpu_ctx.match_selectors, gid2, run.sid)
    refused("geodata id", gpu_ctx.match_selectors, 10**6, run.sid)
    refused("selectors id", gpu_ctx.match_selectors, run.gid, 10**6)
    # a later registration does not disturb an earlier set
    gpu_ctx.register_selectors(selmatch.SelectorSet([(NODE, [])]))
    same(run.rematch(), run.want)
    other.close()
    run.close()


def test_bindings_per_class(gpu_ctx, tmp_path):
    """a few hundred ways and multipolygons, a dozen selectors with zoom ranges, three zooms: the per-class styles expanded on
    the device and the per-entity table expanded here build the same tile batch, byte for byte; a class with 0 styles, a class
    with 3, no class with styles; the refusals"""
    rng = np.random.default_rng(37)
    w = sm.World()
    pool = [{"highway": "primary"}, {"highway": "path", "bridge": "yes"}, {"building": "yes"}, {"building": "yes", "layer": "1"}, {"landuse": "grass"}, {},
            {"natural": "water", "layer": "-1"}, {"highway": "primary", "lanes": "4"}]
    for i in range(260):
        (w.closed_way if i % 3 else w.open_way)(pool[int(rng.integers(0, len(pool)))])
    for _ in range(60):
        w.mp(pool[int(rng.integers(0, len(pool)))])
    sels = [(WAY, [(E, "highway")], None, 16), (WAY, [(EQ, "highway", "primary")], 17, None), (AREA, [(EQ, "building", "yes")], 16, None),
            (AREA, [(E, "landuse")]), (WAY, [(T, "bridge")], 17, 17), (AREA, [(EQ, "natural", "water")], None, 17), (WAY, [(GE, "lanes", 3.0)]),
            (NODE, []), (WAY, [(NE, "highway"), (NE, "building")], 18, 18), (AREA, []), (WAY, [(EQ, "highway", "path")], 10, 12), (WAY, [], 18, None)]
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels, max_zoom_tile=tq.max_zoom_tile)
    gpu_ctx.register_tile_index(run.gid, tq.index_of(run.w.refs))
    st, dashes = fill_only_styles(rng, 24)
    first = gpu_ctx.register_styles(recs_of(st), dashes)
    n_nodes, n_ways = len(w.nodes), len(w.ways)
    cx, cy = tq.max_zoom_tile(sm.LAT0, sm.LON0)
    sizes = set()
    for zoom in (16, 17, 18):
        # the "cascade" of the test: the selectors that survive the zoom filter, falling, at most 3, as style ids
        per_class = []
        for c in run.cls:
            ids = run.set.at_zoom(run.pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]], zoom).tolist()
            per_class.append([first + (5 * s + int(c["slot"])) % 24 for s in sorted(ids, reverse=True)[:3]])
        sizes |= {len(v) for v in per_class}
        by_class = run.m.register_style_bindings(zoom, zoom, per_class)
        ws = [per_class[c] for c in run.ent[n_nodes:n_nodes + n_ways]]
        ms = [per_class[c] for c in run.ent[n_nodes + n_ways:]]
        by_entity = gpu_ctx.register_style_bindings(styled.StyleBindings(run.gid, zoom, zoom, ws, ms))
        sh = 18 - zoom
        tiles = [(zoom, cx >> sh, cy >> sh), (zoom, (cx >> sh) + 1, cy >> sh), (zoom, cx >> sh, (cy >> sh) - 1)]
        scenes = [gpu_ctx.build_tiles(styled.TileBatch(run.gid, tiles, {zoom: b})) for b in (by_class, by_entity)]
        (t0, a0), (t1, a1) = [s.read_styled_areas() for s in scenes]
        assert len(a0) > 100 and t0.tobytes() == t1.tobytes() and a0.tobytes() == a1.tobytes(), zoom
        d0, d1 = [s.read_display_list() for s in scenes]
        for name in ("jobs", "ops", "rings", "coords", "dashes"):
            assert getattr(d0, name).tobytes() == getattr(d1, name).tobytes(), (zoom, name)
        for s in scenes:
            s.free()
    assert {0, 3} <= sizes
    # no class with styles: a table that binds nothing
    empty = run.m.register_style_bindings(0, 18, [[] for _ in run.cls])
    scene = gpu_ctx.build_tiles(styled.TileBatch(run.gid, [(18, cx, cy)], {18: empty}))
    assert len(scene.read_styled_areas()[1]) == 0
    scene.free()
    # the refusals
    L = lib.load()
    n_cls = len(run.cls)

    def refused(word, ctx_h=None, n=n_cls, off=None, styles=None, zoom=(0, 18)):
        off = np.arange(n + 1, dtype=np.uint32) if off is None else np.asarray(off, np.uint32)
        styles = np.full(max(int(off[-1]), 1), first, np.uint32) if styles is None else np.asarray(styles, np.uint32)
        out = C.c_uint32()
        rc = L.osmt_register_style_bindings_matched(ctx_h or gpu_ctx._h, run.m._h, zoom[0], zoom[1], C.c_void_p(off.ctypes.data), C.c_void_p(styles.ctypes.data),
                                                    n, C.byref(out))
        assert rc == A.INVALID_ARG and word in L.osmt_last_error().decode(), L.osmt_last_error()

    from osm_renderer_amd.renderer import Context

    stranger = Context(0)
    refused("another context", ctx_h=stranger._h)
    stranger.close()
    refused("classes, the match has", n=n_cls - 1)
    off = np.arange(n_cls + 1)
    off[0] = 1
    refused("class_style_off[0] is 1", off=off)
    off = np.arange(n_cls + 1)
    off[2] = 0
    refused("less than the entry before", off=off)
    refused("is not a registered style", styles=np.full(n_cls, 10**6))
    refused("zoom range", zoom=(5, 19))
    refused("zoom range", zoom=(7, 6))
    run.close()


def test_cpp_binding_runs_the_declined_and_retry_loop(tmp_path):
    """tests/selmatch_host_demo.cpp over the C ABI: a decline answered with osmt::HostNumbers, the result equal to the mirror"""
    w = sm.World()
    tagsets = [{"highway": "x", "width": "3"}, {"highway": "y", "width": "1e23"}, {"building": "yes", "width": "2.5000000000000000000001"}, {"width": "wide"}, {}]
    for i in range(40):
        w.node({"ele": ("12", "1e400", "99.999999999999999999999", "x")[i % 4]})
    for i in range(60):
        (w.closed_way if i % 2 else w.open_way)(tagsets[i % len(tagsets)])
    w.mp({"building": "yes"})
    w.write(tmp_path / "w.bin").close()
    out = subprocess.run([sm.build_demo(), str(tmp_path / "w.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    word, n_classes, n_declined = out.stdout.split()
    assert word == "OK" and int(n_classes) >= 6 and int(n_declined) == 4
