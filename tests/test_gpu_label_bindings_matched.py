"""Label bindings per class on the device (osmt_register_label_bindings_matched, osmt_register_area_label_bindings_matched,
osm_renderer_amd/csrc/osmt_labelbind.hip) and the read calls of label binding tables.

Every table is read back with osmt_read_label_bindings / osmt_read_area_label_bindings and compared byte for byte, array by
array, with the host mirror osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host (host/osmt_selmatch.hpp,
through tests/labelbind_shim.cpp), which tests/test_label_bindings_matched_cpu.py holds against a Python restatement.  Where a
case is about one decision (a key, a value, a text id), the decision is also asserted directly.  The worlds are written with
tests/_geodata.write_geodata; what the writer cannot produce (ill-formed UTF-8, overlapping value ranges) is edited into the tags
as numpy arrays before they are registered.  Nothing outside the repository is read."""
import ctypes as C

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, selmatch, styled
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _labelbind as lb
from tests import _selmatch as sm
from tests import _tilelabels as tl
from tests import _tilequery as tq
from tests._styled_feed import geodata_of

pytestmark = pytest.mark.gpu
A = abi
NODE, WAY, AREA = A.SEL_NODE, A.SEL_WAY, A.SEL_AREA
E, EQ = A.TEST_EXISTS, A.TEST_EQUAL
NONE = A.TEXT_NONE
CX, CY = tq.center_z18()


@pytest.fixture(scope="module")
def first_style(gpu_ctx):
    """eight label styles without icon and text: the tables here are read back, not drawn"""
    return gpu_ctx.register_label_styles(tl.label_styles([{} for _ in range(8)]))


class Run:
    """a world registered with its tags (edited by `edit` first), a tile index and Mercator factors, a selector set, the match"""

    def __init__(self, ctx, path, w, sels=(), edit=None, max_zoom_tile=None):
        self.ctx, self.w = ctx, w
        self.r = w.write(path, max_zoom_tile)
        self.gid = ctx.register_geodata(geodata_of(self.r))
        t = sm.TagsOf(self.r)
        self.tags = lb.tags_of(t)
        t.close()
        if edit:
            edit(self.tags)
        ctx.register_tags(self.gid, self.tags)
        ctx.register_tile_index(self.gid, tq.index_of(w.refs) if max_zoom_tile else styled.TileIndex([((CX, CY), [], [])]))
        ctx.register_node_mercator(self.gid, an.mercator_factors(self.r.node_table()))
        self.m = ctx.match_selectors(self.gid, ctx.register_selectors(selmatch.SelectorSet(list(sels))))
        self.ent, self.cls, self.pooled = self.m.read()
        self.n = (self.r.n_nodes, self.r.n_ways, self.r.n_multipolygons)
        self.pool = self.tags.strings.tobytes()

    def class_of(self, kind, i):
        """kind: 0 node, 1 way, 2 multipolygon"""
        return int(self.ent[(0, self.n[0], self.n[0] + self.n[1])[kind] + i])

    def read(self, bid, area):
        if area:
            return lb.Table(*self.ctx.read_area_label_bindings(bid, self.n[1], self.n[2]))
        off, bind, text_off, chars = self.ctx.read_label_bindings(bid, self.n[0])
        return lb.Table(off, bind, np.zeros(0, np.uint32), np.zeros(0, styled.LABEL_BINDING_DTYPE), text_off, chars)

    def table(self, b, area):
        """the matched table registered, read back and held against the mirror; returns the table read back"""
        bid = (self.m.register_area_label_bindings if area else self.m.register_label_bindings)(b.zoom_lo, b.zoom_hi, b)
        got, want = self.read(bid, area), lb.mirror(self.tags, self.ent, b, area)
        same(got, want)
        return got

    def both(self, b):
        return self.table(b, False), self.table(b, True)

    def close(self):
        self.m.close()
        self.r.close()


def same(got, want):
    for name, g, w in zip(("off 0", "bindings 0", "off 1", "bindings 1", "text_off", "chars"), got.arrays(), want.arrays()):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero(g.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))[:8])


def per_class(run, rows_of):
    """selmatch.ClassLabelBindings with rows_of(class index, class record) per class"""
    return [rows_of(c, rec) for c, rec in enumerate(run.cls)]


NAMES = ["Main Street", "Side Street", "", "Каменный мост", "Main Street", "京都", "Rue de l'Église"]
SELS = [(NODE, [(E, "name")]), (WAY, [(E, "name")]), (NODE, [(EQ, "kind", "a")]), (WAY, [(EQ, "kind", "a")])]


def _fill(w, n_nodes, n_ways, n_mps):
    """names on two entities of three, three layers and two kinds: a dozen classes, values shared by many entities"""
    def tags(i):
        t = {"name": NAMES[i % len(NAMES)]} if i % 3 else {}
        if i % 4 == 1:
            t["kind"] = "a"
        if i % 5 == 2:
            t["layer"] = str(i % 3 - 1)
        if i % 7 == 3:
            t["ref"] = f"R{i % 11}"
        return t

    for i in range(n_nodes):
        w.node(tags(i))
    for i in range(n_ways):  # the ways share the first nodes: only their tags matter here
        w.way([0, min(1, n_nodes - 1), 0][: 3 if i % 2 else 2], tags(i + 1))
    for i in range(n_mps):
        w.mps.append((9000 + i, [], tags(i + 2)))
    return w


def _rows(first_style, keys=(0, 1)):
    """classes with 0, 1, 2 and 3 bindings, by class index; the third binding has no text"""
    return lambda c, rec: [(first_style + c % 5, keys[0]), (first_style + 1, keys[1]), (first_style + 2, None)][: c % 4]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_entity_counts(gpu_ctx, tmp_path, first_style, n):
    """n nodes, n ways and n multipolygons; classes with 0, 1, 2, 3 bindings"""
    run = Run(gpu_ctx, tmp_path / "w.bin", _fill(sm.World(), n, n if n else 0, n), SELS)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, _rows(first_style)), ["name", "ref"])
    node, area = run.both(b)
    assert len(node.off[0]) == n + 1 and len(area.off[0]) == n + 1 and len(area.off[1]) == n + 1
    if n >= 63:
        sizes = {len(v) for v in per_class(run, _rows(first_style))}
        assert sizes == {0, 1, 2, 3} and len(node.text_off) - 1 >= 5 and len(area.text_off) - 1 >= 5
    run.close()


@pytest.mark.parametrize("kind", [0, 2])
def test_a_file_with_one_kind_only(gpu_ctx, tmp_path, first_style, kind):
    w = sm.World()
    for i in range(70):
        if kind == 0:
            w.node({"name": NAMES[i % len(NAMES)]})
        else:
            w.mps.append((9000 + i, [], {"name": NAMES[i % len(NAMES)]}))
    run = Run(gpu_ctx, tmp_path / "w.bin", w, SELS)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    node, area = run.both(b)
    full, empty = (node, area) if kind == 0 else (area, node)
    assert len(full.text_off) - 1 == len(set(NAMES)) and len(empty.text_off) == 1 and len(empty.chars) == 0
    assert sum(len(x) for x in empty.bind) == 0 and sum(len(x) for x in full.bind) == 70
    run.close()


def test_keys(gpu_ctx, tmp_path, first_style):
    """the looked-up key absent; the first, the last and the only tag; sorting in front of all tags, behind all, between; nam /
    name / name:en; the empty key; a UTF-8 key beside ASCII ones; a key that is a selector test key and one that is not;
    entities with 0, 1, 2, 3, 64, 65 tags; duplicate keys in the descriptor; a class whose two bindings name one key; two keys
    whose tags share one interned value"""
    w = sm.World()
    many = [f"k{i:02d}" for i in range(65)]
    counts = [w.node({k: f"v{k}" for k in many[:n]}) for n in (0, 1, 2, 3, 64, 65)]
    first, last, only = w.node({"name": "F", "z": "1"}), w.node({"a": "1", "name": "L"}), w.node({"name": "O"})
    front, behind, between = w.node({"o": "1", "p": "2"}), w.node({"a": "1", "b": "2"}), w.node({"a": "1", "z": "2"})
    names = [w.node(t) for t in ({"nam": "x1"}, {"name": "x2"}, {"name:en": "x3"}, {"nam": "y1", "name": "y2", "name:en": "y3"}, {"nam": "z1", "name:en": "z3"})]
    empty_key = [w.node({"": "nameless", "name": "N"}), w.node({"name": "M"})]
    utf = [w.node({"z": "1", "имя": "Ока"}), w.node({"имя": "Кама", "name": "Kama"}), w.node({"é": "1", "name": "E"})]
    shared = w.node({"name": "Same", "ref": "Same"})
    keys = ["name", "nam", "name:en", "", "имя", "k00", "k63", "k64", "name", "ref", "absent everywhere"]
    rows = [(first_style, k) for k in range(len(keys))] + [(first_style + 1, 0)]  # the last names key 0 once more
    # "name" is a test key of the selectors, the others are not; every node falls into one of two classes with the same list
    run = Run(gpu_ctx, tmp_path / "w.bin", w, [(NODE, [(E, "name")])])
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: rows), keys)
    got = run.table(b, False)
    text = lambda node, k: got.texts_of(0, node)[k][1]
    for node, n in zip(counts, (0, 1, 2, 3, 64, 65)):
        assert [text(node, k) for k in (5, 6, 7)] == ["vk00" if n > 0 else None, "vk63" if n > 63 else None, "vk64" if n > 64 else None]
    assert (text(first, 0), text(last, 0), text(only, 0)) == ("F", "L", "O")
    assert text(front, 0) is None and text(behind, 0) is None and text(between, 0) is None
    assert [[text(n, k) for k in (1, 0, 2)] for n in names] == [["x1", None, None], [None, "x2", None], [None, None, "x3"], ["y1", "y2", "y3"], ["z1", None, "z3"]]
    assert text(empty_key[0], 3) == "nameless" and text(empty_key[1], 3) is None
    assert [text(n, 4) for n in utf] == ["Ока", "Кама", None] and text(utf[2], 0) == "E" and text(utf[1], 0) == "Kama"
    for node in (first, only, shared):  # keys 0 and 8 are the same bytes, and the last binding names key 0 again: one text
        ids = got.bind[0][got.off[0][node]:got.off[0][node + 1]]["text"]
        assert ids[0] == ids[8] == ids[11] != NONE
    ids = got.bind[0][got.off[0][shared]:got.off[0][shared + 1]]["text"]
    assert ids[0] == ids[9] and text(shared, 9) == "Same"  # the writer interns: two tags, one value range, one text
    assert all(text(n, 10) is None for n in range(run.n[0]))
    texts = [got.text(i) for i in range(len(got.text_off) - 1)]
    assert len(set(texts)) == len(texts)
    run.close()


EDGES = [0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF]


def test_values(gpu_ctx, tmp_path, first_style):
    """the empty value is a text of 0 chars, not NONE; the scalars at the edges of every sequence length alone and mixed; values of
    1 .. 1000 bytes; a value that ends where the string pool ends"""
    w = sm.World()
    empty = w.node({"name": ""})
    alone = [w.node({"name": chr(c)}) for c in EDGES]
    mixed = w.node({"name": "".join(chr(c) for c in EDGES + EDGES[::-1])})
    lengths = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000]
    unit = "aé€😀"  # 1 + 2 + 3 + 4 bytes
    by_len = []
    for n in lengths:
        s = (unit * (n // 10 + 1)).encode()[:n].decode("utf-8", "ignore")
        s += "x" * (n - len(s.encode()))
        assert len(s.encode()) == n
        by_len.append((w.node({"name": s}), s))
    w.mps.append((9000, [], {"name": "the very last bytes €"}))
    run = Run(gpu_ctx, tmp_path / "w.bin", w)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    node, area = run.both(b)
    i = int(node.bind[0][node.off[0][empty]]["text"])
    assert i != NONE and node.text_off[i] == node.text_off[i + 1]
    for n, c in zip(alone, EDGES):
        i = int(node.bind[0][node.off[0][n]]["text"])
        assert node.chars[node.text_off[i]:node.text_off[i + 1]].tolist() == [c]
    i = int(node.bind[0][node.off[0][mixed]]["text"])
    assert node.chars[node.text_off[i]:node.text_off[i + 1]].tolist() == EDGES + EDGES[::-1]
    for n, s in by_len:
        assert node.texts_of(0, n) == [(first_style, s)]
    q = run.tags.multipolygon_tags[0]
    assert int(q[2]) + int(q[3]) == len(run.pool)  # the value ends where the pool ends
    assert area.texts_of(1, 0) == [(first_style, "the very last bytes €")]
    run.close()


ILL_FORMED = [b"\x80", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf",
              b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff"]
CUT_OFF = ["é", "€", "😀"]  # 2, 3, 4 bytes: the value range ends one byte early, the next byte of the pool would complete it


def _ill_formed_world():
    """node i carries case i under "name" and the same bytes under "note"; placeholders of the right length, unique per tag"""
    w = sm.World()
    cases = []
    for i, bad in enumerate(ILL_FORMED):
        marks = [bytes([0x41 + i]) * len(bad) + b"!", bytes([0x61 + i]) * len(bad) + b"?"]
        w.node({"name": marks[0].decode(), "note": marks[1].decode()})
        cases.append((marks, b"<" + bad))  # a good byte, then the ill-formed ones: the placeholder is one byte longer
    for i, s in enumerate(CUT_OFF):
        w.node({"name": f"{i}{s}", "note": f"{i}{i}{s}"})
    return w, cases


def _edit_ill_formed(cases, which_tag):
    """which_tag(i) -> the tags of node i to spoil: 0 name, 1 note"""
    def edit(tags):
        pool = tags.strings.tobytes()
        for i, (marks, bad) in enumerate(cases):
            for k in which_tag(i):
                at = pool.index(marks[k])
                tags.strings[at:at + len(bad)] = np.frombuffer(bad, np.uint8)
        for j in range(len(CUT_OFF)):
            node = len(cases) + j
            for k in which_tag(node):
                tags.node_tags[tags.node_tag_off[node] + k][3] -= 1
    return edit


def _refused(run, b, area=False):
    call = run.m.register_area_label_bindings if area else run.m.register_label_bindings
    with pytest.raises(OsmtError, match="not well-formed UTF-8") as e:
        call(0, 18, b)
    assert e.value.code == A.INVALID_ARG and "nothing is registered" in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("case", range(len(ILL_FORMED) + len(CUT_OFF)))
def test_ill_formed_value_is_refused_naming_the_tag(gpu_ctx, tmp_path, first_style, case):
    """one used value is ill-formed: OSMT_INVALID_ARG naming kind, entity and v_off; the mirror refuses the same tag; the same
    bytes under a tag no binding reads are accepted; after the refusal the context registers a good table"""
    w, cases = _ill_formed_world()
    run = Run(gpu_ctx, tmp_path / "w.bin", w, edit=_edit_ill_formed(cases, lambda i: (0, 1) if i == case else ()))
    name = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    q = run.tags.node_tags[run.tags.node_tag_off[case]]  # "name" sorts in front of "note"
    msg = _refused(run, name)
    assert f"tag 0 of node {case} (v_off {int(q[2])}, v_len {int(q[3])})" in msg, msg
    with pytest.raises(lb.Refused) as e:
        lb.mirror(run.tags, run.ent, name, False)
    assert (e.value.kind, e.value.entity, e.value.tag, e.value.v_off) == ("node", case, 0, int(q[2]))
    if case >= len(ILL_FORMED):  # cut off by v_len: the byte behind the range would have completed the sequence
        s = CUT_OFF[case - len(ILL_FORMED)].encode()
        assert run.pool[int(q[2]) + 1:int(q[2]) + 1 + len(s)] == s and int(q[3]) == len(s)
    run.close()
    # the same bytes where no binding looks
    run = Run(gpu_ctx, tmp_path / "v.bin", w, edit=_edit_ill_formed(cases, lambda i: (1,) if i == case else ()))
    got = run.table(name, False)
    assert len(got.text_off) - 1 == run.n[0]
    note = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["note"])
    assert f"tag 1 of node {case} " in _refused(run, note)
    run.table(name, False)  # and a good table after the refusal
    run.close()


def test_two_ill_formed_values_name_the_lower_tag(gpu_ctx, tmp_path, first_style):
    w, cases = _ill_formed_world()
    run = Run(gpu_ctx, tmp_path / "w.bin", w, edit=_edit_ill_formed(cases, lambda i: (0,) if i in (3, 9, 13) else ()))
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    assert "of node 3 " in _refused(run, b)
    run.close()
    # in the area table the way tags are numbered in front of the multipolygon tags
    w = sm.World()
    w.node(), w.node()
    w.way([0, 1], {"name": "fine"}), w.way([0, 1], {"name": "WWWW"})
    w.mps.append((9000, [], {"name": "MMMM"}))

    def edit(tags):
        pool = tags.strings.tobytes()
        for word in (b"WWWW", b"MMMM"):
            at = pool.index(word)
            tags.strings[at:at + 4] = np.frombuffer(b"\xf4\x90\x80\x80", np.uint8)

    run = Run(gpu_ctx, tmp_path / "a.bin", w, edit=edit)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    assert "tag 0 of way 1 " in _refused(run, b, area=True)
    only_mp = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)] if rec["slot"] == 3 else []), ["name"])
    assert "tag 0 of multipolygon 0 " in _refused(run, only_mp, area=True)
    run.table(b, False)  # the node table reads none of them
    run.close()


@pytest.mark.parametrize("distinct", [False, True])
def test_4097_entities_one_value_or_4097_values(gpu_ctx, tmp_path, first_style, distinct):
    w = sm.World()
    for i in range(4097):
        w.node({"name": f"N{i}" if distinct else "Everywhere"})
    run = Run(gpu_ctx, tmp_path / "w.bin", w)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0)]), ["name"])
    got = run.table(b, False)
    assert len(got.text_off) - 1 == (4097 if distinct else 1)
    assert got.bind[0]["text"].tolist() == (list(range(4097)) if distinct else [0] * 4097)
    run.close()


def test_overlapping_ranges_and_numbering_by_the_lowest_used_tag(gpu_ctx, tmp_path, first_style):
    """hand-built value ranges (5, 3), (5, 4), (5, 4): two texts; a value whose lowest-numbered tag belongs to an entity whose
    class has no bindings is numbered by its lowest USED tag; a way and a multipolygon that share a value get one text of the
    area pool, numbered by the way"""
    w = sm.World()
    w.node({"layer": "7", "name": "shared"})  # a class of its own, without bindings
    w.node({"name": "zzz"})
    w.node({"name": "shared"})
    ov = [w.node({"name": f"ov{i}"}) for i in range(3)]
    w.way([0, 1], {"name": "mp first?"}), w.way([0, 1], {"name": "both"})
    w.mps.append((9000, [], {"name": "both"}))
    w.mps.append((9001, [], {"name": "mp first?"}))

    def edit(tags):
        for node, (off, ln) in zip(ov, ((5, 3), (5, 4), (5, 4))):
            q = tags.node_tags[tags.node_tag_off[node]]
            q[2], q[3] = off, ln

    run = Run(gpu_ctx, tmp_path / "w.bin", w, edit=edit)
    assert run.class_of(0, 0) != run.class_of(0, 1) == run.class_of(0, 2)
    quiet = run.class_of(0, 0)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [] if c == quiet else [(first_style, 0)]), ["name"])
    node, area = run.both(b)
    ids = node.bind[0]["text"].tolist()
    assert ids == [0, 1, 2, 3, 3] and node.text(0) == "zzz" and node.text(1) == "shared"  # node 0 has no binding
    assert node.text(2) == run.pool[5:8].decode() and node.text(3) == run.pool[5:9].decode()
    assert area.bind[0]["text"].tolist() == [0, 1] and area.bind[1]["text"].tolist() == [1, 0]
    assert [area.text(i) for i in range(2)] == ["mp first?", "both"]
    run.close()


def test_hash_bits_and_two_runs(gpu_ctx, tmp_path, first_style):
    """the text table's hash cut to 0, 1 and 8 bits (0: every value in one probe chain), and two runs in a row: identical bytes"""
    rng = np.random.default_rng(41)
    w = sm.World()
    w.node(), w.node()
    for i in range(900):
        t = {"name": f"v{int(rng.integers(0, 300))}", "ref": f"v{int(rng.integers(0, 300))}"}
        (w.node, lambda t: w.way([0, 1], t), lambda t: w.mps.append((9000 + i, [], t)))[i % 3](t)
    run = Run(gpu_ctx, tmp_path / "w.bin", w, SELS)
    b = selmatch.ClassLabelBindings(0, 18, per_class(run, lambda c, rec: [(first_style, 0), (first_style + 1, 1)]), ["name", "ref"])
    base = [[a.tobytes() for a in t.arrays()] for t in run.both(b)]
    assert len(base[0][5]) > 4 * 300
    try:
        for bits in (0, 1, 8, 32, 32):
            gpu_ctx.debug_match_hash_bits(bits)
            assert [[a.tobytes() for a in t.arrays()] for t in run.both(b)] == base, bits
    finally:
        gpu_ctx.debug_match_hash_bits(32)
    run.close()


def _host_node_table(gid, zoom_lo, zoom_hi, t):
    b = styled.LabelBindings(gid, zoom_lo, zoom_hi, [], [])
    b.node_off, b.bindings, b.text_off, b.chars = t.off[0], t.bind[0], t.text_off, t.chars
    return b


def _host_area_table(gid, zoom_lo, zoom_hi, t):
    b = styled.AreaLabelBindings(gid, zoom_lo, zoom_hi, [], [], [])
    b.way_off, b.way_bindings, b.multipolygon_off, b.multipolygon_bindings, b.text_off, b.chars = t.off[0], t.bind[0], t.off[1], t.bind[1], t.text_off, t.chars
    return b


def test_host_registered_tables_come_back_as_they_went_in(gpu_ctx, tmp_path, first_style):
    """osmt_read_label_bindings / osmt_read_area_label_bindings serve any registered table; counts, NULL outputs and small caps"""
    run = Run(gpu_ctx, tmp_path / "w.bin", _fill(sm.World(), 40, 30, 20), SELS)
    rows = lambda n: [[(first_style + (i + j) % 8, None if (i + j) % 3 == 0 else (i * j) % 4) for j in range(i % 4)] for i in range(n)]
    texts = ["AB", "", "Каменный мост", "京"]
    nb = styled.LabelBindings(run.gid, 2, 9, rows(40), texts)
    ab = styled.AreaLabelBindings(run.gid, 2, 9, rows(30), rows(20)[::-1], texts)
    nid, aid = gpu_ctx.register_label_bindings(nb), gpu_ctx.register_area_label_bindings(ab)
    got = run.read(nid, False)
    assert [a.tobytes() for a in got.arrays()] == [nb.node_off.tobytes(), nb.bindings.tobytes(), b"", b"", nb.text_off.tobytes(), nb.chars.tobytes()]
    got = run.read(aid, True)
    assert [a.tobytes() for a in got.arrays()] == [ab.way_off.tobytes(), ab.way_bindings.tobytes(), ab.multipolygon_off.tobytes(),
                                                   ab.multipolygon_bindings.tobytes(), ab.text_off.tobytes(), ab.chars.tobytes()]
    L = lib.load()
    n3, n4 = (C.c_size_t * 3)(), (C.c_size_t * 4)()
    assert L.osmt_read_label_bindings(gpu_ctx._h, nid, None, None, None, None, None, n3) == A.OK
    assert list(n3) == [len(nb.bindings), len(texts), len(nb.chars)]
    assert L.osmt_read_area_label_bindings(gpu_ctx._h, aid, None, None, None, None, None, None, None, n4) == A.OK
    assert list(n4) == [len(ab.way_bindings), len(ab.multipolygon_bindings), len(texts), len(ab.chars)]
    buf = np.zeros(1 << 12, np.uint32)
    p = C.c_void_p(buf.ctypes.data)
    for k in range(3):  # each cap one short, with its output asked for
        caps, m3 = (C.c_size_t * 3)(*[v - (i == k) for i, v in enumerate(n3)]), (C.c_size_t * 3)()
        args = [p if k == 0 else None, p if k == 1 else None, p if k == 2 else None]
        assert L.osmt_read_label_bindings(gpu_ctx._h, nid, None, *args, caps, m3) == A.INVALID_ARG and list(m3) == list(n3)
    for k in range(4):
        caps, m4 = (C.c_size_t * 4)(*[v - (i == k) for i, v in enumerate(n4)]), (C.c_size_t * 4)()
        args = [None, p if k == 0 else None, None, p if k == 1 else None, p if k == 2 else None, p if k == 3 else None]
        assert L.osmt_read_area_label_bindings(gpu_ctx._h, aid, *args, caps, m4) == A.INVALID_ARG and list(m4) == list(n4)
    assert L.osmt_read_label_bindings(gpu_ctx._h, nid, p, None, None, None, None, n3) == A.INVALID_ARG  # an output without caps
    assert L.osmt_read_label_bindings(gpu_ctx._h, 1 << 20, None, None, None, None, None, n3) == A.INVALID_ARG
    assert L.osmt_read_area_label_bindings(gpu_ctx._h, 1 << 20, None, None, None, None, None, None, None, n4) == A.INVALID_ARG
    run.close()


def test_refusals(gpu_ctx, tmp_path, first_style):
    """every OSMT_INVALID_ARG of the two registrations, and 257 keys"""
    run = Run(gpu_ctx, tmp_path / "w.bin", _fill(sm.World(), 9, 6, 4), SELS)
    L = lib.load()
    n_cls = len(run.cls)
    good = lambda: selmatch.ClassLabelBindings(0, 18, [[(first_style, 0)] for _ in range(n_cls)], ["name"])
    calls = (L.osmt_register_label_bindings_matched, L.osmt_register_area_label_bindings_matched)

    def refused(word, b=None, ctx_h=None, match_h=None, code=A.INVALID_ARG, only=None):
        d, out = (b or good()).as_desc(), C.c_uint32()
        for call in calls if only is None else (calls[only],):
            assert call(ctx_h or gpu_ctx._h, match_h or run.m._h, C.byref(d), C.byref(out)) == code
            assert word in L.osmt_last_error().decode(), L.osmt_last_error()
        if ctx_h is None and match_h is None:
            assert L.osmt_validate_class_label_bindings(C.byref(d), run.m._h, gpu_ctx._h) == code

    from osm_renderer_amd.renderer import Context

    stranger = Context(0)
    refused("another context", ctx_h=stranger._h)
    stranger.close()
    refused("classes, the match has", selmatch.ClassLabelBindings(0, 18, [[] for _ in range(n_cls - 1)], []))
    b = good()
    b.class_off[0] = 1
    refused("class_off[0] is 1", b)
    b = good()
    b.class_off[2] = 0
    refused("less than the entry before", b)
    b = good()
    b.class_off[-1] += 1
    refused("does not end at", b)
    b = good()
    b.key_off[-1] += 1
    refused("key_off", b)
    b = good()
    b.bindings["style"][1] = 10**6
    refused("is not a registered label style", b)
    b = good()
    b.bindings["text_key"][0] = 1
    refused("text_key = 1", b)
    refused("zoom range", selmatch.ClassLabelBindings(5, 19, [[] for _ in range(n_cls)], []))
    refused("zoom range", selmatch.ClassLabelBindings(7, 6, [[] for _ in range(n_cls)], []))
    b = selmatch.ClassLabelBindings(0, 18, [[] for _ in range(n_cls)], [f"k{i}" for i in range(A.LABEL_TEXT_KEYS_MAX + 1)])
    refused("257 keys (> OSMT_LABEL_TEXT_KEYS_MAX = 256)", b, code=A.UNSUPPORTED)
    run.table(selmatch.ClassLabelBindings(0, 18, [[] for _ in range(n_cls)], [f"k{i}" for i in range(A.LABEL_TEXT_KEYS_MAX)]), True)
    # a declined match
    w = sm.World()
    w.open_way({"lanes": "1e23"})
    r = w.write(tmp_path / "d.bin")
    gid = gpu_ctx.register_geodata(geodata_of(r))
    t = sm.TagsOf(r)
    gpu_ctx.register_tags(gid, t.desc())
    sid = gpu_ctx.register_selectors(selmatch.SelectorSet([(WAY, [(A.TEST_GREATER, "lanes", 2.0)])]))
    h = C.c_void_p()
    assert L.osmt_match_selectors(gpu_ctx._h, gid, sid, None, 0, C.byref(h)) == A.UNSUPPORTED and h.value
    refused("declined state", match_h=h)
    L.osmt_match_free(h)
    # what the area table demands of the geodata id: a tile index, then Mercator factors; the node table needs neither
    m = gpu_ctx.match_selectors(gid, gpu_ctx.register_selectors(selmatch.SelectorSet([])))
    one = selmatch.ClassLabelBindings(0, 18, [[(first_style, None)] for _ in m.read()[1]], [])
    refused("has no tile index", one, match_h=m._h, only=1)
    gpu_ctx.register_tile_index(gid, styled.TileIndex([((CX, CY), [0], [])]))
    refused("has no Mercator factors", one, match_h=m._h, only=1)
    nid = m.register_label_bindings(0, 18, one)
    gpu_ctx.register_node_mercator(gid, an.mercator_factors(r.node_table()))
    aid = m.register_area_label_bindings(0, 18, one)
    m.close()  # the tables do not depend on the match
    off, bind, _, _ = gpu_ctx.read_label_bindings(nid, r.n_nodes)
    assert off.tolist() == [0, 1, 2] and bind["text"].tolist() == [NONE, NONE]
    assert gpu_ctx.read_area_label_bindings(aid, 1, 0)[1]["style"].tolist() == [first_style]
    t.close()
    r.close()
    run.close()


# ---- downstream: the ids serve osmt_scene_build_tile_labels_all like any other ---------------------------------------------------
NS = len(labels.SYNTH_GLYPHS)


@pytest.fixture(scope="module")
def tables(gpu_ctx):
    """the font and icons of tests/test_gpu_area_labels.py: the letters A .. L and the space"""
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    shapes = [NS - 1] + [(g - 1) % (NS - 1) for g in range(1, 13)] + [NS - 1]
    cmap = [(0x20, 13)] + [(0x41 + i, 1 + i) for i in range(12)]
    font = labels.FontTable(cmap, [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]], [syn.first_id + s for s in shapes], [(1, 2, 17), (3, 5, -45)])
    gpu_ctx.register_font(font)
    rng = np.random.default_rng(23)
    ids = []
    for h, wd in ((16, 16), (5, 7)):
        img = rng.integers(0, 256, size=(h, wd, 4)).astype(np.uint8)
        img[: h // 2, :, 3] = 255
        ids.append(gpu_ctx.register_image(img))
    return font, ids


def test_scenes_labelled_from_matched_tables_equal_scenes_labelled_per_entity(gpu_ctx, tmp_path, tables):
    """a scene of osmt_scene_build_tiles over three zooms, labelled twice by osmt_scene_build_tile_labels_all: once from the
    matched tables, once from per-entity tables registered from the mirror's arrays; the node batch, the area batch and the
    framebuffers are byte-identical"""
    font, icons = tables
    f = font.font_id
    first = gpu_ctx.register_label_styles(tl.label_styles([
        dict(font_size=11.0, font_id=f),
        dict(icon=icons[0], font_size=9.0, font_id=f, text_color=(150, 20, 60), text_position=A.LABEL_POSITION_CENTER),
        dict(layer=1, icon=icons[1]),
        dict(z_index=2.5, font_size=13.0, font_id=f, text_color=(0, 90, 200)),
    ]))
    words = ["CAFE", "BAKED", "A", "HIGH GLADE", "", "LAKE", "BIG FIELD"]
    rng = np.random.default_rng(43)
    w = sm.World()
    node_fn = lambda la, lo: w.node(None, la, lo)
    for k in range(40):
        ids = tq.square(node_fn, k)
        t = {"name": words[k % len(words)]} if k % 4 else {}
        if k % 3 == 0:
            t["highway" if k % 2 else "building"] = "yes"
        if k % 5 == 0:
            t["ref"] = "A" * (1 + k % 3)
        w.way(ids if k % 2 else ids[:3], t)
        if k % 6 == 0:
            w.nodes[ids[0]][3].update({"name": words[(k + 2) % len(words)], "shop": "yes"} if k % 12 else {"shop": "yes"})
    for m in range(8):
        w.polygons.append(tq.square(node_fn, 3 * m + 1, size=0.0007))
        w.mps.append((9000 + m, [len(w.polygons) - 1], {"name": words[(m + 3) % len(words)], "building": "yes"} if m % 3 else {"building": "yes"}))
    sels = [(NODE, [(E, "shop")]), (WAY, [(E, "highway")]), (AREA, [(EQ, "building", "yes")]), (WAY, [(E, "ref")]), (WAY, [])]
    run = Run(gpu_ctx, tmp_path / "w.bin", w, sels, max_zoom_tile=tq.max_zoom_tile)
    gpu_ctx.register_node_index(run.gid, tl.node_index_of(run.r, w.refs))
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
    draw = gpu_ctx.register_styles(st)
    draw_bind = gpu_ctx.register_style_bindings(styled.StyleBindings(run.gid, 0, 18, [[draw] if len(x[1]) > 3 else [] for x in w.ways], [[] for _ in w.mps]))
    matched, per_entity = ({}, {}), ({}, {})
    n_texts = 0
    for zoom in (16, 17, 18):
        # the "cascade" of the test: by class and zoom, up to three label styles; the key is the name, the reference, or none
        rows = per_class(run, lambda c, rec: [(first + (c + zoom + j) % 4, (0, 1, None)[(c + j) % 3]) for j in range((c + zoom) % 4)] if rec["n_sels"] else [])
        b = selmatch.ClassLabelBindings(zoom, zoom, rows, ["name", "ref"])
        for area in (False, True):
            matched[area][zoom] = (run.m.register_area_label_bindings if area else run.m.register_label_bindings)(zoom, zoom, b)
            t = lb.mirror(run.tags, run.ent, b, area)
            same(run.read(matched[area][zoom], area), t)
            n_texts += len(t.text_off) - 1
            if area:
                per_entity[area][zoom] = gpu_ctx.register_area_label_bindings(_host_area_table(run.gid, zoom, zoom, t))
            else:
                per_entity[area][zoom] = gpu_ctx.register_label_bindings(_host_node_table(run.gid, zoom, zoom, t))
    assert n_texts > 6
    tiles = []
    for zoom in (16, 17, 18):
        sh = 18 - zoom
        tiles += [(zoom, CX >> sh, CY >> sh), (zoom, (CX >> sh) + 1, CY >> sh)]
    out = []
    for ids in (matched, per_entity):
        sc = gpu_ctx.build_tiles(styled.TileBatch(run.gid, tiles, {z: draw_bind for z in (16, 17, 18)}))
        area, node = sc.build_tile_labels_all(ids[True], ids[False])
        out.append((node, area, gpu_ctx.render(sc).cpu().numpy()))
        sc.free()
    (n0, a0, px0), (n1, a1, px1) = out
    assert len(n0.labels) > 0 and len(a0.labels) > 10 and a0.labels["has_text"].any() and len(a0.chars) + len(n0.chars) > 20
    for got, want in ((n0, n1), (a0, a1)):
        assert got.job_label_off.tobytes() == want.job_label_off.tobytes()
        for name in ("labels", "runs", "chars", "way_pts", "way_sincos"):
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    assert np.array_equal(px0, px1)
    bare = gpu_ctx.build_tiles(styled.TileBatch(run.gid, tiles, {z: draw_bind for z in (16, 17, 18)}))
    assert not np.array_equal(gpu_ctx.render(bare).cpu().numpy(), px0)  # the labels are in the pixels
    bare.free()
    run.close()
