"""String-label cases for the shaper tests (tests/test_text_shaper_cpu.py, tests/test_text_edge_cases_cpu.py on the host,
tests/test_gpu_text_edges.py on the device).

A case is a name, a builder and a check:

  * case.build(ids) returns (labels.StringLabelList, [labels.FontTable]).  The runs name their font by its index in
    the list; bind_fonts() rewrites them once the fonts have ids of their own.  `ids` (Outlines) says which outline ids
    the fonts may name: on the device they must be ids of registered outlines;
  * case.check(got, ids) holds the literal expectations on `got`, the TEXT_GLYPH_DTYPE records in slot order
    (osmt_scene_read_text_glyphs, the host mirror, or the model).

The tables and probe lists are the ones the host tests always had; behind them come the cases shaped by k_text_shape
(osmt_textshape.hip): one lane per char in blocks of 256, the char in front found by index."""
import functools
import json
import os

import numpy as np

from osm_renderer_amd import abi, labels

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEXTS = json.load(open(os.path.join(GOLD, "ref_text_runs.json")))
RUNS = json.load(open(os.path.join(GOLD, "ref_glyph_runs.json")))
FONT = json.load(open(os.path.join(GOLD, "ref_font_tables.json")))


class Outlines:
    """The outline ids a case may use: base .. base + 1039 for the synthetic fonts (glyph g draws outline base + g), `one`
    for the font whose 70001 glyphs share an outline, ref_first / ref_empty for ref_font()."""

    def __init__(self, base=1000, one=9, ref_first=0, ref_empty=None):
        self.base, self.one, self.ref_first, self.ref_empty = base, one, ref_first, ref_empty


HOST = Outlines()  # what the host tests always used: nothing is drawn there


def ref_font(first_id=0, empty_id=None):
    """The reference's font as a FontTable: glyph g's outline is first_id + its position in ref_glyph_runs.json's
    glyphs; the glyphs the fixture has no outline for share the empty outline empty_id (default: right behind)."""
    empty_id = first_id + len(RUNS["glyphs"]) if empty_id is None else empty_id
    outline = [empty_id if o is None else first_id + o for o in FONT["outline"]]
    a, d, g = FONT["v_metrics"]
    return labels.FontTable(FONT["cmap"], FONT["advance"], outline, FONT["kern"], a, d, g)


def string_labels(specs, n_jobs=1):
    """One tile of string labels from dicts: chars (a str or code points), font (id), font_size, position, y_offset,
    center, pts (already in walking order), has_text (default 1)."""
    labs, runs, chars, pts = [], [], [], []
    n_ch = n_pt = 0
    for s in specs:
        l, r = np.zeros((), labels.LABEL_DTYPE), np.zeros((), labels.STRING_RUN_DTYPE)
        c = s.get("chars", [])
        c = np.array([ord(ch) for ch in c] if isinstance(c, str) else list(c), dtype=np.uint32)
        l["has_text"], l["text_color"] = s.get("has_text", 1), s.get("color", (10, 20, 30))
        if "icon" in s:
            l["has_icon"], l["image_id"], l["icon_center_x"], l["icon_center_y"] = 1, s["icon"], s["center"][0], s["center"][1]
        l["seg_off"], l["n_segs"] = (n_ch if len(c) else 0), len(c)
        r["position"], r["font_id"], r["font_size"] = s.get("position", abi.TEXT_CENTER), s.get("font", 0), s.get("font_size", 11.0)
        if r["position"] == abi.TEXT_LINE:
            p = np.array(s.get("pts", []), dtype=np.int32).reshape(-1, 2)
            r["pt_off"], r["n_pts"] = (n_pt if len(p) else 0), len(p)
            pts.append(p)
            n_pt += len(p)
        else:
            r["y_offset"] = s.get("y_offset", 0)
            r["center_x"], r["center_y"] = s.get("center", (100.0, 100.0))
        labs.append(l)
        runs.append(r)
        chars.append(c)
        n_ch += len(c)
    way = np.concatenate(pts) if pts else np.zeros((0, 2), np.int32)
    sincos = np.concatenate([labels.way_sincos(p) for p in pts]) if pts else np.zeros((0, 2))
    offs = [0] + [len(labs)] * n_jobs
    return labels.StringLabelList(np.array(labs, dtype=labels.LABEL_DTYPE), offs, np.array(runs, dtype=labels.STRING_RUN_DTYPE),
                                  np.concatenate(chars) if chars else np.zeros(0, np.uint32), way, sincos)


def synth_font(n_cmap, kern=(), first_cp=0x30, step=3, n_glyphs=None, base=1000):
    """n_cmap code points first_cp, first_cp + step, ... (gaps between them) -> glyphs 1, 2, ... cycling through n_glyphs
    - 1 glyphs; glyph g has advance 100 + 7 g and outline base + g."""
    n_glyphs = n_glyphs or min(n_cmap + 1, 40)
    cmap = [(first_cp + step * i, 1 + i % (n_glyphs - 1)) for i in range(n_cmap)]
    return labels.FontTable(cmap, [100 + 7 * g for g in range(n_glyphs)], [base + g for g in range(n_glyphs)], kern)


def bind_fonts(sl, fonts):
    """Rewrites the runs' font indices into the ids the fonts have now (FontTable.font_id); returns sl."""
    sl.runs["font_id"] = np.array([f.font_id for f in fonts], dtype=np.uint32)[sl.runs["font_id"]]
    return sl


def reverse_pool(sl):
    """The same labels with their char ranges in reverse label order in the pool."""
    lab, c, cur = sl.labels.copy(), np.zeros_like(sl.chars), 0
    for i in reversed(range(len(lab))):
        off, n = int(lab[i]["seg_off"]), int(lab[i]["n_segs"])
        if n:
            c[cur : cur + n] = sl.chars[off : off + n]
            lab[i]["seg_off"] = cur
            cur += n
    return labels.StringLabelList(lab, sl.job_label_off.copy(), sl.runs.copy(), c, sl.way_pts.copy(), sl.way_sincos.copy())


class Case:
    """make(ids) -> (label dicts of string_labels() with `font` an index, [FontTable]); literal(parts, ids): the literal
    expectations on the per-label slices of the records."""

    def __init__(self, name, make, literal, reverse=False):
        self.name, self.make, self.literal, self.reverse = name, make, literal, reverse

    def __repr__(self):
        return f"Case({self.name})"

    def build(self, ids=HOST):
        specs, fonts = self.make(ids)
        for i, f in enumerate(fonts):
            f.font_id = i
        sl = string_labels(specs)
        return (reverse_pool(sl) if self.reverse else sl), fonts

    def check(self, got, ids=HOST):
        sl, _ = self.build(ids)
        assert len(got) == len(sl.chars)
        self.literal([got[int(l["seg_off"]) : int(l["seg_off"]) + int(l["n_segs"])] if l["has_text"] else got[:0] for l in sl.labels], ids)


def _spread(specs):
    """Centres apart from each other, so that the texts of a batch do not all lie on one spot."""
    for i, s in enumerate(specs):
        s.setdefault("center", (40.0 + 30.0 * (i % 6), 40.0 + 25.0 * (i // 6)))
    return specs


# ---- cmap bisection ---------------------------------------------------------------------------------------------------
CMAP_SIZES = (1, 2, 7, 8, 9, 1024, 1025)


def cmap_probes(n_cmap):
    first, last = 0x30, 0x30 + 3 * (n_cmap - 1)
    probes = [0, first - 1, first, first + 1, last - 1, last, last + 1, last + 2, 0x10FFFF, 0xD7FF, 0xE000]
    return probes + [first + 3 * i + d for i in range(0, n_cmap, max(1, n_cmap // 50)) for d in (0, 1, 2)]  # entries and the gaps behind them


def _cmap(n_cmap):
    def make(ids):
        font = synth_font(n_cmap, base=ids.base)
        return _spread([dict(chars=cmap_probes(n_cmap)), dict(chars=font.cmap["code_point"].tolist())]), [font]  # ... and every entry of the table, in one text

    def literal(p, ids):
        got, entries = p
        font, probes = synth_font(n_cmap), cmap_probes(n_cmap)
        listed = dict(font.cmap.tolist())
        assert got["glyph_id"].tolist() == [ids.base + listed.get(c, 0) for c in probes]
        assert got["advance"].tolist() == [100 + 7 * listed.get(c, 0) for c in probes]
        assert got["glyph_id"][2] != ids.base and got["glyph_id"][5] != ids.base and got["glyph_id"][0] == got["glyph_id"][1] == got["glyph_id"][6] == ids.base
        assert entries["glyph_id"].tolist() == [ids.base + g for g in font.cmap["glyph"].tolist()]

    return Case(f"cmap-{n_cmap}", make, literal)


# ---- kern tables ------------------------------------------------------------------------------------------------------
cp = lambda g: 0x30 + 3 * (g - 1)  # the code point of glyph g in synth_font (g >= 1)
BIG_KERN = [(2, 70000, 4), (3, 1, 6), (65536, 65536, 9), (70000, 2, -4)]


def big_font(one):
    """Glyph indices beyond 16 bits: (2, 70000), (65536, 65536) and (70000, 2) keep their order only in a key that gives
    each index 32 bits.  (3, 1) is there for a key of 16 bits per index computed in 64: (2 << 16 | 70000) > (3 << 16 | 1)."""
    return labels.FontTable([(0x41, 70000), (0x42, 2), (0x43, 65536)], [5] * 70001, [one] * 70001, BIG_KERN)


def _kern_tables():
    text = [cp(3), cp(5), cp(3), cp(5), cp(9)]  # pairs (3, 5), (5, 3), (3, 5), (5, 9)
    many = [(l, r, 10 * l - r) for l in range(1, 20) for r in range(1, 20) if (l, r) not in ((3, 5), (5, 3), (5, 9))]
    firstp = [(3, 5, 33)] + [(l, r, 1) for l in range(4, 20) for r in range(1, 20)]
    lastp = [(l, r, -1) for l in range(1, 3) for r in range(1, 20)] + [(3, 5, -65535)]
    zero = [(0, 0, 7), (0, 3, 11), (3, 0, -13), (3, 3, 17)]
    tables = [[], [(3, 5, -40)], [(5, 3, 25)], many, firstp, lastp]

    def make(ids):
        fonts = [synth_font(20, k, base=ids.base) for k in tables] + [synth_font(20, zero, base=ids.base), big_font(ids.one)]
        specs = [dict(chars=text, font=i) for i in range(len(tables))]
        specs += [dict(chars=[cp(3), cp(3), 0x10FFFF, 0x10FFFF, cp(3)], font=len(tables)), dict(chars=[0x41, 0x42, 0x41, 0x43, 0x43], font=len(tables) + 1)]
        return _spread(specs), fonts

    def literal(p, ids):
        assert p[0]["kern"].tolist() == [0, 0, 0, 0, 0]  # no kern table
        assert p[1]["kern"].tolist() == [0, -40, 0, -40, 0]  # one pair
        assert p[2]["kern"].tolist() == [0, 0, 25, 0, 0]  # only the other order is listed
        assert p[3]["kern"].tolist() == [0, 0, 0, 0, 0]  # everything but the wanted pairs
        assert p[4]["kern"].tolist() == [0, 33, 1, 33, 1]  # the wanted pair is the first entry
        assert p[5]["kern"].tolist() == [0, -65535, 0, -65535, 0]  # ... the last entry
        # the first glyph has no kern even when (glyph 0, g) and (g, g) are listed; a missing code point is glyph 0 and pairs as such
        assert p[6]["kern"].tolist() == [0, 17, -13, 7, 11] and p[6]["glyph_id"].tolist() == [ids.base + g for g in (3, 3, 0, 0, 3)]
        # left and right glyph indices beyond 16 bits keep their order in the key
        assert p[7]["kern"].tolist() == [0, -4, 4, 0, 9] and p[7]["glyph_id"].tolist() == [ids.one] * 5 and p[7]["advance"].tolist() == [5] * 5

    return Case("kern-tables", make, literal)


# ---- whitespace -------------------------------------------------------------------------------------------------------
def whitespace_probes():
    ws = sorted(labels.WHITE_SPACE)
    return sorted(set(ws) | {c + d for c in ws for d in (-1, 1)} | {0x1C, 0x1D, 0x1E, 0x1F, 0x180E, 0x200B, 0xFEFF, 0x2060, 0x10FFFF})


def _whitespace():
    def literal(p, ids):
        (got,) = p
        probes, ws = whitespace_probes(), sorted(labels.WHITE_SPACE)
        assert len(ws) == 25
        assert got["flags"].tolist() == [1 if c in labels.WHITE_SPACE else 0 for c in probes]
        assert [c for c, f in zip(probes, got["flags"]) if f] == ws

    return Case("whitespace", lambda ids: ([dict(chars=whitespace_probes())], [synth_font(9, base=ids.base)]), literal)


# ---- label boundaries -------------------------------------------------------------------------------------------------
def _two_fonts(ids):
    """Font 0: (3, 5) -> -40, (5, 3) -> 9.  Font 1 starts one code point earlier: the same code point is the next glyph."""
    return [synth_font(20, [(3, 5, -40), (5, 3, 9)], base=ids.base), synth_font(20, [(3, 5, 77)], first_cp=0x30 - 3, base=ids.base)]


def _label_boundary():
    def make(ids):
        return _spread([dict(chars=[cp(3), cp(5), cp(3)]), dict(chars=[cp(5), cp(3)]), dict(has_text=0), dict(chars=[]),
                        dict(chars=[cp(5), cp(2), cp(4)], font=1), dict(chars=[cp(5)])]), _two_fonts(ids)

    def literal(p, ids):
        got = np.concatenate(p)
        # the first char of label 1 sits behind a 3 | 5 boundary (-40 if the pool's neighbour leaked in); in font 1 the chars of
        # label 4 are glyphs 6, 3, 5
        assert got["kern"].tolist() == [0, -40, 9, 0, 9, 0, 0, 77, 0]
        assert got["glyph_id"][5] == ids.base + 6 and got["glyph_id"][3] == ids.base + 5  # cp(5) is glyph 6 in font 1

    return Case("kern-label-boundary", make, literal)


def _block_borders(reverse):
    """k_text_shape runs blocks of 256 lanes, one lane per char.  Label 5 has 600 chars and starts at pool slot 512, a
    block's first lane: its pair 3 | 5 lies across chars 63 | 64, 255 | 256 and 511 | 512, the last two across a block
    border.  In front of it the same pair lies across label boundaries at pool slots 255 | 256 and, with 5 | 3,
    256 | 257, where no kern may be applied; a label without text and an empty one stand in between, and label 4 is
    set in font 1, where the code points are other glyphs.  With the pool reversed the char in front of a first char is
    another label's last one."""
    fill = cp(7)

    def long_text():
        t = [fill] * 600
        for k in (63, 255, 511):
            t[k], t[k + 1] = cp(3), cp(5)
        return t

    def make(ids):
        a = [fill] * 255 + [cp(3)]  # slots 0 .. 255
        d = [cp(5)]  # slot 256
        e = [cp(3), cp(2), cp(4)] + [fill] * 252  # slots 257 .. 511, font 1: glyphs 4, 3, 5, ...
        return _spread([dict(chars=a), dict(has_text=0), dict(chars=[]), dict(chars=d), dict(chars=e, font=1), dict(chars=long_text(), font_size=9.0)]), _two_fonts(ids)

    def literal(p, ids):
        a, _, _, d, e, long = p
        assert len(a) == 256 and len(d) == 1 and len(e) == 255 and len(long) == 600
        assert not a["kern"].any() and d["kern"].tolist() == [0]  # 3 | 5 across the boundary at 255 | 256
        assert e["kern"][:4].tolist() == [0, 0, 77, 0] and not e["kern"][4:].any()  # 5 | 3 across 256 | 257; (3, 5) of font 1 inside
        assert e["glyph_id"][:3].tolist() == [ids.base + 4, ids.base + 3, ids.base + 5]
        assert np.nonzero(long["kern"])[0].tolist() == [64, 256, 512] and long["kern"][[64, 256, 512]].tolist() == [-40] * 3
        assert long["glyph_id"][[255, 256, 511, 512]].tolist() == [ids.base + 3, ids.base + 5] * 2

    return Case("kern-at-block-borders-reversed-pool" if reverse else "kern-at-block-borders", make, literal, reverse=reverse)


# ---- the reference's texts --------------------------------------------------------------------------------------------
def _reference_texts():
    def make(ids):
        specs = [dict(chars=t["text"], font_size=t["font_size"]) for t in TEXTS["texts"]]
        return _spread(specs), [ref_font(ids.ref_first, ids.ref_empty)]

    def literal(p, ids):
        assert len(p) == len(TEXTS["texts"]) == 12
        empty = ids.ref_first + len(RUNS["glyphs"]) if ids.ref_empty is None else ids.ref_empty
        for got, t in zip(p, TEXTS["texts"]):
            # the fixture's [glyph, advance, kern, whitespace]; its glyph is the outline's position in ref_glyph_runs.json's
            # glyphs, and one behind the last of them for a glyph without an outline
            want = np.array([tuple(c) for c in t["chars"]], dtype=labels.TEXT_GLYPH_DTYPE)
            assert (want["glyph_id"] <= len(RUNS["glyphs"])).all()
            want["glyph_id"] = np.where(want["glyph_id"] == len(RUNS["glyphs"]), empty, ids.ref_first + want["glyph_id"])
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), want.view(np.uint8)), t["text"]

    return Case("reference-texts", make, literal)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order (tuple of Case)."""
    return tuple([_cmap(n) for n in CMAP_SIZES] + [_kern_tables(), _whitespace(), _label_boundary(), _block_borders(False), _block_borders(True),
                                                   _reference_texts()])


def case(name):
    return next(c for c in cases() if c.name == name)
