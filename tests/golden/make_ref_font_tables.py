#!/usr/bin/env python
"""Builds tests/golden/ref_font_tables.json: the flat tables osmt_register_font takes (osmt_font_desc), read out of the
reference's font src/draw/font/NotoSans-Regular.ttf through the TrueType reader of make_ref_label_patches.py — what an
integrator fills once per font with stb_truetype's find_glyph_index, get_glyph_h_metrics, get_glyph_kern_advance and
get_v_metrics.  Data only, no font file:

  * `cmap`: every code point the font maps to a glyph other than 0, as [code_point, glyph] pairs in rising code point
    order (find_glyph_index over U+0000..U+10FFFF without the surrogates; a code point not listed is glyph 0);
  * `advance`: get_glyph_h_metrics(g).advance_width for every glyph index g < num_glyphs;
  * `kern`: the [left, right, value] triples of the font's `kern` table (format 0, horizontal) in rising (left, right)
    order — possibly none: this font keeps its kerning in GPOS, which stb_truetype's get_glyph_kern_advance of the
    reference's version does not read;
  * `v_metrics`: get_v_metrics() = [ascent, descent, line_gap];
  * `outline`: per glyph index, the position of its outline in `glyphs` of ref_glyph_runs.json, or null ("none": the
    tests register one empty outline for all of those).

The script checks itself against ref_text_runs.json: every char of every text there maps, through these tables, to that
fixture's [glyph, advance, kern] (tests/test_text_shaper_cpu.py makes the same comparison with the mirror and the model).

Run in the build container only (reads the reference's font); the JSON it writes is the fixture.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_label_patches import REF, Font  # noqa: E402


def kern_triples(font):
    k = font.kern
    if not k or font.u16(k + 2) < 1 or font.u16(k + 8) != 1:  # the conditions of kern_advance
        return []
    return [[font.u16(k + 18 + 6 * m), font.u16(k + 20 + 6 * m), font.i16(k + 22 + 6 * m)] for m in range(font.u16(k + 10))]


def main():
    font = Font(open(os.path.join(REF, "src/draw/font/NotoSans-Regular.ttf"), "rb").read())
    runs = json.load(open(os.path.join(HERE, "ref_glyph_runs.json")))
    cmap = []
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        g = font.find_glyph_index(cp)
        if g:
            cmap.append([cp, g])
    n_glyphs = font.num_glyphs
    assert all(g < n_glyphs for _, g in cmap)
    outline = [None] * n_glyphs
    for i, g in enumerate(runs["glyphs"]):
        outline[font.find_glyph_index(ord(g["char"]))] = i
    kern = kern_triples(font)
    assert kern == sorted(kern) and all(font.kern_advance(a, b) == v for a, b, v in kern)
    out = {"_provenance": __doc__, "v_metrics": [int(v) for v in font.v_metrics()], "n_glyphs": n_glyphs, "cmap": cmap,
           "advance": [int(font.h_metrics(g)[0]) for g in range(n_glyphs)], "kern": kern, "outline": outline}
    # the same chars as ref_text_runs.json has them
    lookup = dict(cmap)
    texts = json.load(open(os.path.join(HERE, "ref_text_runs.json")))
    assert texts["v_metrics"] == out["v_metrics"]
    for t in texts["texts"]:
        for ch, want in zip(t["text"], t["chars"]):
            g = lookup.get(ord(ch), 0)
            assert [outline[g], out["advance"][g], 0] == want[:3], (t["text"], ch)
    path = os.path.join(HERE, "ref_font_tables.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print(len(cmap), "code points;", n_glyphs, "glyphs;", len(kern), "kern pairs;", sum(o is not None for o in outline), "outlines;",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
