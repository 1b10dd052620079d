#!/usr/bin/env python
"""Builds tests/golden/ref_text_runs.json: a few label texts as TEXT RUNS (osmt_text_label_batch) — what
TextPlacer::text_to_glyphs (font/text_placer.rs:170-197) hands to the placement — from the reference's font
src/draw/font/NotoSans-Regular.ttf through the TrueType reader of make_ref_label_patches.py.

  * `v_metrics`: font.get_v_metrics() = [ascent, descent, line_gap] in font units (1069, -293, 0);
  * `texts`: for every text of TEXTS and every font size of SIZES, `scale` = f64::from(scale_for_pixel_height(size as
    f32)) and, per char, [glyph, advance, kern, whitespace]: the index of the char's outline in `glyphs` of
    ref_glyph_runs.json, get_glyph_h_metrics(g).advance_width, get_glyph_kern_advance(prev, g) (0 for the first char)
    and ch.is_whitespace();
  * `rows`: the number of rows TextPosition::Center lays the text out in, counted here with the placement of
    make_ref_glyph_runs.py's reader and the row rule of text_placer.rs:119-133.

This font has NO kern pairs for these texts: every kern is 0 (the script asserts it), so a non-zero kern is covered by
the synthetic tests only (tests/test_text_placer_cpu.py), not by anything derived from the reference's data.

Run in the build container only (reads the reference's font); the JSON it writes is the fixture.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_label_patches import REF, Font  # noqa: E402

TEXTS = ["Арбатская", "Улица Новый Арбат", "AVATAR To Wave", "a b c d e f g h i j k"]
SIZES = [9.0, 11.0, 14.0]


def rows_of(widths, spaces):
    rows, cur = 0, 0.0
    for k, (w, ws) in enumerate(zip(widths, spaces)):
        cur += w
        if (ws and cur + w > 256 / 8.0) or k + 1 == len(widths):
            rows += 1
            cur = 0.0
    return rows


def main():
    font = Font(open(os.path.join(REF, "src/draw/font/NotoSans-Regular.ttf"), "rb").read())
    table = {g["char"]: i for i, g in enumerate(json.load(open(os.path.join(HERE, "ref_glyph_runs.json")))["glyphs"])}
    out = {"_provenance": __doc__, "v_metrics": [int(v) for v in font.v_metrics()], "texts": []}
    for text in TEXTS:
        for size in SIZES:
            scale = font.scale_for_pixel_height(size)
            chars, widths, prev = [], [], None
            for ch in text:
                g = font.find_glyph_index(ord(ch))
                adv = int(font.h_metrics(g)[0])
                kern = int(font.kern_advance(prev, g)) if prev is not None else 0
                assert kern == 0, (text, ch, kern)
                chars.append([table[ch], adv, kern, 1 if ch.isspace() else 0])
                w = float(adv) * scale
                if prev is not None:
                    w += float(kern) * scale
                widths.append(w)
                prev = g
            out["texts"].append({"text": text, "font_size": size, "scale": scale, "chars": chars,
                                 "rows": rows_of(widths, [c[3] for c in chars])})
    path = os.path.join(HERE, "ref_text_runs.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print(len(out["texts"]), "texts;", os.path.getsize(path), "bytes;", [(t["text"], t["font_size"], t["rows"]) for t in out["texts"]])


if __name__ == "__main__":
    main()
