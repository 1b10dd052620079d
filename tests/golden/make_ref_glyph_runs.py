#!/usr/bin/env python
"""Builds tests/golden/ref_glyph_runs.json: the metro-station label "Арбатская" of ref_label_patches.json as GLYPH RUNS
(osmt_glyph_label_batch) instead of draw_line calls, plus the outlines of a few dozen Latin and Cyrillic glyphs.

Everything comes from the reference's font src/draw/font/NotoSans-Regular.ttf through the TrueType reader of
make_ref_label_patches.py (a restatement of the stb_truetype crate for the calls font/text_placer.rs makes):

  * `glyphs`: the outline (stb_truetype Vertex list: type M / L / Q, x, y, cx, cy in font units) and advance width of
    every character of the station's name and of GLYPH_CHARS; index i of this list is glyph id i of the fixture;
  * `station` (z17, font-size 11) and `station_z14_from_the_tile_above` (z14, font-size 9): the label as
    TextPlacer::place, TextPosition::Center lays it out (font/text_placer.rs:103-155, one row): `scale` =
    f64::from(scale_for_pixel_height(size)) and, per glyph, the fixture glyph id, x_offset and baseline of its `tr`;
    the icon and the text colour as in ref_label_patches.json.

Expanding these runs with Glyph::rasterize (osm_renderer_amd.labels.GlyphLabelList.to_label_list) gives exactly the
draw_line calls of ref_label_patches.json (tests/test_glyph_runs_cpu.py).

Run in the build container only (reads /root/reference); the JSON it writes is the fixture.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_label_patches import REF, Font  # noqa: E402

TEXT = "Арбатская"
GLYPH_CHARS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789 .,-АБВГДЕЖЗИЙКЛМНОПРСТУФХЦЧШЩЪЫЬЭЮЯбвгдежзийклмнопуфхцчшщъыьэюя"


def station_run(font, table, font_size, cx, cy, y_offset):
    """TextPlacer::place, TextPosition::Center, one row (text_placer.rs:41-56,103-155) -> glyph instances."""
    scale = font.scale_for_pixel_height(font_size)
    asc, desc, gap = [v * scale for v in font.v_metrics()]
    glyphs, prev = [], None
    for ch in TEXT:
        g = font.find_glyph_index(ord(ch))
        w = float(font.h_metrics(g)[0]) * scale
        if prev is not None:
            w += float(font.kern_advance(prev, g)) * scale
        glyphs.append((table[ch], w))
        prev = g
    row_width = 0.0
    for _, w in glyphs:
        row_width += w
    row_height = asc - desc + gap
    cur_y = cy + float(y_offset) if y_offset > 0 else cy - row_height * 1.0 / 2.0
    cur_x = cx - row_width / 2.0
    out = []
    for gid, w in glyphs:
        out.append({"glyph": gid, "x_offset": cur_x, "baseline": cur_y + asc})
        cur_x += w
    return scale, out


def main():
    font = Font(open(os.path.join(REF, "src/draw/font/NotoSans-Regular.ttf"), "rb").read())
    patches = json.load(open(os.path.join(HERE, "ref_label_patches.json")))
    chars = []
    for ch in TEXT + GLYPH_CHARS:
        if ch not in chars:
            chars.append(ch)
    table, glyphs = {}, []
    for ch in chars:
        g = font.find_glyph_index(ord(ch))
        shape = font.glyph_shape(g) or []
        table[ch] = len(glyphs)
        glyphs.append({"char": ch, "font_glyph_index": g, "advance_width": font.h_metrics(g)[0],
                       "vertices": [[t, int(x), int(y), int(cx), int(cy)] for t, x, y, cx, cy in shape]})
    out = {"_provenance": __doc__, "glyphs": glyphs}
    for key, size in (("station", 11.0), ("station_z14_from_the_tile_above", 9.0)):
        p = patches[key]
        icon_h = len(p["icon_rgba"])
        cx, cy = p["icon_center"]
        scale, run = station_run(font, table, size, float(cx), float(cy), icon_h // 2)
        out[key] = {"font_size": size, "scale": scale, "icon_center": p["icon_center"], "icon_from": "ref_label_patches.json",
                    "text_color": p["text_color"], "glyphs": run}
    with open(os.path.join(HERE, "ref_glyph_runs.json"), "w") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print(len(glyphs), "glyphs,", sum(len(g["vertices"]) for g in glyphs), "vertices;",
          os.path.getsize(os.path.join(HERE, "ref_glyph_runs.json")), "bytes")


if __name__ == "__main__":
    main()
