"""TextPlacer::text_to_glyphs (src/draw/font/text_placer.rs:170-197) restated in Python over the flat font tables of
osmt_register_font — the third witness beside the host mirror (osm_renderer_amd/host/osmt_textshaper.hpp) and the device
kernel (k_text_shape).  Written against the reference's text, not against the library: the lookups are bisections of the
sorted tables as stb_truetype's own are, the whitespace test is the White_Space property list of Rust's
char::is_whitespace spelled out range by range.

    for (i, ch) in text.chars().enumerate() {
        let glyph_id = font.find_glyph_index(ch as u32);            -> cmap, 0 when missing
        let advance = get_glyph_h_metrics(glyph_id).advance_width;   -> advance[glyph]
        let kern = if i > 0 { get_glyph_kern_advance(prev, glyph_id) } else { 0 };   -> kern, 0 when missing
        ... is_whitespace: ch.is_whitespace()
        prev = glyph_id
    }
"""
import bisect

import numpy as np

from osm_renderer_amd import labels

# Unicode White_Space (PropList.txt), as inclusive ranges
_WHITE_SPACE_RANGES = [(0x0009, 0x000D), (0x0020, 0x0020), (0x0085, 0x0085), (0x00A0, 0x00A0), (0x1680, 0x1680), (0x2000, 0x200A),
                       (0x2028, 0x2029), (0x202F, 0x202F), (0x205F, 0x205F), (0x3000, 0x3000)]


def is_whitespace(cp):
    return any(a <= cp <= b for a, b in _WHITE_SPACE_RANGES)


def is_char(cp):
    return 0 <= cp <= 0x10FFFF and not 0xD800 <= cp <= 0xDFFF


class Font:
    """Sorted key lists over a labels.FontTable."""

    def __init__(self, table):
        self.table = table
        self.cps = table.cmap["code_point"].tolist()
        self.glyphs = table.cmap["glyph"].tolist()
        self.pairs = [(int(l) << 32) | int(r) for l, r in zip(table.kern["left"], table.kern["right"])]
        self.values = table.kern["value"].tolist()
        self.advance = table.advance.tolist()
        self.outline = table.outline_id.tolist()

    def find_glyph_index(self, cp):
        i = bisect.bisect_left(self.cps, cp)
        return self.glyphs[i] if i < len(self.cps) and self.cps[i] == cp else 0

    def kern_advance(self, left, right):
        key = (left << 32) | right
        i = bisect.bisect_left(self.pairs, key)
        return self.values[i] if i < len(self.pairs) and self.pairs[i] == key else 0

    def scale(self, font_size):
        return float(np.float32(font_size) / np.float32(self.table.ascent - self.table.descent))


def shape_text(font, chars):
    """TEXT_GLYPH_DTYPE records of one text (chars: code points), glyph_id = the outline id."""
    out = np.zeros(len(chars), labels.TEXT_GLYPH_DTYPE)
    prev = None
    for i, cp in enumerate(int(c) for c in chars):
        g = font.find_glyph_index(cp)
        kern = font.kern_advance(prev, g) if i > 0 else 0
        out[i] = (font.outline[g], font.advance[g], kern, 1 if is_whitespace(cp) else 0)
        prev = g
    return out


def shape_labels(sl, fonts):
    """The records of a whole labels.StringLabelList in slot order (fonts: model Fonts indexed by font id); slots no
    has_text label names stay zero."""
    out = np.zeros(len(sl.chars), labels.TEXT_GLYPH_DTYPE)
    for l, r in zip(sl.labels, sl.runs):
        if l["has_text"] and l["n_segs"]:
            a, n = int(l["seg_off"]), int(l["n_segs"])
            out[a : a + n] = shape_text(fonts[int(r["font_id"])], sl.chars[a : a + n])
    return out
