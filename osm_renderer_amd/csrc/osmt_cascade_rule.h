/*
 * osmt_cascade_rule.h — the parts of the cascade that the library's kernels (osmt_cascade.hip), its registration and the
 * host mirror (host/osmt_cascade.hpp) share, so that each is stated once:
 *
 *   osmt_cs_prop        a property as the device sees it: no string, identifiers resolved to codes, `text` to a key index
 *   osmt_cs_style_of    property_map_to_style (mapcss/styler.rs:277-429) over a row of last writers: the 96-byte area record
 *                       with its dashes as ranges of the registered number pool, the 48-byte label record, the text key
 *
 * Records are canonical: a field whose has_* byte is 0, and all padding, is zero.  casing_width = base + multiplier * w is
 * written as two statements and the translation units are built with -ffp-contract=off: a multiplication, then an addition.
 */
#ifndef OSMT_CASCADE_RULE_H
#define OSMT_CASCADE_RULE_H

#include <stdint.h>
#include <string.h>

#include "../../include/osmtile.h"

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

#define OSMT_CS_NONE 0xFFFFFFFFu
#define OSMT_CS_ZOOMS (OSMT_MAX_ZOOM + 1u)
/* a row: the last writer of each of the 20 names in a layer, then the last writer of `width` in the layer "default" of the
 * same (class, zoom), the pair (class * 19 + zoom) and the position of the layer among the pair's styles */
enum { OSMT_CS_ROW_BASE_WIDTH = OSMT_PROP_NAMES, OSMT_CS_ROW_PAIR, OSMT_CS_ROW_POSITION, OSMT_CS_ROW_WORDS };

/* identifier codes */
#define OSMT_CS_ID_CAP_MASK 3u       /* osmt_line_cap of the identifier as a line cap (none | butt -> BUTT) */
#define OSMT_CS_ID_POS_SHIFT 2u      /* OSMT_LABEL_POSITION_* of the identifier as a text position, 2 bits */
#define OSMT_CS_ID_BACKGROUND 16u    /* the identifier is "background" */
#define OSMT_CS_F_COLOR 1u
#define OSMT_CS_F_IMAGE 2u

struct osmt_cs_prop { /* 32 bytes */
    double num;        /* NUMBERS of length 1: the number; WIDTH_DELTA: the delta */
    uint32_t num_off, n_nums; /* NUMBERS: the range of the registered number pool */
    uint32_t aux;      /* icon-image / fill-image: the image id; text: the key index */
    uint8_t kind;      /* OSMT_PV_* */
    uint8_t flags;     /* OSMT_CS_F_* */
    uint8_t id_code;   /* IDENTIFIER: OSMT_CS_ID_* */
    uint8_t rgb[3];
    uint8_t _pad[6];
};

/* what the records of one style are built from besides its row */
struct osmt_cs_env {
    const osmt_cs_prop* props;
    double casing_width_multiplier, font_size_multiplier; /* the latter 1.0 without */
    uint32_t font_id;
};

/* z-index default by cache slot (styler.rs:531-557, 559-579): node, closed way, open way, multipolygon (closed, reader.rs:520) */
OSMT_HD double osmt_cs_default_z(uint32_t slot) { return slot == 0u ? 4.0 : slot == 2u ? 3.0 : 1.0; }

/* get_num of a last writer */
OSMT_HD bool osmt_cs_num(const osmt_cs_prop* props, uint32_t i, double* v) {
    if (i == OSMT_CS_NONE || props[i].kind != OSMT_PV_NUMBERS || props[i].n_nums != 1u) return false;
    *v = props[i].num;
    return true;
}
/* get_color */
OSMT_HD uint8_t osmt_cs_color(const osmt_cs_prop* props, uint32_t i, uint8_t* rgb) {
    if (i == OSMT_CS_NONE) return 0;
    const osmt_cs_prop& p = props[i];
    if ((p.kind != OSMT_PV_COLOR && p.kind != OSMT_PV_IDENTIFIER) || !(p.flags & OSMT_CS_F_COLOR)) return 0;
    rgb[0] = p.rgb[0], rgb[1] = p.rgb[1], rgb[2] = p.rgb[2];
    return 1;
}
/* get_line_cap */
OSMT_HD uint8_t osmt_cs_cap(const osmt_cs_prop* props, uint32_t i) {
    if (i == OSMT_CS_NONE || props[i].kind != OSMT_PV_IDENTIFIER) return OSMT_CAP_NONE;
    return (uint8_t)(props[i].id_code & OSMT_CS_ID_CAP_MASK);
}
/* get_string(..) of an image property, looked up in the icon cache */
OSMT_HD uint8_t osmt_cs_image(const osmt_cs_prop* props, uint32_t i, uint32_t* id) {
    if (i == OSMT_CS_NONE) return 0;
    const osmt_cs_prop& p = props[i];
    if ((p.kind != OSMT_PV_IDENTIFIER && p.kind != OSMT_PV_STRING) || !(p.flags & OSMT_CS_F_IMAGE)) return 0;
    *id = p.aux;
    return 1;
}
/* get_dashes: a range of the registered number pool */
OSMT_HD uint8_t osmt_cs_dashes(const osmt_cs_prop* props, uint32_t i, uint32_t* off, uint32_t* n) {
    if (i == OSMT_CS_NONE || props[i].kind != OSMT_PV_NUMBERS) return 0;
    *off = props[i].n_nums ? props[i].num_off : 0u; /* Some([]): canonical offset 0 */
    *n = props[i].n_nums;
    return 1;
}

/* property_map_to_style.  row: OSMT_CS_ROW_WORDS words.  *text_key: the key index of text_style.text or OSMT_TEXT_NONE.
 * Returns whether the style has an icon or a text style (what a label draws something for). */
OSMT_HD bool osmt_cs_style_of(const osmt_cs_env& E, const uint32_t* row, const osmt_match_class& cls, osmt_style_rec* a, osmt_label_style_rec* l,
                              uint32_t* text_key) {
    const osmt_cs_prop* P = E.props;
    memset(a, 0, sizeof *a);
    memset(l, 0, sizeof *l);
    a->has_layer = l->has_layer = cls.has_layer ? 1 : 0;
    if (cls.has_layer) a->layer = l->layer = cls.layer;
    double z;
    if (!osmt_cs_num(P, row[OSMT_PROP_Z_INDEX], &z)) z = osmt_cs_default_z(cls.slot);
    a->z_index = l->z_index = z;
    {
        const uint32_t i = row[OSMT_PROP_FILL_POSITION];
        const bool background = i != OSMT_CS_NONE && P[i].kind == OSMT_PV_IDENTIFIER && (P[i].id_code & OSMT_CS_ID_BACKGROUND);
        a->is_foreground_fill = background ? 0 : 1;
    }
    double width = 0.0, base = 0.0;
    const bool has_width = osmt_cs_num(P, row[OSMT_PROP_WIDTH], &width);
    if (has_width)
        base = width;
    else if (!osmt_cs_num(P, row[OSMT_CS_ROW_BASE_WIDTH], &base))
        base = 0.0;
    a->has_width = has_width ? 1 : 0;
    if (has_width) a->width = width;
    {
        const uint32_t i = row[OSMT_PROP_CASING_WIDTH];
        double w = 0.0;
        bool has = false;
        if (i != OSMT_CS_NONE) {
            if (P[i].kind == OSMT_PV_NUMBERS && P[i].n_nums == 1u)
                has = true, w = P[i].num;
            else if (P[i].kind == OSMT_PV_WIDTH_DELTA)
                has = true, w = base + P[i].num;
        }
        if (has) {
            const double m = E.casing_width_multiplier * w; /* rounded here: no FMA (-ffp-contract=off) */
            a->has_casing_width = 1;
            a->casing_width = base + m;
        }
    }
    a->has_color = osmt_cs_color(P, row[OSMT_PROP_COLOR], a->color);
    a->has_fill_color = osmt_cs_color(P, row[OSMT_PROP_FILL_COLOR], a->fill_color);
    a->has_background_color = osmt_cs_color(P, row[OSMT_PROP_BACKGROUND_COLOR], a->background_color);
    a->has_casing_color = osmt_cs_color(P, row[OSMT_PROP_CASING_COLOR], a->casing_color);
    a->has_opacity = osmt_cs_num(P, row[OSMT_PROP_OPACITY], &a->opacity) ? 1 : 0;
    a->has_fill_opacity = osmt_cs_num(P, row[OSMT_PROP_FILL_OPACITY], &a->fill_opacity) ? 1 : 0;
    a->has_dashes = osmt_cs_dashes(P, row[OSMT_PROP_DASHES], &a->dashes_off, &a->n_dashes);
    a->has_casing_dashes = osmt_cs_dashes(P, row[OSMT_PROP_CASING_DASHES], &a->casing_dashes_off, &a->n_casing_dashes);
    a->line_cap = osmt_cs_cap(P, row[OSMT_PROP_LINECAP]);
    a->casing_line_cap = osmt_cs_cap(P, row[OSMT_PROP_CASING_LINECAP]);
    a->has_fill_image = osmt_cs_image(P, row[OSMT_PROP_FILL_IMAGE], &a->fill_image);
    l->has_icon = osmt_cs_image(P, row[OSMT_PROP_ICON_IMAGE], &l->icon_image);
    *text_key = OSMT_TEXT_NONE;
    {
        const uint32_t i = row[OSMT_PROP_TEXT];
        if (i != OSMT_CS_NONE && (P[i].kind == OSMT_PV_IDENTIFIER || P[i].kind == OSMT_PV_STRING)) {
            l->has_text_style = 1;
            *text_key = P[i].aux;
            double fs;
            if (osmt_cs_num(P, row[OSMT_PROP_FONT_SIZE], &fs)) {
                l->has_font_size = 1;
                l->font_size = fs * E.font_size_multiplier;
                l->font_id = E.font_id;
            }
            l->has_text_color = osmt_cs_color(P, row[OSMT_PROP_TEXT_COLOR], l->text_color);
            const uint32_t j = row[OSMT_PROP_TEXT_POSITION];
            if (j != OSMT_CS_NONE && P[j].kind == OSMT_PV_IDENTIFIER) l->text_position = (uint8_t)((P[j].id_code >> OSMT_CS_ID_POS_SHIFT) & 3u);
        }
    }
    return l->has_icon || l->has_text_style;
}

/* Style equality of two area records (up to the sign of a zero, as their bytes): every field but the dash offsets, then the
 * dashes themselves */
OSMT_HD bool osmt_cs_same_area(const osmt_style_rec& x, const osmt_style_rec& y, const double* numbers) {
    osmt_style_rec u = x, v = y;
    u.dashes_off = u.casing_dashes_off = v.dashes_off = v.casing_dashes_off = 0u;
    const uint64_t *p = (const uint64_t*)&u, *q = (const uint64_t*)&v;
    for (uint32_t i = 0; i < sizeof(osmt_style_rec) / 8u; ++i)
        if (p[i] != q[i]) return false;
    const uint64_t* nb = (const uint64_t*)numbers;
    for (uint32_t i = 0; i < x.n_dashes; ++i)
        if (nb[x.dashes_off + i] != nb[y.dashes_off + i]) return false;
    for (uint32_t i = 0; i < x.n_casing_dashes; ++i)
        if (nb[x.casing_dashes_off + i] != nb[y.casing_dashes_off + i]) return false;
    return true;
}
OSMT_HD bool osmt_cs_same_label(const osmt_label_style_rec& x, const osmt_label_style_rec& y) {
    const uint64_t *p = (const uint64_t*)&x, *q = (const uint64_t*)&y;
    for (uint32_t i = 0; i < sizeof(osmt_label_style_rec) / 8u; ++i)
        if (p[i] != q[i]) return false;
    return true;
}

#endif
