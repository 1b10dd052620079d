/*
 * osmt_cascade.hpp — the host side of the cascade (include/osmtile.h, "the cascade"):
 *
 *   osmt::RuleSet       builds an osmt_rules_desc over a selector set, fed rule by rule with selector layers and properties
 *                       as the reference's parser has them (mapcss/parser.rs: Rule { selectors, properties })
 *   osmt::cascade_host  a plain sequential statement of what osmt_cascade_classes computes, producing exactly the arrays
 *                       osmt_cascade_read returns
 *
 * The fold is written with a list of layers in insertion order, as Styler::style_area has its IndexMap
 * (styler.rs:205-242).  Turning a layer's last writers into the two records is osmt_cs_style_of of csrc/osmt_cascade_rule.h,
 * the one statement of property_map_to_style the kernels use too; tests hold both against a restatement in Python.
 */
#ifndef OSMT_CASCADE_HPP
#define OSMT_CASCADE_HPP

#include <array>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/osmtile.h"
#include "../csrc/osmt_cascade_tables.h"

namespace osmt {

/* "z-index" -> OSMT_PROP_Z_INDEX ...; any other name is OSMT_PROP_OTHER */
inline uint8_t prop_name_of(std::string_view name) {
    static const char* const names[OSMT_PROP_NAMES] = {"z-index",   "fill-position", "width",         "casing-width",     "text",    "font-size", "text-color",
                                                       "text-position", "color",     "fill-color",    "background-color", "opacity", "fill-opacity", "dashes",
                                                       "linecap",   "casing-color",  "casing-dashes", "casing-linecap",   "icon-image", "fill-image"};
    for (uint8_t i = 0; i < OSMT_PROP_NAMES; ++i)
        if (name == names[i]) return i;
    return OSMT_PROP_OTHER;
}

/* Rules in stylesheet order: rule() starts one, selector() names the layer of its next selector (the selectors are those of
 * the SelectorSet, in the same order), then the properties in file order. */
class RuleSet {
  public:
    void rule() { rule_prop_off_.push_back((uint32_t)props_.size()); }
    /* layer: the selector's `::layer`, or nothing */
    void selector(const std::optional<std::string_view>& layer = std::nullopt) {
        need_rule();
        sel_rule_.push_back((uint32_t)rule_prop_off_.size() - 1u);
        if (!layer) {
            sel_layer_.push_back(OSMT_LAYER_DEFAULT);
            return;
        }
        sel_layer_.push_back((uint32_t)layer_off_.size() - 1u);
        layer_bytes_.append(*layer);
        layer_off_.push_back((uint32_t)layer_bytes_.size());
    }
    /* color: from_color_name(id), resolved by the caller; image: the registered icon of the string, for icon-image / fill-image */
    void identifier(std::string_view name, std::string_view id, const std::optional<std::array<uint8_t, 3>>& color = std::nullopt,
                    const std::optional<uint32_t>& image = std::nullopt) {
        osmt_rule_prop p = start(name, OSMT_PV_IDENTIFIER);
        stringy(p, id, image);
        if (color) p.has_color = 1, p.rgb[0] = (*color)[0], p.rgb[1] = (*color)[1], p.rgb[2] = (*color)[2];
        props_.push_back(p);
    }
    void string(std::string_view name, std::string_view s, const std::optional<uint32_t>& image = std::nullopt) {
        osmt_rule_prop p = start(name, OSMT_PV_STRING);
        stringy(p, s, image);
        props_.push_back(p);
    }
    void color(std::string_view name, uint8_t r, uint8_t g, uint8_t b) {
        osmt_rule_prop p = start(name, OSMT_PV_COLOR);
        p.has_color = 1, p.rgb[0] = r, p.rgb[1] = g, p.rgb[2] = b;
        props_.push_back(p);
    }
    void numbers(std::string_view name, const std::vector<double>& v) {
        osmt_rule_prop p = start(name, OSMT_PV_NUMBERS);
        p.num_off = (uint32_t)numbers_.size(), p.n_nums = (uint32_t)v.size();
        numbers_.insert(numbers_.end(), v.begin(), v.end());
        props_.push_back(p);
    }
    void width_delta(std::string_view name, double d) {
        osmt_rule_prop p = start(name, OSMT_PV_WIDTH_DELTA);
        p.delta = d;
        props_.push_back(p);
    }
    /* valid until the next call that adds something or the end of this object */
    const osmt_rules_desc& desc(uint32_t selectors_id, double casing_width_multiplier, const std::optional<double>& font_size_multiplier, uint32_t font_id) {
        off_ = rule_prop_off_;
        off_.push_back((uint32_t)props_.size());
        desc_.selectors_id = selectors_id, desc_.font_id = font_id;
        desc_.selector_rule = sel_rule_.data(), desc_.selector_layer = sel_layer_.data(), desc_.n_selectors = sel_rule_.size();
        desc_.layer_off = layer_off_.data(), desc_.layer_bytes = (const uint8_t*)layer_bytes_.data();
        desc_.n_layers = layer_off_.size() - 1, desc_.n_layer_bytes = layer_bytes_.size();
        desc_.rule_prop_off = off_.data(), desc_.props = props_.data(), desc_.n_rules = off_.size() - 1, desc_.n_props = props_.size();
        desc_.numbers = numbers_.data(), desc_.n_numbers = numbers_.size();
        desc_.strings = (const uint8_t*)strings_.data(), desc_.n_string_bytes = strings_.size();
        desc_.casing_width_multiplier = casing_width_multiplier;
        desc_.has_font_size_multiplier = font_size_multiplier ? 1u : 0u;
        desc_.font_size_multiplier = font_size_multiplier.value_or(0.0);
        return desc_;
    }
    /* OSMT_RULES_CLASS_LAYERS: up to OSMT_CASCADE_MAX_LAYER_NAMES names, at most OSMT_CASCADE_MAX_CLASS_LAYERS layers per class */
    void class_layers(bool on) { flags_ = on ? OSMT_RULES_CLASS_LAYERS : 0u; }
    uint32_t flags() const { return flags_; }
    /* the last desc() through the library with this set's flags (for callers that link it) */
    int validate(osmt_ctx* ctx) const { return osmt_validate_rules_ex(&desc_, flags_, ctx); }
    int register_in(osmt_ctx* ctx, uint32_t* out_rules_id) const { return osmt_register_rules_ex(ctx, &desc_, flags_, out_rules_id); }

  private:
    void need_rule() const {
        if (rule_prop_off_.empty()) throw std::logic_error("RuleSet: rule() comes first");
    }
    osmt_rule_prop start(std::string_view name, uint8_t kind) {
        need_rule();
        osmt_rule_prop p{};
        p.name = prop_name_of(name), p.kind = kind;
        return p;
    }
    void stringy(osmt_rule_prop& p, std::string_view s, const std::optional<uint32_t>& image) {
        p.str_off = (uint32_t)strings_.size(), p.str_len = (uint32_t)s.size();
        strings_.append(s);
        if (image && (p.name == OSMT_PROP_ICON_IMAGE || p.name == OSMT_PROP_FILL_IMAGE)) p.has_image = 1, p.image = *image;
    }
    std::vector<uint32_t> rule_prop_off_, off_, sel_rule_, sel_layer_, layer_off_{0u};
    std::vector<osmt_rule_prop> props_;
    std::vector<double> numbers_;
    std::string strings_, layer_bytes_;
    osmt_rules_desc desc_{};
    uint32_t flags_ = 0u;
};

/* the arrays of osmt_cascade_read */
struct HostCascade {
    std::vector<osmt_style_rec> styles;
    std::vector<double> dashes;
    std::vector<osmt_label_style_rec> label_styles;
    std::vector<uint8_t> key_bytes;
    std::vector<uint32_t> key_off;
    std::vector<uint8_t> zoom_lo, zoom_hi;
    std::vector<uint32_t> class_style_off, class_styles, range_style_base;
    std::vector<uint32_t> class_off, range_binding_base;
    std::vector<osmt_class_label_binding> bindings;
};

/* `rules` has passed osmt_validate_rules and is over `selectors`; `classes` / `class_selectors` are a match's. */
inline HostCascade cascade_host(const osmt_rules_desc& rules, const osmt_selectors_desc& selectors, const osmt_match_class* classes, size_t n_classes,
                                const uint32_t* class_selectors, bool labels_all) {
    osmt_cs_tables T;
    size_t n_names = 0;
    osmt_cs_resolve(rules, T, &n_names);
    if (n_names > 255) throw std::runtime_error("cascade_host: more than 255 layer names"); /* the mirror is not bound by OSMT_CASCADE_MAX_LAYERS */
    osmt_cs_env E{T.props.data(), rules.casing_width_multiplier, rules.has_font_size_multiplier ? rules.font_size_multiplier : 1.0, rules.font_id};
    HostCascade H;
    H.key_off = T.key_off, H.key_bytes = T.key_bytes;
    using Row = std::array<uint32_t, OSMT_PROP_NAMES>;
    struct Layer {
        uint32_t name;
        Row last;
    };
    /* distinct records by their bytes, dashes by value; ids in order of first appearance = lowest user */
    std::map<std::string, uint32_t> area_ids, label_ids;
    struct Entry {
        uint32_t style, label, key; /* label: OSMT_CS_NONE when the style is no binding */
    };
    std::vector<std::vector<Entry>> lists(n_classes * OSMT_CS_ZOOMS);
    for (size_t c = 0; c < n_classes; ++c)
        for (uint32_t zoom = 0; zoom < OSMT_CS_ZOOMS; ++zoom) {
            std::vector<Layer> layers; /* the IndexMap of style_area */
            auto find = [&](uint32_t name) -> Layer* {
                for (Layer& l : layers)
                    if (l.name == name) return &l;
                return nullptr;
            };
            for (uint32_t i = 0; i < classes[c].n_sels; ++i) {
                const uint32_t s = class_selectors[classes[c].sel_off + i];
                const osmt_selector_rec& sel = selectors.selectors[s];
                if ((sel.has_min_zoom && zoom < sel.min_zoom) || (sel.has_max_zoom && zoom > sel.max_zoom)) continue;
                const uint32_t name = T.sel_layer[s];
                const uint32_t* rule = T.rule_last.data() + (size_t)rules.selector_rule[s] * OSMT_PROP_NAMES;
                auto update = [&](Layer& l) {
                    for (uint32_t k = 0; k < OSMT_PROP_NAMES; ++k)
                        if (rule[k] != OSMT_CS_NONE) l.last[k] = rule[k];
                };
                if (!find(name)) {
                    Layer fresh{name, {}};
                    fresh.last.fill(OSMT_CS_NONE);
                    if (const Layer* parent = T.star != OSMT_CS_NONE ? find(T.star) : nullptr) fresh.last = parent->last;
                    layers.push_back(fresh);
                }
                update(*find(name));
                if (name == T.star)
                    for (Layer& l : layers)
                        if (l.name != T.star) update(l);
            }
            const Layer* base = T.base != OSMT_CS_NONE ? find(T.base) : nullptr;
            uint32_t position = 0;
            for (const Layer& l : layers) {
                if (l.name == T.star) continue;
                uint32_t row[OSMT_CS_ROW_WORDS];
                for (uint32_t k = 0; k < OSMT_PROP_NAMES; ++k) row[k] = l.last[k];
                row[OSMT_CS_ROW_BASE_WIDTH] = base ? base->last[OSMT_PROP_WIDTH] : OSMT_CS_NONE;
                row[OSMT_CS_ROW_PAIR] = (uint32_t)(c * OSMT_CS_ZOOMS + zoom), row[OSMT_CS_ROW_POSITION] = position++;
                osmt_style_rec a;
                osmt_label_style_rec lab;
                uint32_t key;
                const bool draws = osmt_cs_style_of(E, row, classes[c], &a, &lab, &key);
                /* the dashes of the record's canonical key by value, its offsets left out */
                osmt_style_rec k = a;
                k.dashes_off = k.casing_dashes_off = 0;
                std::string bytes((const char*)&k, sizeof k);
                bytes.append((const char*)(rules.numbers + a.dashes_off), a.n_dashes * 8u);
                bytes.append((const char*)(rules.numbers + a.casing_dashes_off), a.n_casing_dashes * 8u);
                auto it = area_ids.find(bytes);
                if (it == area_ids.end()) {
                    it = area_ids.emplace(bytes, (uint32_t)H.styles.size()).first;
                    if (a.n_dashes) {
                        const double* src = rules.numbers + a.dashes_off;
                        a.dashes_off = (uint32_t)H.dashes.size();
                        H.dashes.insert(H.dashes.end(), src, src + a.n_dashes);
                    }
                    if (a.n_casing_dashes) {
                        const double* src = rules.numbers + a.casing_dashes_off;
                        a.casing_dashes_off = (uint32_t)H.dashes.size();
                        H.dashes.insert(H.dashes.end(), src, src + a.n_casing_dashes);
                    }
                    H.styles.push_back(a);
                }
                Entry e{it->second, OSMT_CS_NONE, key};
                if (labels_all || draws) {
                    const std::string lb((const char*)&lab, sizeof lab);
                    auto jt = label_ids.find(lb);
                    if (jt == label_ids.end()) {
                        jt = label_ids.emplace(lb, (uint32_t)H.label_styles.size()).first;
                        H.label_styles.push_back(lab);
                    }
                    e.label = jt->second;
                }
                lists[c * OSMT_CS_ZOOMS + zoom].push_back(e);
            }
        }
    /* a zoom joins the range of the zoom below iff every class has the same two lists at both */
    auto same = [&](const std::vector<Entry>& x, const std::vector<Entry>& y) {
        if (x.size() != y.size()) return false;
        for (size_t i = 0; i < x.size(); ++i)
            if (x[i].style != y[i].style) return false;
        std::vector<std::pair<uint32_t, uint32_t>> bx, by;
        for (const Entry& e : x)
            if (e.label != OSMT_CS_NONE) bx.emplace_back(e.label, e.key);
        for (const Entry& e : y)
            if (e.label != OSMT_CS_NONE) by.emplace_back(e.label, e.key);
        return bx == by;
    };
    for (uint32_t zoom = 0; zoom < OSMT_CS_ZOOMS; ++zoom) {
        bool joins = zoom > 0;
        for (size_t c = 0; c < n_classes && joins; ++c) joins = same(lists[c * OSMT_CS_ZOOMS + zoom - 1], lists[c * OSMT_CS_ZOOMS + zoom]);
        if (joins) {
            H.zoom_hi.back() = (uint8_t)zoom;
        } else {
            H.zoom_lo.push_back((uint8_t)zoom);
            H.zoom_hi.push_back((uint8_t)zoom);
        }
    }
    H.range_style_base.push_back(0u), H.range_binding_base.push_back(0u);
    for (size_t r = 0; r < H.zoom_lo.size(); ++r) {
        const size_t s0 = H.class_styles.size(), b0 = H.bindings.size();
        for (size_t c = 0; c < n_classes; ++c) {
            H.class_style_off.push_back((uint32_t)(H.class_styles.size() - s0));
            H.class_off.push_back((uint32_t)(H.bindings.size() - b0));
            for (const Entry& e : lists[c * OSMT_CS_ZOOMS + H.zoom_lo[r]]) {
                H.class_styles.push_back(e.style);
                if (e.label != OSMT_CS_NONE) H.bindings.push_back(osmt_class_label_binding{e.label, e.key});
            }
        }
        H.class_style_off.push_back((uint32_t)(H.class_styles.size() - s0));
        H.class_off.push_back((uint32_t)(H.bindings.size() - b0));
        H.range_style_base.push_back((uint32_t)H.class_styles.size());
        H.range_binding_base.push_back((uint32_t)H.bindings.size());
    }
    return H;
}

}  // namespace osmt

#endif
