/*
 * osmt_selmatch.hpp — host side of selector matching (include/osmtile.h "style bindings from tags"):
 *
 *   SelectorSet            builder that fills an osmt_selectors_desc, selectors in stylesheet order
 *   match_selectors_host   the literal restatement of area_matches / matches_by_tags (mapcss/styler.rs:450-520) over
 *                          Tags::get_by_key, with the class numbering of osmt_match_read: the yardstick of the GPU tests and
 *                          the figure a caller's per-entity loop is compared with
 *   parse_f64 / parse_i64  str::parse::<f64> (Rust's grammar check, then a correctly rounded conversion) and
 *                          str::parse::<i64>
 *   number_fast_path       the device's rule "exact by construction, else declined" (csrc/osmt_numparse.h), stated once
 *   HostNumbers            the overrides for the values osmt_match_selectors declined
 *   selectors_at_zoom      the zoom filter of area_matches, applied by the caller per class before it cascades
 *   ClassLabelBindings     builder that fills an osmt_class_label_bindings_desc and pools the text keys
 *   label_bindings_matched_host / area_label_bindings_matched_host
 *                          the rule of osmt_register_label_bindings_matched / osmt_register_area_label_bindings_matched in
 *                          plain C++: the arrays osmt_read_label_bindings / osmt_read_area_label_bindings return
 *
 * Host only; compile with -ffp-contract=off like everything that must agree with the device bit for bit.
 */
#ifndef OSMT_SELMATCH_HPP
#define OSMT_SELMATCH_HPP

#include <cerrno>
#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <string_view>
#include <tuple>
#include <vector>

#include "../../include/osmtile.h"
#include "../csrc/osmt_numparse.h"
#include "../csrc/osmt_utf8.h"
#include "osmt_geodata.hpp"

namespace osmt {

/* str::parse::<f64>: Sign? ( inf | infinity | nan | Number ), Number ::= (Digit+ | Digit+ '.' Digit* | Digit* '.' Digit+) Exp?,
 * Exp ::= 'e' Sign? Digit+, case-insensitive; then strtod, which glibc rounds correctly, as Rust does */
inline bool parse_f64(std::string_view s, double* out) {
    size_t i = 0;
    const size_t n = s.size();
    auto lower = [](char c) { return (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; };
    auto word = [&](size_t from, const char* w) {
        size_t k = 0;
        for (; w[k]; ++k)
            if (from + k >= n || lower(s[from + k]) != w[k]) return false;
        return from + k == n;
    };
    auto digit = [&](size_t k) { return k < n && s[k] >= '0' && s[k] <= '9'; };
    if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
    if (i == n) return false;
    const bool special = word(i, "inf") || word(i, "infinity") || word(i, "nan");
    if (!special) {
        size_t n_int = 0, n_frac = 0;
        while (digit(i)) ++i, ++n_int;
        if (i < n && s[i] == '.') {
            ++i;
            while (digit(i)) ++i, ++n_frac;
        }
        if (n_int + n_frac == 0) return false;
        if (i < n) {
            if (s[i] != 'e' && s[i] != 'E') return false;
            ++i;
            if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
            if (!digit(i)) return false;
            while (digit(i)) ++i;
            if (i != n) return false;
        }
    }
    const std::string z(s); /* the grammar admits nothing strtod reads differently (no hex, no whitespace, no locale point in "C") */
    char* end = nullptr;
    *out = std::strtod(z.c_str(), &end);
    return end == z.c_str() + z.size();
}

/* str::parse::<i64>: [+-]? Digit+, an error on overflow */
inline bool parse_i64(std::string_view s, int64_t* out) {
    size_t i = 0;
    bool neg = false;
    if (!s.empty() && (s[0] == '+' || s[0] == '-')) neg = s[0] == '-', i = 1;
    if (i == s.size()) return false;
    __int128 v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (s[i] - '0');
        if (v > ((__int128)1 << 63)) return false;
    }
    if (neg) v = -v;
    if (v > (__int128)INT64_MAX || v < (__int128)INT64_MIN) return false;
    *out = (int64_t)v;
    return true;
}

/* the device's rule: OSMT_NUM_OK with the exact value, OSMT_NUM_ERROR for a grammar error, OSMT_NUM_DECLINED otherwise */
inline int number_fast_path(std::string_view s, double* out) { return osmt_parse_f64_fast((const uint8_t*)s.data(), (uint32_t)s.size(), out); }

/* the values osmt_match_selectors declined, computed here: Rust's grammar check, then a correctly rounded conversion */
struct HostNumbers {
    std::vector<osmt_number_override> overrides; /* ascending by (v_off, v_len), as `declined` is */

    HostNumbers() = default;
    HostNumbers(const uint8_t* strings, const osmt_declined_number* declined, size_t n) {
        overrides.resize(n);
        for (size_t i = 0; i < n; ++i) {
            osmt_number_override o{};
            o.v_off = declined[i].v_off, o.v_len = declined[i].v_len;
            double v = 0.0;
            o.has_value = parse_f64(std::string_view((const char*)strings + o.v_off, o.v_len), &v) ? 1u : 0u;
            o.value = o.has_value ? v : 0.0;
            overrides[i] = o;
        }
    }
};

/* selectors in stylesheet order: add() starts one, test() appends to the last one */
class SelectorSet {
  public:
    size_t add(uint8_t object_type, int min_zoom = -1, int max_zoom = -1) {
        osmt_selector_rec r{};
        r.object_type = object_type;
        r.has_min_zoom = min_zoom >= 0, r.min_zoom = (uint8_t)(min_zoom >= 0 ? min_zoom : 0);
        r.has_max_zoom = max_zoom >= 0, r.max_zoom = (uint8_t)(max_zoom >= 0 ? max_zoom : 0);
        r.test_off = (uint32_t)tests_.size();
        sels_.push_back(r);
        return sels_.size() - 1;
    }
    void test(uint32_t kind, std::string_view key, std::string_view value = {}, double number = 0.0) {
        osmt_selector_test t{};
        t.kind = kind;
        t.key_off = put(key), t.key_len = (uint32_t)key.size();
        if (kind == OSMT_TEST_EQUAL || kind == OSMT_TEST_NOT_EQUAL) t.value_off = put(value), t.value_len = (uint32_t)value.size();
        t.value = number;
        tests_.push_back(t);
        ++sels_.back().n_tests;
    }
    const osmt_selectors_desc& desc() {
        desc_.selectors = sels_.data(), desc_.n_selectors = sels_.size();
        desc_.tests = tests_.data(), desc_.n_tests = tests_.size();
        desc_.strings = (const uint8_t*)strings_.data(), desc_.n_string_bytes = strings_.size();
        return desc_;
    }

  private:
    uint32_t put(std::string_view s) {
        const uint32_t off = (uint32_t)strings_.size();
        strings_.append(s);
        return off;
    }
    std::vector<osmt_selector_rec> sels_;
    std::vector<osmt_selector_test> tests_;
    std::string strings_;
    osmt_selectors_desc desc_{};
};

/* matches_by_tags (styler.rs:450-499) */
inline bool test_matches(const Tags& tags, const osmt_selectors_desc& d, const osmt_selector_test& t) {
    const std::string_view key((const char*)d.strings + t.key_off, t.key_len);
    std::string_view v;
    const bool present = tags.get_by_key(key, &v);
    auto is_true_value = [](std::string_view x) { return x == "yes" || x == "true" || x == "1"; };
    switch (t.kind) {
        case OSMT_TEST_EXISTS: return present;
        case OSMT_TEST_NOT_EXISTS: return !present;
        case OSMT_TEST_TRUE: return present && is_true_value(v);
        case OSMT_TEST_FALSE: return !(present && is_true_value(v));
        case OSMT_TEST_EQUAL: return present && v == std::string_view((const char*)d.strings + t.value_off, t.value_len);
        case OSMT_TEST_NOT_EQUAL: return !(present && v == std::string_view((const char*)d.strings + t.value_off, t.value_len));
        default: break;
    }
    double x = 0.0;
    if (!present || !parse_f64(v, &x)) return false;
    switch (t.kind) {
        case OSMT_TEST_LESS: return x < t.value;
        case OSMT_TEST_LESS_OR_EQUAL: return x <= t.value;
        case OSMT_TEST_GREATER: return x > t.value;
        default: return x >= t.value;
    }
}

struct HostMatch {
    std::vector<uint32_t> entity_class; /* nodes, then ways, then multipolygons */
    std::vector<osmt_match_class> classes;
    std::vector<uint32_t> class_selectors;
};

/* area_matches without its zoom test (styler.rs:501-520) for every entity and selector; cache slots of styler.rs:559-579;
 * classes numbered by their lowest-numbered member */
inline HostMatch match_selectors_host(const GeodataReader& r, const osmt_selectors_desc& d) {
    HostMatch out;
    using key_t = std::tuple<uint8_t, uint8_t, int64_t, std::vector<uint32_t>>;
    std::map<key_t, uint32_t> seen;
    const size_t n_nodes = r.node_count(), n_ways = r.way_count(), n_mps = r.multipolygon_count();
    std::vector<uint32_t> matched;
    for (size_t e = 0; e < n_nodes + n_ways + n_mps; ++e) {
        const bool node = e < n_nodes, way = !node && e < n_nodes + n_ways;
        const Tags tags = node ? r.node_tags(e) : way ? r.way_tags(e - n_nodes) : r.multipolygon_tags(e - n_nodes - n_ways);
        const bool closed = node ? false : way ? r.way_is_closed(e - n_nodes) : true;
        const uint8_t slot = node ? 0 : way ? (closed ? 1 : 2) : 3;
        matched.clear();
        for (size_t s = 0; s < d.n_selectors; ++s) {
            const osmt_selector_rec& sel = d.selectors[s];
            const bool good_type = node ? sel.object_type == OSMT_SEL_NODE : (sel.object_type == OSMT_SEL_WAY || (sel.object_type == OSMT_SEL_AREA && closed));
            if (!good_type) continue;
            bool all = true;
            for (uint32_t j = 0; all && j < sel.n_tests; ++j) all = test_matches(tags, d, d.tests[sel.test_off + j]);
            if (all) matched.push_back((uint32_t)s);
        }
        std::string_view lv;
        int64_t layer = 0;
        const bool has_layer = tags.get_by_key("layer", &lv) && parse_i64(lv, &layer);
        if (!has_layer) layer = 0;
        const auto ins = seen.emplace(key_t{slot, (uint8_t)has_layer, layer, matched}, (uint32_t)out.classes.size());
        if (ins.second) {
            osmt_match_class c{};
            c.layer = layer;
            c.sel_off = (uint32_t)out.class_selectors.size(), c.n_sels = (uint32_t)matched.size();
            c.first_entity = (uint32_t)e;
            c.slot = slot, c.has_layer = has_layer;
            out.classes.push_back(c);
            out.class_selectors.insert(out.class_selectors.end(), matched.begin(), matched.end());
        }
        out.entity_class.push_back(ins.first->second);
    }
    return out;
}

/* the zoom filter of area_matches (styler.rs:505-515) over a class's selectors: what the caller cascades at `zoom` */
inline std::vector<uint32_t> selectors_at_zoom(const osmt_selectors_desc& d, const uint32_t* class_selectors, size_t n, uint8_t zoom) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < n; ++i) {
        const osmt_selector_rec& s = d.selectors[class_selectors[i]];
        if (s.has_min_zoom && zoom < s.min_zoom) continue;
        if (s.has_max_zoom && zoom > s.max_zoom) continue;
        out.push_back(class_selectors[i]);
    }
    return out;
}

/* label bindings per class: add_class() starts the list of the next class, bind() appends to it; equal keys share one entry */
class ClassLabelBindings {
  public:
    ClassLabelBindings(uint8_t zoom_lo, uint8_t zoom_hi) { desc_.zoom_lo = zoom_lo, desc_.zoom_hi = zoom_hi; }
    void add_class() { off_.push_back((uint32_t)bindings_.size()); }
    /* a style without text: has_key = false */
    void bind(uint32_t style, std::string_view text_key, bool has_key = true) {
        osmt_class_label_binding b{};
        b.style = style, b.text_key = has_key ? key(text_key) : OSMT_TEXT_NONE;
        bindings_.push_back(b);
        off_.back() = (uint32_t)bindings_.size();
    }
    const osmt_class_label_bindings_desc& desc() {
        desc_.class_off = off_.data(), desc_.bindings = bindings_.data();
        desc_.n_classes = off_.size() - 1, desc_.n_bindings = bindings_.size();
        desc_.key_off = key_off_.data(), desc_.key_bytes = (const uint8_t*)key_bytes_.data();
        desc_.n_keys = key_off_.size() - 1, desc_.n_key_bytes = key_bytes_.size();
        return desc_;
    }

  private:
    uint32_t key(std::string_view k) {
        const auto ins = ids_.emplace(std::string(k), (uint32_t)ids_.size());
        if (ins.second) {
            key_bytes_.append(k);
            key_off_.push_back((uint32_t)key_bytes_.size());
        }
        return ins.first->second;
    }
    std::vector<uint32_t> off_{0u}, key_off_{0u};
    std::vector<osmt_class_label_binding> bindings_;
    std::string key_bytes_;
    std::map<std::string, uint32_t> ids_;
    osmt_class_label_bindings_desc desc_{};
};

/* what osmt_read_label_bindings (kind 0 = nodes) or osmt_read_area_label_bindings (kind 0 = ways, 1 = multipolygons) return */
struct HostLabelTable {
    bool ok = true; /* false: a used value is not well-formed UTF-8; bad_* name the lowest-numbered such tag, the arrays are empty */
    const char* bad_kind = nullptr;
    size_t bad_entity = 0, bad_tag = 0; /* the entity within its kind; the tag within the entity */
    uint32_t bad_v_off = 0, bad_v_len = 0;
    std::vector<uint32_t> off[2];
    std::vector<osmt_label_binding> bindings[2];
    std::vector<uint32_t> text_off{0u}, chars;
};

namespace labelbind_detail {
struct Kind {
    const char* name;
    size_t first, count; /* in the numbering of entity_class: nodes, then ways, then multipolygons */
};

inline Tags tags_of(const osmt_tags_desc& t, size_t e) {
    const uint32_t *off = t.node_tag_off, *kv = t.node_tags;
    if (e >= t.n_nodes + t.n_ways)
        e -= t.n_nodes + t.n_ways, off = t.multipolygon_tag_off, kv = t.multipolygon_tags;
    else if (e >= t.n_nodes)
        e -= t.n_nodes, off = t.way_tag_off, kv = t.way_tags;
    return Tags(kv + 4 * (size_t)off[e], 4 * (size_t)(off[e + 1] - off[e]), (const char*)t.strings);
}

/* The rule, kind after kind, entity after entity: every element of the class's list is pushed; its text is the value of the
 * tag whose key equals the key's bytes.  A text is a distinct (v_off, v_len) among the USED tags, numbered by its lowest user in
 * the table's tag order; every used value must be well-formed UTF-8. */
inline HostLabelTable table(const osmt_tags_desc& r, const uint32_t* entity_class, const osmt_class_label_bindings_desc& d, const Kind* kinds, int n_kinds) {
    HostLabelTable out;
    struct Use {
        int kind;
        size_t entity, tag, number; /* number: the tag's in the table */
    };
    using range_t = std::pair<uint32_t, uint32_t>;
    std::map<range_t, Use> lowest; /* value range -> its lowest-numbered user */
    std::vector<range_t> provisional[2]; /* per binding its value range; (NONE, NONE): no text */
    const range_t none{OSMT_TEXT_NONE, OSMT_TEXT_NONE};
    size_t tag_number = 0;
    for (int k = 0; k < n_kinds; ++k) {
        out.off[k].push_back(0u);
        for (size_t i = 0; i < kinds[k].count; ++i) {
            const Tags tags = tags_of(r, kinds[k].first + i);
            const uint32_t c = entity_class[kinds[k].first + i];
            for (uint32_t j = d.class_off[c]; j < d.class_off[c + 1]; ++j) {
                const osmt_class_label_binding& b = d.bindings[j];
                range_t found = none;
                if (b.text_key != OSMT_TEXT_NONE) {
                    const std::string_view key((const char*)d.key_bytes + d.key_off[b.text_key], d.key_off[b.text_key + 1] - d.key_off[b.text_key]);
                    /* the keys of an entity are distinct: at most one tag has the key, however it is searched for */
                    for (size_t t = 0; t < tags.size(); ++t)
                        if (tags.get_kv(t).first == key) {
                            found = range_t{tags.raw()[4 * t + 2], tags.raw()[4 * t + 3]};
                            const Use u{k, i, t, tag_number + t};
                            const auto ins = lowest.emplace(found, u);
                            if (!ins.second && u.number < ins.first->second.number) ins.first->second = u;
                        }
                }
                out.bindings[k].push_back(osmt_label_binding{b.style, OSMT_TEXT_NONE});
                provisional[k].push_back(found);
            }
            out.off[k].push_back((uint32_t)out.bindings[k].size());
            tag_number += tags.size();
        }
    }
    /* the texts in the order of their lowest users */
    std::vector<std::pair<size_t, range_t>> order;
    for (const auto& kv : lowest) order.push_back({kv.second.number, kv.first});
    std::sort(order.begin(), order.end());
    std::map<range_t, uint32_t> id;
    for (const auto& o : order) {
        const range_t v = o.second;
        const uint8_t* s = r.strings + v.first;
        uint32_t n_scalars = 0;
        if (osmt_utf8_validate(s, v.second, &n_scalars) != v.second) {
            const Use& u = lowest[v];
            HostLabelTable bad;
            bad.ok = false, bad.bad_kind = kinds[u.kind].name, bad.bad_entity = u.entity, bad.bad_tag = u.tag;
            bad.bad_v_off = v.first, bad.bad_v_len = v.second;
            bad.text_off.clear();
            return bad; /* `order` ascends by tag number: this is the lowest-numbered offender */
        }
        id[v] = (uint32_t)out.text_off.size() - 1u;
        const size_t at = out.chars.size();
        out.chars.resize(at + n_scalars);
        osmt_utf8_decode(s, v.second, out.chars.data() + at);
        out.text_off.push_back((uint32_t)out.chars.size());
    }
    for (int k = 0; k < n_kinds; ++k)
        for (size_t j = 0; j < provisional[k].size(); ++j)
            if (provisional[k][j] != none) out.bindings[k][j].text = id[provisional[k][j]];
    return out;
}
}  // namespace labelbind_detail

/* osmt_register_label_bindings_matched, on the host: `tags` as osmt_register_tags took them (osmt::TagsDesc over a reader),
 * entity_class as osmt_match_read returns it (or HostMatch::entity_class) */
inline HostLabelTable label_bindings_matched_host(const osmt_tags_desc& tags, const uint32_t* entity_class, const osmt_class_label_bindings_desc& d) {
    const labelbind_detail::Kind kinds[1] = {{"node", 0, tags.n_nodes}};
    return labelbind_detail::table(tags, entity_class, d, kinds, 1);
}

/* osmt_register_area_label_bindings_matched, on the host: the way tags are numbered in front of the multipolygon tags */
inline HostLabelTable area_label_bindings_matched_host(const osmt_tags_desc& tags, const uint32_t* entity_class, const osmt_class_label_bindings_desc& d) {
    const labelbind_detail::Kind kinds[2] = {{"way", tags.n_nodes, tags.n_ways}, {"multipolygon", tags.n_nodes + tags.n_ways, tags.n_multipolygons}};
    return labelbind_detail::table(tags, entity_class, d, kinds, 2);
}

/* the C calls over the builder and the table struct (these four need libosmtile) */
inline int register_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, ClassLabelBindings& b, uint32_t* out_id) {
    return osmt_register_label_bindings_matched(ctx, match, &b.desc(), out_id);
}
inline int register_area_label_bindings_matched(osmt_ctx* ctx, osmt_match* match, ClassLabelBindings& b, uint32_t* out_id) {
    return osmt_register_area_label_bindings_matched(ctx, match, &b.desc(), out_id);
}
inline int read_label_bindings(osmt_ctx* ctx, uint32_t id, size_t n_nodes, HostLabelTable* out) {
    size_t n[3] = {};
    int rc = osmt_read_label_bindings(ctx, id, nullptr, nullptr, nullptr, nullptr, nullptr, n);
    if (rc != OSMT_OK) return rc;
    out->off[0].assign(n_nodes + 1, 0u), out->bindings[0].assign(n[0], osmt_label_binding{}), out->text_off.assign(n[1] + 1, 0u), out->chars.assign(n[2], 0u);
    return osmt_read_label_bindings(ctx, id, out->off[0].data(), out->bindings[0].data(), out->text_off.data(), out->chars.data(), n, n);
}
inline int read_area_label_bindings(osmt_ctx* ctx, uint32_t id, size_t n_ways, size_t n_multipolygons, HostLabelTable* out) {
    size_t n[4] = {};
    int rc = osmt_read_area_label_bindings(ctx, id, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n);
    if (rc != OSMT_OK) return rc;
    out->off[0].assign(n_ways + 1, 0u), out->off[1].assign(n_multipolygons + 1, 0u);
    out->bindings[0].assign(n[0], osmt_label_binding{}), out->bindings[1].assign(n[1], osmt_label_binding{});
    out->text_off.assign(n[2] + 1, 0u), out->chars.assign(n[3], 0u);
    return osmt_read_area_label_bindings(ctx, id, out->off[0].data(), out->bindings[0].data(), out->off[1].data(), out->bindings[1].data(),
                                         out->text_off.data(), out->chars.data(), n, n);
}

}  // namespace osmt
#endif
