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
 *
 * Host only; compile with -ffp-contract=off like everything that must agree with the device bit for bit.
 */
#ifndef OSMT_SELMATCH_HPP
#define OSMT_SELMATCH_HPP

#include <cerrno>
#include <cstdlib>
#include <map>
#include <string>
#include <string_view>
#include <tuple>
#include <vector>

#include "../../include/osmtile.h"
#include "../csrc/osmt_numparse.h"
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

}  // namespace osmt
#endif
