/*
 * osmt_cascade_tables.h — host only: osmt_rules_desc -> the tables the cascade's kernels read (osmt_cs_resolve), used by the
 * registration (osmt_api.cpp) and by the host mirror (host/osmt_cascade.hpp): the properties as osmt_cs_prop, rule x name ->
 * last property, the layer index of every selector, the pooled text keys.
 */
#ifndef OSMT_CASCADE_TABLES_H
#define OSMT_CASCADE_TABLES_H

#include "osmt_cascade_rule.h"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

/* the device tables of a rule set, made on the host at registration (and by the mirror) */
struct osmt_cs_tables {
    std::vector<osmt_cs_prop> props;       /* the properties with one of the 20 names, file order */
    std::vector<uint32_t> rule_last;       /* [n_rules][20] index into props of the rule's last property of the name, or NONE */
    std::vector<uint8_t> sel_layer;        /* [n_selectors] the layer of the selector, 0 .. n_layers - 1 */
    uint32_t n_layers = 0, star = OSMT_CS_NONE, base = OSMT_CS_NONE; /* distinct names used by selectors; "*" and "default" among them or NONE */
    std::vector<uint32_t> key_off{0u};     /* the distinct `text` strings, by first appearance in file order */
    std::vector<uint8_t> key_bytes;
};

/* `d` has passed the validator.  Returns the number of distinct layer names, which the caller compares with
 * OSMT_CASCADE_MAX_LAYERS, in *n_names, and the number of keys in key_off.size() - 1; tables are complete only when both are
 * within their limits. */
inline void osmt_cs_resolve(const osmt_rules_desc& d, osmt_cs_tables& T, size_t* n_names) {
    auto str = [&](uint32_t off, uint32_t len) { return std::string((const char*)d.strings + off, len); };
    /* layers: "default" for OSMT_LAYER_DEFAULT, equal bytes are one layer; numbered by first use in selector order, names
     * no selector uses after them */
    std::map<std::string, size_t> names;
    std::vector<std::string> in_order;
    auto layer_of = [&](const std::string& s) {
        const auto it = names.emplace(s, in_order.size());
        if (it.second) in_order.push_back(s);
        return it.first->second;
    };
    T.sel_layer.resize(d.n_selectors);
    for (size_t i = 0; i < d.n_selectors; ++i) {
        const uint32_t L = d.selector_layer[i];
        const std::string s = L == OSMT_LAYER_DEFAULT ? std::string("default")
                                                      : std::string((const char*)d.layer_bytes + d.layer_off[L], d.layer_off[L + 1] - d.layer_off[L]);
        T.sel_layer[i] = (uint8_t)std::min<size_t>(layer_of(s), 255);
    }
    T.n_layers = (uint32_t)in_order.size();
    for (size_t i = 0; i < in_order.size(); ++i) {
        if (in_order[i] == "*") T.star = (uint32_t)i;
        if (in_order[i] == "default") T.base = (uint32_t)i;
    }
    for (size_t L = 0; L < d.n_layers; ++L) (void)layer_of(std::string((const char*)d.layer_bytes + d.layer_off[L], d.layer_off[L + 1] - d.layer_off[L]));
    *n_names = in_order.size();
    std::map<std::string, uint32_t> keys;
    T.rule_last.assign(d.n_rules * (size_t)OSMT_PROP_NAMES, OSMT_CS_NONE);
    for (size_t r = 0; r < d.n_rules; ++r)
        for (uint32_t i = d.rule_prop_off[r]; i < d.rule_prop_off[r + 1]; ++i) {
            const osmt_rule_prop& p = d.props[i];
            if (p.name >= OSMT_PROP_NAMES) continue;
            osmt_cs_prop q;
            memset(&q, 0, sizeof q);
            q.kind = p.kind;
            const bool stringy = p.kind == OSMT_PV_IDENTIFIER || p.kind == OSMT_PV_STRING;
            if (p.kind == OSMT_PV_NUMBERS) {
                q.num_off = p.num_off, q.n_nums = p.n_nums;
                if (p.n_nums == 1u) q.num = d.numbers[p.num_off];
            } else if (p.kind == OSMT_PV_WIDTH_DELTA) {
                q.num = p.delta;
            }
            if ((p.kind == OSMT_PV_COLOR || p.kind == OSMT_PV_IDENTIFIER) && p.has_color) {
                q.flags |= OSMT_CS_F_COLOR;
                q.rgb[0] = p.rgb[0], q.rgb[1] = p.rgb[1], q.rgb[2] = p.rgb[2];
            }
            if (stringy && (p.name == OSMT_PROP_ICON_IMAGE || p.name == OSMT_PROP_FILL_IMAGE) && p.has_image) {
                q.flags |= OSMT_CS_F_IMAGE;
                q.aux = p.image;
            }
            if (p.kind == OSMT_PV_IDENTIFIER) {
                const std::string s = str(p.str_off, p.str_len);
                uint32_t code = (s == "none" || s == "butt") ? OSMT_CAP_BUTT : s == "round" ? OSMT_CAP_ROUND : s == "square" ? OSMT_CAP_SQUARE : OSMT_CAP_NONE;
                code |= (s == "center" ? OSMT_LABEL_POSITION_CENTER : s == "line" ? OSMT_LABEL_POSITION_LINE : OSMT_LABEL_POSITION_NONE) << OSMT_CS_ID_POS_SHIFT;
                if (s == "background") code |= OSMT_CS_ID_BACKGROUND;
                q.id_code = (uint8_t)code;
            }
            if (stringy && p.name == OSMT_PROP_TEXT) {
                const std::string s = str(p.str_off, p.str_len);
                const auto it = keys.emplace(s, (uint32_t)keys.size());
                if (it.second) {
                    T.key_bytes.insert(T.key_bytes.end(), s.begin(), s.end());
                    T.key_off.push_back((uint32_t)T.key_bytes.size());
                }
                q.aux = it.first->second;
            }
            T.rule_last[r * OSMT_PROP_NAMES + p.name] = (uint32_t)T.props.size();
            T.props.push_back(q);
        }
}

#endif
