// Stand-alone host program over host/osmt_cascade.hpp, built with AddressSanitizer and UBSan by tests/_cascade.py: osmt::RuleSet
// and osmt::cascade_host over a small rule set whose arrays each sit in a heap block of exactly their size (the builder's
// vectors are copied out), so one element read past an end is a heap overflow.  Prints the counts and the zoom ranges.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../osm_renderer_amd/host/osmt_cascade.hpp"
#include "../osm_renderer_amd/host/osmt_selmatch.hpp"

using namespace osmt;

template <class T>
static std::unique_ptr<T[]> at_end(const T*& p, size_t n) {
    std::unique_ptr<T[]> b(new T[n ? n : 1]);
    if (n) memcpy(b.get(), p, n * sizeof(T));
    p = n ? b.get() : nullptr;
    return b;
}

int main() {
    SelectorSet sels;
    RuleSet rules;
    // way|z10-[highway] { width: 2; color: red; casing-width: eval(+1); dashes: 4,2; }
    sels.add(OSMT_SEL_WAY, 10, -1), sels.test(OSMT_TEST_EXISTS, "highway");
    rules.rule(), rules.selector();
    rules.numbers("width", {2.0}), rules.identifier("color", "red", std::array<uint8_t, 3>{255, 0, 0}), rules.width_delta("casing-width", 1.0);
    rules.numbers("dashes", {4.0, 2.0});
    // way::*, way|z14-::labels { text: name; font-size: 11; text-position: line; unknown: 1; }
    sels.add(OSMT_SEL_WAY), sels.add(OSMT_SEL_WAY, 14, -1);
    rules.rule(), rules.selector("*"), rules.selector("labels");
    rules.identifier("text", "name"), rules.numbers("font-size", {11.0}), rules.identifier("text-position", "line"), rules.numbers("unknown", {1.0});
    // node::default { icon-image: "pin.png"; z-index: 9; } with a registered icon
    sels.add(OSMT_SEL_NODE);
    rules.rule(), rules.selector("default");
    rules.string("icon-image", "pin.png", 3u), rules.numbers("z-index", {9.0});
    osmt_rules_desc d = rules.desc(0, 2.0, 1.5, 0);
    const osmt_selectors_desc& sd = sels.desc();
    if (d.n_selectors != sd.n_selectors || d.n_rules != 3 || d.n_layers != 3) return 2;
    auto k0 = at_end(d.selector_rule, d.n_selectors);
    auto k1 = at_end(d.selector_layer, d.n_selectors);
    auto k2 = at_end(d.layer_off, d.n_layers + 1);
    auto k3 = at_end(d.layer_bytes, d.n_layer_bytes);
    auto k4 = at_end(d.rule_prop_off, d.n_rules + 1);
    auto k5 = at_end(d.props, d.n_props);
    auto k6 = at_end(d.numbers, d.n_numbers);
    auto k7 = at_end(d.strings, d.n_string_bytes);
    // classes: an open way matching selectors 0, 1, 2; a closed way with a layer matching 1; a node matching 3; one matching nothing
    const uint32_t pooled_src[] = {0, 1, 2, 1, 3};
    const uint32_t* pooled = pooled_src;
    auto k8 = at_end(pooled, 5);
    osmt_match_class cls_src[4] = {};
    cls_src[0].sel_off = 0, cls_src[0].n_sels = 3, cls_src[0].slot = 2;
    cls_src[1].sel_off = 3, cls_src[1].n_sels = 1, cls_src[1].slot = 1, cls_src[1].has_layer = 1, cls_src[1].layer = -2;
    cls_src[2].sel_off = 4, cls_src[2].n_sels = 1, cls_src[2].slot = 0;
    cls_src[3].sel_off = 5, cls_src[3].n_sels = 0, cls_src[3].slot = 3;
    const osmt_match_class* cls = cls_src;
    auto k9 = at_end(cls, 4);
    for (int labels_all = 0; labels_all < 2; ++labels_all) {
        const HostCascade h = cascade_host(d, sd, cls, 4, pooled, labels_all != 0);
        printf("labels_all %d: %zu styles %zu dashes %zu label styles %zu keys %zu class styles %zu bindings, ranges", labels_all, h.styles.size(),
               h.dashes.size(), h.label_styles.size(), h.key_off.size() - 1, h.class_styles.size(), h.bindings.size());
        for (size_t r = 0; r < h.zoom_lo.size(); ++r) printf(" %u-%u", h.zoom_lo[r], h.zoom_hi[r]);
        printf("\n");
        if (h.zoom_lo.size() != 3 || h.zoom_lo[1] != 10 || h.zoom_lo[2] != 14) return 3;
        // the open way at z14: default = (width 2, casing 2 + 2 * (2 + 1) = 8), then labels with the text and 11 * 1.5
        const uint32_t* off = h.class_style_off.data() + 2 * 5;
        if (off[1] - off[0] != 2) return 4;
        const osmt_style_rec& s = h.styles[h.class_styles[h.range_style_base[2] + off[0]]];
        if (!s.has_casing_width || s.casing_width != 8.0 || s.n_dashes != 2 || h.dashes[s.dashes_off] != 4.0 || s.z_index != 3.0) return 5;
    }
    return 0;
}
