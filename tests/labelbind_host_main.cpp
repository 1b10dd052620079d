// Stand-alone host program over host/osmt_selmatch.hpp and csrc/osmt_utf8.h, built with AddressSanitizer and UBSan by
// tests/_labelbind.py: the two label-binding mirrors over a geodata file given on the command line, with classes from
// osmt::match_selectors_host and a fixed binding per class, and the decoder over strings that each sit at the very end of a
// heap block of their own size.  Prints "node <bindings> <texts> <chars>", "area <way bindings> <multipolygon bindings> <texts>
// <chars>", one line per text of the area table, then "utf8 <well-formed> <ill-formed>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../osm_renderer_amd/host/osmt_selmatch.hpp"

using namespace osmt;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const GeodataReader r(argv[1]);
    const TagsDesc tags(r);
    SelectorSet set;
    set.add(OSMT_SEL_WAY);
    set.test(OSMT_TEST_EXISTS, "highway");
    set.add(OSMT_SEL_NODE);
    set.test(OSMT_TEST_EXISTS, "place");
    const HostMatch m = match_selectors_host(r, set.desc());
    // a class that matched a selector shows its name and its reference; every other class nothing
    ClassLabelBindings b(0, 18);
    for (const osmt_match_class& c : m.classes) {
        b.add_class();
        if (c.n_sels) {
            b.bind(7, "name");
            b.bind(8, "", false);
            b.bind(9, "ref");
            b.bind(7, "name");
        }
    }
    const osmt_class_label_bindings_desc& d = b.desc();
    if (d.n_keys > 2) return 3; /* the builder pools equal keys */
    const HostLabelTable node = label_bindings_matched_host(tags.desc, m.entity_class.data(), d);
    const HostLabelTable area = area_label_bindings_matched_host(tags.desc, m.entity_class.data(), d);
    if (!node.ok || !area.ok) return 4;
    if (node.off[0].size() != r.node_count() + 1 || area.off[0].size() != r.way_count() + 1 || area.off[1].size() != r.multipolygon_count() + 1) return 5;
    printf("node %zu %zu %zu\n", node.bindings[0].size(), node.text_off.size() - 1, node.chars.size());
    printf("area %zu %zu %zu %zu\n", area.bindings[0].size(), area.bindings[1].size(), area.text_off.size() - 1, area.chars.size());
    for (size_t t = 0; t + 1 < area.text_off.size(); ++t) {
        for (uint32_t i = area.text_off[t]; i < area.text_off[t + 1]; ++i) printf("%sU+%04X", i == area.text_off[t] ? "" : " ", area.chars[i]);
        printf("\n");
    }
    const char* corpus[] = {"", "a", "\x7F", "\xC2\x80", "\xDF\xBF", "\xE0\xA0\x80", "\xED\x9F\xBF", "\xEE\x80\x80", "\xEF\xBF\xBF", "\xF0\x90\x80\x80",
                            "\xF4\x8F\xBF\xBF", "na\xC3\xAFve \xE2\x82\xAC \xF0\x9F\x98\x80", "\x80", "\xC0\x80", "\xC1\xBF", "\xE0\x80\x80", "\xE0\x9F\xBF",
                            "\xF0\x80\x80\x80", "\xF0\x8F\xBF\xBF", "\xED\xA0\x80", "\xED\xBF\xBF", "\xF4\x90\x80\x80", "\xF5\x80\x80\x80", "\xFF", "\xC3",
                            "\xE2\x82", "\xF0\x9F\x98", "ab\xE2", "ab\xF0\x9F"};
    int good = 0, bad = 0;
    for (const char* s : corpus) {
        const size_t n = strlen(s);
        // the string at the end of an allocation of exactly its size: one byte read past v_off + v_len is a heap overflow
        std::unique_ptr<uint8_t[]> at_end(new uint8_t[n ? n : 1]);
        memcpy(at_end.get(), s, n);
        std::unique_ptr<uint32_t[]> out(new uint32_t[n ? n : 1]);
        uint32_t count = 0;
        const uint32_t stop = osmt_utf8_validate(at_end.get(), (uint32_t)n, &count);
        if (stop == n) {
            if (osmt_utf8_decode(at_end.get(), (uint32_t)n, out.get()) != count) return 6;
            ++good;
        } else {
            ++bad;
        }
    }
    printf("utf8 %d %d\n", good, bad);
    return 0;
}
