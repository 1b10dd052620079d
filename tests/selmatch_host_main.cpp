// Stand-alone host program over host/osmt_selmatch.hpp, built with AddressSanitizer and UBSan by tests/_selmatch.py: the
// mirror over a geodata file given on the command line with a fixed selector set, and the parsers over a fixed corpus.
// Prints "classes <n> pairs <n>", one line per class, then "numbers <ok> <declined> <errors>".
#include <cstdio>
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
    set.add(OSMT_SEL_AREA, 12);
    set.test(OSMT_TEST_EQUAL, "building", "yes");
    set.add(OSMT_SEL_NODE, -1, 15);
    set.test(OSMT_TEST_GREATER_OR_EQUAL, "population", "", 1000.0);
    set.test(OSMT_TEST_NOT_EQUAL, "place", "hamlet");
    set.add(OSMT_SEL_WAY);
    set.test(OSMT_TEST_TRUE, "bridge");
    set.test(OSMT_TEST_LESS, "lanes", "", 3.0);
    set.add(OSMT_SEL_OTHER);
    set.add(OSMT_SEL_WAY);
    set.test(OSMT_TEST_FALSE, "tunnel");
    set.test(OSMT_TEST_NOT_EXISTS, "name:en");
    const osmt_selectors_desc& d = set.desc();
    const HostMatch m = match_selectors_host(r, d);
    if (m.entity_class.size() != r.node_count() + r.way_count() + r.multipolygon_count()) return 3;
    size_t n_tags = tags.desc.n_node_tags + tags.desc.n_way_tags + tags.desc.n_multipolygon_tags;
    printf("classes %zu pairs %zu tags %zu\n", m.classes.size(), m.class_selectors.size(), n_tags);
    for (const osmt_match_class& c : m.classes) {
        printf("%u %u %u %lld", (unsigned)c.slot, (unsigned)c.has_layer, c.first_entity, (long long)c.layer);
        for (uint32_t s : selectors_at_zoom(d, m.class_selectors.data() + c.sel_off, c.n_sels, 14)) printf(" %u", s);
        printf("\n");
    }
    const char* corpus[] = {"5", "-0", "+3.5", ".5", "5.", "1e3", "1E-2", "0.1", "4.35", "inf", "-Infinity", "NaN", "-nan", "", ".", "e5", "1e", " 1", "1 ",
                            "0x10", "1_0", "9007199254740992", "9007199254740993", "123456789012345678901234567890", "1e22", "1e23", "1e99999999999",
                            "0.000000000000000000000000000000000001", "+", "-", "1.e5", ".e5", "1e+", "infinit"};
    int ok = 0, declined = 0, errors = 0;
    for (const char* s : corpus) {
        double a = 0.0, b = 0.0;
        const int rc = number_fast_path(s, &a);
        const bool good = parse_f64(s, &b);
        if ((rc == OSMT_NUM_ERROR) == good) return 4; /* the two grammars differ */
        if (rc == OSMT_NUM_OK && !(a == b || (a != a && b != b))) return 5;
        ok += rc == OSMT_NUM_OK, declined += rc == OSMT_NUM_DECLINED, errors += rc == OSMT_NUM_ERROR;
        int64_t i = 0, j = 0;
        if (parse_i64(s, &i) != osmt_parse_i64((const uint8_t*)s, (uint32_t)std::string(s).size(), &j) || i != j) return 6;
    }
    const osmt_declined_number dn[1] = {{0u, 0u}};
    const HostNumbers hn(tags.desc.strings, dn, 1);
    if (hn.overrides.size() != 1 || hn.overrides[0].has_value) return 7; /* the empty string is an error */
    printf("numbers %d %d %d\n", ok, declined, errors);
    return 0;
}
