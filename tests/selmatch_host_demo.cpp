// The C++ binding of selector matching, linked to libosmtile.so: registers a geodata file given on the command line with its
// tags and a small selector set, runs osmt_match_selectors, answers a decline with osmt::HostNumbers and runs it again, and
// compares the result with osmt::match_selectors_host element by element.  Prints "OK <classes> <declined>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../osm_renderer_amd/host/osmt_selmatch.hpp"

using namespace osmt;

#define CHECK(call)                                                            \
    do {                                                                       \
        const int rc_ = (call);                                                \
        if (rc_ != OSMT_OK) {                                                  \
            fprintf(stderr, "%s: %d %s\n", #call, rc_, osmt_last_error());     \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const GeodataReader r(argv[1]);
    const GeodataDesc geo(r);
    const TagsDesc tags(r);
    SelectorSet set;
    set.add(OSMT_SEL_WAY);
    set.test(OSMT_TEST_EXISTS, "highway");
    set.add(OSMT_SEL_WAY);
    set.test(OSMT_TEST_GREATER, "width", "", 2.5);
    set.add(OSMT_SEL_AREA);
    set.test(OSMT_TEST_EQUAL, "building", "yes");
    set.add(OSMT_SEL_NODE);
    set.test(OSMT_TEST_LESS_OR_EQUAL, "ele", "", 100.0);
    osmt_ctx* ctx = nullptr;
    CHECK(osmt_create(nullptr, &ctx));
    uint32_t gid = 0, sid = 0;
    CHECK(osmt_register_geodata(ctx, &geo.desc, &gid));
    CHECK(osmt_register_tags(ctx, gid, &tags.desc));
    CHECK(osmt_register_selectors(ctx, &set.desc(), &sid));
    osmt_match* m = nullptr;
    HostNumbers numbers;
    size_t n_declined = 0;
    int rc = osmt_match_selectors(ctx, gid, sid, nullptr, 0, &m);
    if (rc == OSMT_UNSUPPORTED && m) { /* declined: compute the values here and run again */
        CHECK(osmt_match_read_declined_numbers(m, nullptr, 0, &n_declined));
        std::vector<osmt_declined_number> d(n_declined);
        CHECK(osmt_match_read_declined_numbers(m, d.data(), d.size(), &n_declined));
        osmt_match_free(m);
        m = nullptr;
        numbers = HostNumbers(tags.desc.strings, d.data(), d.size());
        rc = osmt_match_selectors(ctx, gid, sid, numbers.overrides.data(), numbers.overrides.size(), &m);
    }
    if (rc != OSMT_OK) {
        fprintf(stderr, "osmt_match_selectors: %d %s\n", rc, osmt_last_error());
        return 1;
    }
    size_t counts[3] = {};
    CHECK(osmt_match_read(m, nullptr, nullptr, nullptr, nullptr, counts));
    std::vector<uint32_t> ent(counts[0]), sels(counts[2]);
    std::vector<osmt_match_class> cls(counts[1]);
    CHECK(osmt_match_read(m, ent.data(), cls.data(), sels.data(), counts, counts));
    const HostMatch want = match_selectors_host(r, set.desc());
    if (ent != want.entity_class || sels != want.class_selectors || cls.size() != want.classes.size() ||
        (!cls.empty() && memcmp(cls.data(), want.classes.data(), cls.size() * sizeof(osmt_match_class)) != 0)) {
        fprintf(stderr, "the device's match differs from the mirror's\n");
        return 1;
    }
    osmt_match_free(m);
    osmt_destroy(ctx);
    printf("OK %zu %zu\n", counts[1], n_declined);
    return 0;
}
