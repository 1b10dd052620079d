// Host build of the list arena's slices (osmt_list_slices.h) for tests/test_list_slices_cpu.py.
#include "../osm_renderer_amd/csrc/osmt_list_slices.h"

#include <vector>

extern "C" {

uint32_t shim_list_slices() { return OSMT_LIST_SLICES; }
uint32_t shim_list_min_jobs() { return OSMT_LIST_SLICE_MIN_JOBS; }

// the layout of a batch: out = {n_slices, slice_cap, total}
void shim_list_layout(uint32_t n_jobs, uint64_t ent_cap, uint64_t* out) {
    const osmt_list_layout l = osmt_list_layout_make(n_jobs, ent_cap);
    out[0] = l.n_slices;
    out[1] = l.slice_cap;
    out[2] = l.total;
}

// What k_sublist's workgroups do, one after the other in the order given: tile order[k] reserves counts[order[k]] entries with
// its slice's cursor and, if that does not fit, with the overflow cursor.  base[t] = the tile's first entry, or UINT64_MAX for a
// tile that was refused; where[t] = 0 slice, 1 overflow, 2 refused, 3 nothing to reserve.  Returns the number of refused tiles.
uint32_t shim_list_play(uint32_t n_jobs, uint64_t ent_cap, const uint32_t* counts, const uint32_t* order, uint64_t* base, uint8_t* where) {
    const osmt_list_layout l = osmt_list_layout_make(n_jobs, ent_cap);
    std::vector<unsigned long long> cur(l.n_slices + 1u, 0ull);
    uint32_t refused = 0;
    for (uint32_t k = 0; k < n_jobs; ++k) {
        const uint32_t t = order[k];
        const unsigned long long n = counts[t];
        base[t] = 0;
        where[t] = 3;
        if (!n) continue;
        const uint32_t slice = osmt_list_slice_of(l, t);
        unsigned long long first = cur[slice], b = 0;
        cur[slice] += n; // atomicAdd
        if (osmt_list_place(l, slice, first, n, &b)) {
            base[t] = b;
            where[t] = 0;
            continue;
        }
        if (l.n_slices > 1u) {
            first = cur[l.n_slices];
            cur[l.n_slices] += n;
            if (osmt_list_place_overflow(l, ent_cap, first, n, &b)) {
                base[t] = b;
                where[t] = 1;
                continue;
            }
        }
        base[t] = ~0ull;
        where[t] = 2;
        ++refused;
    }
    return refused;
}
}
