// Host build of the pool layout (osmt_pool_layout.h) for tests/test_pool_layout_cpu.py.
#include "../osm_renderer_amd/csrc/osmt_pool_layout.h"

#include <cstdint>

#include "../include/osmtile.h"

using osmt_host::pool_layout;

extern "C" {

uint64_t shim_pool_align() { return osmt_host::POOL_ALIGN; }
uint64_t shim_pool_min_bytes() { return osmt_host::POOL_MIN_BYTES; }
uint64_t shim_sizeof_label_binding() { return sizeof(osmt_label_binding); }

// n arrays added one after the other: offs[i] = the offset of array i; returns size()
uint64_t shim_pool_layout(const uint64_t* bytes, uint32_t n, uint64_t* offs) {
    pool_layout pl;
    for (uint32_t i = 0; i < n; ++i) offs[i] = pl.add((size_t)bytes[i]);
    return pl.size();
}

// the table of osmt_register_label_bindings, array by array in the order register_label_bindings_body adds them — restated
// here, not taken from that function (it needs a device): this pins pool_layout's rule on that table's sizes, it would not
// notice the function adding its arrays in another order.  offs = {node_off, bindings, text_off, chars}; returns size()
uint64_t shim_label_bindings_layout(uint64_t n_nodes, uint64_t n_bindings, uint64_t n_texts, uint64_t n_chars, uint64_t* offs) {
    pool_layout pl;
    offs[0] = pl.add((n_nodes + 1) * 4);
    offs[1] = pl.add(n_bindings * sizeof(osmt_label_binding));
    offs[2] = pl.add((n_texts + 1) * 4);
    offs[3] = pl.add(n_chars * 4);
    return pl.size();
}

}  // extern "C"
