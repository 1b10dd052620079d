// Host build of the fill-slot arithmetic (osmt_fill_slots.h) for tests/test_fill_slots_cpu.py: k_opinfo's placement of
// the descriptors, played workgroup by workgroup in a given order with the header's own functions.
#include "../osm_renderer_amd/csrc/osmt_fill_slots.h"

#include <vector>

extern "C" {

uint32_t shim_fill_wg_ops(void) { return OSMT_FILL_SLOT_WG_OPS; }
uint32_t shim_fill_pass_slots(void) { return OSMT_FILL_PASS_SLOTS; }
uint32_t shim_fill_slots_round(uint32_t total) { return osmt_fill_slots_round(total); }
uint32_t shim_fill_slot_wgs(uint32_t n_ops) { return osmt_fill_slot_wgs(n_ops); }
uint64_t shim_fill_slot_capacity(uint64_t groups, uint64_t n_fills, uint32_t sub_rows, uint32_t n_ops) {
    return osmt_fill_slot_capacity(groups, n_fills, sub_rows, n_ops);
}
uint32_t shim_fill_pass_count(uint64_t cursor, uint64_t capacity) { return osmt_fill_pass_count(cursor, capacity); }

// descriptor round trip: packs with osmt_fill_slot_make, unpacks with the accessors -> out[0..6] = op, word0, sr, c0, ncols, simple, edges
void shim_fill_slot_pack(uint32_t op, uint32_t arena_off, uint32_t r, uint32_t sr0, uint32_t c0, uint32_t ncols, uint32_t n_rings,
                         uint32_t n_edges, uint32_t first_pt, uint32_t* out) {
    const osmt_fill_slot s = osmt_fill_slot_make(op, arena_off, r, sr0, c0, ncols, n_rings, n_edges, first_pt);
    out[0] = s.op;
    out[1] = s.word0;
    out[2] = osmt_fill_slot_sr(s.geom);
    out[3] = osmt_fill_slot_c0(s.geom);
    out[4] = osmt_fill_slot_ncols(s.geom);
    out[5] = osmt_fill_slot_simple(s.geom);
    out[6] = osmt_fill_slot_edges(s.geom);
    out[7] = s.first_pt;
}

// The placement of k_opinfo: workgroups reserve in `order` (a permutation of the workgroup indices).  owner[i] = op that
// stored slot i, 0xFFFFFFFE for a slot of the rounding; hits[i] = stores into slot i; a store at or past `cap` is dropped
// and counted in the return value's high half.  Returns the cursor (low 32 bits) | dropped << 32.
uint64_t shim_fill_slots_play(uint32_t n_ops, const uint32_t* nsr, const uint32_t* order, uint32_t n_wg, uint32_t* owner, uint32_t* hits,
                              uint64_t cap) {
    const uint32_t wg_ops = OSMT_FILL_SLOT_WG_OPS, wave_ops = 64u;
    uint64_t cursor = 0, dropped = 0;
    auto store = [&](uint64_t idx, uint32_t who) {
        if (idx >= cap) {
            ++dropped;
            return;
        }
        owner[idx] = who;
        ++hits[idx];
    };
    for (uint32_t w = 0; w < n_wg; ++w) {
        const uint32_t o0 = order[w] * wg_ops;
        // wave totals
        std::vector<uint32_t> wave_tot(wg_ops / wave_ops, 0u);
        uint32_t total = 0;
        for (uint32_t i = 0; i < wg_ops; ++i) {
            const uint32_t n = o0 + i < n_ops ? nsr[o0 + i] : 0u;
            wave_tot[i / wave_ops] += n;
            total += n;
        }
        if (total == 0u) continue;
        const uint32_t res = osmt_fill_slots_round(total);
        const uint64_t base = cursor;
        cursor += res;
        uint32_t before_wave = 0;
        for (uint32_t wv = 0; wv < wg_ops / wave_ops; ++wv) {
            uint32_t incl = 0;
            for (uint32_t l = 0; l < wave_ops; ++l) {
                const uint32_t o = o0 + wv * wave_ops + l;
                const uint32_t n = o < n_ops ? nsr[o] : 0u;
                incl += n;
                const uint32_t first = osmt_fill_slot_first(before_wave, incl, n);
                for (uint32_t r = 0; r < n; ++r) store(base + first + r, o);
            }
            before_wave += wave_tot[wv];
        }
        for (uint32_t i = total; i < res; ++i) store(base + i, 0xFFFFFFFEu);
    }
    return (cursor & 0xFFFFFFFFull) | (dropped << 32);
}
}
