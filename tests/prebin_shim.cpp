// Host build of k_prebin's block-to-role mapping (osmt_prebin_roles.h) for tests/test_prebin_roles.py.
// The interleaved mapping is what is tested, whichever layout the library's build selects.
#define OSMT_V_PREBIN_INTERLEAVE 1
#include "../osm_renderer_amd/csrc/osmt_prebin_roles.h"

#include <vector>

extern "C" {

// role (1 = stroke block, 0 = fill group) and index of block b
uint32_t shim_prebin_role(uint32_t n_vblk, uint32_t n_fgrp, uint32_t b, uint32_t* idx) {
    return osmt_prebin_role(osmt_prebin_map_make(n_vblk, n_fgrp), b, idx);
}

// The three properties over EVERY block of a grid: 0 when they hold, else 1 + the first offending block index.
//   every block maps to one in-range (role, index); every index of both roles is hit exactly once;
//   the stroke blocks among [0, b) are within one of b * n_vblk / (n_vblk + n_fgrp), for every b.
uint64_t shim_prebin_check_all(uint32_t n_vblk, uint32_t n_fgrp) {
    const osmt_prebin_map m = osmt_prebin_map_make(n_vblk, n_fgrp);
    const uint64_t T = (uint64_t)n_vblk + n_fgrp;
    std::vector<uint8_t> hit_v(n_vblk, 0), hit_f(n_fgrp, 0);
    uint64_t strokes = 0; // among [0, b)
    for (uint64_t b = 0; b < T; ++b) {
        // |strokes - b * n_vblk / T| <= 1  <=>  |strokes * T - b * n_vblk| <= T
        const __int128 d = (__int128)strokes * (__int128)T - (__int128)b * n_vblk;
        if (d > (__int128)T || d < -(__int128)T) return 1 + b;
        uint32_t idx = 0xFFFFFFFFu;
        const uint32_t role = osmt_prebin_role(m, (uint32_t)b, &idx);
        if (role > 1u) return 1 + b;
        if (role) {
            if (idx >= n_vblk || hit_v[idx]++) return 1 + b;
            ++strokes;
        } else {
            if (idx >= n_fgrp || hit_f[idx]++) return 1 + b;
        }
    }
    if (strokes != n_vblk) return 1 + T;
    for (uint32_t i = 0; i < n_vblk; ++i)
        if (hit_v[i] != 1) return 1 + T;
    for (uint32_t i = 0; i < n_fgrp; ++i)
        if (hit_f[i] != 1) return 1 + T;
    return 0;
}

// The same properties at one block b of a grid too large to enumerate, from the mapping alone:
//   in range; the stroke count of the prefix [0, b) follows from the answer (a stroke block i has exactly i stroke blocks
//   in front of it, a fill group j has b - j) and must be within one of the share; the neighbours b - 1 and b + 1 must carry
//   on from it (same role: index + 1, other role: the index the prefix count demands), which is what makes every index
//   hit exactly once by induction from block 0.
// 0 when they hold, else a code 1 .. 5.
uint32_t shim_prebin_check_at(uint32_t n_vblk, uint32_t n_fgrp, uint32_t b) {
    const osmt_prebin_map m = osmt_prebin_map_make(n_vblk, n_fgrp);
    const uint64_t T = (uint64_t)n_vblk + n_fgrp;
    if (b >= T) return 1;
    uint32_t idx = 0xFFFFFFFFu;
    const uint32_t role = osmt_prebin_role(m, b, &idx);
    if (role > 1u || idx >= (role ? n_vblk : n_fgrp)) return 2;
    const uint64_t strokes = role ? idx : (uint64_t)b - idx; // among [0, b)
    if (strokes > b || strokes > n_vblk || (uint64_t)b - strokes > n_fgrp) return 3;
    const __int128 d = (__int128)strokes * (__int128)T - (__int128)b * n_vblk;
    if (d > (__int128)T || d < -(__int128)T) return 4;
    if (b == 0 && idx != 0u) return 5;
    if (b + 1ull < T) {
        uint32_t idx1 = 0xFFFFFFFFu;
        const uint32_t role1 = osmt_prebin_role(m, b + 1u, &idx1);
        const uint64_t strokes1 = strokes + role, fills1 = (uint64_t)b + 1u - strokes1;
        if (role1 > 1u || (uint64_t)idx1 != (role1 ? strokes1 : fills1)) return 5;
    } else if (strokes + role != n_vblk) {
        return 5; // the last block closes both counts
    }
    return 0;
}

uint32_t shim_prebin_n_vblk(uint32_t n_vsegs, uint32_t bin_segs) { return osmt_prebin_n_vblk(n_vsegs, bin_segs); }
uint32_t shim_prebin_bin_segs_default(void) { return OSMT_BIN_SEGS; }
}
