/*
 * osmt_textshape.hip — label text given as strings (osmt_scene_set_string_labels): TextPlacer::text_to_glyphs of the
 * reference (font/text_placer.rs:170-197) on the GPU, writing the osmt_text_glyph array that the text-run form uploads
 * from the host.  k_text_place (osmt_textplace.hip) reads it on the same stream.  gfx950 only.
 *
 *   k_text_shape   one lane per char, over the (label, slot) pairs the count pass of the glyph expansion is given anyway
 *                  (pairs in label order: a wave's lanes read neighbouring chars and, mostly, one font).  A lane looks
 *                  its own code point up in the font's cmap and, unless it is the first char of ITS label, the code
 *                  point in front of it a second time: the predecessor is found by index, not handed from lane to lane,
 *                  so neither a wave boundary nor the label in front of it in the pool can get between the two.  Two
 *                  bisections of the cmap and one of the kern pairs per char; integer work, no LDS, no scratch; one
 *                  16-byte store per char.
 *
 * The host twin is host/osmt_textshaper.hpp (the same records; it also holds the validation every call runs first, so
 * that every index read here is inside its table: slot < n_chars, font id < the snapshot's fonts, and — checked when the
 * font was registered — every glyph index of cmap and kern < n_glyphs).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

/* char::is_whitespace: the Unicode White_Space set (not isspace: U+001C-001F, 180E, 200B, FEFF are not in it) */
__device__ __forceinline__ bool is_whitespace(uint32_t cp) {
    return (cp >= 0x0009u && cp <= 0x000Du) || cp == 0x0020u || cp == 0x0085u || cp == 0x00A0u || cp == 0x1680u ||
           (cp >= 0x2000u && cp <= 0x200Au) || cp == 0x2028u || cp == 0x2029u || cp == 0x202Fu || cp == 0x205Fu || cp == 0x3000u;
}

/* find_glyph_index: glyph 0 for a code point the font does not list */
__device__ __forceinline__ uint32_t find_glyph(const osmt_font_dev& f, uint32_t cp) {
    const uint2* __restrict__ cmap = reinterpret_cast<const uint2*>(f.cmap);
    uint32_t lo = 0u, hi = f.n_cmap;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cmap[mid].x < cp)
            lo = mid + 1u;
        else
            hi = mid;
    }
    if (lo < f.n_cmap) {
        const uint2 e = cmap[lo];
        if (e.x == cp) return e.y;
    }
    return 0u;
}

/* get_glyph_kern_advance: 0 for a pair the font does not list */
__device__ __forceinline__ int32_t find_kern(const osmt_font_dev& f, uint32_t left, uint32_t right) {
    const osmt_kern_pair* __restrict__ kern = f.kern;
    const uint64_t key = ((uint64_t)left << 32) | right;
    uint32_t lo = 0u, hi = f.n_kern;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((((uint64_t)kern[mid].left << 32) | kern[mid].right) < key)
            lo = mid + 1u;
        else
            hi = mid;
    }
    if (lo < f.n_kern) {
        const osmt_kern_pair e = kern[lo];
        if (e.left == left && e.right == right) return e.value;
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_text_shape(osmt_shape_pass a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n_pairs) return;
    const uint32_t slot = a.pair_inst[p], l = a.pair_label[p];
    const uint32_t first = a.labels[l].seg_off;
    const osmt_font_dev f = a.fonts[a.label_font[l]];
    const uint32_t cp = a.chars[slot];
    const uint32_t g = find_glyph(f, cp);
    int32_t kern = 0;
    if (slot != first) kern = find_kern(f, find_glyph(f, a.chars[slot - 1u]), g);
    uint4 o;
    o.x = f.outline[g];
    o.y = (uint32_t)f.advance[g];
    o.z = (uint32_t)kern;
    o.w = is_whitespace(cp) ? 1u : 0u;
    reinterpret_cast<uint4*>(a.out)[slot] = o;
}

}  // namespace

hipError_t osmt_launch_text_shape(const osmt_shape_pass& a, hipStream_t st) {
    if (!a.n_pairs) return hipSuccess;
    hipLaunchKernelGGL(k_text_shape, dim3((a.n_pairs + 255u) / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}
