// png_adam7_core.hpp -- the geometry and the arithmetic of every PNG form beside "8 bits, not interlaced", written once for the host
// parser (png_parse.hpp: the expected length of the stream), the device (png_dec.hip: png_unfilter_any_kernel) and the CPU form of that
// kernel (tests/native/png_any_sim.cpp).  Plain C++17, no HIP header: every function is IRE_HD, as in png_inflate_core.hpp.
//
// A PNG's stream is the scanlines of 1 pass (not interlaced) or 7 passes (Adam7) back to back.  Pass p is the sub-image of the pixels
// (y0 + r dy, x0 + c dx): pw x ph of them, none at all where the image is narrower than x0 + 1 or lower than y0 + 1.  Each pass is a
// small image of its own: ph scanlines of 1 filter byte and ceil(pw * bits per pixel / 8) bytes, samples packed from the most significant
// bit down, the first row filtered against a row of zeros.  The filter works on UNITS of max(1, bits per pixel / 8) bytes -- 1, 2, 3,
// 4, 6 or 8 -- which this file carries as one uint64, the unit's first byte in bits 0..7.  A unit of a sub-8-bit row is one byte and
// holds 8 / depth pixels; the last unit of a row may hold fewer.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef IRE_HD
#if defined(__HIPCC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif
#endif

namespace ire {
namespace pngdec {

constexpr uint32_t kMaxPasses = 7;

IRE_HD uint32_t pass_count(uint32_t interlace) { return interlace ? kMaxPasses : 1u; }
IRE_HD uint32_t channels_of(uint32_t ctype) { return ctype == 2 ? 3u : ctype == 4 ? 2u : ctype == 6 ? 4u : 1u; }
IRE_HD uint32_t pixel_bits(uint32_t ctype, uint32_t depth) { return channels_of(ctype) * depth; }
IRE_HD uint32_t filter_unit(uint32_t ctype, uint32_t depth) { const uint32_t b = pixel_bits(ctype, depth); return b < 8 ? 1u : b / 8; }
// the pixels one unit holds: 8 / depth in a sub-8-bit row, else 1
IRE_HD uint32_t unit_pixels(uint32_t ctype, uint32_t depth) { const uint32_t b = pixel_bits(ctype, depth); return b < 8 ? 8u / b : 1u; }

// one pass of an h x w image: where it starts, how it steps, its size, its scanlines' place in the stream
struct Pass {
    uint32_t x0, y0, dx, dy;
    uint32_t pw, ph;        // 0 x 0 when the pass has no pixel: then it has no scanline either
    uint32_t row_bytes;     // behind the filter byte
    uint64_t off;           // of its first scanline, from the stream's first byte
};

IRE_HD uint32_t pass_extent(uint32_t n, uint32_t o, uint32_t d) { return n > o ? (n - o + d - 1) / d : 0u; }

// pass p < pass_count(interlace); h, w in 1..8192, so nothing here leaves 32 bits but the offset
IRE_HD Pass pass_of(uint32_t h, uint32_t w, uint32_t ctype, uint32_t depth, uint32_t interlace, uint32_t p) {
    const uint8_t X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    const uint32_t bits = pixel_bits(ctype, depth);
    Pass P{0, 0, 1, 1, 0, 0, 0, 0};
    uint64_t off = 0;
    for (uint32_t k = 0; k <= p && k < kMaxPasses; ++k) {
        if (interlace) { P.x0 = X0[k]; P.y0 = Y0[k]; P.dx = DX[k]; P.dy = DY[k]; }
        P.pw = pass_extent(w, P.x0, P.dx); P.ph = pass_extent(h, P.y0, P.dy);
        if (P.pw == 0 || P.ph == 0) { P.pw = 0; P.ph = 0; }
        P.row_bytes = (P.pw * bits + 7) / 8;
        P.off = off;
        off += (uint64_t)P.ph * (1u + P.row_bytes);
    }
    return P;
}
// the stream's length: the sum over the passes of rows * (1 + row bytes)
IRE_HD uint64_t scan_total(uint32_t h, uint32_t w, uint32_t ctype, uint32_t depth, uint32_t interlace) {
    const Pass P = pass_of(h, w, ctype, depth, interlace, pass_count(interlace) - 1);
    return P.off + (uint64_t)P.ph * (1u + P.row_bytes);
}

// unfilter_px for a unit of up to 8 bytes.  x: the filtered unit; a, b, c: the raw units to the left, above and above left (0 outside
// the pass).  Every byte on its own: no carry passes from one to the next.
IRE_HD uint64_t unfilter_unit(uint32_t ft, uint32_t unit, uint64_t x, uint64_t a, uint64_t b, uint64_t c) {
    uint64_t r = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        if (k >= unit) break;
        const int xa = (int)(a >> (8 * k) & 255u), xb = (int)(b >> (8 * k) & 255u), xc = (int)(c >> (8 * k) & 255u);
        int pred = 0;
        if (ft == 1) pred = xa;
        else if (ft == 2) pred = xb;
        else if (ft == 3) pred = (xa + xb) >> 1;
        else if (ft == 4) {
            const int pp = xa + xb - xc;
            const int pa = pp > xa ? pp - xa : xa - pp, pb = pp > xb ? pp - xb : xb - pp, pc = pp > xc ? pp - xc : xc - pp;
            pred = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        }
        r |= (uint64_t)(((uint32_t)(x >> (8 * k)) + (uint32_t)pred) & 255u) << (8 * k);
    }
    return r;
}

// sample k (from the left) of a sub-8-bit unit: packed from the most significant bit down
IRE_HD uint32_t sample_of(uint32_t byte, uint32_t depth, uint32_t k) { return (byte >> (8 - depth * (k + 1))) & ((1u << depth) - 1); }

// pixel k < unit_pixels of a raw unit -> R | G << 8 | B << 16, what PIL's convert("RGB") gives: a sub-8-bit grey sample times 255, 85 or
// 17; a palette index looked up (pal: 768 bytes, zeros behind the last entry, so an index past it is black); of a 16-bit sample its HIGH
// byte, the first of the two; alpha dropped.  (16-bit grey is not here: the parser refuses it.)
IRE_HD uint32_t rgb_of_unit(uint32_t ctype, uint32_t depth, uint64_t raw, uint32_t k, const uint8_t* pal) {
    if (depth == 16) {
        const uint32_t r = (uint32_t)raw & 255u;
        if (ctype == 2 || ctype == 6) return r | (uint32_t)(raw >> 16 & 255u) << 8 | (uint32_t)(raw >> 32 & 255u) << 16;
        return r | r << 8 | r << 16;
    }
    if (depth == 8) {
        if (ctype == 2 || ctype == 6) return (uint32_t)raw & 0xFFFFFFu;
        const uint32_t g = (uint32_t)raw & 255u;
        if (ctype == 3) return (uint32_t)pal[3 * g] | (uint32_t)pal[3 * g + 1] << 8 | (uint32_t)pal[3 * g + 2] << 16;
        return g | g << 8 | g << 16;
    }
    const uint32_t s = sample_of((uint32_t)raw & 255u, depth, k);
    if (ctype == 3) return (uint32_t)pal[3 * s] | (uint32_t)pal[3 * s + 1] << 8 | (uint32_t)pal[3 * s + 2] << 16;
    const uint32_t g = s * (255u / ((1u << depth) - 1));
    return g | g << 8 | g << 16;
}

}  // namespace pngdec
}  // namespace ire
