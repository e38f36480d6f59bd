// png_sim.hpp -- csrc/png_dec.hip's two kernels on the CPU, with the lanes as a loop: the phases of csrc/png_inflate_core.hpp in the
// kernel's order, a barrier where a lane loop ends, and the unfilter's skewed wavefront with the cross-lane shifts as array reads of
// the step before.  Every buffer has exactly the size the device is promised, so ASan sees what the device would not forgive.
// "--poison BYTE" in front of a program's mode (sim_poison.hpp): the inflate state before begin, the scanlines, the hand-off row and
// the pixels -- LDS, and device scratch that png_dec_launch never clears -- start as that byte, not as zero.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/png_inflate_core.hpp"
#include "../../image_restoration_platform_amd/csrc/png_parse.hpp"
#include "sim_poison.hpp"

namespace pngsim {
using namespace ire;
using pngdec::kLanes;

using simpoison::dirty;
using simpoison::take_poison;

// the inflate kernel: in[0 .. in_len) -> out[0 .. total); the status
inline int inflate(const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t total, long* rounds = nullptr) {
    std::vector<pngdec::Inflate> mem = dirty<pngdec::Inflate>(1);          // __shared__ Inflate S: LDS is never cleared
    pngdec::Inflate& S = mem[0];
    pngdec::begin(S, in, in_len, out, total);
    for (;;) {
        for (int l = 0; l < kLanes; ++l) pngdec::window_load(S, l);
        pngdec::window_commit(S);                                     // lane 0 ...
        pngdec::block_begin(S);
        if (S.done) break;
        if (S.kind == pngdec::kKindHuff) for (int l = 0; l < kLanes; ++l) pngdec::fill_fast(S, l);
        bool end = false;
        do {
            for (int l = 0; l < kLanes; ++l) pngdec::window_load(S, l);
            pngdec::window_commit(S);                                 // lane 0 ...
            pngdec::walk(S);
            end = S.block_end != 0;
            for (int l = kLanes - 1; l >= 0; --l) pngdec::place(S, l);       // (any lane order gives the same bytes: downwards here)
            if (rounds) ++*rounds;
        } while (!end);
    }
    pngdec::finish(S);
    return S.status;
}

// the unfilter kernel: scan -> rgb (h * w * 3); the status (a filter byte outside 0..4)
inline int unfilter(const pngparse::File& f, const uint8_t* scan, uint8_t* rgb) {
    const uint32_t h = (uint32_t)f.h, w = (uint32_t)f.w, bpp = (uint32_t)f.bpp;
    const size_t stride = 1 + (size_t)w * bpp;
    std::vector<uint32_t> hand = dirty<uint32_t>(w);
    int status = 0;
    for (uint32_t r0 = 0; r0 < h; r0 += kLanes) {
        uint32_t cur[kLanes] = {}, prev[kLanes] = {}, ft[kLanes] = {};
        for (int i = 0; i < kLanes; ++i)
            if (r0 + i < h) { ft[i] = scan[stride * (r0 + i)]; if (ft[i] > 4) { status = pngdec::kStFilter; ft[i] = 0; } }
        for (uint32_t t = 0; t < w + kLanes - 1; ++t) {
            uint32_t ocur[kLanes], oprev[kLanes];
            for (int i = 0; i < kLanes; ++i) { ocur[i] = cur[i]; oprev[i] = prev[i]; }
            for (int i = 0; i < kLanes; ++i) {
                const uint32_t r = r0 + i, x = t - (uint32_t)i;
                if (r >= h || t < (uint32_t)i || x >= w) continue;
                uint32_t px = 0;
                for (uint32_t k = 0; k < bpp; ++k) px |= (uint32_t)scan[stride * r + 1 + (size_t)x * bpp + k] << (8 * k);
                const uint32_t up = i ? ocur[i - 1] : hand[x], upleft = i ? oprev[i - 1] : (x ? hand[x - 1] : 0);
                const uint32_t a = x ? ocur[i] : 0, b = r ? up : 0, c = (r && x) ? upleft : 0;
                const uint32_t raw = pngdec::unfilter_px(ft[i], bpp, px, a, b, c);
                prev[i] = ocur[i]; cur[i] = raw;
                const uint32_t v = pngdec::rgb_of((uint32_t)f.ctype, raw, f.pal);
                uint8_t* o = rgb + ((size_t)r * w + x) * 3;
                o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
            }
            // lane 63 hands its row to the next band, 63 pixels behind lane 0's reads
            if (t >= (uint32_t)(kLanes - 1) && t - (kLanes - 1) < w && r0 + kLanes - 1 < h) hand[t - (kLanes - 1)] = cur[kLanes - 1];
        }
    }
    return status;
}

struct Result { bool refused = false; std::string why; pngparse::File f; int status = 0; std::vector<uint8_t> scan, rgb; long rounds = 0; };

inline Result decode(const uint8_t* file, size_t bytes, uint32_t flags = 0) {
    Result R;
    if (!pngparse::plan_file(file, bytes, flags, R.f, R.why)) { R.refused = true; return R; }
    std::vector<uint8_t> in(R.f.idat_bytes);
    if (pngparse::stage(R.f, file, bytes, in.data(), in.size(), R.why) != in.size()) { R.refused = true; return R; }
    R.scan = dirty<uint8_t>(R.f.scan_bytes());
    R.rgb = dirty<uint8_t>((size_t)R.f.h * R.f.w * 3);
    R.status = inflate(in.data(), (uint32_t)in.size(), R.scan.data(), (uint32_t)R.scan.size(), &R.rounds);
    if (R.status == 0) R.status = unfilter(R.f, R.scan.data(), R.rgb.data());
    return R;
}

inline std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> v;
    if (FILE* fp = std::fopen(path, "rb")) {
        uint8_t buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), fp)) > 0) v.insert(v.end(), buf, buf + n);
        std::fclose(fp);
    }
    return v;
}

}  // namespace pngsim
