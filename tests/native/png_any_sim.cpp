// png_any_sim.cpp -- csrc/png_dec.hip's png_unfilter_any_kernel on the CPU, behind png_sim.hpp's inflate: the functions of
// csrc/png_adam7_core.hpp with the lanes as a loop, one (image, pass) after another as the device runs its workgroups, the cross-lane
// shifts as array reads of the step before.  Every buffer has exactly the size the device is promised (the scanlines, the pixels, a
// hand-off row of the pass's own units), so ASan sees what the device would not forgive.  Stand-alone, built plain and under
// ASan + UBSan by tests/test_png_depths_native.py.
//   [--poison BYTE] in front of either mode: png_sim.hpp
//   dump <in.png> <rgb.bin> <scan.bin> <flags>   "refused <reason>" | "head h w ctype bpp orientation idat_bytes spans depth interlace" and
//                                                "status N"; the RGB pixels and the filtered scanlines to the two files
//   fuzz <in.png> <seed> <count> <flags>         png_fuzz.cpp's lines for a file of any form: the file cut at every tenth byte, then
//                                                <count> single-byte mutations of its IDAT payload
#include <cstdlib>
#include <cstring>

#include "png_sim.hpp"

namespace anysim {
using namespace ire;
using pngdec::kLanes;

// one pass of one image: scan (the whole stream) -> its pixels of rgb (h * w * 3); false: a filter byte outside 0..4
static bool unfilter_pass(const pngparse::File& f, uint32_t p, const std::vector<uint8_t>& scan_all, std::vector<uint8_t>& rgb) {
    const uint32_t h = (uint32_t)f.h, w = (uint32_t)f.w, ctype = (uint32_t)f.ctype, depth = (uint32_t)f.depth;
    const pngdec::Pass P = pngdec::pass_of(h, w, ctype, depth, (uint32_t)f.interlace, p);
    if (P.pw == 0 || P.ph == 0) return true;
    const uint32_t unit = pngdec::filter_unit(ctype, depth), per = pngdec::unit_pixels(ctype, depth), nu = P.row_bytes / unit;
    const size_t stride = 1 + (size_t)P.row_bytes;
    // the pass's scanlines as their own allocation: a read past them is a report, not a read of the next pass
    const std::vector<uint8_t> scan(scan_all.begin() + (long)P.off, scan_all.begin() + (long)(P.off + (uint64_t)P.ph * stride));
    std::vector<uint64_t> hand = pngsim::dirty<uint64_t>(nu);
    bool ok = true;
    for (uint32_t r0 = 0; r0 < P.ph; r0 += kLanes) {
        uint64_t cur[kLanes] = {}, prev[kLanes] = {};
        uint32_t ft[kLanes] = {};
        for (int i = 0; i < kLanes; ++i)
            if (r0 + i < P.ph) { ft[i] = scan.at(stride * (r0 + i)); if (ft[i] > 4) { ok = false; ft[i] = 0; } }
        for (uint32_t t = 0; t < nu + kLanes - 1; ++t) {
            uint64_t ocur[kLanes], oprev[kLanes];
            for (int i = 0; i < kLanes; ++i) { ocur[i] = cur[i]; oprev[i] = prev[i]; }
            for (int i = 0; i < kLanes; ++i) {
                const uint32_t r = r0 + i, x = t - (uint32_t)i;
                if (r >= P.ph || t < (uint32_t)i || x >= nu) continue;
                uint64_t px = 0;
                for (uint32_t k = 0; k < unit; ++k) px |= (uint64_t)scan.at(stride * r + 1 + (size_t)x * unit + k) << (8 * k);
                const uint64_t up = i ? ocur[i - 1] : hand.at(x), upleft = i ? oprev[i - 1] : (x ? hand.at(x - 1) : 0);
                const uint64_t a = x ? ocur[i] : 0, b = r ? up : 0, c = (r && x) ? upleft : 0;
                const uint64_t raw = pngdec::unfilter_unit(ft[i], unit, px, a, b, c);
                prev[i] = ocur[i]; cur[i] = raw;
                for (uint32_t k = 0; k < per; ++k) {
                    const uint32_t q = x * per + k;
                    if (q >= P.pw) break;
                    const uint32_t v = pngdec::rgb_of_unit(ctype, depth, raw, k, f.pal);
                    const size_t o = ((size_t)(P.y0 + r * P.dy) * w + P.x0 + (size_t)q * P.dx) * 3;
                    rgb.at(o) = (uint8_t)v; rgb.at(o + 1) = (uint8_t)(v >> 8); rgb.at(o + 2) = (uint8_t)(v >> 16);
                }
            }
            if (t >= (uint32_t)(kLanes - 1) && t - (kLanes - 1) < nu && r0 + kLanes - 1 < P.ph) hand.at(t - (kLanes - 1)) = cur[kLanes - 1];
        }
    }
    return ok;
}

static pngsim::Result decode(const uint8_t* file, size_t bytes, uint32_t flags) {
    pngsim::Result R;
    if (!pngparse::plan_file(file, bytes, flags, R.f, R.why)) { R.refused = true; return R; }
    std::vector<uint8_t> in(R.f.idat_bytes);
    if (pngparse::stage(R.f, file, bytes, in.data(), in.size(), R.why) != in.size()) { R.refused = true; return R; }
    R.scan = pngsim::dirty<uint8_t>(R.f.scan_bytes());
    R.rgb = pngsim::dirty<uint8_t>((size_t)R.f.h * R.f.w * 3);
    R.status = pngsim::inflate(in.data(), (uint32_t)in.size(), R.scan.data(), (uint32_t)R.scan.size(), &R.rounds);
    if (R.status != 0) return R;
    if (R.f.depth == 8 && R.f.interlace == 0) { R.status = pngsim::unfilter(R.f, R.scan.data(), R.rgb.data()); return R; }      // the branch the kernel takes per record
    for (uint32_t p = 0; p < pngdec::pass_count((uint32_t)R.f.interlace); ++p)
        if (!unfilter_pass(R.f, p, R.scan, R.rgb)) R.status = pngdec::kStFilter;
    return R;
}

static void report(const pngsim::Result& R) {
    if (R.refused) std::printf("refused\n"); else std::printf("status %d\n", R.status);
}
}  // namespace anysim

static void put(const char* path, const std::vector<uint8_t>& v) {
    if (FILE* fp = std::fopen(path, "wb")) { std::fwrite(v.data(), 1, v.size(), fp); std::fclose(fp); }
}

int main(int argc, char** argv) {
    pngsim::take_poison(argc, argv);
    if (argc == 6 && !std::strcmp(argv[1], "dump")) {
        const std::vector<uint8_t> file = pngsim::read_file(argv[2]);
        const pngsim::Result R = anysim::decode(file.data(), file.size(), (uint32_t)std::atoi(argv[5]));
        if (R.refused) { std::printf("refused %s\n", R.why.c_str()); return 0; }
        std::printf("head %d %d %d %d %d %zu %zu %d %d\n", R.f.h, R.f.w, R.f.ctype, R.f.bpp, R.f.orientation, R.f.idat_bytes, R.f.spans.size(), R.f.depth, R.f.interlace);
        std::printf("status %d\n", R.status);
        put(argv[3], R.rgb);
        put(argv[4], R.scan);
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "fuzz")) {
        const std::vector<uint8_t> good = pngsim::read_file(argv[2]);
        uint64_t x = std::strtoull(argv[3], nullptr, 10);
        const int count = std::atoi(argv[4]);
        const uint32_t flags = (uint32_t)std::atoi(argv[5]);
        const pngsim::Result G = anysim::decode(good.data(), good.size(), flags);
        if (G.refused || G.status != 0 || G.f.spans.size() != 1) { std::fprintf(stderr, "the file must decode and have one IDAT chunk\n"); return 2; }
        for (size_t n = 0; n < good.size(); n += 10) {
            const std::vector<uint8_t> cut(good.begin(), good.begin() + (long)n);
            std::printf("cut %zu ", n);
            anysim::report(anysim::decode(cut.data(), cut.size(), flags));
        }
        const ire::pngparse::Span sp = G.f.spans[0];
        for (int k = 0; k < count; ++k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const size_t off = (size_t)((x >> 33) % sp.len);
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            unsigned v = (unsigned)(x >> 40) & 255u;
            std::vector<uint8_t> bad = good;
            if (bad[sp.off + off] == v) v ^= 1u;
            bad[sp.off + off] = (uint8_t)v;
            std::printf("mut %zu %u ", off, v);
            anysim::report(anysim::decode(bad.data(), bad.size(), flags));
        }
        return 0;
    }
    std::fprintf(stderr, "usage: png_any_sim dump <in.png> <rgb.bin> <scan.bin> <flags> | fuzz <in.png> <seed> <count> <flags>\n");
    return 2;
}
