// png_fuzz.cpp -- malformed PNG files through csrc/png_parse.hpp and the decoder's CPU form (png_sim.hpp): stand-alone, built plain and
// under ASan + UBSan by tests/test_png_native.py.
//   png_fuzz [--poison BYTE] <in.png> <seed> <count>
// First the file cut at every tenth byte: "cut <bytes> refused|status N".  Then <count> single-byte mutations of the IDAT payload,
// positions and values from a 64-bit LCG started at <seed>: "mut <offset in the payload> <new value> refused|status N".  The test
// repeats every mutation from the printed numbers and asks zlib about the same bytes.
#include <cstdlib>

#include "png_sim.hpp"

static void report(const pngsim::Result& R) {
    if (R.refused) std::printf("refused\n"); else std::printf("status %d\n", R.status);
}

int main(int argc, char** argv) {
    pngsim::take_poison(argc, argv);
    if (argc != 4) { std::fprintf(stderr, "usage: png_fuzz <in.png> <seed> <count>\n"); return 2; }
    const std::vector<uint8_t> good = pngsim::read_file(argv[1]);
    uint64_t x = std::strtoull(argv[2], nullptr, 10);
    const int count = std::atoi(argv[3]);
    pngsim::Result G = pngsim::decode(good.data(), good.size());
    if (G.refused || G.status != 0 || G.f.spans.size() != 1) { std::fprintf(stderr, "the file must decode and have one IDAT chunk\n"); return 2; }
    for (size_t n = 0; n < good.size(); n += 10) {
        const std::vector<uint8_t> cut(good.begin(), good.begin() + (long)n);
        std::printf("cut %zu ", n);
        report(pngsim::decode(cut.data(), cut.size()));
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
        report(pngsim::decode(bad.data(), bad.size()));
    }
    return 0;
}
