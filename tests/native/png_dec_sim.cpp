// png_dec_sim.cpp -- the device's PNG decoder on the CPU (png_sim.hpp): stand-alone, built plain and under ASan + UBSan by
// tests/test_png_native.py.
//   [--poison BYTE] in front of either mode: png_sim.hpp
//   dump <in.png> <rgb.bin> <scan.bin> [flags]   "refused <reason>" | "head h w ctype bpp orientation idat_bytes spans" and "status N rounds R";
//                                                the RGB pixels and the filtered scanlines to the two files
//   batch <pack>                                 a pack of [u32 length | file] records: one line each, "refused <reason>" | "status N"
#include <cstdlib>
#include <cstring>

#include "png_sim.hpp"

static void put(const char* path, const std::vector<uint8_t>& v) {
    if (FILE* fp = std::fopen(path, "wb")) { std::fwrite(v.data(), 1, v.size(), fp); std::fclose(fp); }
}

int main(int argc, char** argv) {
    pngsim::take_poison(argc, argv);
    if (argc >= 5 && !std::strcmp(argv[1], "dump")) {
        const std::vector<uint8_t> file = pngsim::read_file(argv[2]);
        const pngsim::Result R = pngsim::decode(file.data(), file.size(), argc > 5 ? (uint32_t)std::atoi(argv[5]) : 0u);
        if (R.refused) { std::printf("refused %s\n", R.why.c_str()); return 0; }
        std::printf("head %d %d %d %d %d %zu %zu\n", R.f.h, R.f.w, R.f.ctype, R.f.bpp, R.f.orientation, R.f.idat_bytes, R.f.spans.size());
        std::printf("status %d rounds %ld\n", R.status, R.rounds);
        put(argv[3], R.rgb);
        put(argv[4], R.scan);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "batch")) {
        const std::vector<uint8_t> pack = pngsim::read_file(argv[2]);
        size_t i = 0;
        while (i + 4 <= pack.size()) {
            uint32_t len = 0;
            std::memcpy(&len, pack.data() + i, 4);
            i += 4;
            if (len > pack.size() - i) return 2;
            const std::vector<uint8_t> file(pack.begin() + (long)i, pack.begin() + (long)(i + len));     // its own allocation: ASan guards its end
            i += len;
            const pngsim::Result R = pngsim::decode(file.data(), file.size());
            if (R.refused) std::printf("refused %s\n", R.why.c_str());
            else std::printf("status %d\n", R.status);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: png_dec_sim dump <in.png> <rgb.bin> <scan.bin> [flags] | batch <pack>\n");
    return 2;
}
