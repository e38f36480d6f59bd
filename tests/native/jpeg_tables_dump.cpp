// jpeg_tables_dump.cpp -- test infrastructure for csrc/jpeg_tables.hpp (tests/test_jpeg_model.py): prints every table, the head of a
// few sizes and the bounds as "name: values" lines for comparison with tests/jpeg_model.py, and checks the quantiser's
// multiply-for-divide identity over every divisor and every 16-bit magnitude.  Plain g++; no GPU.
#include <cstdio>
#include <cstdlib>

#include "../../image_restoration_platform_amd/csrc/jpeg_tables.hpp"

using namespace ire::jpegtab;

static void codes(const char* name, const HuffCodes& t) {
    std::printf("%s:", name);
    for (int s = 0; s < 256; ++s) if (t.code[s]) std::printf(" %d/%u/%u", s, t.code[s] & 0xffffu, t.code[s] >> 16);
    std::printf("\n");
}

int main(int argc, char** argv) {
    std::printf("R: %d\nheader_bytes: %d\n", kJpegR, kHeaderBytes);
    for (int t = 0; t < 2; ++t) {
        std::printf("quant%d:", t);
        for (int k = 0; k < 64; ++k) std::printf(" %d", quant_at(t, k));
        std::printf("\nsize_max%d:", t);
        for (int k = 0; k < 64; ++k) std::printf(" %d", size_max(t, k));
        std::printf("\nblock_bits_max%d: %u\n", t, block_bits_max(t));
    }
    std::printf("zigzag:");
    for (int k = 0; k < 64; ++k) std::printf(" %d", kZigzag[k]);
    std::printf("\ncoef_max:");
    for (int k = 0; k < 64; ++k) std::printf(" %d", kCoefMax[k]);
    std::printf("\n");
    codes("dc0", dc_codes(0)); codes("dc1", dc_codes(1)); codes("ac0", ac_codes(0)); codes("ac1", ac_codes(1));
    std::printf("mcu_bits_max: %u\n", kMcuBitsMax);
    for (int k = 1; k + 1 < argc; k += 2) {        // pairs h w
        const int h = std::atoi(argv[k]), w = std::atoi(argv[k + 1]);
        const JpegHeader hd = jpeg_header(h, w);
        std::printf("header %d %d: ", h, w);
        for (int i = 0; i < kHeaderBytes; ++i) std::printf("%02x", hd.b[i]);
        std::printf("\nbound %d %d: %zu %zu\n", h, w, jpeg_file_bound(h, w), jpeg_base64_bound(h, w));
    }
    // floor((x + d / 2) / d) == ((x + d / 2) * M) >> 32 with M = quant_recip: every divisor of the two tables, every x < 2^16
    unsigned long long checked = 0;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const unsigned d = 8u * (unsigned)quant_at(t, k), M = quant_recip(t, k);
            for (unsigned x = 0; x < 65536u; ++x) {
                const unsigned n = x + d / 2;
                if ((unsigned)(((unsigned long long)n * M) >> 32) != n / d) { std::printf("recip MISMATCH t %d k %d x %u\n", t, k, x); return 1; }
                ++checked;
            }
        }
    std::printf("recip_checked: %llu\n", checked);
    return 0;
}
