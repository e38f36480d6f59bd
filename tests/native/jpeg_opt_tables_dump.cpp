// jpeg_opt_tables_dump.cpp -- test infrastructure for the (quality, sampling) forms of csrc/jpeg_tables.hpp
// (tests/test_jpeg_opt_model.py): prints the tables, the head of a few sizes and the bounds per setting as "name: values" lines for
// comparison with tests/jpeg_opt_model.py; checks the quantiser's multiply-for-divide identity for EVERY divisor a baseline table
// can hold (8 q, q in 1..255) and every 16-bit magnitude; checks that the bound of an MCU never falls as the quality rises, which
// is what lets jpeg.hip size its buffers by quality 100.  Plain g++; no GPU.
//   argv: "q" quality..., "s" sampling..., "hw" h w ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/jpeg_tables.hpp"

using namespace ire::jpegtab;

int main(int argc, char** argv) {
    std::vector<int> qs, ss, hw;
    std::vector<int>* into = nullptr;
    for (int k = 1; k < argc; ++k) {
        if (!std::strcmp(argv[k], "q")) into = &qs;
        else if (!std::strcmp(argv[k], "s")) into = &ss;
        else if (!std::strcmp(argv[k], "hw")) into = &hw;
        else if (into) into->push_back(std::atoi(argv[k]));
    }
    std::printf("header_bytes: %d\nR: %d %d\n", kHeaderBytes, restart_mcus(0), restart_mcus(2));
    for (int q : qs) {
        for (int t = 0; t < 2; ++t) {
            std::printf("quant%d q%d:", t, q);
            for (int k = 0; k < 64; ++k) std::printf(" %d", quant_at(t, k, q));
            std::printf("\nsize_max%d q%d:", t, q);
            for (int k = 0; k < 64; ++k) std::printf(" %d", size_max(t, k, q));
            std::printf("\nblock_bits_max%d q%d: %u\n", t, q, block_bits_max(t, q));
        }
        for (int s : ss) {
            std::printf("mcu_bits_max q%d s%d: %u\n", q, s, mcu_bits_max(q, s));
            std::printf("interval_bound q%d s%d: %zu %zu\n", q, s, interval_bound(1, q, s), interval_bound((unsigned)restart_mcus(s), q, s));
            for (size_t k = 0; k + 1 < hw.size(); k += 2) {
                const int h = hw[k], w = hw[k + 1];
                const JpegHeader hd = jpeg_header(h, w, q, s);
                std::printf("header %d %d q%d s%d: ", h, w, q, s);
                for (int i = 0; i < kHeaderBytes; ++i) std::printf("%02x", hd.b[i]);
                std::printf("\nbound %d %d q%d s%d: %zu %zu\n", h, w, q, s, jpeg_file_bound(h, w, q, s), jpeg_base64_bound(h, w, q, s));
            }
        }
    }
    // the names without settings are the (85, 0) instance
    bool same = kMcuBitsMax == mcu_bits_max(85, 0) && interval_bound(16) == interval_bound(16, 85, 0);
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) same = same && quant_at(t, k) == quant_at(t, k, 85) && quant_recip(t, k) == quant_recip(t, k, 85) && size_max(t, k) == size_max(t, k, 85);
    for (size_t k = 0; k + 1 < hw.size(); k += 2) {
        const JpegHeader a = jpeg_header(hw[k], hw[k + 1]), b = jpeg_header(hw[k], hw[k + 1], 85, 0);
        same = same && !std::memcmp(a.b, b.b, kHeaderBytes) && jpeg_file_bound(hw[k], hw[k + 1]) == jpeg_file_bound(hw[k], hw[k + 1], 85, 0);
    }
    std::printf("default_is_85_0: %d\n", same ? 1 : 0);
    // floor((x + d / 2) / d) == ((x + d / 2) * M) >> 32 with M = recip_of(d): every d = 8 q, every x < 2^16
    unsigned long long checked = 0;
    for (unsigned q = 1; q <= 255; ++q) {
        const unsigned d = 8u * q, M = recip_of(d);
        for (unsigned x = 0; x < 65536u; ++x) {
            const unsigned n = x + d / 2;
            if ((unsigned)(((unsigned long long)n * M) >> 32) != n / d) { std::printf("recip MISMATCH q %u x %u\n", q, x); return 1; }
            ++checked;
        }
    }
    std::printf("recip_checked: %llu\n", checked);
    // every quality: the largest categories have codes, and the bound does not fall as the quality rises
    int monotone = 1, dc_size = 0, ac_size = 0;
    unsigned prev[2] = {0, 0};
    for (int q = 1; q <= 100; ++q) {
        for (int t = 0; t < 2; ++t) {
            if (size_max(t, 0, q) > dc_size) dc_size = size_max(t, 0, q);
            for (int k = 1; k < 64; ++k) if (size_max(t, k, q) > ac_size) ac_size = size_max(t, k, q);
        }
        const unsigned now[2] = {mcu_bits_max(q, 0), mcu_bits_max(q, 2)};
        if (now[0] < prev[0] || now[1] < prev[1] || now[0] >= kNoCode || now[1] >= kNoCode) monotone = 0;
        prev[0] = now[0]; prev[1] = now[1];
    }
    std::printf("largest_sizes: %d %d\nbound_monotone: %d\n", dc_size, ac_size, monotone);
    // the size class jpeg.hip's interval kernel runs in, for all two hundred settings (tests/test_jpeg_opt_cases.py): 1 = big
    std::printf("raw_classes: %u %u\n", kRawSmall, kRawBig);
    for (int s : {0, 2}) {
        std::printf("big_class s%d:", s);
        for (int q = 1; q <= 100; ++q) std::printf(" %d", big_class(q, s) ? 1 : 0);
        std::printf("\nraw_bound s%d:", s);
        for (int q = 1; q <= 100; ++q) std::printf(" %u", raw_bound_of(s, mcu_bits_max(q, s)));
        std::printf("\nfits_a_class s%d:", s);
        for (int q = 1; q <= 100; ++q) std::printf(" %d", fits_a_class(s, mcu_bits_max(q, s)) ? 1 : 0);
        std::printf("\n");
    }
    return 0;
}
