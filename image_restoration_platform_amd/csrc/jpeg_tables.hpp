// jpeg_tables.hpp -- everything about the device's JPEG file that needs no GPU: the two quantisation tables at any IJG quality, the
// zig-zag order, the Annex K Huffman tables as (code, length) per symbol, the file's head for a given (h, w, quality, sampling), and
// the size bound with its derivation.  Host-only, header-only, plain C++17: jpeg.hip builds the tables it passes to its kernels from
// the constexpr functions here, tests/native/jpeg_tables_dump.cpp and jpeg_opt_tables_dump.cpp print all of it for comparison with
// tests/jpeg_model.py and tests/jpeg_opt_model.py.
//
// The format (the two models state it in full): baseline sequential DCT, 8 bit, one interleaved scan of Y Cb Cr, a restart interval
// in raster order of MCUs.  Two settings: quality 1..100 and sampling, numbered as ire_decode_jpeg_plan numbers it: 0 = 4:4:4 (an MCU
// is Y Cb Cr, 8 x 8 pixels, kJpegR = 16 MCUs per interval), 2 = 4:2:0 (an MCU is Y00 Y01 Y10 Y11 Cb Cr, 16 x 16 pixels, kJpegR420 = 8
// MCUs per interval: 48 blocks and 128 pixels across either way).  Every name without the two settings is the (85, 0) instance.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "jpeg_huff_core.hpp"
#include "jpeg_progenc_core.hpp"

namespace ire {
namespace jpegtab {

constexpr int kJpegR = 16;               // MCUs per restart interval at 4:4:4
constexpr int kJpegR420 = 8;             // ... at 4:2:0
constexpr int kJpegQuality = 85;
constexpr bool settings_ok(int quality, int sampling) { return quality >= 1 && quality <= 100 && (sampling == 0 || sampling == 2); }
constexpr int restart_mcus(int sampling) { return sampling == 2 ? kJpegR420 : kJpegR; }
constexpr int mcu_pixels(int sampling) { return sampling == 2 ? 16 : 8; }      // per side
constexpr int kHeaderBytes = 629;        // SOI 2 | APP0 18 | DQT 69 x 2 | SOF0 19 | DHT 33 + 183 + 33 + 183 | DRI 6 | SOS 14
constexpr int kSofDims = 2 + 18 + 69 + 69 + 5;      // file offset of SOF0's height (2 bytes, then the width's 2)

constexpr unsigned char kK1Luminance[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kK2Chrominance[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// kZigzag[k]: the natural (row-major) index of the k-th coefficient in zig-zag order
constexpr unsigned char kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// IJG quality scaling, baseline: (q * scale + 50) / 100 clamped to 1..255, scale = 200 - 2 * quality above 50.  table 0: luminance,
// 1: chrominance; natural order.
constexpr int quant_at(int table, int natural, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = ((table ? kK2Chrominance[natural] : kK1Luminance[natural]) * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}
constexpr int quant_at(int table, int natural) { return quant_at(table, natural, kJpegQuality); }

// ---- the quantiser's division as a multiplication --------------------------------------------------------------------------------
// q(c) = sign(c) * floor((|c| + d / 2) / d), d = 8 * quant.  With M = ceil(2^32 / d), e = M d - 2^32 lies in [0, d) and
// floor(x / d) = (x * M) >> 32 for every x with x * e < 2^32: x <= 8208 + 1020 < 2^14 here and e < d <= 2040 < 2^11.  That holds
// for every divisor the clamp 1..255 allows (d = 8 .. 2040), so for every quality.  tests/native/jpeg_tables_dump.cpp checks the
// identity for the divisors of quality 85 and every x < 2^16, jpeg_opt_tables_dump.cpp for every d = 8 q, q in 1..255.
constexpr unsigned recip_of(unsigned d) { return (unsigned)(((1ull << 32) + d - 1) / d); }
constexpr unsigned quant_recip(int table, int natural, int quality) { return recip_of(8u * (unsigned)quant_at(table, natural, quality)); }
constexpr unsigned quant_recip(int table, int natural) { return quant_recip(table, natural, kJpegQuality); }

// ---- Annex K Huffman tables -------------------------------------------------------------------------------------------------------
constexpr unsigned char kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Annex C: the symbols of a BITS / HUFFVAL list get consecutive codes, shortest first.  code[sym] = value | length << 16 (0: no code).
struct HuffCodes { unsigned code[256]; };
constexpr HuffCodes huff_codes(const unsigned char* bits, const unsigned char* vals) {
    HuffCodes t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t.code[vals[k++]] = code++ | ((unsigned)len << 16);
        code <<= 1;
    }
    return t;
}
constexpr HuffCodes dc_codes(int table) { return huff_codes(table ? kDcChrBits : kDcLumBits, kDcVals); }
constexpr HuffCodes ac_codes(int table) { return huff_codes(table ? kAcChrBits : kAcLumBits, table ? kAcChrVals : kAcLumVals); }

// ---- the file's head --------------------------------------------------------------------------------------------------------------
struct JpegHeader { unsigned char b[kHeaderBytes]; };
constexpr JpegHeader jpeg_header(int h, int w, int quality, int sampling) {
    JpegHeader o{};
    int n = 0;
    auto put = [&](int v) { o.b[n++] = (unsigned char)v; };
    auto seg = [&](int marker, int payload) { put(0xff); put(marker); put((payload + 2) >> 8); put((payload + 2) & 0xff); };
    put(0xff); put(0xd8);
    seg(0xe0, 14);
    for (int v : {(int)'J', (int)'F', (int)'I', (int)'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);      // version 1.01, density 1:1 without units, no thumbnail
    for (int t = 0; t < 2; ++t) {
        seg(0xdb, 65);
        put(t);
        for (int k = 0; k < 64; ++k) put(quant_at(t, kZigzag[k], quality));
    }
    seg(0xc0, 15);
    put(8); put(h >> 8); put(h & 0xff); put(w >> 8); put(w & 0xff); put(3);
    for (int v : {1, sampling == 2 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);      // Y at 2 x 2 for 4:2:0
    for (int t = 0; t < 2; ++t) {
        seg(0xc4, 1 + 16 + 12);
        put(t);
        for (int k = 0; k < 16; ++k) put((t ? kDcChrBits : kDcLumBits)[k]);
        for (int k = 0; k < 12; ++k) put(kDcVals[k]);
        seg(0xc4, 1 + 16 + 162);
        put(0x10 | t);
        for (int k = 0; k < 16; ++k) put((t ? kAcChrBits : kAcLumBits)[k]);
        for (int k = 0; k < 162; ++k) put((t ? kAcChrVals : kAcLumVals)[k]);
    }
    seg(0xdd, 2);
    put(restart_mcus(sampling) >> 8); put(restart_mcus(sampling) & 0xff);
    seg(0xda, 10);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    return o;      // n == kHeaderBytes (checked by the native test)
}
constexpr JpegHeader jpeg_header(int h, int w) { return jpeg_header(h, w, kJpegQuality, 0); }

// ---- the size bound ---------------------------------------------------------------------------------------------------------------
// 1. Amplitudes.  The forward DCT's output, scaled by 8 as the "islow" algorithm leaves it, of samples in -128..127 is in magnitude at
//    most 8 * 128 * a(u) * a(v), a(u) = C(u) / 2 * sum_x |cos((2x + 1) u pi / 16)| (every sample at full scale with the sign of its
//    basis value).  kCoefMax holds that product rounded, plus 16 for islow's own error: its 13-bit constants are off by at most
//    2^-14 relative, and it rounds twice per pass, which comes to a few units of the output scale.  Natural order.
constexpr unsigned short kCoefMax[64] = {
    8208, 7439, 7584, 7439, 8208, 7439, 7584, 7439,
    7439, 6742, 6874, 6742, 7439, 6742, 6874, 6742,
    7584, 6874, 7008, 6874, 7584, 6874, 7008, 6874,
    7439, 6742, 6874, 6742, 7439, 6742, 6874, 6742,
    8208, 7439, 7584, 7439, 8208, 7439, 7584, 7439,
    7439, 6742, 6874, 6742, 7439, 6742, 6874, 6742,
    7584, 6874, 7008, 6874, 7584, 6874, 7008, 6874,
    7439, 6742, 6874, 6742, 7439, 6742, 6874, 6742};
constexpr int bit_length(unsigned v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }
//    Four terms are EXACT in islow, formed by additions and shifts alone: those with both frequencies in {0, 4}.  The first pass
//    leaves 4 * (a sum or difference of the row's samples), the second descales a sum or difference of eight of those by 2 bits.  So
//    the DC is the sum of the 64 samples, in -8192 .. 8128, and each of the other three is a sum of 32 samples minus a sum of 32
//    others, at most 32 * 128 + 32 * 127 = 8160 in magnitude.  At quality 100 (every divisor 8) the slack in kCoefMax would put
//    them into categories the Huffman tables do not have; the exact values do not.
constexpr unsigned kDcNegMax = 8192, kDcPosMax = 8128, kExactAcMax = 8160;
constexpr unsigned coef_bound(int natural) { return (natural == 4 || natural == 32 || natural == 36) ? kExactAcMax : kCoefMax[natural]; }
// 2. Categories.  The largest magnitude category ("size") at zig-zag position k of the quantised amplitude bound; at k = 0 of the
//    largest DC DIFFERENCE, the most negative quantised DC against the most positive.  At the smallest divisor that is 1024 + 1016 =
//    2040: category 11, the last the DC tables have.  An AC amplitude is at most (8160 + 4) / 8 = 1020: category 10, the last the AC
//    tables have (libjpeg's own limit).
constexpr int size_max(int table, int k, int quality) {
    const int nat = kZigzag[k];
    const unsigned q = (unsigned)quant_at(table, nat, quality);
    if (k == 0) return bit_length((kDcNegMax + 4u * q) / (8u * q) + (kDcPosMax + 4u * q) / (8u * q));
    return bit_length((coef_bound(nat) + 4u * q) / (8u * q));
}
constexpr int size_max(int table, int k) { return size_max(table, k, kJpegQuality); }
// 3. One block.  The exact maximum, over every sequence of (run, size) symbols whose sizes respect step 2, of the bits they take with
//    the fixed tables: dynamic programming over the position p of the last non-zero coefficient so far.  best[p] = the most bits of
//    the DC and positions 1..p when p is non-zero; a run of r zeros before p costs floor(r / 16) ZRL codes and the code of
//    (r mod 16, size); a block whose last non-zero lies before 63 ends with EOB.  A size without a code costs kNoCode bits, not none:
//    were step 2 ever to allow one, every bound below would be absurd and jpeg.hip's static_asserts would refuse to compile.
constexpr unsigned kNoCode = 1u << 20;
constexpr unsigned symbol_bits(const HuffCodes& t, int sym, int size) { return (t.code[sym] >> 16) ? (t.code[sym] >> 16) + (unsigned)size : kNoCode; }
constexpr unsigned block_bits_max(int table, int quality) {
    const HuffCodes dc = dc_codes(table), ac = ac_codes(table);
    int smax[64] = {};
    for (int k = 0; k < 64; ++k) smax[k] = size_max(table, k, quality);
    unsigned best[64] = {};
    for (int s = 0; s <= smax[0]; ++s) if (symbol_bits(dc, s, s) > best[0]) best[0] = symbol_bits(dc, s, s);
    for (int p = 1; p < 64; ++p)
        for (int prev = 0; prev < p; ++prev) {
            const int run = p - prev - 1;
            unsigned sym = 0;
            for (int s = 1; s <= smax[p]; ++s) { const unsigned v = symbol_bits(ac, ((run & 15) << 4) | s, s); if (v > sym) sym = v; }
            const unsigned v = best[prev] + (unsigned)(run >> 4) * (ac.code[0xf0] >> 16) + sym;
            if (v > best[p]) best[p] = v;
        }
    unsigned out = best[63];
    for (int p = 0; p < 63; ++p) if (best[p] + (ac.code[0x00] >> 16) > out) out = best[p] + (ac.code[0x00] >> 16);
    return out;
}
constexpr unsigned block_bits_max(int table) { return block_bits_max(table, kJpegQuality); }
//    An MCU: one luminance block at 4:4:4, four at 4:2:0 (a dummy block of a partial MCU takes far less than the bound), and two
//    chrominance blocks.  A smaller divisor never lowers a category, and the divisors fall as the quality rises, so the bound does
//    not fall as the quality rises: quality 100 is the worst (jpeg_opt_tables_dump.cpp checks all hundred).
constexpr unsigned mcu_bits_max(int quality, int sampling) { return (sampling == 2 ? 4u : 1u) * block_bits_max(0, quality) + 2 * block_bits_max(1, quality); }
constexpr unsigned kMcuBitsMax = mcu_bits_max(kJpegQuality, 0);
static_assert(kMcuBitsMax == 2343, "897 bits for a luminance block, 723 for a chrominance block");
// 4. One interval of nmcu MCUs of at most mcu_bits each: its bits padded to a byte, every byte doubled by stuffing (a 0x00 behind
//    each 0xFF), the marker.
constexpr size_t interval_bound_of(unsigned nmcu, unsigned mcu_bits) { return 2 * (((size_t)nmcu * mcu_bits + 7) / 8) + 2; }
constexpr size_t interval_bound(unsigned nmcu, int quality, int sampling) { return interval_bound_of(nmcu, mcu_bits_max(quality, sampling)); }
constexpr size_t interval_bound(unsigned nmcu) { return interval_bound_of(nmcu, kMcuBitsMax); }
// 5. The file: the head, the full intervals, the last one.  (mcu_bits: mcu_bits_max(quality, sampling), for a caller that keeps it.)
constexpr size_t jpeg_file_bound_of(int h, int w, int sampling, unsigned mcu_bits) {
    const size_t p = (size_t)mcu_pixels(sampling), r = (size_t)restart_mcus(sampling);
    const size_t nmcu = (((size_t)h + p - 1) / p) * (((size_t)w + p - 1) / p);
    const size_t full = nmcu / r, tail = nmcu % r;
    return kHeaderBytes + full * interval_bound_of((unsigned)r, mcu_bits) + (tail ? interval_bound_of((unsigned)tail, mcu_bits) : 0);
}
constexpr size_t jpeg_file_bound(int h, int w, int quality, int sampling) { return jpeg_file_bound_of(h, w, sampling, mcu_bits_max(quality, sampling)); }
constexpr size_t jpeg_file_bound(int h, int w) { return jpeg_file_bound_of(h, w, 0, kMcuBitsMax); }
constexpr size_t jpeg_base64_bound(int h, int w, int quality, int sampling) { return (jpeg_file_bound(h, w, quality, sampling) + 2) / 3 * 4; }
constexpr size_t jpeg_base64_bound(int h, int w) { return (jpeg_file_bound(h, w) + 2) / 3 * 4; }

// ---- the two size classes of jpeg.hip's interval kernel ---------------------------------------------------------------------------
// The kernel's LDS is sized by an interval's entropy-coded bytes BEFORE stuffing, at most raw_bound_of.  "Small" holds every setting
// whose bound is at most that of quality 85 at 4:2:0 (every quality up to 86 at 4:4:4 and up to 85 at 4:2:0), "big" holds quality 100
// at either sampling.  The rule stands here, not in jpeg.hip, so that tests/native/jpeg_opt_tables_dump.cpp can print it for every
// setting (tests/test_jpeg_opt_cases.py holds it against its restatement in Python).
constexpr unsigned raw_bound_of(int sampling, unsigned mcu_bits) { return ((unsigned)restart_mcus(sampling) * mcu_bits + 7) / 8; }
constexpr unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
constexpr unsigned kBits85[2] = {mcu_bits_max(85, 0), mcu_bits_max(85, 2)}, kBits100[2] = {mcu_bits_max(100, 0), mcu_bits_max(100, 2)};
constexpr unsigned kRawSmall = umax(raw_bound_of(0, kBits85[0]), raw_bound_of(2, kBits85[1]));       // 5034
constexpr unsigned kRawBig = umax(raw_bound_of(0, kBits100[0]), raw_bound_of(2, kBits100[1]));       // 9448
static_assert(kRawSmall == 5034 && kRawBig == 9448, "quality 85 and quality 100 at 4:2:0");
static_assert(kBits100[0] < kNoCode && kBits100[1] < kNoCode, "no bound prices a symbol the tables do not have");
constexpr bool big_class_of(int sampling, unsigned mcu_bits) { return raw_bound_of(sampling, mcu_bits) > kRawSmall; }
constexpr bool fits_a_class(int sampling, unsigned mcu_bits) { return raw_bound_of(sampling, mcu_bits) <= kRawBig; }
constexpr bool big_class(int quality, int sampling) { return big_class_of(sampling, mcu_bits_max(quality, sampling)); }

// ---- optimised Huffman tables: the bound under ANY table ---------------------------------------------------------------------------
// With the image's own tables (jpeg_huff_core.hpp) a symbol's code can be 16 bits, whatever the symbol.  Price each of a block's 64
// positions at 16 bits plus the largest category it can have (step 2): a coded coefficient costs at most that; a ZRL code (at most 16
// bits) stands for 16 zero positions and the EOB (at most 16 bits) for at least one, each of them priced at 16 bits or more.  At
// quality 100 that is 1665 bits per block (16 * 64 + 11 + 63 * 10) and 9990 bytes per interval of 48 blocks, above kRawBig (9448),
// which was sized under the fixed tables.  ONE size class, sized for quality 100: the optimised path runs a count pass and a table
// kernel beside the emit pass, so the emit pass's occupancy is a smaller share of its time than of the fixed path's, and the head's
// length (at most the fixed head's: a DC table has at most 12 symbols, an AC table 162) already varies per image.
constexpr unsigned block_bits_any(int table, int quality) {
    unsigned b = 0;
    for (int k = 0; k < 64; ++k) b += 16u + (unsigned)size_max(table, k, quality);
    return b;
}
constexpr unsigned mcu_bits_any(int quality, int sampling) { return (sampling == 2 ? 4u : 1u) * block_bits_any(0, quality) + 2 * block_bits_any(1, quality); }
constexpr unsigned kBitsAny100[2] = {mcu_bits_any(100, 0), mcu_bits_any(100, 2)};
constexpr unsigned kRawAny = umax(raw_bound_of(0, kBitsAny100[0]), raw_bound_of(2, kBitsAny100[1]));
static_assert(block_bits_any(0, 100) == 1665 && kRawAny == 9990, "48 blocks of 1665 bits");
static_assert(kRawAny >= kRawBig, "no table is worse than every table");
constexpr bool fits_any_class(int sampling, unsigned mcu_bits) { return raw_bound_of(sampling, mcu_bits) <= kRawAny; }      // (every setting: the dump checks all 200)
constexpr size_t jpeg_opt_file_bound(int h, int w, int quality, int sampling) { return jpeg_file_bound_of(h, w, sampling, mcu_bits_any(quality, sampling)); }
constexpr size_t jpeg_opt_base64_bound(int h, int w, int quality, int sampling) { return (jpeg_opt_file_bound(h, w, quality, sampling) + 2) / 3 * 4; }
// The head of such a file: the fixed parts of jpeg_header and four tables (bits_vals[4][jpeghuff::kBitsVals] and nvals[4], in the
// order of the DHT segments: 0x00, 0x10, 0x01, 0x11) -> out[<= kHeaderBytes]; returns its length.  Byte by byte through the function
// jpeg.hip's gather kernel uses.
inline size_t jpeg_header_opt(int h, int w, int quality, int sampling, const unsigned char* bits_vals, const int32_t* nvals, unsigned char* out) {
    const JpegHeader fixed = jpeg_header(h, w, quality, sampling);
    const unsigned n = jpeghuff::opt_head_bytes(nvals);
    for (unsigned k = 0; k < n && k < (unsigned)kHeaderBytes; ++k) out[k] = jpeghuff::opt_head_byte(k, fixed.b, bits_vals, nvals);
    return n;
}
static_assert(jpeghuff::kHeadFixedBytes == (unsigned)kHeaderBytes, "one head length");

// ---- progressive files (jpeg_progenc_core.hpp): the bound ---------------------------------------------------------------------------
// Ten scans, each under a table of its own, so a code has at most 16 bits.  Per scan and block:
//   DC first        16 + the largest category of a difference of two SHIFTED DCs: the quantised DC lies in -A..B (step 2), the
//                   shifted one in -ceil(A / 2^Al)..floor(B / 2^Al)
//   DC refinement   1 bit
//   AC first        every position of the band at 16 + the largest category of its magnitude after the shift (a ZRL stands for 16 zero
//                   positions, each priced at 16 or more), and one EOBn symbol with 14 extra bits
//   AC refinement   every position at 16 + 1 (the sign) + 1 (a correction bit), and one EOBn symbol with 14 extra bits
// An interval -- one block row of the scan -- is its blocks' bits rounded up to bytes, doubled for the stuffing, and 2 bytes of
// marker.  A scan's head is at most two DHT segments of 16 + 256 entries, a DRI and a three-component SOS.  The bound sizes the
// interval stride, the file's place and the public bound; ByteSink writes nothing beyond it.
constexpr unsigned kProgScanHeadMax = 2 * (5 + 16 + 256) + 6 + 14, kProgEobnBits = 16 + 14;
inline unsigned prog_block_bits(int scan, int comp, int quality) {
    const jpegprog::Scan sc = jpegprog::scan_of(scan);
    const int table = comp ? 1 : 0;
    if (sc.ss == 0) {
        if (sc.ah) return 1;
        const unsigned q = (unsigned)quant_at(table, 0, quality);
        const unsigned a = (kDcNegMax + 4u * q) / (8u * q), b = (kDcPosMax + 4u * q) / (8u * q), r = (1u << sc.al) - 1u;
        return 16u + (unsigned)bit_length((b >> sc.al) + ((a + r) >> sc.al));
    }
    if (sc.ah) return (unsigned)(sc.se - sc.ss + 1) * 18u + kProgEobnBits;
    unsigned bits = kProgEobnBits;
    for (int k = sc.ss; k <= sc.se; ++k) {
        const int nat = kZigzag[k];
        const unsigned q = (unsigned)quant_at(table, nat, quality);
        bits += 16u + (unsigned)bit_length(((coef_bound(nat) + 4u * q) / (8u * q)) >> sc.al);
    }
    return bits;
}
inline size_t prog_interval_bound(const jpegprog::Geom& g, int quality, int scan) {
    const jpegprog::Scan sc = jpegprog::scan_of(scan);
    const size_t bits = sc.ncomp == 3 ? (size_t)g.mw * ((g.sampling == 2 ? 4u : 1u) * prog_block_bits(scan, 0, quality) + 2u * prog_block_bits(scan, 1, quality))
                                      : (size_t)g.ocols[sc.comp] * prog_block_bits(scan, sc.comp, quality);
    return 2 * ((bits + 7) / 8) + 2;
}
inline size_t jpeg_prog_file_bound(int h, int w, int quality, int sampling) {
    const jpegprog::Geom g = jpegprog::geom_of(h, w, sampling);
    size_t n = jpegprog::kFixedHead + 2;
    for (int s = 0; s < jpegprog::kScans; ++s) n += kProgScanHeadMax + (size_t)jpegprog::scan_rows(g, s) * prog_interval_bound(g, quality, s);
    return n;
}
inline size_t jpeg_prog_base64_bound(int h, int w, int quality, int sampling) { return (jpeg_prog_file_bound(h, w, quality, sampling) + 2) / 3 * 4; }

}  // namespace jpegtab
}  // namespace ire
