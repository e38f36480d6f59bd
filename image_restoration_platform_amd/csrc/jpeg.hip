// jpeg.hip -- restored RGB pixels -> the base64 text of a baseline JPEG file, on the device.
//
// The two PNG results are large (4.2 MB of text per 1024^2 image stored, 0.5 - 0.93 of that Huffman-coded), and the hosts above the
// engine are bound by exactly that payload (profiles/r04_codec_seam.json).  This file writes a baseline sequential DCT file: Y Cb Cr in
// one interleaved scan, the standard's Annex K tables scaled to an IJG quality of 1..100, chroma at 4:4:4 or 4:2:0, and a restart
// interval of 48 blocks (16 MCUs at 4:4:4, 8 at 4:2:0) -- which is what makes the entropy coder parallel: an interval's bits depend on
// its own MCUs alone (DC predictors restart at 0, the interval ends on a byte).  The default, quality 85 at 4:4:4, is what the
// reference itself puts on the wire (imagePreprocess.js:57-64).  Every step is libjpeg's published integer algorithm;
// tests/jpeg_model.py and tests/jpeg_opt_model.py restate them, equal libjpeg-turbo's file byte for byte (tests/test_jpeg_model.py,
// tests/test_jpeg_opt_model.py), and the device's bytes equal the models' (tests/test_jpeg_gpu.py, tests/test_jpeg_opt_gpu.py, and
// tests/test_jpeg_opt_cases_gpu.py on the cases of tests/jpeg_opt_cases.py: the last category of either table, chains of ZRL codes,
// dummy blocks behind a full DC swing, both sides of the size-class switch, every job kind).
//
// Three launches per BATCH, none depending on n (image and interval are grid dimensions), no memset, no host round trip:
//   K1 jpeg_interval_kernel   one workgroup per restart interval: pixels -> LDS (edge replication by clamped coordinates), colour
//                             transform (at 4:2:0 with libjpeg's h2v2 downsample and its dummy blocks), the two DCT passes through
//                             LDS, quantiser + zig-zag, one WAVE per block for the symbols (lane k = coefficient k: runs from a
//                             ballot, bit offsets from a wave scan), MSB-first bit packing into LDS by atomic OR, byte stuffing, the
//                             interval's bytes with their RSTm / EOI marker and byte count to a fixed-stride scratch
//   K2 jpeg_gather_kernel     one workgroup per interval: prefix sum over the interval sizes, the interval's bytes to their place
//                             behind the head; the first writes the head, the last the two lengths
//   K3 deflate_base64_kernel  (deflate.hip) base64 over the device-side length
// Everything is integer work, LDS integer atomics and fixed-order sums: the bytes are a pure function of the pixels and the two
// settings.  The quantiser's tables and the file's head are built on the host from jpeg_tables.hpp per launch and travel as kernel
// arguments (768 and 629 bytes); K1 copies the tables to LDS, so one kernel body serves every quality.
//
// LDS.  The bit buffer and the stuffed bytes are sized by the worst interval, which grows with the quality (jpeg_tables.hpp: quality
// 100 is the worst).  Two size classes, a template parameter: "small" holds every setting whose interval bound is at most that of
// quality 85 at 4:2:0 (5034 bytes before stuffing; every quality up to 86 at 4:4:4 and up to 85 at 4:2:0), "big" holds quality 100;
// the rule is jpeg_tables.hpp::big_class_of, held on the CPU for all two hundred settings (tests/test_jpeg_opt_cases.py).  Per
// workgroup, of the CU's 160 KiB: small 4:4:4 31.1 KB (5 workgroups per CU, as before the settings existed: 30.0 KB), small 4:2:0
// 34.2 KB (4), big 4:4:4 35.5 KB (4), big 4:2:0 38.7 KB (4).
//
// Optimised Huffman tables (optimize: libjpeg's optimize_coding; tests/jpeg_huffopt_model.py equals Pillow's optimize=True file, the
// device equals the model: tests/test_jpeg_huffopt_gpu.py).  The file carries the image's own four tables.  A memset of the histograms
// and five launches per BATCH, none depending on n, no host round trip:
//   K1 in count mode          the same front end; the symbols of every block are counted into four LDS histograms (DC and AC, for Y and
//                             for Cb and Cr together) and those added to the image's in global memory by integer atomics
//   jpeg_table_kernel         one wave per (table, image): jpeg_huff_core.hpp turns a histogram into bits[16], vals[], the symbol count
//                             and the code array, in device scratch
//   K1 in emit mode           the front end again (the DCT is recomputed: storing the coefficients would write and read 6 bytes per
//                             pixel, more than the 3 bytes per pixel the second read of the pixels costs) with the image's codes in LDS
//   K2 with the head built from the fixed parts and the device's DHT segments, behind a per-image head length; K3 as it is
// Under an arbitrary table a code can be 16 bits whatever the symbol, so an interval is bounded by jpeg_tables.hpp::mcu_bits_any (9990
// bytes before stuffing at quality 100) and the emit pass has ONE size class of its own, kClassAny: 36.2 KB at 4:4:4, 39.3 KB at 4:2:0
// (4 workgroups per CU).  The count pass packs no bits and runs in the small class's LDS less the code tables: 28.8 / 32.0 KB (5).
// The fixed path's four instances are compiled from the same template and keep their LDS, registers and bytes.
#include "jpeg.hpp"

#include <atomic>

#include "deflate.hpp"
#include "jpeg_tables.hpp"
#include "png_bits.hpp"

namespace ire {

namespace {

using namespace jpegtab;
using pngbits::PngSrc;

constexpr int kThreads = 256;
constexpr int kBlocks = 48;                      // 8 x 8 blocks per interval at either sampling, in scan order
constexpr int kPlane = 72;                       // ints per block in LDS: rows of 9, so that neither DCT pass has a bank conflict
static_assert(kJpegR * 3 == kBlocks && kJpegR420 * 6 == kBlocks, "an interval is 48 blocks");

// what depends on the sampling (kSamp: 0 | 2) and the size class (jpeg_tables.hpp: raw_bound_of, kRawSmall, kRawBig, big_class_of; kRawAny:
// the one class of the optimised path, any table at quality 100)
constexpr int kClassSmall = 0, kClassBig = 1, kClassAny = 2;
template <int kSamp, int kClass>
struct Shape {
    static constexpr unsigned kWorstBits = kClass == kClassAny ? kBitsAny100[kSamp / 2] : kClass == kClassBig ? kBits100[kSamp / 2] : kBits85[kSamp / 2];
    static constexpr int kR = restart_mcus(kSamp);                  // MCUs per interval
    static constexpr int kP = mcu_pixels(kSamp);                    // an MCU's pixels per side
    static constexpr int kPer = kSamp == 2 ? 6 : 3;                 // blocks per MCU
    static constexpr int kRowDw = 3 * kP / 4;                       // dwords of one MCU's pixel row
    static constexpr int kPxWords = kR * kP * kRowDw;               // the interval's pixels: MCU m, row r at dword (m * kP + r) * kRowDw
    static constexpr unsigned kRawBytes = kClass == kClassAny ? kRawAny : kClass == kClassBig ? kRawBig : kRawSmall;
    static constexpr int kOutWords = (kRawBytes + 3) / 4 + 1;
    static constexpr unsigned kIntBound = 2 * kRawBytes + 2;        // stuffed, with the marker
    static constexpr int kStuffWords = (kIntBound + 3) / 4 + 1;     // (+ 1: the dword the gather may read behind the last byte)
    static constexpr unsigned kIntStride = (kStuffWords * 4 + 63) / 64 * 64;      // scratch bytes per interval
    static constexpr int kWorkWords = kPxWords + kBlocks * kPlane + kBlocks * 32; // pixels | DCT planes | quantised coefficients
    static_assert(kRawBytes >= raw_bound_of(kSamp, kWorstBits), "the class holds its worst quality");
    static_assert(kIntBound >= interval_bound_of(kR, kWorstBits), "and that interval stuffed");
    static_assert(kOutWords >= 4 * 256, "the count pass keeps its four histograms where the emit pass keeps its bits");
    static_assert(kWorkWords >= kStuffWords, "the stuffed bytes reuse the pixels, the DCT planes and the coefficients");
};
static_assert(Shape<0, kClassSmall>::kIntBound >= interval_bound(kJpegR), "the default's bound");

struct JpegGeom {
    int h, w;
    unsigned mcus_w;           // MCUs per row
    unsigned nmcu, nint;       // <= 2^20 MCUs, 2^16 intervals at 8192 x 8192
    unsigned mcu_bits;         // jpegtab::mcu_bits_max of the settings (optimised tables: mcu_bits_any)
    unsigned int_stride;       // scratch bytes per interval: Shape::kIntStride of the launch
    int quality, sampling;
    bool big;                  // the size class
    bool optimize;             // the image's own Huffman tables: the one class kClassAny
    unsigned long long file_bound;
};
// the bound of an MCU runs a dynamic programme over the Huffman tables: once per setting and process
unsigned mcu_bits_of(int quality, int sampling) {
    if (quality == kJpegQuality) return kBits85[sampling / 2];
    static std::atomic<unsigned> cache[101][2];
    std::atomic<unsigned>& c = cache[quality][sampling / 2];
    unsigned v = c.load(std::memory_order_relaxed);
    if (!v) { v = mcu_bits_max(quality, sampling); c.store(v, std::memory_order_relaxed); }
    return v;
}
JpegGeom geom_of(int h, int w, int quality, int sampling, bool optimize) {
    if (!settings_ok(quality, sampling)) fail(IRE_ERR_INVALID_INPUT, "invalid settings for the JPEG encoder (quality 1..100; sampling 0 = 4:4:4 or 2 = 4:2:0)");
    JpegGeom g;
    const unsigned p = (unsigned)mcu_pixels(sampling), r = (unsigned)restart_mcus(sampling);
    g.h = h; g.w = w; g.quality = quality; g.sampling = sampling;
    g.mcus_w = ((unsigned)w + p - 1) / p;
    g.nmcu = g.mcus_w * (((unsigned)h + p - 1) / p);
    g.nint = (g.nmcu + r - 1) / r;
    g.optimize = optimize;
    g.mcu_bits = optimize ? mcu_bits_any(quality, sampling) : mcu_bits_of(quality, sampling);
    g.big = !optimize && big_class_of(sampling, g.mcu_bits);
    if (!(optimize ? fits_any_class(sampling, g.mcu_bits) : fits_a_class(sampling, g.mcu_bits))) fail(IRE_ERR_INTERNAL, "internal: a JPEG interval bound beyond the largest size class");
    g.int_stride = optimize ? (sampling == 2 ? Shape<2, kClassAny>::kIntStride : Shape<0, kClassAny>::kIntStride) : sampling == 2 ? (g.big ? Shape<2, kClassBig>::kIntStride : Shape<2, kClassSmall>::kIntStride) : (g.big ? Shape<0, kClassBig>::kIntStride : Shape<0, kClassSmall>::kIntStride);
    g.file_bound = jpegtab::jpeg_file_bound_of(h, w, sampling, g.mcu_bits);
    return g;
}

// the quantiser per NATURAL index: the reciprocal of 8 q (jpeg_tables.hpp) and half the divisor; a kernel argument
struct QuantArg { unsigned recip[2][64]; unsigned short half[2][64]; };
QuantArg make_quant(int quality) {
    QuantArg q{};
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) { q.recip[t][k] = quant_recip(t, k, quality); q.half[t][k] = (unsigned short)(4 * quant_at(t, k, quality)); }
    return q;
}
struct ZigzagDev { unsigned char zzpos[64]; };      // the coefficient's zig-zag position per natural index
constexpr ZigzagDev make_zigzag() {
    ZigzagDev z{};
    for (int k = 0; k < 64; ++k) z.zzpos[kZigzag[k]] = (unsigned char)k;
    return z;
}
struct HuffDev { unsigned ac[2][256]; unsigned dc[2][12]; };      // value | length << 16
constexpr HuffDev make_huff() {
    HuffDev h{};
    for (int t = 0; t < 2; ++t) {
        const HuffCodes a = ac_codes(t), d = dc_codes(t);
        for (int s = 0; s < 256; ++s) h.ac[t][s] = a.code[s];
        for (int s = 0; s < 12; ++s) h.dc[t][s] = d.code[s];
    }
    return h;
}
__constant__ ZigzagDev kZ = make_zigzag();
__constant__ HuffDev kH = make_huff();

// ---- libjpeg's "islow" forward DCT (jfdctint.c): 13-bit constants, 2 extra bits kept between the passes -----------------------------
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633;
constexpr int F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool kFirst>
__device__ __forceinline__ void fdct_1d(int* d) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = kFirst ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
    if (kFirst) { d[0] = (t10 + t11) * (1 << kPass1Bits); d[4] = (t10 - t11) * (1 << kPass1Bits); }
    else { d[0] = descale(t10 + t11, kPass1Bits); d[4] = descale(t10 - t11, kPass1Bits); }
    const int z1 = (t12 + t13) * F_0_541196100;
    d[2] = descale(z1 + t13 * F_0_765366865, n);
    d[6] = descale(z1 - t12 * F_1_847759065, n);
    const int z5 = (t4 + t6 + t5 + t7) * F_1_175875602;
    const int y1 = -(t4 + t7) * F_0_899976223, y2 = -(t5 + t6) * F_2_562915447;
    const int y3 = -(t4 + t6) * F_1_961570560 + z5, y4 = -(t5 + t7) * F_0_390180644 + z5;
    d[7] = descale(t4 * F_0_298631336 + y1 + y3, n);
    d[5] = descale(t5 * F_2_053119869 + y2 + y4, n);
    d[3] = descale(t6 * F_3_072711026 + y2 + y3, n);
    d[1] = descale(t7 * F_1_501321110 + y1 + y4, n);
}

// MSB-first bit packer into a zeroed LDS buffer of nwords big-endian words: v (< 2^l, l in 1..32) at bit position pos, by atomic OR
__device__ __forceinline__ void put_bits(unsigned* out, unsigned nwords, unsigned pos, unsigned v, unsigned l) {
    const unsigned wi = pos >> 5, off = pos & 31u;
    const unsigned long long x = (unsigned long long)v << (64u - off - l);
    if (wi < nwords) atomicOr(&out[wi], (unsigned)(x >> 32));
    if (off + l > 32u && wi + 1 < nwords) atomicOr(&out[wi + 1], (unsigned)x);
}

// What lane `lane` of a wave sends for coefficient c (zig-zag position `lane`; lane 0 holds the DC DIFFERENCE) of a block whose
// non-zero AC positions are the set bits of mask: nzrl ZRL codes, then `bits` (nb of them: the symbol's code and the value's bits).
// kOwn: the DC codes are the image's own, in LDS (s_dc[2][16]); else the fixed ones in constant memory.
struct LaneSym { unsigned bits, nb, nzrl; };
template <bool kOwn>
__device__ __forceinline__ LaneSym lane_symbol(int c, unsigned lane, unsigned long long mask, int tb, const unsigned* s_ac, const unsigned* s_dc) {
    LaneSym o{0u, 0u, 0u};
    const unsigned mag = (unsigned)(c < 0 ? -c : c);
    const unsigned s = 32u - (unsigned)__clz((int)mag);                         // the magnitude category (__clz(0) = 32)
    const unsigned vb = (unsigned)(c < 0 ? c - 1 : c) & ((1u << s) - 1u);      // a negative value is sent as v - 1
    if (lane == 0) {
        const unsigned code = kOwn ? s_dc[tb * 16 + (s < 11u ? s : 11u)] : kH.dc[tb][s < 11u ? s : 11u];
        o.bits = ((code & 0xffffu) << s) | vb; o.nb = (code >> 16) + s;
    } else if (c != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const unsigned prev = below ? 63u - (unsigned)__clzll((long long)below) : 0u;
        const unsigned run = lane - prev - 1u;
        const unsigned code = s_ac[tb * 256 + (((run & 15u) << 4) | s)];
        o.bits = ((code & 0xffffu) << s) | vb; o.nb = (code >> 16) + s; o.nzrl = run >> 4;
    } else if (lane == 63) {                                                     // the last coefficient is zero: end of block
        const unsigned code = s_ac[tb * 256];
        o.bits = code & 0xffffu; o.nb = code >> 16;
    }
    return o;
}

// The interval's blocks in scan order.  4:4:4: block 3 m + c is component c of MCU m.  4:2:0: block 6 m + j is Y00 Y01 Y10 Y11 Cb Cr
// of MCU m.  table_of: 0 luminance, 1 chrominance.  pred_of: the block whose DC this block's is sent against, -1: none (0).  Three
// chains; at 4:2:0 Y's runs through the four blocks of an MCU and on to the next MCU's first.
template <int kSamp>
__device__ __forceinline__ int table_of(unsigned blk) { return kSamp == 2 ? (blk % 6u >= 4u ? 1 : 0) : (blk % 3u ? 1 : 0); }
template <int kSamp>
__device__ __forceinline__ int pred_of(unsigned blk) {
    if (kSamp != 2) return (int)blk - 3;
    const unsigned j = blk % 6u;
    if (j >= 1u && j < 4u) return (int)blk - 1;
    return j == 0u ? (int)blk - 3 : (int)blk - 6;                  // (negative in the first MCU: none)
}

// K1.  blockIdx.x: the interval, blockIdx.y: the image.  kMode: kEmitFixed, the fixed-table path; kCount, the optimised path's first
// pass: the same front end, but the symbols are counted into four LDS histograms (DHT order: DC 0, AC 0, DC 1, AC 1) and those added
// to the image's in `hist` -- integer sums, so their order does not matter; kEmitOwn, its second pass: the front end again
// (recomputing costs less than 6 bytes per pixel of coefficients written and read back) and the bits under the image's own codes,
// which the table kernel left in `codes` ([image][4][256], value | length << 16).
// kCoefs, the progressive path's coefficient pass (jpeg_progenc.hip): the same front end once per image, the quantised coefficients
// as int16 to the image's planes behind `intbuf` (jpeg_progenc_core.hpp: Geom), nothing else -- ten scans in two passes each would
// otherwise run the DCT twenty times, so there "store" beats "recompute".
constexpr int kEmitFixed = 0, kCount = 1, kEmitOwn = 2, kCoefs = 3;
template <int kSamp, int kClass, int kMode>
__global__ __launch_bounds__(kThreads) void jpeg_interval_kernel(PngSrc src, JpegGeom g, QuantArg qa, unsigned char* __restrict__ intbuf, unsigned* __restrict__ int_bytes,
                                                                  const unsigned* __restrict__ codes, unsigned* __restrict__ hist) {
    using S = Shape<kSamp, kClass>;
    constexpr bool kOwn = kMode == kEmitOwn;
    constexpr int kR = S::kR, kP = S::kP, kPer = S::kPer, kRowDw = S::kRowDw, kOutWords = S::kOutWords;
    __shared__ unsigned s_work[S::kWorkWords];                // pixels | planes | coefficients; later the stuffed bytes over all three
    __shared__ unsigned s_out[kOutWords];                     // the entropy-coded bits, big-endian words
    __shared__ unsigned s_ac[2 * 256 + (kOwn ? 2 * 16 : 0)];  // the AC codes; behind them the image's own DC codes (kEmitOwn)
    const unsigned* const s_dc = s_ac + 2 * 256;
    __shared__ unsigned s_recip[2 * 64];                      // the quantiser (QuantArg), natural order
    __shared__ unsigned short s_half[2 * 64];
    __shared__ unsigned s_blkoff[kBlocks + 1];
    __shared__ unsigned s_scan[kThreads / 64];
    __shared__ unsigned char s_dummy[kBlocks];                // 4:2:0: a Y block outside the image's own blocks (jpeg_opt_model.py)
    unsigned* const s_px = s_work;                            // the interval's pixels: MCU m, row r at byte (m * kP + r) * 3 kP
    int* const s_plane = reinterpret_cast<int*>(s_work + S::kPxWords);          // level-shifted samples, then coefficients
    short* const s_q = reinterpret_cast<short*>(s_work + S::kPxWords + kBlocks * kPlane);      // quantised coefficients, zig-zag order
    const unsigned iv = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned m0 = iv * (unsigned)kR;
    const unsigned nm = g.nmcu - m0 < (unsigned)kR ? g.nmcu - m0 : (unsigned)kR;
    const unsigned nblk = (unsigned)kPer * nm;
    const unsigned char* __restrict__ rgb = src.rgb + (unsigned long long)img * src.image_pitch;

    for (int k = t; k < kOutWords; k += kThreads) s_out[k] = 0;
    if (kOwn) {
        const unsigned* own = codes + (unsigned long long)img * (4 * 256);
        for (int k = t; k < 512; k += kThreads) s_ac[k] = own[(2 * (k >> 8) + 1) * 256 + (k & 255)];
        if (t < 32) s_ac[512 + t] = own[2 * (t >> 4) * 256 + (t & 15u)];
    } else if (kMode == kEmitFixed) {
        for (int k = t; k < 512; k += kThreads) s_ac[k] = kH.ac[k >> 8][k & 255];
    }
    if (t < 128) { s_recip[t] = qa.recip[t >> 6][t & 63u]; s_half[t] = qa.half[t >> 6][t & 63u]; }
    if (kSamp == 2 && t < nblk) {
        const unsigned m = t / 6u, j = t % 6u, mcu = m0 + m, my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
        s_dummy[t] = j < 4u && ((2 * mx + (j & 1u)) * 8 >= (unsigned)g.w || (2 * my + (j >> 1)) * 8 >= (unsigned)g.h) ? 1 : 0;
    }

    // 1. pixels -> LDS.  Item = one dword of one MCU's pixel row; consecutive threads take consecutive dwords of a pixel row across
    //    the interval's MCUs.  A dword that is 4-aligned in memory and inside the row is loaded whole, any other byte by byte with
    //    the coordinates clamped (edge replication).
    const unsigned row_bytes = 3u * (unsigned)g.w;
    for (unsigned idx = t; idx < (unsigned)S::kPxWords; idx += kThreads) {
        const unsigned r = idx / (kR * kRowDw), rem = idx % (kR * kRowDw), m = rem / kRowDw, k = rem % kRowDw;
        if (m >= nm) continue;
        const unsigned mcu = m0 + m, my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
        const unsigned y = min(my * kP + r, (unsigned)g.h - 1);
        const unsigned char* __restrict__ p = rgb + (unsigned long long)y * src.row_pitch;
        const unsigned b0 = mx * (3 * kP) + 4 * k;
        unsigned v;
        if (b0 + 4 <= row_bytes && ((reinterpret_cast<unsigned long long>(p) + b0) & 3u) == 0) v = *reinterpret_cast<const unsigned*>(p + b0);
        else {
            v = 0;
#pragma unroll
            for (unsigned b = 0; b < 4; ++b) {
                const unsigned x = min((b0 + b) / 3, (unsigned)g.w - 1), ch = (b0 + b) % 3;
                v |= (unsigned)p[3 * x + ch] << (8 * b);
            }
        }
        s_px[(m * kP + r) * kRowDw + k] = v;
    }
    __syncthreads();

    // 2. RGB -> Y Cb Cr (jccolor.c: 16-bit fixed point, + 32768 to round, chroma offset 128), level shift by 128
    const unsigned char* s_pb = reinterpret_cast<const unsigned char*>(s_px);
    if (kSamp != 2) {
        for (unsigned pix = t; pix < nm * 64; pix += kThreads) {
            const unsigned m = pix >> 6, r = (pix >> 3) & 7u, c = pix & 7u;
            const unsigned char* q = s_pb + (m * 8 + r) * 24 + 3 * c;
            const int R = q[0], G = q[1], B = q[2];
            int* o = s_plane + 3 * m * kPlane + r * 9 + c;
            o[0] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
            o[kPlane] = ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128;
            o[2 * kPlane] = ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128;
        }
    } else {
        // Y of every pixel of the 16 x 16 MCU into its four blocks (the clamped load is libjpeg's padding of Y; a dummy block's
        // samples are never used)
        for (unsigned pix = t; pix < nm * 256; pix += kThreads) {
            const unsigned m = pix >> 8, r = (pix >> 4) & 15u, c = pix & 15u;
            const unsigned char* q = s_pb + (m * 16 + r) * 48 + 3 * c;
            const int R = q[0], G = q[1], B = q[2];
            s_plane[(6 * m + 2 * (r >> 3) + (c >> 3)) * kPlane + (r & 7u) * 9 + (c & 7u)] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
        }
        // Cb and Cr: jcsample.c's h2v2_downsample, (a + b + c + d + bias) >> 2 over the 2 x 2 cell, bias 1 in even output columns and
        // 2 in odd ones.  To the right the cell's pixels are the clamped load's (the last column replicated).  Downwards libjpeg
        // replicates the last DOWNSAMPLED row, which took rows 2 J and min(2 J + 1, h - 1), J = ceil(h / 2) - 1: so chroma row cy
        // takes the cell of row min(cy, J), whose second row is again the clamped load's.
        const unsigned last_cy = ((unsigned)g.h + 1) / 2 - 1;
        for (unsigned idx = t; idx < nm * 64; idx += kThreads) {
            const unsigned m = idx >> 6, cr = (idx >> 3) & 7u, cc = idx & 7u;
            const unsigned my = (m0 + m) / g.mcus_w;
            const unsigned la = 2 * (min(my * 8 + cr, last_cy) - my * 8);      // the cell's first row inside the MCU: 0..14
            const unsigned char* q = s_pb + (m * 16 + la) * 48 + 6 * cc;
            int cb = (int)(cc & 1u) + 1, crv = cb;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned char* e = q + (k >> 1) * 48 + (k & 1) * 3;
                const int R = e[0], G = e[1], B = e[2];
                cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                crv += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            }
            int* o = s_plane + (6 * m + 4) * kPlane + cr * 9 + cc;
            o[0] = (cb >> 2) - 128;
            o[kPlane] = (crv >> 2) - 128;
        }
    }
    __syncthreads();

    // 3. the DCT: rows, then columns; item = one row / one column of one block.  4. quantiser and zig-zag behind the column pass.
    for (unsigned item = t; item < nblk * 8; item += kThreads) {
        int* p = s_plane + (item >> 3) * kPlane + (item & 7u) * 9;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        fdct_1d<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = d[k];
    }
    __syncthreads();
    for (unsigned item = t; item < nblk * 8; item += kThreads) {
        const unsigned blk = item >> 3, col = item & 7u;
        const int tb = table_of<kSamp>(blk);
        const bool dummy = kSamp == 2 && s_dummy[blk];
        const int* p = s_plane + blk * kPlane + col;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[9 * k];
        fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned nat = 8 * k + col;
            const unsigned mag = (unsigned)(d[k] < 0 ? -d[k] : d[k]) + s_half[tb * 64 + nat];
            const int qv = (int)__umulhi(mag, s_recip[tb * 64 + nat]);         // floor(mag / (8 q)): jpeg_tables.hpp
            s_q[blk * 64 + kZ.zzpos[nat]] = dummy ? (short)0 : (short)(d[k] < 0 ? -qv : qv);
        }
    }
    __syncthreads();
    if (kSamp == 2) {
        // a dummy block's quantised DC is that of the block before it in the MCU (jccoefct.c): one thread per MCU walks its Y blocks
        if (t < nm)
            for (unsigned j = 1; j < 4; ++j)
                if (s_dummy[6 * t + j]) s_q[(6 * t + j) * 64] = s_q[(6 * t + j - 1) * 64];
        __syncthreads();
    }

    if constexpr (kMode == kCoefs) {
        // the interval's blocks to their places in the component planes, a dword (two coefficients) per thread and step
        const jpegprog::Geom pg = jpegprog::geom_of(g.h, g.w, kSamp);
        unsigned* const planes = reinterpret_cast<unsigned*>(intbuf) + (unsigned long long)img * pg.nblocks * 32ull;
        const unsigned* const s_qw = s_work + S::kPxWords + kBlocks * kPlane;
        for (unsigned idx = t; idx < nblk * 32u; idx += kThreads) {
            const unsigned blk = idx >> 5, m = blk / (unsigned)kPer, j = blk % (unsigned)kPer, mcu = m0 + m, my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
            unsigned comp, by, bx;
            if (kSamp == 2 && j < 4u) { comp = 0; by = 2 * my + (j >> 1); bx = 2 * mx + (j & 1u); }
            else { comp = kSamp == 2 ? j - 3u : j; by = my; bx = mx; }
            planes[((unsigned long long)jpegprog::comp_off(pg, (int)comp) + (unsigned long long)by * jpegprog::y_or_c(pg.cols[0], pg.cols[1], (int)comp) + bx) * 32ull + (idx & 31u)] = s_qw[idx];
        }
        return;
    }
    const unsigned wv = t >> 6, lane = t & 63u;
    if constexpr (kMode == kCount) {
        // 5c. the symbols counted: one wave per block, lane k = zig-zag position k, as the emit pass finds them below
        unsigned* const s_hist = s_out;                          // (zeroed above) [DC 0 | AC 0 | DC 1 | AC 1][256]
        for (unsigned blk = wv; blk < nblk; blk += kThreads / 64) {
            int c = s_q[blk * 64 + lane];
            const int pb = pred_of<kSamp>(blk);
            if (lane == 0 && pb >= 0) c -= s_q[pb * 64];
            const unsigned long long mask = __ballot(c != 0) & ~1ull;
            unsigned* const h = s_hist + table_of<kSamp>(blk) * 512;
            const unsigned mag = (unsigned)(c < 0 ? -c : c);
            const unsigned s = 32u - (unsigned)__clz((int)mag);
            if (lane == 0) atomicAdd(&h[s < 11u ? s : 11u], 1u);
            else if (c != 0) {
                const unsigned long long below = mask & ((1ull << lane) - 1ull);
                const unsigned prev = below ? 63u - (unsigned)__clzll((long long)below) : 0u;
                const unsigned run = lane - prev - 1u;
                atomicAdd(&h[256 + (((run & 15u) << 4) | (s & 15u))], 1u);
                if (run >> 4) atomicAdd(&h[256 + 0xf0], run >> 4);
            } else if (lane == 63) atomicAdd(&h[256], 1u);
        }
        __syncthreads();
        unsigned* const dst = hist + (unsigned long long)img * (4 * 256);
        for (unsigned k = t; k < 4 * 256; k += kThreads) { const unsigned v = s_hist[k]; if (v) atomicAdd(&dst[k], v); }
        return;
    }
    // 5. bits per block: one wave per block, lane k = zig-zag position k.  The DC differences need no order: every DC is known.
    for (unsigned blk = wv; blk < nblk; blk += kThreads / 64) {
        int c = s_q[blk * 64 + lane];
        const int pb = pred_of<kSamp>(blk);
        if (lane == 0 && pb >= 0) c -= s_q[pb * 64];
        const unsigned long long mask = __ballot(c != 0) & ~1ull;
        const int tb = table_of<kSamp>(blk);
        const LaneSym sy = lane_symbol<kOwn>(c, lane, mask, tb, s_ac, s_dc);
        unsigned bits = sy.nb + sy.nzrl * (s_ac[tb * 256 + 0xf0] >> 16);
        for (int off = 32; off >= 1; off >>= 1) bits += __shfl_down(bits, off, 64);
        if (lane == 0) s_blkoff[blk + 1] = bits;
    }
    __syncthreads();
    // 6. bit offsets of the blocks (at most 48 of them: one thread)
    if (t == 0) {
        unsigned run = 0;
        s_blkoff[0] = 0;
        for (unsigned b = 1; b <= nblk; ++b) { run += s_blkoff[b]; s_blkoff[b] = run; }
    }
    __syncthreads();
    // 7. emit: a wave scan gives each lane its place in the block
    for (unsigned blk = wv; blk < nblk; blk += kThreads / 64) {
        int c = s_q[blk * 64 + lane];
        const int pb = pred_of<kSamp>(blk);
        if (lane == 0 && pb >= 0) c -= s_q[pb * 64];
        const unsigned long long mask = __ballot(c != 0) & ~1ull;
        const int tb = table_of<kSamp>(blk);
        const LaneSym sy = lane_symbol<kOwn>(c, lane, mask, tb, s_ac, s_dc);
        const unsigned zrl = s_ac[tb * 256 + 0xf0];
        const unsigned mine = sy.nb + sy.nzrl * (zrl >> 16);
        unsigned inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc += o; }
        unsigned pos = s_blkoff[blk] + inc - mine;
        for (unsigned k = 0; k < sy.nzrl; ++k) { put_bits(s_out, kOutWords, pos, zrl & 0xffffu, zrl >> 16); pos += zrl >> 16; }
        if (sy.nb) put_bits(s_out, kOutWords, pos, sy.bits, sy.nb);
    }
    const unsigned total_bits = s_blkoff[nblk];
    unsigned raw = (total_bits + 7) / 8;                         // bytes before stuffing; the last one is padded with 1-bits
    if (raw > S::kRawBytes) raw = S::kRawBytes;                  // (cannot happen: jpeg_tables.hpp; nothing is ever written past the bound)
    if (t == 0 && (total_bits & 7u)) put_bits(s_out, kOutWords, total_bits, (1u << (8 - (total_bits & 7u))) - 1u, 8 - (total_bits & 7u));
    __syncthreads();

    // 8. stuffing: thread t takes bytes [per t, per t + per); a scan over the 0xFF counts gives each byte its place
    const unsigned per = (raw + kThreads - 1) / kThreads;
    const unsigned i0 = min(t * per, raw), i1 = min(i0 + per, raw);
    unsigned nff = 0;
    for (unsigned i = i0; i < i1; ++i) nff += ((s_out[i >> 2] >> (24 - 8 * (i & 3u))) & 0xffu) == 0xffu ? 1u : 0u;
    unsigned inc = nff;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc += o; }
    if (lane == 63) s_scan[wv] = inc;
    __syncthreads();
    unsigned before = inc - nff, all_ff = 0;
#pragma unroll
    for (unsigned k = 0; k < kThreads / 64; ++k) { const unsigned x = s_scan[k]; if (k < wv) before += x; all_ff += x; }
    unsigned char* s_st = reinterpret_cast<unsigned char*>(s_work);            // (pixels, planes and coefficients were last read before two barriers)
    unsigned o = i0 + before;
    for (unsigned i = i0; i < i1; ++i) {
        const unsigned b = (s_out[i >> 2] >> (24 - 8 * (i & 3u))) & 0xffu;
        if (o < S::kIntBound) s_st[o] = (unsigned char)b;
        ++o;
        if (b == 0xffu) { if (o < S::kIntBound) s_st[o] = 0; ++o; }
    }
    unsigned bytes = raw + all_ff + 2;
    const unsigned bound = (unsigned)interval_bound_of(nm, g.mcu_bits);      // (<= S::kIntBound: geom_of chose the class by it)
    if (bytes > bound) bytes = bound;
    if (t == 0) {                                                // RST(m mod 8) behind every interval but the last, EOI behind the last
        s_st[bytes - 2] = 0xff;
        s_st[bytes - 1] = iv + 1 == g.nint ? 0xd9 : (unsigned char)(0xd0 + (iv & 7u));
    }
    __syncthreads();
    // 9. the interval's bytes and their count to the scratch
    const unsigned long long slot = (unsigned long long)img * g.nint + iv;
    unsigned* dst = reinterpret_cast<unsigned*>(intbuf + slot * g.int_stride);
    for (unsigned k = t; k < (bytes + 3) / 4 + 1; k += kThreads) dst[k] = s_work[k];      // (+ 1: the dword the gather may read behind the last byte)
    if (t == 0) int_bytes[slot] = bytes;
}

// The optimised path's table kernel, between its two passes: one wave per (table, image) turns a histogram into the table as its DHT
// segment carries it (bits[16] | vals[256]), its symbol count and the code array the emit pass reads.  jpeg_huff_core.hpp holds the
// algorithm (tests/native/jpeg_huffopt_dump.cpp runs it on the CPU); here the wave is a wave.
// The wave-wide minimum is on the merge loop's critical path twice per merge, so it goes through DPP moves, not through LDS
// permutes: shifts by 1, 2, 4 and 8 inside the rows of 16 lanes (a lane without a source keeps its own value), then lane 15 of a
// row to the next row (rows 1 and 3), then lane 31 to rows 2 and 3; lane 63 holds the minimum, read into scalar registers.  All
// 64 lanes are active wherever this is called.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long dpp_min64(unsigned long long v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, kRowMask, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, kRowMask, 0xf, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o < v ? o : v;
}
struct DevWave {
    struct Own { jpeghuff::Entries e; __device__ __forceinline__ jpeghuff::Entries& operator[](unsigned) { return e; } };
    unsigned lane;
    template <typename F> __device__ __forceinline__ void lanes(F f) { f(lane); }
    template <typename F> __device__ __forceinline__ unsigned long long min64(F f) {
        unsigned long long v = f(lane);
        v = dpp_min64<0x111, 0xf>(v);      // row_shr:1
        v = dpp_min64<0x112, 0xf>(v);      // row_shr:2
        v = dpp_min64<0x114, 0xf>(v);      // row_shr:4
        v = dpp_min64<0x118, 0xf>(v);      // row_shr:8
        v = dpp_min64<0x142, 0xa>(v);      // row_bcast:15
        v = dpp_min64<0x143, 0xc>(v);      // row_bcast:31
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
        return ((unsigned long long)hi << 32) | lo;
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void add1(int& x) { atomicAdd(&x, 1); }
};
__global__ __launch_bounds__(jpeghuff::kLanes) void jpeg_table_kernel(const unsigned* hist, unsigned char* bits_vals, int* nvals, unsigned* codes) {
    __shared__ jpeghuff::Work s_work;
    DevWave wv{threadIdx.x};
    const unsigned long long slot = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;      // (4 tables per image, or the progressive path's 10)
    jpeghuff::build_table(wv, s_work, hist + slot * 256, bits_vals + slot * jpeghuff::kBitsVals, nvals + slot, codes ? codes + slot * 256 : nullptr);
}

// K2.  The interval's bytes to their place in the file; the head by interval 0, the lengths by the last interval.  kOwn: the head
// carries the image's own tables (bits_vals, nvals: the table kernel's), so its length is the image's own too.
template <bool kOwn>
__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(JpegGeom g, JpegHeader head, const unsigned char* __restrict__ intbuf, const unsigned* __restrict__ int_bytes,
                                                                unsigned char* __restrict__ files, unsigned long long file_pitch, unsigned long long* __restrict__ flen,
                                                                unsigned char* __restrict__ lens, unsigned long long lens_pitch,
                                                                const unsigned char* __restrict__ bits_vals, const int* __restrict__ nvals) {
    __shared__ unsigned s_red[2][kThreads / 64];
    const unsigned iv = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned* sizes = int_bytes + (unsigned long long)img * g.nint;
    unsigned before = 0, all = 0;                                 // (integers: a sum in any order; < 2^16 * 18898 < 2^31)
    for (unsigned k = t; k < g.nint; k += kThreads) { const unsigned s = sizes[k]; all += s; if (k < iv) before += s; }
    for (int off = 32; off >= 1; off >>= 1) { before += __shfl_down(before, off, 64); all += __shfl_down(all, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = before; s_red[1][t >> 6] = all; }
    __syncthreads();
    before = all = 0;
    for (int k = 0; k < kThreads / 64; ++k) { before += s_red[0][k]; all += s_red[1][k]; }
    unsigned char* __restrict__ file = files + (unsigned long long)img * file_pitch;
    const unsigned char* __restrict__ srcb = intbuf + ((unsigned long long)img * g.nint + iv) * g.int_stride;
    const unsigned size = sizes[iv];
    const unsigned head_len = kOwn ? jpeghuff::opt_head_bytes(nvals + 4ull * img) : (unsigned)kHeaderBytes;
    const unsigned d0 = head_len + before;                        // file offset of the interval's first byte (file_pitch is a multiple of 4)
    // [d0, d0 + size): bytes up to the first dword boundary, whole dwords, bytes again: no dword is shared with a neighbour's stores
    const unsigned hd = (4u - (d0 & 3u)) & 3u;
    const unsigned nhead = hd < size ? hd : size;
    const unsigned ndw = (size - nhead) / 4, ntail = size - nhead - 4 * ndw;
    if (t < nhead) file[d0 + t] = srcb[t];
    const unsigned* srcw = reinterpret_cast<const unsigned*>(srcb);
    const unsigned sh = 8 * (nhead & 3u);                         // source dword q holds bytes 4 q ..; the output's dword k starts at source byte nhead + 4 k
    unsigned* dstw = reinterpret_cast<unsigned*>(file + d0 + nhead);
    for (unsigned k = t; k < ndw; k += kThreads) {
        const unsigned q = (nhead + 4 * k) >> 2;
        const unsigned lo = srcw[q], hi = srcw[q + 1];
        dstw[k] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    if (t < ntail) file[d0 + nhead + 4 * ndw + t] = srcb[nhead + 4 * ndw + t];
    if (iv == 0) {
        if (kOwn) for (unsigned k = t; k < head_len; k += kThreads) file[k] = jpeghuff::opt_head_byte(k, head.b, bits_vals + 4ull * jpeghuff::kBitsVals * img, nvals + 4ull * img);
        else for (unsigned k = t; k < (unsigned)kHeaderBytes; k += kThreads) file[k] = head.b[k];      // (jpeg_header of the launch's h, w and settings)
    }
    if (iv + 1 == g.nint) {
        const unsigned long long fl = (unsigned long long)head_len + all;
        if (t < 48) { const unsigned long long o = fl + t; if (o < file_pitch) file[o] = 0; }      // what the last base64 thread reads behind the file
        if (t == 64) {
            flen[img] = fl;
            const unsigned long long chars = (fl + 2) / 3 * 4;
            unsigned char* lp = lens + (unsigned long long)img * lens_pitch;
            if ((reinterpret_cast<unsigned long long>(lp) & 7u) == 0) *reinterpret_cast<unsigned long long*>(lp) = chars;
            else for (int k = 0; k < 8; ++k) lp[k] = (unsigned char)(chars >> (8 * k));
        }
    }
}

struct ScratchLayout { size_t flen, int_bytes, intbuf, files, file_pitch, hist, codes, bits_vals, nvals, total; };
ScratchLayout layout_of(int n, const JpegGeom& g) {
    ScratchLayout L;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.flen = 0;                                                      // n x u64
    L.int_bytes = up((size_t)n * 8);                                 // n x nint u32
    L.intbuf = up(L.int_bytes + (size_t)n * g.nint * 4);             // n x nint x int_stride
    L.files = up(L.intbuf + (size_t)n * g.nint * g.int_stride);
    L.file_pitch = up(((size_t)g.file_bound + 11) / 12 * 12 + 16);   // (the 12-byte groups of the last base64 threads stay inside)
    L.total = L.files + L.file_pitch * (size_t)n;
    L.hist = L.codes = L.bits_vals = L.nvals = 0;
    if (g.optimize) {                                                // per image and table: 256 counts | 256 codes | bits and vals | the symbol count
        L.hist = up(L.total);
        L.codes = L.hist + (size_t)n * 4 * 256 * 4;
        L.bits_vals = L.codes + (size_t)n * 4 * 256 * 4;
        L.nvals = up(L.bits_vals + (size_t)n * 4 * jpeghuff::kBitsVals);
        L.total = L.nvals + (size_t)n * 4 * 4;
    }
    return L;
}

}  // namespace

size_t jpeg_file_bound(int h, int w, int quality, int sampling, bool optimize) { return geom_of(h, w, quality, sampling, optimize).file_bound; }
size_t jpeg_base64_bound(int h, int w, int quality, int sampling, bool optimize) { return ((size_t)geom_of(h, w, quality, sampling, optimize).file_bound + 2) / 3 * 4; }
size_t jpeg_scratch_bytes(int n, int h, int w, int quality, int sampling, bool optimize) { return layout_of(n, geom_of(h, w, quality, sampling, optimize)).total; }

void encode_jpeg_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch, unsigned char* d_chars,
                               size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, int quality, int sampling, bool optimize, hipStream_t s) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG encoder (1..8192 per side)");
    if (row_pitch < (size_t)3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row pitch for the JPEG encoder (< 3*w)");
    const JpegGeom g = geom_of(h, w, quality, sampling, optimize);
    const ScratchLayout L = layout_of(n, g);
    unsigned long long* flen = reinterpret_cast<unsigned long long*>(d_scratch + L.flen);
    unsigned* int_bytes = reinterpret_cast<unsigned*>(d_scratch + L.int_bytes);
    unsigned char* intbuf = d_scratch + L.intbuf;
    unsigned char* files = d_scratch + L.files;
    const PngSrc src{d_rgb, (unsigned long long)row_pitch, (unsigned long long)image_pitch};
    const QuantArg qa = make_quant(quality);
    const dim3 grid(g.nint, n);
    const unsigned* no_codes = nullptr;
    unsigned* no_hist = nullptr;
    if (optimize) {
        // count pass | table kernel | emit pass: a memset and two launches more than the fixed path, none depending on n
        unsigned* hist = reinterpret_cast<unsigned*>(d_scratch + L.hist);
        unsigned* codes = reinterpret_cast<unsigned*>(d_scratch + L.codes);
        unsigned char* bits_vals = d_scratch + L.bits_vals;
        int* nvals = reinterpret_cast<int*>(d_scratch + L.nvals);
        IRE_HIP(hipMemsetAsync(hist, 0, (size_t)n * 4 * 256 * 4, s));
        if (sampling == 2) hipLaunchKernelGGL((jpeg_interval_kernel<2, kClassSmall, kCount>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, hist);
        else hipLaunchKernelGGL((jpeg_interval_kernel<0, kClassSmall, kCount>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, hist);
        hipLaunchKernelGGL(jpeg_table_kernel, dim3(4, n), dim3(jpeghuff::kLanes), 0, s, (const unsigned*)hist, bits_vals, nvals, codes);
        if (sampling == 2) hipLaunchKernelGGL((jpeg_interval_kernel<2, kClassAny, kEmitOwn>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, (const unsigned*)codes, no_hist);
        else hipLaunchKernelGGL((jpeg_interval_kernel<0, kClassAny, kEmitOwn>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, (const unsigned*)codes, no_hist);
        hipLaunchKernelGGL(jpeg_gather_kernel<true>, grid, dim3(kThreads), 0, s, g, jpeg_header(h, w, quality, sampling), intbuf, int_bytes, files, (unsigned long long)L.file_pitch,
                           flen, d_lens, (unsigned long long)lens_pitch, (const unsigned char*)bits_vals, (const int*)nvals);
        base64_device_length_launch(files, L.file_pitch, flen, (size_t)g.file_bound, n, d_chars, text_pitch, s);
        IRE_HIP(hipGetLastError());
        return;
    }
    const unsigned char* no_tables = nullptr;
    const int* no_nvals = nullptr;
    if (sampling == 2) {
        if (g.big) hipLaunchKernelGGL((jpeg_interval_kernel<2, kClassBig, kEmitFixed>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, no_hist);
        else hipLaunchKernelGGL((jpeg_interval_kernel<2, kClassSmall, kEmitFixed>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, no_hist);
    } else {
        if (g.big) hipLaunchKernelGGL((jpeg_interval_kernel<0, kClassBig, kEmitFixed>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, no_hist);
        else hipLaunchKernelGGL((jpeg_interval_kernel<0, kClassSmall, kEmitFixed>), grid, dim3(kThreads), 0, s, src, g, qa, intbuf, int_bytes, no_codes, no_hist);
    }
    hipLaunchKernelGGL(jpeg_gather_kernel<false>, grid, dim3(kThreads), 0, s, g, jpeg_header(h, w, quality, sampling), intbuf, int_bytes, files, (unsigned long long)L.file_pitch, flen,
                       d_lens, (unsigned long long)lens_pitch, no_tables, no_nvals);
    base64_device_length_launch(files, L.file_pitch, flen, (size_t)g.file_bound, n, d_chars, text_pitch, s);
    IRE_HIP(hipGetLastError());
}

// The progressive path's coefficient pass (jpeg_progenc.hip): the front end of K1 alone, one workgroup per 48 blocks in MCU order
void jpeg_coefs_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, int quality, int sampling, short* d_coefs, hipStream_t s) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG encoder (1..8192 per side)");
    if (row_pitch < (size_t)3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row pitch for the JPEG encoder (< 3*w)");
    const JpegGeom g = geom_of(h, w, quality, sampling, false);
    const PngSrc src{d_rgb, (unsigned long long)row_pitch, (unsigned long long)image_pitch};
    const QuantArg qa = make_quant(quality);
    unsigned* no_u = nullptr;
    const unsigned* no_codes = nullptr;
    unsigned char* planes = reinterpret_cast<unsigned char*>(d_coefs);
    if (sampling == 2) hipLaunchKernelGGL((jpeg_interval_kernel<2, kClassSmall, kCoefs>), dim3(g.nint, n), dim3(kThreads), 0, s, src, g, qa, planes, no_u, no_codes, no_u);
    else hipLaunchKernelGGL((jpeg_interval_kernel<0, kClassSmall, kCoefs>), dim3(g.nint, n), dim3(kThreads), 0, s, src, g, qa, planes, no_u, no_codes, no_u);
    IRE_HIP(hipGetLastError());
}

// The table kernel on ntab histograms per image, with the code arrays (the progressive path: ntab = 10)
void jpeg_tables_launch(const unsigned* d_counts, int ntab, int n, unsigned char* d_bits_vals, int* d_nvals, unsigned* d_codes, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_table_kernel, dim3(ntab, n), dim3(jpeghuff::kLanes), 0, s, d_counts, d_bits_vals, d_nvals, d_codes);
    IRE_HIP(hipGetLastError());
}

// The table kernel alone (ire_debug_jpeg_huffman): n x 4 histograms of 256 counts on the device -> their tables and symbol counts
void jpeg_huffman_tables_launch(const unsigned* d_counts, int n, unsigned char* d_bits_vals, int* d_nvals, hipStream_t s) {
    unsigned* no_codes = nullptr;
    hipLaunchKernelGGL(jpeg_table_kernel, dim3(4, n), dim3(jpeghuff::kLanes), 0, s, d_counts, d_bits_vals, d_nvals, no_codes);
    IRE_HIP(hipGetLastError());
}

}  // namespace ire
