// jpeg.hip -- restored RGB pixels -> the base64 text of a baseline JPEG file, on the device.
//
// The two PNG results are large (4.2 MB of text per 1024^2 image stored, 0.5 - 0.93 of that Huffman-coded), and the hosts above the
// engine are bound by exactly that payload (profiles/r04_codec_seam.json).  This file writes what the reference itself puts on the
// wire (imagePreprocess.js:57-64: JPEG, quality 85, 4:4:4): baseline sequential DCT, Y Cb Cr at 1 x 1 each, one interleaved scan, the
// standard's Annex K tables, and a restart interval of 16 MCUs -- which is what makes the entropy coder parallel: an interval's bits
// depend on its own MCUs alone (DC predictors restart at 0, the interval ends on a byte).  Every step is libjpeg's published integer
// algorithm; tests/jpeg_model.py restates them, equals libjpeg-turbo's file byte for byte (tests/test_jpeg_model.py), and the
// device's bytes equal the model's (tests/test_jpeg_gpu.py).
//
// Three launches per BATCH, none depending on n (image and interval are grid dimensions), no memset, no host round trip:
//   K1 jpeg_interval_kernel   one workgroup per restart interval: pixels -> LDS (edge replication by clamped coordinates), colour
//                             transform, the two DCT passes through LDS, quantiser + zig-zag, one WAVE per block for the symbols
//                             (lane k = coefficient k: runs from a ballot, bit offsets from a wave scan), MSB-first bit packing into
//                             LDS by atomic OR, byte stuffing, the interval's bytes with their RSTm / EOI marker and byte count to a
//                             fixed-stride scratch
//   K2 jpeg_gather_kernel     one workgroup per interval: prefix sum over the interval sizes, the interval's bytes to their place
//                             behind the head; the first writes the head, the last the two lengths
//   K3 deflate_base64_kernel  (deflate.hip) base64 over the device-side length
// Everything is integer work, LDS integer atomics and fixed-order sums: the bytes are a pure function of the pixels.
#include "jpeg.hpp"

#include "deflate.hpp"
#include "jpeg_tables.hpp"
#include "png_bits.hpp"

namespace ire {

namespace {

using namespace jpegtab;
using pngbits::PngSrc;

constexpr int kThreads = 256;
constexpr int kR = kJpegR;                       // MCUs per interval
constexpr int kBlocks = 3 * kR;                  // 8 x 8 blocks per interval, in scan order: block 3 m + c is component c of MCU m
constexpr int kPlane = 72;                       // ints per block in LDS: rows of 9, so that neither DCT pass has a bank conflict
constexpr unsigned kRawBytes = (kR * kMcuBitsMax + 7) / 8;                 // 4686: an interval's entropy-coded bytes before stuffing
constexpr int kOutWords = (kRawBytes + 3) / 4 + 1;
constexpr unsigned kIntBound = (unsigned)interval_bound(kR);               // 9374: stuffed, with the marker
constexpr int kStuffWords = (kIntBound + 3) / 4 + 1;                       // (+ 1: the dword the gather may read behind the last byte)
constexpr unsigned kIntStride = (kStuffWords * 4 + 63) / 64 * 64;          // scratch bytes per interval
static_assert(kBlocks * kPlane >= kStuffWords, "the stuffed bytes reuse the DCT planes");

struct JpegGeom {
    int h, w;
    unsigned mcus_w;           // MCUs per row
    unsigned nmcu, nint;       // <= 2^20 MCUs, 2^16 intervals at 8192 x 8192
    unsigned long long file_bound;
};
JpegGeom geom_of(int h, int w) {
    JpegGeom g;
    g.h = h; g.w = w;
    g.mcus_w = (unsigned)(w + 7) / 8;
    g.nmcu = g.mcus_w * ((unsigned)(h + 7) / 8);
    g.nint = (g.nmcu + kR - 1) / kR;
    g.file_bound = jpegtab::jpeg_file_bound(h, w);
    return g;
}

// the quantiser per NATURAL index: the reciprocal of 8 q (jpeg_tables.hpp), half the divisor, the coefficient's zig-zag position
struct QuantDev { unsigned recip[2][64]; unsigned short half[2][64]; unsigned char zzpos[64]; };
constexpr QuantDev make_quant() {
    QuantDev q{};
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) { q.recip[t][k] = quant_recip(t, k); q.half[t][k] = (unsigned short)(4 * quant_at(t, k)); }
    for (int k = 0; k < 64; ++k) q.zzpos[kZigzag[k]] = (unsigned char)k;
    return q;
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
__constant__ QuantDev kQ = make_quant();
__constant__ HuffDev kH = make_huff();
__constant__ JpegHeader kHead = jpeg_header(0, 0);      // the gather fills in SOF0's height and width

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

// MSB-first bit packer into a zeroed LDS buffer of big-endian words: v (< 2^l, l in 1..32) at bit position pos, by atomic OR
__device__ __forceinline__ void put_bits(unsigned* out, unsigned pos, unsigned v, unsigned l) {
    const unsigned wi = pos >> 5, off = pos & 31u;
    const unsigned long long x = (unsigned long long)v << (64u - off - l);
    if (wi < (unsigned)kOutWords) atomicOr(&out[wi], (unsigned)(x >> 32));
    if (off + l > 32u && wi + 1 < (unsigned)kOutWords) atomicOr(&out[wi + 1], (unsigned)x);
}

// What lane `lane` of a wave sends for coefficient c (zig-zag position `lane`; lane 0 holds the DC DIFFERENCE) of a block whose
// non-zero AC positions are the set bits of mask: nzrl ZRL codes, then `bits` (nb of them: the symbol's code and the value's bits).
struct LaneSym { unsigned bits, nb, nzrl; };
__device__ __forceinline__ LaneSym lane_symbol(int c, unsigned lane, unsigned long long mask, int tb, const unsigned* s_ac) {
    LaneSym o{0u, 0u, 0u};
    const unsigned mag = (unsigned)(c < 0 ? -c : c);
    const unsigned s = 32u - (unsigned)__clz((int)mag);                         // the magnitude category (__clz(0) = 32)
    const unsigned vb = (unsigned)(c < 0 ? c - 1 : c) & ((1u << s) - 1u);      // a negative value is sent as v - 1
    if (lane == 0) {
        const unsigned code = kH.dc[tb][s < 11u ? s : 11u];
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

// K1.  blockIdx.x: the interval, blockIdx.y: the image.
__global__ __launch_bounds__(kThreads) void jpeg_interval_kernel(PngSrc src, JpegGeom g, unsigned char* __restrict__ intbuf, unsigned* __restrict__ int_bytes) {
    __shared__ unsigned s_px[kR * 8 * 6];                     // the interval's pixels: MCU m, row r at byte (m * 8 + r) * 24
    __shared__ int s_plane[kBlocks * kPlane];                 // level-shifted samples, then coefficients; later the stuffed bytes
    __shared__ short s_q[kBlocks * 64];                       // quantised coefficients, zig-zag order
    __shared__ unsigned s_out[kOutWords];                     // the entropy-coded bits, big-endian words
    __shared__ unsigned s_ac[2 * 256];
    __shared__ unsigned s_blkoff[kBlocks + 1];
    __shared__ unsigned s_scan[kThreads / 64];
    const unsigned iv = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned m0 = iv * (unsigned)kR;
    const unsigned nm = g.nmcu - m0 < (unsigned)kR ? g.nmcu - m0 : (unsigned)kR;
    const unsigned nblk = 3 * nm;
    const unsigned char* __restrict__ rgb = src.rgb + (unsigned long long)img * src.image_pitch;

    for (int k = t; k < kOutWords; k += kThreads) s_out[k] = 0;
    for (int k = t; k < 512; k += kThreads) s_ac[k] = kH.ac[k >> 8][k & 255];

    // 1. pixels -> LDS.  Item = one dword of one MCU's pixel row; consecutive threads take consecutive dwords of a pixel row across
    //    the interval's MCUs.  A dword that is 4-aligned in memory and inside the row is loaded whole, any other byte by byte with
    //    the coordinates clamped (edge replication).
    const unsigned row_bytes = 3u * (unsigned)g.w;
    for (unsigned idx = t; idx < (unsigned)(kR * 48); idx += kThreads) {
        const unsigned r = idx / (kR * 6), rem = idx % (kR * 6), m = rem / 6, k = rem % 6;
        if (m >= nm) continue;
        const unsigned mcu = m0 + m, my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
        const unsigned y = min(my * 8 + r, (unsigned)g.h - 1);
        const unsigned char* __restrict__ p = rgb + (unsigned long long)y * src.row_pitch;
        const unsigned b0 = mx * 24 + 4 * k;
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
        s_px[(m * 8 + r) * 6 + k] = v;
    }
    __syncthreads();

    // 2. RGB -> Y Cb Cr (jccolor.c: 16-bit fixed point, + 32768 to round, chroma offset 128), level shift by 128
    const unsigned char* s_pb = reinterpret_cast<const unsigned char*>(s_px);
    for (unsigned pix = t; pix < nm * 64; pix += kThreads) {
        const unsigned m = pix >> 6, r = (pix >> 3) & 7u, c = pix & 7u;
        const unsigned char* q = s_pb + (m * 8 + r) * 24 + 3 * c;
        const int R = q[0], G = q[1], B = q[2];
        int* o = s_plane + 3 * m * kPlane + r * 9 + c;
        o[0] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
        o[kPlane] = ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128;
        o[2 * kPlane] = ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128;
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
        const int tb = blk % 3 ? 1 : 0;
        const int* p = s_plane + blk * kPlane + col;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[9 * k];
        fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned nat = 8 * k + col;
            const unsigned mag = (unsigned)(d[k] < 0 ? -d[k] : d[k]) + kQ.half[tb][nat];
            const int qv = (int)__umulhi(mag, kQ.recip[tb][nat]);              // floor(mag / (8 q)): jpeg_tables.hpp
            s_q[blk * 64 + kQ.zzpos[nat]] = (short)(d[k] < 0 ? -qv : qv);
        }
    }
    __syncthreads();

    // 5. bits per block: one wave per block, lane k = zig-zag position k.  The DC differences need no order: every DC is known.
    const unsigned wv = t >> 6, lane = t & 63u;
    for (unsigned blk = wv; blk < nblk; blk += kThreads / 64) {
        int c = s_q[blk * 64 + lane];
        if (lane == 0 && blk >= 3) c -= s_q[(blk - 3) * 64];
        const unsigned long long mask = __ballot(c != 0) & ~1ull;
        const LaneSym sy = lane_symbol(c, lane, mask, blk % 3 ? 1 : 0, s_ac);
        unsigned bits = sy.nb + sy.nzrl * (s_ac[(blk % 3 ? 256 : 0) + 0xf0] >> 16);
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
        if (lane == 0 && blk >= 3) c -= s_q[(blk - 3) * 64];
        const unsigned long long mask = __ballot(c != 0) & ~1ull;
        const int tb = blk % 3 ? 1 : 0;
        const LaneSym sy = lane_symbol(c, lane, mask, tb, s_ac);
        const unsigned zrl = s_ac[tb * 256 + 0xf0];
        const unsigned mine = sy.nb + sy.nzrl * (zrl >> 16);
        unsigned inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc += o; }
        unsigned pos = s_blkoff[blk] + inc - mine;
        for (unsigned k = 0; k < sy.nzrl; ++k) { put_bits(s_out, pos, zrl & 0xffffu, zrl >> 16); pos += zrl >> 16; }
        if (sy.nb) put_bits(s_out, pos, sy.bits, sy.nb);
    }
    const unsigned total_bits = s_blkoff[nblk];
    unsigned raw = (total_bits + 7) / 8;                         // bytes before stuffing; the last one is padded with 1-bits
    if (raw > kRawBytes) raw = kRawBytes;                        // (cannot happen: jpeg_tables.hpp; nothing is ever written past the bound)
    if (t == 0 && (total_bits & 7u)) put_bits(s_out, total_bits, (1u << (8 - (total_bits & 7u))) - 1u, 8 - (total_bits & 7u));
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
    unsigned char* s_st = reinterpret_cast<unsigned char*>(s_plane);           // (the planes were last read before two barriers)
    unsigned o = i0 + before;
    for (unsigned i = i0; i < i1; ++i) {
        const unsigned b = (s_out[i >> 2] >> (24 - 8 * (i & 3u))) & 0xffu;
        if (o < kIntBound) s_st[o] = (unsigned char)b;
        ++o;
        if (b == 0xffu) { if (o < kIntBound) s_st[o] = 0; ++o; }
    }
    unsigned bytes = raw + all_ff + 2;
    const unsigned bound = (unsigned)interval_bound(nm);
    if (bytes > bound) bytes = bound;
    if (t == 0) {                                                // RST(m mod 8) behind every interval but the last, EOI behind the last
        s_st[bytes - 2] = 0xff;
        s_st[bytes - 1] = iv + 1 == g.nint ? 0xd9 : (unsigned char)(0xd0 + (iv & 7u));
    }
    __syncthreads();
    // 9. the interval's bytes and their count to the scratch
    const unsigned long long slot = (unsigned long long)img * g.nint + iv;
    unsigned* dst = reinterpret_cast<unsigned*>(intbuf + slot * kIntStride);
    const unsigned* s_sw = reinterpret_cast<const unsigned*>(s_plane);
    for (unsigned k = t; k < (bytes + 3) / 4 + 1; k += kThreads) dst[k] = s_sw[k];      // (+ 1: the dword the gather may read behind the last byte)
    if (t == 0) int_bytes[slot] = bytes;
}

// K2.  The interval's bytes to their place in the file; the head by interval 0, the lengths by the last interval.
__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(JpegGeom g, const unsigned char* __restrict__ intbuf, const unsigned* __restrict__ int_bytes,
                                                                unsigned char* __restrict__ files, unsigned long long file_pitch, unsigned long long* __restrict__ flen,
                                                                unsigned char* __restrict__ lens, unsigned long long lens_pitch) {
    __shared__ unsigned s_red[2][kThreads / 64];
    const unsigned iv = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned* sizes = int_bytes + (unsigned long long)img * g.nint;
    unsigned before = 0, all = 0;                                 // (integers: a sum in any order; < 2^16 * 9374 < 2^30)
    for (unsigned k = t; k < g.nint; k += kThreads) { const unsigned s = sizes[k]; all += s; if (k < iv) before += s; }
    for (int off = 32; off >= 1; off >>= 1) { before += __shfl_down(before, off, 64); all += __shfl_down(all, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = before; s_red[1][t >> 6] = all; }
    __syncthreads();
    before = all = 0;
    for (int k = 0; k < kThreads / 64; ++k) { before += s_red[0][k]; all += s_red[1][k]; }
    unsigned char* __restrict__ file = files + (unsigned long long)img * file_pitch;
    const unsigned char* __restrict__ srcb = intbuf + ((unsigned long long)img * g.nint + iv) * kIntStride;
    const unsigned size = sizes[iv];
    const unsigned d0 = kHeaderBytes + before;                    // file offset of the interval's first byte (file_pitch is a multiple of 4)
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
    if (iv == 0)
        for (unsigned k = t; k < (unsigned)kHeaderBytes; k += kThreads) {
            const unsigned d = k - (unsigned)kSofDims;            // SOF0: height, width, two big-endian bytes each
            file[k] = d < 4u ? (unsigned char)((d < 2u ? g.h : g.w) >> (d & 1u ? 0 : 8)) : kHead.b[k];
        }
    if (iv + 1 == g.nint) {
        const unsigned long long fl = (unsigned long long)kHeaderBytes + all;
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

struct ScratchLayout { size_t flen, int_bytes, intbuf, files, file_pitch, total; };
ScratchLayout layout_of(int n, const JpegGeom& g) {
    ScratchLayout L;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.flen = 0;                                                      // n x u64
    L.int_bytes = up((size_t)n * 8);                                 // n x nint u32
    L.intbuf = up(L.int_bytes + (size_t)n * g.nint * 4);             // n x nint x kIntStride
    L.files = up(L.intbuf + (size_t)n * g.nint * kIntStride);
    L.file_pitch = up(((size_t)g.file_bound + 11) / 12 * 12 + 16);   // (the 12-byte groups of the last base64 threads stay inside)
    L.total = L.files + L.file_pitch * (size_t)n;
    return L;
}

}  // namespace

size_t jpeg_file_bound(int h, int w) { return jpegtab::jpeg_file_bound(h, w); }
size_t jpeg_base64_bound(int h, int w) { return jpegtab::jpeg_base64_bound(h, w); }
size_t jpeg_scratch_bytes(int n, int h, int w) { return layout_of(n, geom_of(h, w)).total; }

void encode_jpeg_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch, unsigned char* d_chars,
                               size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, hipStream_t s) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG encoder (1..8192 per side)");
    if (row_pitch < (size_t)3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row pitch for the JPEG encoder (< 3*w)");
    const JpegGeom g = geom_of(h, w);
    const ScratchLayout L = layout_of(n, g);
    unsigned long long* flen = reinterpret_cast<unsigned long long*>(d_scratch + L.flen);
    unsigned* int_bytes = reinterpret_cast<unsigned*>(d_scratch + L.int_bytes);
    unsigned char* intbuf = d_scratch + L.intbuf;
    unsigned char* files = d_scratch + L.files;
    const PngSrc src{d_rgb, (unsigned long long)row_pitch, (unsigned long long)image_pitch};
    hipLaunchKernelGGL(jpeg_interval_kernel, dim3(g.nint, n), dim3(kThreads), 0, s, src, g, intbuf, int_bytes);
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3(g.nint, n), dim3(kThreads), 0, s, g, intbuf, int_bytes, files, (unsigned long long)L.file_pitch, flen, d_lens,
                       (unsigned long long)lens_pitch);
    base64_device_length_launch(files, L.file_pitch, flen, (size_t)g.file_bound, n, d_chars, text_pitch, s);
    IRE_HIP(hipGetLastError());
}

}  // namespace ire
