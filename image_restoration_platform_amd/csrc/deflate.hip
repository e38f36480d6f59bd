// deflate.hip -- restored RGB pixels -> the base64 text of a COMPRESSED PNG file, on the device.
//
// encode.hip writes stored deflate blocks: 4.2 MB of text per 1024^2 result, and the hosts above the engine are bound by exactly
// that payload (profiles/r04_codec_seam.json).  This file writes the same kind of file -- signature, IHDR, ONE IDAT, IEND -- with
// Paeth-filtered scanlines and one dynamic-Huffman deflate block per 32 768 bytes of the filtered stream: literals and the
// end-of-block symbol only (no LZ77 matching), canonical codes of at most 15 bits built on the device from the block's own
// histogram by package-merge (the optimal length-limited code), the 259 code lengths sent one by one with a 7-bit-limited
// code-length code (symbols 0..15, no run-length symbols).  Every block but the last ends with an empty stored block (the
// 00 00 FF FF marker), so each block is a whole number of bytes and is written independently.  tests/png_deflate_model.py restates
// every step; the device's bytes equal the model's (tests/test_png_deflate_gpu.py).
//
// The file's length now depends on the data.  Four launches and one memset per BATCH, none depending on n (image and block are
// grid dimensions), no host round trip:
//   K1 deflate_block_kernel   one workgroup per block: filter -> LDS, histogram (LDS integer atomics), code construction, bit
//                             packing into LDS, the block's bytes and byte count to scratch; Adler partial sums
//   K2 deflate_gather_kernel  one workgroup per block: prefix sum over the block sizes, the block's bytes to their place in the
//                             file; the first writes the head (IDAT length), the last Adler-32, IEND and the two lengths
//   K3 deflate_crc_kernel     CRC-32 of the IDAT over a length read from device memory: png_crc_kernel's slices and tree; the
//                             operators of ragged pieces by square-and-multiply on the device
//   K4 deflate_base64_kernel  base64 over that length
// Grids of K3 / K4 are sized from the worst case (png_deflate_file_bound); workgroups past the real length leave at once.
// Everything is integer work on LDS atomics and fixed-order sums: the bytes are a pure function of the pixels.
#include "deflate.hpp"

#include "png_bits.hpp"

namespace ire {

namespace {

using namespace pngbits;

constexpr int kBlk = 32768;                     // filtered bytes per deflate block
constexpr int kThreads = 256;
constexpr int kPer = kBlk / kThreads;           // 128 consecutive symbols per thread when packing
constexpr int kLit = 257;                       // literals + end-of-block
constexpr int kSent = 259;                      // code lengths in the header: 257 + the two one-bit distance codes
constexpr int kHdrBitsMax = 3 + 5 + 5 + 4 + 19 * 3 + kSent * 7;      // 1887
// Worst case of one block of len literals, in bytes: the header; 9 bits per symbol, end-of-block included (the optimal limited
// code costs no more than ANY 15-bit-limited code over 257 symbols, e.g. the flat one of 255 8-bit and 2 9-bit words); the empty
// stored block's 3 bits and its padding; its 4 length bytes.
__host__ __device__ constexpr unsigned blk_bound(unsigned len) { return (kHdrBitsMax + 9u * (len + 1u) + 3u + 7u) / 8u + 4u; }
constexpr unsigned kBlkStride = (blk_bound(kBlk) + 4 + 63) / 64 * 64;      // scratch bytes per block (one readable dword behind the bytes)
constexpr int kOutWords = kBlkStride / 4;
constexpr int kFiltBytes = kBlk + (kBlk / kPer) * 4;                       // the filtered block in LDS, 4 bytes of padding per 128: thread t's run starts in bank t

constexpr int kSlice = 256;                     // bytes of the IDAT chunk a thread runs its CRC over
constexpr int kCrcWG = 256;                     // slices per workgroup: 64 KB of the chunk

struct DeflGeom {
    int h, w;
    unsigned row;              // bytes of a filtered scanline: 1 + 3 w
    unsigned raw;              // bytes of the filtered stream (< 2^28 at 8192 x 8192)
    unsigned nblk;
    unsigned long long file_bound;
};
DeflGeom geom_of(int h, int w) {
    DeflGeom g;
    g.h = h; g.w = w;
    g.row = 1u + 3u * (unsigned)w;
    g.raw = (unsigned)h * g.row;
    g.nblk = (g.raw + kBlk - 1) / kBlk;
    const unsigned full = g.raw / kBlk, tail = g.raw % kBlk;
    // signature 8 | IHDR 25 | IDAT length, type 8 | zlib header 2 | blocks | Adler 4 | CRC 4 | IEND 12
    g.file_bound = 8 + 25 + 8 + 2 + (unsigned long long)full * blk_bound(kBlk) + (tail ? blk_bound(tail) : 0) + 4 + 4 + 12;
    return g;
}
constexpr unsigned kZ0 = 8 + 25 + 8;            // file offset of the zlib stream
constexpr unsigned kIdatType = 8 + 25 + 4;      // file offset of "IDAT": the chunk's CRC starts here

__constant__ unsigned char kTail[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
__constant__ unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int filt_at(int i) { return i + (i >> 7) * 4; }      // LDS position of filtered byte i of the block

// exclusive scan of one value per thread over the workgroup (256 threads), total in *total.  s_w: 4 words.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_w, unsigned* total) {
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(inc, off, 64); if ((int)(threadIdx.x & 63) >= off) inc += o; }
    __syncthreads();                             // (s_w may still be read from the previous scan)
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) { const unsigned x = s_w[k]; if (k < (int)(threadIdx.x >> 6)) base += x; tot += x; }
    *total = tot;
    return base + inc - v;
}

// LDS state of the code construction
struct CodeLds {
    unsigned w[2][2 * kLit + 2];     // the merged list of the level at hand / of the one below
    unsigned pk[kLit + 1];           // packages of the level at hand
    unsigned leafw[kLit + 1];        // counts of the used symbols, ascending by (count, symbol)
    unsigned short leafsym[kLit + 1];
    unsigned short pos[15][kLit + 1];     // where each leaf lies in each level's list
    unsigned a[15];                  // leaves selected per level
    unsigned n;
};

__device__ __forceinline__ unsigned lower_bound_u32(const unsigned* v, unsigned n, unsigned x) {      // elements < x
    unsigned lo = 0, hi = n;
    while (lo < hi) { const unsigned m = (lo + hi) >> 1; if (v[m] < x) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ unsigned upper_bound_u32(const unsigned* v, unsigned n, unsigned x) {      // elements <= x
    unsigned lo = 0, hi = n;
    while (lo < hi) { const unsigned m = (lo + hi) >> 1; if (v[m] <= x) lo = m + 1; else hi = m; }
    return lo;
}

// Optimal code lengths <= maxbits for the nsym counts in hist (>= 2 of them non-zero), by package-merge; the whole workgroup calls
// it.  Level 0 holds the leaves alone; level j merges the leaves with the pairs ("packages") of level j - 1, a leaf before a
// package of equal weight; the first 2 n - 2 items of the top level are selected, a selected package selects its two items one
// level down; a symbol's length is the number of levels that select its leaf.  Weights stay below 2^15 * 32769 < 2^31.
__device__ void limited_lengths(const unsigned* hist, int nsym, int maxbits, unsigned char* len_out, CodeLds& L) {
    if (threadIdx.x == 0) L.n = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < nsym; s += kThreads) {
        len_out[s] = 0;
        const unsigned c = hist[s];
        if (c) {
            unsigned rank = 0;
            for (int o = 0; o < nsym; ++o) { const unsigned co = hist[o]; rank += (co && (co < c || (co == c && o < s))) ? 1u : 0u; }
            L.leafw[rank] = c; L.leafsym[rank] = (unsigned short)s; L.w[0][rank] = c; L.pos[0][rank] = (unsigned short)rank;
            atomicAdd(&L.n, 1u);
        }
    }
    __syncthreads();
    const unsigned n = L.n;
    unsigned curlen = n;
    for (int j = 1; j < maxbits; ++j) {
        const unsigned* prev = L.w[(j - 1) & 1];
        unsigned* cur = L.w[j & 1];
        const unsigned npk = curlen >> 1;
        for (unsigned k = threadIdx.x; k < npk; k += kThreads) L.pk[k] = prev[2 * k] + prev[2 * k + 1];
        __syncthreads();
        for (unsigned r = threadIdx.x; r < n; r += kThreads) {
            const unsigned p = r + lower_bound_u32(L.pk, npk, L.leafw[r]);
            cur[p] = L.leafw[r]; L.pos[j][r] = (unsigned short)p;
        }
        for (unsigned k = threadIdx.x; k < npk; k += kThreads) cur[k + upper_bound_u32(L.leafw, n, L.pk[k])] = L.pk[k];
        __syncthreads();
        curlen = n + npk;
    }
    if (threadIdx.x == 0) {
        unsigned take = 2 * n - 2;
        for (int j = maxbits - 1; j >= 0; --j) {
            unsigned lo = 0, hi = n;
            while (lo < hi) { const unsigned m = (lo + hi) >> 1; if (L.pos[j][m] < take) lo = m + 1; else hi = m; }
            L.a[j] = lo;
            take = 2 * (take - lo);
        }
    }
    __syncthreads();
    for (unsigned r = threadIdx.x; r < n; r += kThreads) {
        unsigned l = 0;
        for (int j = 0; j < maxbits; ++j) l += r < L.a[j] ? 1u : 0u;
        len_out[L.leafsym[r]] = (unsigned char)l;
    }
    __syncthreads();
}

// Canonical codes (RFC 1951 3.2.2) of nsym lengths, bit-reversed for the LSB-first packer: code[s] = value | length << 16.
__device__ void canonical_codes(const unsigned char* len, int nsym, unsigned* code, unsigned* s_cnt /* 17 */) {
    if (threadIdx.x < 17) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < nsym; s += kThreads) if (len[s]) atomicAdd(&s_cnt[len[s]], 1u);
    __syncthreads();
    for (int s = threadIdx.x; s < nsym; s += kThreads) {
        const unsigned l = len[s];
        unsigned c = 0;
        if (l) {
            unsigned first = 0;
            for (unsigned b = 1; b <= l; ++b) first = (first + s_cnt[b - 1]) << 1;
            unsigned rank = 0;
            for (int o = 0; o < s; ++o) rank += len[o] == l ? 1u : 0u;
            c = __brev(first + rank) >> (32 - l);
        }
        code[s] = c | (l << 16);
    }
    __syncthreads();
}

// LSB-first bit packer into a zeroed LDS buffer: whole words and the ragged ones alike go in by atomic OR
struct BitPut {
    unsigned* out;
    unsigned long long acc;
    unsigned nb, wi;
    __device__ __forceinline__ BitPut(unsigned* o, unsigned bitpos) : out(o), acc(0), nb(bitpos & 31u), wi(bitpos >> 5) {}
    __device__ __forceinline__ void put(unsigned v, unsigned l) {
        acc |= (unsigned long long)v << nb;
        nb += l;
        if (nb >= 32) { if (wi < (unsigned)kOutWords) atomicOr(&out[wi], (unsigned)acc); ++wi; acc >>= 32; nb -= 32; }
    }
    __device__ __forceinline__ void flush() { if (nb && wi < (unsigned)kOutWords) atomicOr(&out[wi], (unsigned)acc); }
};

// K1.  blockIdx.x: the block, blockIdx.y: the image.
__global__ __launch_bounds__(kThreads) void deflate_block_kernel(PngSrc src, DeflGeom g, unsigned char* __restrict__ blkbuf, unsigned* __restrict__ blk_bytes,
                                                                  unsigned long long* __restrict__ acc) {
    __shared__ unsigned s_out[kOutWords];
    __shared__ unsigned s_filt[kFiltBytes / 4];
    __shared__ CodeLds s_L;
    __shared__ unsigned s_hist[kLit + 3], s_clhist[19], s_code[kLit], s_clcode[19], s_cnt[17], s_scan[4], s_red[2][kThreads / 64];
    __shared__ unsigned char s_len[kSent + 1], s_cllen[20];
    unsigned char* s_fb = reinterpret_cast<unsigned char*>(s_filt);
    const unsigned blk = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned char* __restrict__ rgb = src.rgb + (unsigned long long)img * src.image_pitch;
    const unsigned base = blk * (unsigned)kBlk;
    const unsigned len = g.raw - base < (unsigned)kBlk ? g.raw - base : (unsigned)kBlk;
    const bool final = blk + 1 == g.nblk;

    for (int k = t; k < kOutWords; k += kThreads) s_out[k] = 0;
    for (int k = t; k < kLit + 3; k += kThreads) s_hist[k] = 0;
    if (t < 19) s_clhist[t] = 0;
    __syncthreads();

    // the filtered bytes of the block (Paeth, 3 bytes per pixel; off the image a = b = c = 0), their histogram and Adler sums
    unsigned S = 0, T = 0;
    for (int k = 0; k < kPer; ++k) {
        const unsigned i = (unsigned)k * kThreads + t;
        if (i >= len) break;
        const unsigned gi = base + i, y = gi / g.row, c = gi - y * g.row;
        unsigned v = 4;
        if (c) {
            const unsigned x = c - 1;
            const unsigned char* p = rgb + (unsigned long long)y * src.row_pitch + x;
            const int cur = p[0];
            const int a = x >= 3 ? p[-3] : 0;
            const int b = y ? *(p - src.row_pitch) : 0;
            const int cc = (x >= 3 && y) ? *(p - src.row_pitch - 3) : 0;
            const int pp = a + b - cc;
            const int pa = abs(pp - a), pb = abs(pp - b), pc = abs(pp - cc);
            const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
            v = (unsigned)(cur - pred) & 0xffu;
        }
        s_fb[filt_at((int)i)] = (unsigned char)v;
        atomicAdd(&s_hist[v], 1u);
        S += v;
        T += (gi % kAdlerBase) * v;              // <= 128 * 65520 * 255 < 2^32 per thread
    }
    T %= kAdlerBase;
    for (int off = 32; off >= 1; off >>= 1) { S += __shfl_down(S, off, 64); T += __shfl_down(T, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = S; s_red[1][t >> 6] = T; }
    __syncthreads();
    if (t == 0) {
        unsigned ws = 0, wt = 0;
        for (int k = 0; k < kThreads / 64; ++k) { ws += s_red[0][k]; wt += s_red[1][k]; }
        atomicAdd(&acc[2 * img], (unsigned long long)ws);          // (integers: any order of the adds gives the same sums)
        atomicAdd(&acc[2 * img + 1], (unsigned long long)wt);
        s_hist[256] = 1;                         // end-of-block
    }
    __syncthreads();

    // the two codes
    limited_lengths(s_hist, kLit, 15, s_len, s_L);
    if (t == 0) { s_len[257] = 1; s_len[258] = 1; }                // the distance tree zlib writes for literal-only data
    __syncthreads();
    for (int k = t; k < kSent; k += kThreads) atomicAdd(&s_clhist[s_len[k]], 1u);
    __syncthreads();
    limited_lengths(s_clhist, 19, 7, s_cllen, s_L);
    canonical_codes(s_len, kLit, s_code, s_cnt);
    canonical_codes(s_cllen, 19, s_clcode, s_cnt);

    // header: fixed part by one thread, the 259 code lengths by all (item t by thread t, the last three by thread 255)
    int hclen = 4;
    for (int k = 4; k < 19; ++k) if (s_cllen[kClOrder[k]]) hclen = k + 1;
    const unsigned fixed_bits = 17u + 3u * (unsigned)hclen;
    if (t == 0) {
        BitPut bp(s_out, 0);
        bp.put(final ? 1u : 0u, 1); bp.put(2u, 2); bp.put(0u, 5); bp.put(1u, 5); bp.put((unsigned)hclen - 4u, 4);
        for (int k = 0; k < hclen; ++k) bp.put(s_cllen[kClOrder[k]], 3);
        bp.flush();
    }
    unsigned total = 0;
    {
        const int last = t == kThreads - 1 ? kSent : (int)t + 1;
        unsigned bits = 0;
        for (int k = t; k < last; ++k) bits += s_cllen[s_len[k]];
        const unsigned at = block_scan(bits, s_scan, &total);
        BitPut bp(s_out, fixed_bits + at);
        for (int k = t; k < last; ++k) { const unsigned c = s_clcode[s_len[k]]; bp.put(c & 0xffffu, c >> 16); }
        bp.flush();
    }
    const unsigned hdr_bits = fixed_bits + total;

    // symbols: thread t packs bytes [128 t, 128 t + 128) of the block; the last thread adds end-of-block
    const unsigned i0 = t * (unsigned)kPer, i1 = i0 + kPer < len ? i0 + kPer : len;
    unsigned bits = 0;
    for (unsigned i = i0; i < i1; ++i) bits += s_code[s_fb[filt_at((int)i)]] >> 16;
    if (t == kThreads - 1) bits += s_code[256] >> 16;
    const unsigned at = block_scan(bits, s_scan, &total);
    {
        BitPut bp(s_out, hdr_bits + at);
        for (unsigned i = i0; i < i1; ++i) { const unsigned c = s_code[s_fb[filt_at((int)i)]]; bp.put(c & 0xffffu, c >> 16); }
        if (t == kThreads - 1) { const unsigned c = s_code[256]; bp.put(c & 0xffffu, c >> 16); }
        bp.flush();
    }
    const unsigned all_bits = hdr_bits + total;
    unsigned bytes = final ? (all_bits + 7) / 8 : (all_bits + 3 + 7) / 8 + 4;
    if (bytes > blk_bound(len)) bytes = blk_bound(len);          // (cannot happen with an optimal code; nothing is ever written past the bound)
    __syncthreads();
    if (!final && t == 0) {                                      // the empty stored block: 000, padding, LEN 0000, NLEN FFFF
        const unsigned o = bytes - 2;
        atomicOr(&s_out[o >> 2], 0xffu << (8 * (o & 3)));
        atomicOr(&s_out[(o + 1) >> 2], 0xffu << (8 * ((o + 1) & 3)));
    }
    __syncthreads();
    unsigned* dst = reinterpret_cast<unsigned*>(blkbuf + ((unsigned long long)img * g.nblk + blk) * kBlkStride);
    for (unsigned k = t; k < (bytes + 3) / 4 + 1; k += kThreads) dst[k] = s_out[k];      // (+ 1: the dword the gather may read behind the last byte)
    if (t == 0) blk_bytes[(unsigned long long)img * g.nblk + blk] = bytes;
}

// K2.  The block's bytes to their place in the file; head by block 0, tail and lengths by the last block.
__global__ __launch_bounds__(kThreads) void deflate_gather_kernel(DeflGeom g, PngIhdr ihdr, const unsigned char* __restrict__ blkbuf, const unsigned* __restrict__ blk_bytes,
                                                                   const unsigned long long* __restrict__ acc, unsigned char* __restrict__ files, unsigned long long file_pitch,
                                                                   unsigned long long* __restrict__ flen, unsigned char* __restrict__ lens, unsigned long long lens_pitch) {
    __shared__ unsigned s_red[2][kThreads / 64];
    const unsigned blk = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned* sizes = blk_bytes + (unsigned long long)img * g.nblk;
    unsigned before = 0, all = 0;                                 // (integers: a sum in any order; < 2^28 * 9 / 8)
    for (unsigned k = t; k < g.nblk; k += kThreads) { const unsigned s = sizes[k]; all += s; if (k < blk) before += s; }
    for (int off = 32; off >= 1; off >>= 1) { before += __shfl_down(before, off, 64); all += __shfl_down(all, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = before; s_red[1][t >> 6] = all; }
    __syncthreads();
    before = all = 0;
    for (int k = 0; k < kThreads / 64; ++k) { before += s_red[0][k]; all += s_red[1][k]; }
    unsigned char* __restrict__ file = files + (unsigned long long)img * file_pitch;
    const unsigned char* __restrict__ srcb = blkbuf + ((unsigned long long)img * g.nblk + blk) * kBlkStride;
    const unsigned size = sizes[blk];
    const unsigned d0 = kZ0 + 2 + before;                         // file offset of the block's first byte (file_pitch is a multiple of 4)
    // [d0, d0 + size): bytes up to the first dword boundary, whole dwords, bytes again: no dword is shared with a neighbour's stores
    const unsigned head = (4u - (d0 & 3u)) & 3u;
    const unsigned nhead = head < size ? head : size;
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
    const unsigned zlen = 2 + all + 4;
    if (blk == 0 && t < kZ0 + 2) {
        unsigned v;
        if (t < 33) v = ihdr.b[t];
        else if (t < 37) v = (zlen >> (8 * (36 - t))) & 0xffu;
        else if (t < 41) v = t == 37 ? 'I' : t == 38 ? 'D' : t == 39 ? 'A' : 'T';
        else v = t == 41 ? 0x78u : 0x01u;
        file[t] = (unsigned char)v;
    }
    if (blk + 1 == g.nblk) {
        const unsigned e0 = kZ0 + 2 + all;                        // Adler-32 | CRC-32 (K3) | IEND
        const unsigned long long fl = (unsigned long long)e0 + 4 + 4 + 12;
        if (t < 4) {
            const unsigned long long Ss = acc[2 * img], Tt = acc[2 * img + 1];
            const unsigned n = g.raw % kAdlerBase;
            const unsigned A = (unsigned)((1 + Ss) % kAdlerBase);
            const unsigned B = (unsigned)((n + (unsigned long long)n * (Ss % kAdlerBase) + kAdlerBase - Tt % kAdlerBase) % kAdlerBase);
            const unsigned adler = (B << 16) | A;
            file[e0 + t] = (unsigned char)(adler >> (8 * (3 - t)));
        } else if (t < 4 + 12) file[e0 + 8 + (t - 4)] = kTail[t - 4];      // (e0 + 4 .. e0 + 7: the chunk's CRC, K3)
        else if (t < 64) { const unsigned long long o = fl + (t - 16); if (o < file_pitch) file[o] = 0; }      // what the last base64 thread reads behind the file
        if (t == 64) {
            flen[img] = fl;
            const unsigned long long chars = (fl + 2) / 3 * 4;
            unsigned char* lp = lens + (unsigned long long)img * lens_pitch;
            if ((reinterpret_cast<unsigned long long>(lp) & 7u) == 0) *reinterpret_cast<unsigned long long*>(lp) = chars;
            else for (int k = 0; k < 8; ++k) lp[k] = (unsigned char)(chars >> (8 * k));
        }
    }
}

// K3.  CRC-32 of the IDAT chunk (type + zlib stream) over the length K2 left in flen: a thread runs the byte-wise CRC over its
// 256-byte slice from register 0 (the chunk's first from 0xffffffff), a workgroup combines its slices by a tree (a full right half:
// the host's operator; a ragged one: x^(8 bytes) by square-and-multiply here), the last workgroup to finish (ticket) folds the
// workgroups' registers left to right and writes the CRC.
struct CrcOps { unsigned lvl[8]; unsigned wg; };      // x^(8 * 256 * 2^l), x^(8 * 65536)
__global__ __launch_bounds__(kCrcWG) void deflate_crc_kernel(unsigned char* __restrict__ files, unsigned long long file_pitch, const unsigned long long* __restrict__ flen, CrcOps ops,
                                                              unsigned* __restrict__ part_all, unsigned* __restrict__ tickets) {
    __shared__ unsigned s_tab[256];
    __shared__ unsigned s_reg[kCrcWG];
    __shared__ unsigned s_last;
    const unsigned long long crc_len = flen[blockIdx.y] - kIdatType - 4 - 12;      // "IDAT" ... Adler-32
    const unsigned long long wg_bytes = (unsigned long long)kCrcWG * kSlice;
    const unsigned nact = (unsigned)((crc_len + wg_bytes - 1) / wg_bytes);
    if (blockIdx.x >= nact) return;
    unsigned char* __restrict__ file = files + (unsigned long long)blockIdx.y * file_pitch;
    unsigned* part = part_all + (size_t)blockIdx.y * gridDim.x;
    {   // byte table of the reflected polynomial
        unsigned c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        s_tab[threadIdx.x] = c;
    }
    __syncthreads();
    const unsigned long long lo = (unsigned long long)blockIdx.x * wg_bytes + (unsigned long long)threadIdx.x * kSlice;
    unsigned reg = (blockIdx.x == 0 && threadIdx.x == 0) ? 0xffffffffu : 0u;
    if (lo < crc_len) {
        const unsigned long long hi = lo + kSlice < crc_len ? lo + kSlice : crc_len;
        for (unsigned long long o = lo; o < hi; ++o) reg = s_tab[(reg ^ file[kIdatType + o]) & 0xffu] ^ (reg >> 8);
    }
    s_reg[threadIdx.x] = reg;
    __syncthreads();
    auto bytes_of = [&](unsigned t, unsigned span) -> unsigned long long {      // true byte count of the slices [t, t + span) of this workgroup
        const unsigned long long a = (unsigned long long)blockIdx.x * wg_bytes + (unsigned long long)t * kSlice;
        const unsigned long long b = a + (unsigned long long)span * kSlice;
        const unsigned long long aa = a < crc_len ? a : crc_len, bb = b < crc_len ? b : crc_len;
        return bb - aa;
    };
    for (int l = 0; l < 8; ++l) {
        const unsigned span = 1u << l;
        if ((threadIdx.x & (2 * span - 1)) == 0) {
            const unsigned long long nb = bytes_of(threadIdx.x + span, span);
            const unsigned op = nb == (unsigned long long)span * kSlice ? ops.lvl[l] : gf_x_pow_8n(nb);
            s_reg[threadIdx.x] = gf_mul(op, s_reg[threadIdx.x]) ^ s_reg[threadIdx.x + span];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part[blockIdx.x], s_reg[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(&tickets[blockIdx.y], 1u) == nact - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const unsigned last_op = gf_x_pow_8n(crc_len - (unsigned long long)(nact - 1) * wg_bytes);
    unsigned r = 0;
    for (unsigned k = 0; k < nact; ++k) {
        const unsigned pk = __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r = k == 0 ? pk : gf_mul(k + 1 == nact ? last_op : ops.wg, r) ^ pk;
    }
    const unsigned crc = r ^ 0xffffffffu;
    const unsigned long long co = kIdatType + crc_len;
    file[co] = (unsigned char)(crc >> 24); file[co + 1] = (unsigned char)(crc >> 16); file[co + 2] = (unsigned char)(crc >> 8); file[co + 3] = (unsigned char)crc;
}

// K4.  base64 over the file's real length.
__global__ __launch_bounds__(256) void deflate_base64_kernel(const unsigned char* __restrict__ files, unsigned long long file_pitch, const unsigned long long* __restrict__ flen,
                                                              unsigned char* __restrict__ texts, unsigned long long text_pitch) {
    const unsigned long long n = flen[blockIdx.y];
    const bool dwords = (text_pitch & 3u) == 0 && (reinterpret_cast<unsigned long long>(texts) & 3u) == 0;
    base64_thread(files + (unsigned long long)blockIdx.y * file_pitch, n, (unsigned long long)blockIdx.x * 256 + threadIdx.x, texts + (unsigned long long)blockIdx.y * text_pitch, dwords);
}

struct ScratchLayout { size_t acc, tickets, flen, blk_bytes, parts, blkbuf, files, file_pitch, total; unsigned nwg; };
ScratchLayout layout_of(int n, const DeflGeom& g) {
    ScratchLayout L;
    const size_t crc_bound = (size_t)g.file_bound - kIdatType - 4 - 12;
    L.nwg = (unsigned)((crc_bound + (size_t)kCrcWG * kSlice - 1) / ((size_t)kCrcWG * kSlice));
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.acc = 0;                                                       // n x (S, T) u64
    L.tickets = (size_t)n * 16;                                      // n x u32, directly behind the sums: one memset clears both
    L.flen = up(L.tickets + (size_t)n * 4);                          // n x u64
    L.blk_bytes = up(L.flen + (size_t)n * 8);                        // n x nblk u32
    L.parts = up(L.blk_bytes + (size_t)n * g.nblk * 4);              // n x nwg CRC registers
    L.blkbuf = up(L.parts + (size_t)n * L.nwg * 4);                  // n x nblk x kBlkStride
    L.files = up(L.blkbuf + (size_t)n * g.nblk * kBlkStride);
    L.file_pitch = up(((size_t)g.file_bound + 11) / 12 * 12 + 16);   // (the 12-byte groups of the last base64 threads stay inside)
    L.total = L.files + L.file_pitch * (size_t)n;
    return L;
}

}  // namespace

size_t png_deflate_file_bound(int h, int w) { return (size_t)geom_of(h, w).file_bound; }
size_t png_deflate_base64_bound(int h, int w) { return (png_deflate_file_bound(h, w) + 2) / 3 * 4; }
size_t png_deflate_scratch_bytes(int n, int h, int w) { return layout_of(n, geom_of(h, w)).total; }

void encode_png_deflate_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                                      unsigned char* d_chars, size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, hipStream_t s) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the PNG encoder (1..8192 per side)");
    if (row_pitch < (size_t)3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row pitch for the PNG encoder (< 3*w)");
    const DeflGeom g = geom_of(h, w);
    const ScratchLayout L = layout_of(n, g);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(d_scratch + L.acc);
    unsigned* tickets = reinterpret_cast<unsigned*>(d_scratch + L.tickets);
    unsigned long long* flen = reinterpret_cast<unsigned long long*>(d_scratch + L.flen);
    unsigned* blk_bytes = reinterpret_cast<unsigned*>(d_scratch + L.blk_bytes);
    unsigned* parts = reinterpret_cast<unsigned*>(d_scratch + L.parts);
    unsigned char* blkbuf = d_scratch + L.blkbuf;
    unsigned char* files = d_scratch + L.files;
    IRE_HIP(hipMemsetAsync(d_scratch, 0, (size_t)n * 20, s));       // the sums and the tickets
    const PngSrc src{d_rgb, (unsigned long long)row_pitch, (unsigned long long)image_pitch};
    hipLaunchKernelGGL(deflate_block_kernel, dim3(g.nblk, n), dim3(kThreads), 0, s, src, g, blkbuf, blk_bytes, acc);
    hipLaunchKernelGGL(deflate_gather_kernel, dim3(g.nblk, n), dim3(kThreads), 0, s, g, png_ihdr(h, w), blkbuf, blk_bytes, acc, files, (unsigned long long)L.file_pitch, flen,
                       d_lens, (unsigned long long)lens_pitch);
    CrcOps ops;
    for (int l = 0; l < 8; ++l) ops.lvl[l] = gf_x_pow_8n((unsigned long long)kSlice << l);
    ops.wg = gf_x_pow_8n((unsigned long long)kCrcWG * kSlice);
    hipLaunchKernelGGL(deflate_crc_kernel, dim3(L.nwg, n), dim3(kCrcWG), 0, s, files, (unsigned long long)L.file_pitch, flen, ops, parts, tickets);
    base64_device_length_launch(files, L.file_pitch, flen, (size_t)g.file_bound, n, d_chars, text_pitch, s);
    IRE_HIP(hipGetLastError());
}

void base64_device_length_launch(const unsigned char* d_files, size_t file_pitch, const unsigned long long* d_flen, size_t file_bound, int n, unsigned char* d_chars,
                                 size_t text_pitch, hipStream_t s) {
    const unsigned long long groups12 = ((unsigned long long)file_bound + 11) / 12;
    hipLaunchKernelGGL(deflate_base64_kernel, dim3((unsigned)((groups12 + 255) / 256), n), dim3(256), 0, s, d_files, (unsigned long long)file_pitch, d_flen, d_chars,
                       (unsigned long long)text_pitch);
}

}  // namespace ire
