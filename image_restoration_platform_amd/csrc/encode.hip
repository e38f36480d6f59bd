// encode.hip -- the result side of the restoreImage seam on the device: restored RGB pixels -> the base64 text of a PNG file.
//
// The reference's result contract is a base64 STRING of an ENCODED image (server-node/src/services/restorator.js:108:
// `restoredImage: result.base64Image`; geminiClient.js:75-88 hands the provider's base64 through).  Round 3 measured the whole Node
// seam JS-thread-bound on exactly that: V8's base64 of a raw 3-MB image is 1.03 ms per job on the one JS thread, and with a real codec
// (PIL's PNG of a 1024^2 photo: ~0.2 s of zlib per image and core; JPEG q85: ~15 ms) the codec, not the engine, sets the rate of a
// deployed worker (tools/codec_seam_rate.py).  This file removes the result side's host work altogether: three
// small kernels behind the restore write, for a whole batch (the image is a grid dimension), a complete PNG file per image -- signature, IHDR, ONE IDAT chunk holding a zlib stream of
// STORED deflate blocks (filter type 0 on every scanline), IEND -- with its Adler-32 and CRC-32 computed on the device, and then its
// base64 text.  Every PNG decoder reads it (stored blocks are plain deflate); it is 0.2 % larger than the pixels where a compressed
// PNG of a photograph is 20-30 % smaller -- the trade is host CPU seconds for 1 MB more per result on the wire.  The host receives
// ASCII it can hand to the client as it is (Node: buf.latin1Slice(); Python: bytes.decode('ascii')).
//
// Integer / byte work, bit-exact by construction against zlib.adler32, zlib.crc32, base64.b64encode and PIL's decoder
// (oracle/encode.py; tests/test_encode_gpu.py).  HBM-bound by bytes: ~3 (pixels) + 3 + 3 (file written, read) + 4 (text) = 13 B per
// pixel-byte triple... ~14 MB per 1024^2 image, a few microseconds; in practice three dependent launches per BATCH.  The same file holds
// the two byte movers of the any-size path: the edge-replicate pad in front of the network and the crop of the window behind it.
#include "encode.hpp"

#include <cstring>

namespace ire {

namespace {

constexpr unsigned kCrcPoly = 0xedb88320u;      // reflected CRC-32 (zlib)
constexpr int kStored = 65535;                  // bytes of one stored deflate block
constexpr int kSlice = 256;                     // bytes of the IDAT chunk a thread runs its CRC over
constexpr int kCrcWG = 256;                     // threads (slices) per workgroup: 64 KB of the chunk

// ---- CRC-32 arithmetic in GF(2)[x] / p(x), reflected representation (bit 31 = x^0), as zlib's crc32.c does it -----------------------
__host__ __device__ inline unsigned gf_mul(unsigned a, unsigned b) {        // a(x) * b(x) mod p(x)
    unsigned m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
inline unsigned gf_x_pow_8n(size_t nbytes) {     // x^(8 nbytes) mod p: what feeding nbytes zero bytes does to a CRC register
    unsigned sq = 1u << 30, p = 1u << 31;       // x^1, x^0
    size_t n = nbytes * 8;
    while (n) { if (n & 1) p = gf_mul(sq, p); sq = gf_mul(sq, sq); n >>= 1; }
    return p;
}
unsigned host_crc32(const unsigned char* d, size_t n) {
    unsigned c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) { c ^= d[i]; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1; }
    return c ^ 0xffffffffu;
}

struct PngGeom {
    int h, w;
    unsigned row;             // bytes of a filtered scanline: 1 + 3 w
    unsigned long long raw;   // bytes of the raw (filtered) stream: h * row
    unsigned nblk;            // stored blocks
    unsigned long long zlen;  // zlib stream: 2 + 5 nblk + raw + 4
    unsigned long long file;  // 8 + 25 + (12 + zlen) + 12
    unsigned long long idat;  // file offset of the IDAT chunk's type field ("IDAT": the CRC starts here) = 8 + 25 + 4
    unsigned long long crc_len;   // bytes the IDAT CRC covers: 4 + zlen
};
PngGeom geom_of(int h, int w) {
    PngGeom g;
    g.h = h; g.w = w;
    g.row = 1u + 3u * (unsigned)w;
    g.raw = (unsigned long long)h * g.row;
    g.nblk = (unsigned)((g.raw + kStored - 1) / kStored);
    g.zlen = 2 + 5ull * g.nblk + g.raw + 4;
    g.file = 8 + 25 + 12 + g.zlen + 12;
    g.idat = 8 + 25 + 4;
    g.crc_len = 4 + g.zlen;
    return g;
}

struct PngHead { unsigned char b[41]; };       // signature + IHDR chunk (CRC included) + the IDAT chunk's length and type
__constant__ unsigned char kIend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};

// Where the pixels lie: the encoder reads the top-left h x w window of n images whose rows are row_pitch bytes and whose first
// pixels are image_pitch bytes apart (a tightly packed batch: 3 w and 3 w h).  Nothing about the pitches is assumed: a row may
// start at any byte, so the pixels are read as bytes.
struct PngSrc { const unsigned char* rgb; unsigned long long row_pitch, image_pitch; };

// The Adler-32 schedule.  adler = ((N + N S - T) mod 65521) << 16 | (1 + S) mod 65521 with S = sum d_i, T = sum i d_i over the raw
// stream (i the byte's index in it, N its length).  T is kept small by reducing where it would otherwise grow:
//   per byte      (i mod 65521) * d                      <= 65520 * 255                     (32 bits)
//   per thread    kFrameDwords * 4 such terms, then mod  <= 16 * 65520 * 255 = 267 321 600  (32 bits) -> < 65521
//   per workgroup 256 reduced thread sums                <= 256 * 65520 = 16 773 120        (32 bits)
//   per image     one 64-bit atomic add per workgroup    <= workgroups * 16 773 120         (64 bits: < 2^42 at 16384 x 16384)
// S needs no reduction: 255 * N < 2^38.  tests/test_fit_abi.py::test_adler_schedule_bounds redoes this arithmetic in integers.
constexpr unsigned kAdlerMod = 65521u;
constexpr int kFrameDwords = 4;                 // dwords of the file a thread of K1 writes (256 apart: a workgroup covers 4 KB)
constexpr int kFrameThreads = 256;              // threads of a K1 workgroup
static_assert((unsigned long long)kFrameDwords * 4 * (kAdlerMod - 1) * 255 < (1ull << 32), "a thread's T must fit 32 bits before its mod");
static_assert((unsigned long long)kFrameThreads * (kAdlerMod - 1) < (1ull << 32), "a workgroup's sum of reduced thread sums must fit 32 bits");
static_assert((unsigned long long)kFrameThreads * kFrameDwords * 4 * 255 < (1ull << 32), "a workgroup's S must fit 32 bits");

// K1: every byte of the file except the two checksums, and the Adler sums of what it writes.  A thread writes kFrameDwords dwords
// (the file buffer is padded to a multiple of 4).  File regions: [0, 41) head | zlib header 78 01 | nblk x (5-byte stored-block
// header + <= 65535 raw bytes) | Adler-32 (K2) | IDAT CRC (K2) | IEND chunk.  blockIdx.y is the image.
__global__ __launch_bounds__(kFrameThreads) void png_frame_kernel(PngSrc src, PngGeom g, PngHead head, unsigned char* __restrict__ files, unsigned long long file_pitch,
                                                        unsigned long long* __restrict__ acc) {
    __shared__ unsigned s_s[kFrameThreads / 64], s_t[kFrameThreads / 64];
    const unsigned char* __restrict__ rgb = src.rgb + (unsigned long long)blockIdx.y * src.image_pitch;
    unsigned char* __restrict__ file = files + (unsigned long long)blockIdx.y * file_pitch;
    const unsigned long long z0 = g.idat + 4;                 // first byte of the zlib stream
    const unsigned long long d0 = z0 + 2;                     // first stored block
    const unsigned long long dend = d0 + 5ull * g.nblk + g.raw;
    unsigned S = 0, T = 0;
#pragma unroll
    for (int q = 0; q < kFrameDwords; ++q) {
        const unsigned long long o0 = (((unsigned long long)blockIdx.x * kFrameDwords + q) * kFrameThreads + threadIdx.x) * 4;
        if (o0 >= g.file) break;
        // position inside the stored blocks, kept up byte by byte; the one division by the scanline length happens at the first
        // raw byte of the dword (the raw index runs on across a block header)
        unsigned blk = 0, r = 0;
        if (o0 >= d0) { const unsigned rel = (unsigned)(o0 - d0); blk = rel / (kStored + 5); r = rel - blk * (kStored + 5); }     // (the largest file fits 32 bits)
        bool have = false;
        unsigned i = 0, y = 0, c = 0;
        unsigned out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long o = o0 + k;
            unsigned v = 0;
            if (o < 41) v = head.b[o];
            else if (o < d0) v = o == z0 ? 0x78u : 0x01u;
            else if (o < dend) {
                if (r < 5) {
                    const unsigned long long left = g.raw - (unsigned long long)blk * kStored;
                    const unsigned len = left < (unsigned)kStored ? (unsigned)left : (unsigned)kStored;
                    v = r == 0 ? (blk + 1 == g.nblk ? 1u : 0u) : r == 1 ? (len & 0xffu) : r == 2 ? (len >> 8) : r == 3 ? ((~len) & 0xffu) : (((~len) >> 8) & 0xffu);
                } else {
                    if (!have) { i = blk * kStored + (r - 5); y = i / g.row; c = i - y * g.row; have = true; }
                    if (c) {                                                      // (c == 0: the scanline's filter byte, 0)
                        v = rgb[(unsigned long long)y * src.row_pitch + (c - 1)];
                        S += v;
                        T += (i % kAdlerMod) * v;
                    }
                    ++i;
                    if (++c == g.row) { c = 0; ++y; }
                }
                if (++r == (unsigned)kStored + 5) { r = 0; ++blk; }
            } else if (o < dend + 8) v = 0;                           // Adler-32, CRC-32: written by png_crc_kernel
            else if (o < g.file) v = kIend[o - (dend + 8)];
            out |= v << (8 * k);
        }
        *reinterpret_cast<unsigned*>(file + o0) = out;
    }
    T %= kAdlerMod;
    for (int off = 32; off >= 1; off >>= 1) { S += __shfl_down(S, off, 64); T += __shfl_down(T, off, 64); }
    if ((threadIdx.x & 63) == 0) { s_s[threadIdx.x >> 6] = S; s_t[threadIdx.x >> 6] = T; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ws = 0, wt = 0;
        for (int k = 0; k < kFrameThreads / 64; ++k) { ws += s_s[k]; wt += s_t[k]; }
        if (ws) {                                            // (integers: any order of the adds gives the same sums)
            atomicAdd(&acc[2 * blockIdx.y], (unsigned long long)ws);
            atomicAdd(&acc[2 * blockIdx.y + 1], (unsigned long long)wt);
        }
    }
}

// K2: the Adler-32 into the file, then the CRC-32 of the IDAT chunk (type + zlib stream, Adler included) in two levels: a thread
// runs the byte-wise CRC over its 256-byte slice from register 0 (the chunk's first slice from 0xffffffff); a workgroup combines its
// 256 slices by a tree (level l: reg(A || B) = reg(A) x^(8 |B|) + reg(B), |B| = 256 * 2^l bytes: operators from the host); the per-
// workgroup registers go to `part`, and the LAST workgroup of an image (ticket) folds them left to right with the 64-KB operator and
// the tail's own.  blockIdx.y is the image.
struct CrcOps { unsigned lvl[8]; unsigned wg; unsigned last_wg; };     // x^(8 * 256 * 2^l), x^(8 * 65536), x^(8 * bytes of the last workgroup's share)
__global__ __launch_bounds__(kCrcWG) void png_crc_kernel(unsigned char* __restrict__ files, unsigned long long file_pitch, PngGeom g, CrcOps ops,
                                                          const unsigned long long* __restrict__ acc_all, unsigned* __restrict__ part_all, unsigned* __restrict__ tickets) {
    __shared__ unsigned s_tab[256];
    __shared__ unsigned s_reg[kCrcWG];
    __shared__ unsigned s_last;
    unsigned char* __restrict__ file = files + (unsigned long long)blockIdx.y * file_pitch;
    const unsigned long long* acc = acc_all + 2 * blockIdx.y;
    unsigned* part = part_all + (size_t)blockIdx.y * gridDim.x;
    unsigned* ticket = tickets + blockIdx.y;
    {   // byte table of the reflected polynomial
        unsigned c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        s_tab[threadIdx.x] = c;
    }
    const unsigned long long adler_off = g.idat + 4 + g.zlen - 4;
    // every workgroup derives the same Adler-32 (two loads); the one whose slices hold it patches the bytes in before reading them
    const unsigned long long S = acc[0], T = acc[1];
    const unsigned A = (unsigned)((1 + S) % kAdlerMod);
    const unsigned B = (unsigned)((g.raw % kAdlerMod + (g.raw % kAdlerMod) * (S % kAdlerMod) + kAdlerMod - T % kAdlerMod) % kAdlerMod);
    const unsigned adler = (B << 16) | A;
    __syncthreads();
    const unsigned long long lo = (unsigned long long)blockIdx.x * (kCrcWG * kSlice) + (unsigned long long)threadIdx.x * kSlice;     // offset within the CRC'd range
    unsigned reg = (blockIdx.x == 0 && threadIdx.x == 0) ? 0xffffffffu : 0u;
    if (lo < g.crc_len) {
        const unsigned long long hi = lo + kSlice < g.crc_len ? lo + kSlice : g.crc_len;
        for (unsigned long long o = lo; o < hi; ++o) {
            const unsigned long long fo = g.idat + o;
            unsigned v = file[fo];
            if (fo >= adler_off && fo < adler_off + 4) { v = (adler >> (8 * (3 - (fo - adler_off)))) & 0xffu; file[fo] = (unsigned char)v; }     // big-endian
            reg = s_tab[(reg ^ v) & 0xffu] ^ (reg >> 8);
        }
    }
    // Every slice but the chunk's last is full; a partial / empty slice to the right of it is combined with its TRUE length
    // (0 .. 255 bytes), i.e. the operator x^(8 len) computed here (rare: a few threads per image).
    s_reg[threadIdx.x] = reg;
    __syncthreads();
    // true byte count of the slices [t, t + span) of this workgroup
    auto bytes_of = [&](unsigned t, unsigned span) -> unsigned long long {
        const unsigned long long a = (unsigned long long)blockIdx.x * (kCrcWG * kSlice) + (unsigned long long)t * kSlice;
        const unsigned long long b = a + (unsigned long long)span * kSlice;
        const unsigned long long aa = a < g.crc_len ? a : g.crc_len, bb = b < g.crc_len ? b : g.crc_len;
        return bb - aa;
    };
    for (int l = 0; l < 8; ++l) {
        const unsigned span = 1u << l;
        if ((threadIdx.x & (2 * span - 1)) == 0) {
            const unsigned long long nb = bytes_of(threadIdx.x + span, span);           // bytes of the right half
            unsigned op = ops.lvl[l];
            if (nb != (unsigned long long)span * kSlice) {                               // the chunk's tail: its own operator
                unsigned sq = 1u << 30, p = 1u << 31;
                unsigned long long n = nb * 8;
                while (n) { if (n & 1) p = gf_mul(sq, p); sq = gf_mul(sq, sq); n >>= 1; }
                op = p;
            }
            s_reg[threadIdx.x] = gf_mul(op, s_reg[threadIdx.x]) ^ s_reg[threadIdx.x + span];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part[blockIdx.x], s_reg[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned r = 0;
        for (unsigned k = 0; k < gridDim.x; ++k) {
            const unsigned pk = __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r = k == 0 ? pk : gf_mul(k + 1 == gridDim.x ? ops.last_wg : ops.wg, r) ^ pk;
        }
        const unsigned crc = r ^ 0xffffffffu;
        const unsigned long long co = g.idat + g.crc_len;
        file[co] = (unsigned char)(crc >> 24); file[co + 1] = (unsigned char)(crc >> 16); file[co + 2] = (unsigned char)(crc >> 8); file[co + 3] = (unsigned char)crc;
    }
}

// K3: base64 (RFC 4648, '=' padded): a thread turns 12 file bytes (three dwords) into 16 characters (four dwords).  blockIdx.y is
// the image.
__device__ __forceinline__ unsigned b64_char(unsigned v) {     // 0..63 -> 'A'..'Z' 'a'..'z' '0'..'9' '+' '/'
    return v < 26 ? v + 65 : v < 52 ? v + 71 : v < 62 ? v - 4 : v == 62 ? 43 : 47;
}
__global__ __launch_bounds__(256) void base64_kernel(const unsigned char* __restrict__ files, unsigned long long file_pitch, unsigned long long n,
                                                      unsigned char* __restrict__ texts, unsigned long long text_pitch) {
    const unsigned char* __restrict__ in = files + (unsigned long long)blockIdx.y * file_pitch;
    unsigned char* __restrict__ out = texts + (unsigned long long)blockIdx.y * text_pitch;
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long i0 = t * 12;
    if (i0 >= n) return;
    const unsigned* src = reinterpret_cast<const unsigned*>(in + i0);          // the file buffer is padded to a multiple of 12 readable bytes
    const unsigned w[3] = {src[0], src[1], src[2]};
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                                             // group q: input bytes 3 q .. 3 q + 2
        unsigned b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const int j = 3 * q + k; b[k] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }
        const unsigned long long at = i0 + 3 * q;
        const unsigned have = at >= n ? 0u : (n - at >= 3 ? 3u : (unsigned)(n - at));
        if (have < 3) b[2] = 0;
        if (have < 2) b[1] = 0;
        const unsigned v = (b[0] << 16) | (b[1] << 8) | b[2];
        const unsigned c0 = b64_char(v >> 18), c1 = b64_char((v >> 12) & 63u), c2 = have >= 2 ? b64_char((v >> 6) & 63u) : 61u, c3 = have >= 3 ? b64_char(v & 63u) : 61u;
        o[q] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
    const unsigned long long groups = (n + 2) / 3, g0 = t * 4;
    unsigned char* dst = out + g0 * 4;
    if ((text_pitch & 3u) == 0 && (reinterpret_cast<unsigned long long>(texts) & 3u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (g0 + q < groups) reinterpret_cast<unsigned*>(dst)[q] = o[q];
    } else {                                                                  // a caller's stride that is no multiple of 4: bytes
#pragma unroll
        for (int q = 0; q < 4; ++q) if (g0 + q < groups) { dst[4 * q] = (unsigned char)o[q]; dst[4 * q + 1] = (unsigned char)(o[q] >> 8); dst[4 * q + 2] = (unsigned char)(o[q] >> 16); dst[4 * q + 3] = (unsigned char)(o[q] >> 24); }
    }
}

// ---- any-size jobs: edge-replicate pad in front of the network, crop of the window behind it ---------------------------------------
// [n][h][w][3] -> [n][H][W][3], pixel (y, x) = source (min(y, h - 1), min(x, w - 1)).  3 W is a multiple of 4 (W % 8 == 0) and the
// destination is the engine's own staging: a thread stores one dword of a padded row; the source is read as bytes.
__global__ __launch_bounds__(256) void pad_edge_kernel(const unsigned char* __restrict__ src, int h, int w, unsigned char* __restrict__ dst, int H, int W) {
    const unsigned dw_row = 3u * (unsigned)W / 4u;
    const unsigned xd = blockIdx.x * 256 + threadIdx.x;
    if (xd >= dw_row) return;
    const unsigned y = blockIdx.y, img = blockIdx.z;
    const unsigned sy = y < (unsigned)h ? y : (unsigned)h - 1;
    const unsigned char* __restrict__ srow = src + ((size_t)img * h + sy) * (size_t)w * 3;
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned b = xd * 4 + k, x = b / 3, c = b - x * 3;
        const unsigned sx = x < (unsigned)w ? x : (unsigned)w - 1;
        out |= (unsigned)srow[sx * 3 + c] << (8 * k);
    }
    reinterpret_cast<unsigned*>(dst + ((size_t)img * H + y) * (size_t)W * 3)[xd] = out;
}

// The same pad with a PITCHED source: the h x w window at the top left of images whose rows lie row_pitch and whose first pixels lie
// image_pitch bytes apart (a restored window inside the network's padded output) -> dense [n][H][W][3].  One dword per thread.
__global__ __launch_bounds__(256) void pad_edge_pitched_kernel(const unsigned char* __restrict__ src, unsigned long long row_pitch, unsigned long long image_pitch,
                                                               int h, int w, unsigned char* __restrict__ dst, int H, int W) {
    const unsigned dw_row = 3u * (unsigned)W / 4u;
    const unsigned xd = blockIdx.x * 256 + threadIdx.x;
    if (xd >= dw_row) return;
    const unsigned y = blockIdx.y, img = blockIdx.z;
    const unsigned sy = y < (unsigned)h ? y : (unsigned)h - 1;
    const unsigned char* __restrict__ srow = src + img * image_pitch + sy * row_pitch;
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned b = xd * 4 + k, x = b / 3, c = b - x * 3;
        const unsigned sx = x < (unsigned)w ? x : (unsigned)w - 1;
        out |= (unsigned)srow[sx * 3 + c] << (8 * k);
    }
    reinterpret_cast<unsigned*>(dst + ((size_t)img * H + y) * (size_t)W * 3)[xd] = out;
}

// the top-left h x w window of [n][H][W][3] -> [n][h][w][3] tightly packed.  The packed result is one run of n*h*w*3 bytes; a thread
// moves the 4 of them that share a dword of the destination (`mis` = the destination's address mod 4), so every thread but the
// first and the last of the run stores one aligned dword whatever h*w*3 and the caller's pointer are.
__global__ __launch_bounds__(256) void crop_window_kernel(const unsigned char* __restrict__ src, int H, int W, unsigned char* __restrict__ dst, int n, int h, int w, unsigned mis) {
    const unsigned long long per = (unsigned long long)h * w * 3, total = per * (unsigned long long)n;
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long lo = t * 4 < mis ? 0 : t * 4 - mis, hi = t * 4 + 4 - mis < total ? t * 4 + 4 - mis : total;      // [lo, hi) of the run
    if (lo >= hi) return;
    const unsigned row = 3u * (unsigned)w;
    unsigned long long img = lo / per;
    const unsigned long long rem = lo - img * per;
    unsigned y = (unsigned)(rem / row), c = (unsigned)(rem - (unsigned long long)y * row);
    const unsigned cnt = (unsigned)(hi - lo);
    unsigned v[4] = {0, 0, 0, 0};
    for (unsigned k = 0; k < cnt; ++k) {
        v[k] = src[((size_t)img * H + y) * (size_t)W * 3 + c];
        if (++c == row) { c = 0; if (++y == (unsigned)h) { y = 0; ++img; } }
    }
    if (cnt == 4) *reinterpret_cast<unsigned*>(dst + lo) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    else for (unsigned k = 0; k < cnt; ++k) dst[lo + k] = (unsigned char)v[k];
}

struct ScratchLayout { size_t acc, tickets, parts, files, file_pitch, total; unsigned nwg; };
ScratchLayout layout_of(int n, const PngGeom& g) {
    ScratchLayout L;
    L.nwg = (unsigned)((g.crc_len + (size_t)kCrcWG * kSlice - 1) / ((size_t)kCrcWG * kSlice));
    L.acc = 0;                                                       // n x (S, T) u64
    L.tickets = (size_t)n * 16;                                      // n x u32, directly behind the sums: one memset clears both
    L.parts = (L.tickets + (size_t)n * 4 + 255) / 256 * 256;         // n x nwg CRC registers
    L.files = (L.parts + (size_t)n * L.nwg * 4 + 255) / 256 * 256;
    L.file_pitch = (((size_t)g.file + 11) / 12 * 12 + 16 + 255) / 256 * 256;     // (padded so that the 12-byte groups of the last base64 threads stay inside)
    L.total = L.files + L.file_pitch * (size_t)n;
    return L;
}

}  // namespace

size_t png_file_bytes(int h, int w) { return (size_t)geom_of(h, w).file; }
size_t png_base64_chars(int h, int w) { return (png_file_bytes(h, w) + 2) / 3 * 4; }
size_t png_scratch_bytes(int n, int h, int w) { return layout_of(n, geom_of(h, w)).total; }

// The top-left h x w window of n images (rows row_pitch, images image_pitch bytes apart) -> n texts text_pitch bytes apart
// (png_base64_chars(h, w) bytes of ASCII each).  d_scratch: png_scratch_bytes(n, h, w); nothing in it has to be initialised.
// One memset of the n Adler sums and tickets and three launches on `s`, whatever n is.
void encode_png_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                              unsigned char* d_chars, size_t text_pitch, hipStream_t s) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || h > 16384 || w > 16384) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the PNG encoder (1..16384 per side)");
    if (row_pitch < (size_t)3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row pitch for the PNG encoder (< 3*w)");
    const PngGeom g = geom_of(h, w);
    const ScratchLayout L = layout_of(n, g);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(d_scratch + L.acc);
    unsigned* tickets = reinterpret_cast<unsigned*>(d_scratch + L.tickets);
    unsigned* parts = reinterpret_cast<unsigned*>(d_scratch + L.parts);
    unsigned char* files = d_scratch + L.files;
    PngHead head;
    {
        static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        std::memcpy(head.b, sig, 8);
        unsigned char* c = head.b + 8;
        c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 13; c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
        c[8] = (unsigned char)(w >> 24); c[9] = (unsigned char)(w >> 16); c[10] = (unsigned char)(w >> 8); c[11] = (unsigned char)w;
        c[12] = (unsigned char)(h >> 24); c[13] = (unsigned char)(h >> 16); c[14] = (unsigned char)(h >> 8); c[15] = (unsigned char)h;
        c[16] = 8; c[17] = 2; c[18] = 0; c[19] = 0; c[20] = 0;
        const unsigned crc = host_crc32(c + 4, 17);
        c[21] = (unsigned char)(crc >> 24); c[22] = (unsigned char)(crc >> 16); c[23] = (unsigned char)(crc >> 8); c[24] = (unsigned char)crc;
        unsigned char* d = head.b + 33;
        d[0] = (unsigned char)(g.zlen >> 24); d[1] = (unsigned char)(g.zlen >> 16); d[2] = (unsigned char)(g.zlen >> 8); d[3] = (unsigned char)g.zlen;
        d[4] = 'I'; d[5] = 'D'; d[6] = 'A'; d[7] = 'T';
    }
    IRE_HIP(hipMemsetAsync(d_scratch, 0, (size_t)n * 20, s));       // the sums and the tickets
    const PngSrc src{d_rgb, (unsigned long long)row_pitch, (unsigned long long)image_pitch};
    const unsigned long long dwords = (g.file + 3) / 4;
    const unsigned fgrid = (unsigned)((dwords + (unsigned long long)kFrameThreads * kFrameDwords - 1) / ((unsigned long long)kFrameThreads * kFrameDwords));
    hipLaunchKernelGGL(png_frame_kernel, dim3(fgrid, n), dim3(kFrameThreads), 0, s, src, g, head, files, (unsigned long long)L.file_pitch, acc);
    CrcOps ops;
    for (int l = 0; l < 8; ++l) ops.lvl[l] = gf_x_pow_8n((size_t)kSlice << l);
    const size_t wg_bytes = (size_t)kCrcWG * kSlice;
    ops.wg = gf_x_pow_8n(wg_bytes);
    ops.last_wg = gf_x_pow_8n((size_t)(g.crc_len - (unsigned long long)(L.nwg - 1) * wg_bytes));
    hipLaunchKernelGGL(png_crc_kernel, dim3(L.nwg, n), dim3(kCrcWG), 0, s, files, (unsigned long long)L.file_pitch, g, ops, acc, parts, tickets);
    const unsigned long long groups12 = (g.file + 11) / 12;
    hipLaunchKernelGGL(base64_kernel, dim3((unsigned)((groups12 + 255) / 256), n), dim3(256), 0, s, files, (unsigned long long)L.file_pitch, g.file, d_chars,
                       (unsigned long long)text_pitch);
    IRE_HIP(hipGetLastError());
}

// d_src [n][h][w][3] -> d_dst [n][H][W][3], edge-replicated (H >= h, W >= w, W % 8 == 0).  One launch.
void pad_edge_launch(const unsigned char* d_src, int n, int h, int w, unsigned char* d_dst, int H, int W, hipStream_t s) {
    if (n < 1 || h < 1 || w < 1 || H < h || W < w || W % 8 || H > 65535 || n > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid sizes for the edge pad");
    const unsigned dw_row = 3u * (unsigned)W / 4u;
    hipLaunchKernelGGL(pad_edge_kernel, dim3((dw_row + 255) / 256, H, n), dim3(256), 0, s, d_src, h, w, d_dst, H, W);
    IRE_HIP(hipGetLastError());
}

// the h x w windows of n pitched images -> d_dst [n][H][W][3], edge-replicated (H >= h, W >= w, W % 8 == 0, d_dst 4-byte aligned).  One launch.
void pad_edge_pitched_launch(const unsigned char* d_src, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_dst, int H, int W, hipStream_t s) {
    if (n < 1 || h < 1 || w < 1 || H < h || W < w || W % 8 || H > 65535 || n > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid sizes for the edge pad");
    if (row_pitch < (size_t)3 * w || (n > 1 && image_pitch < row_pitch * (size_t)(h - 1) + (size_t)3 * w)) fail(IRE_ERR_INVALID_INPUT, "invalid pitch for the edge pad: rows or images overlap");
    const unsigned dw_row = 3u * (unsigned)W / 4u;
    hipLaunchKernelGGL(pad_edge_pitched_kernel, dim3((dw_row + 255) / 256, H, n), dim3(256), 0, s, d_src, (unsigned long long)row_pitch, (unsigned long long)image_pitch, h, w,
                       d_dst, H, W);
    IRE_HIP(hipGetLastError());
}

// the top-left h x w window of d_src [n][H][W][3] -> d_dst [n][h][w][3].  One launch.
void crop_window_launch(const unsigned char* d_src, int n, int H, int W, unsigned char* d_dst, int h, int w, hipStream_t s) {
    if (n < 1 || h < 1 || w < 1 || H < h || W < w || n > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid sizes for the window crop");
    const unsigned long long total = (unsigned long long)h * w * 3 * n;
    const unsigned mis = (unsigned)(reinterpret_cast<size_t>(d_dst) & 3u);
    hipLaunchKernelGGL(crop_window_kernel, dim3((unsigned)((total + mis + 1023) / 1024)), dim3(256), 0, s, d_src, H, W, d_dst, n, h, w, mis);
    IRE_HIP(hipGetLastError());
}

}  // namespace ire
