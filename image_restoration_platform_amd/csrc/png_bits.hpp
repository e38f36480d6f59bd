// png_bits.hpp -- what the two PNG encoders (encode.hip: stored blocks; deflate.hip: Huffman-coded blocks) share: CRC-32 arithmetic,
// the base64 alphabet, the description of where the pixels lie, the file's fixed head.
#pragma once
#include <cstring>

#include "common.hpp"

namespace ire {
namespace pngbits {

constexpr unsigned kCrcPoly = 0xedb88320u;      // reflected CRC-32 (zlib)
constexpr unsigned kAdlerBase = 65521u;

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
__host__ __device__ inline unsigned gf_x_pow_8n(unsigned long long nbytes) {     // x^(8 nbytes) mod p: what feeding nbytes zero bytes does to a CRC register
    unsigned sq = 1u << 30, p = 1u << 31;       // x^1, x^0
    unsigned long long n = nbytes * 8;
    while (n) { if (n & 1) p = gf_mul(sq, p); sq = gf_mul(sq, sq); n >>= 1; }
    return p;
}
inline unsigned host_crc32(const unsigned char* d, size_t n) {
    unsigned c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) { c ^= d[i]; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1; }
    return c ^ 0xffffffffu;
}

// Where the pixels lie: the encoders read the top-left h x w window of n images whose rows are row_pitch bytes and whose first
// pixels are image_pitch bytes apart (a tightly packed batch: 3 w and 3 w h).  Nothing about the pitches is assumed: a row may
// start at any byte, so the pixels are read as bytes.
struct PngSrc { const unsigned char* rgb; unsigned long long row_pitch, image_pitch; };

// signature + IHDR chunk (8-bit RGB, CRC included): the first 33 bytes of every file
struct PngIhdr { unsigned char b[33]; };
inline PngIhdr png_ihdr(int h, int w) {
    PngIhdr o;
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::memcpy(o.b, sig, 8);
    unsigned char* c = o.b + 8;
    c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 13; c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
    c[8] = (unsigned char)(w >> 24); c[9] = (unsigned char)(w >> 16); c[10] = (unsigned char)(w >> 8); c[11] = (unsigned char)w;
    c[12] = (unsigned char)(h >> 24); c[13] = (unsigned char)(h >> 16); c[14] = (unsigned char)(h >> 8); c[15] = (unsigned char)h;
    c[16] = 8; c[17] = 2; c[18] = 0; c[19] = 0; c[20] = 0;
    const unsigned crc = host_crc32(c + 4, 17);
    c[21] = (unsigned char)(crc >> 24); c[22] = (unsigned char)(crc >> 16); c[23] = (unsigned char)(crc >> 8); c[24] = (unsigned char)crc;
    return o;
}

__device__ __forceinline__ unsigned b64_char(unsigned v) {     // 0..63 -> 'A'..'Z' 'a'..'z' '0'..'9' '+' '/'
    return v < 26 ? v + 65 : v < 52 ? v + 71 : v < 62 ? v - 4 : v == 62 ? 43 : 47;
}

// base64 (RFC 4648, '=' padded) of a file of n bytes: thread t turns file bytes [12 t, 12 t + 12) (three dwords; the buffer is
// readable up to a multiple of 12) into 16 characters (four dwords, or bytes when the text is not dword-aligned).
__device__ __forceinline__ void base64_thread(const unsigned char* __restrict__ in, unsigned long long n, unsigned long long t, unsigned char* __restrict__ out, bool dwords) {
    const unsigned long long i0 = t * 12;
    if (i0 >= n) return;
    const unsigned* src = reinterpret_cast<const unsigned*>(in + i0);
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
    if (dwords) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (g0 + q < groups) reinterpret_cast<unsigned*>(dst)[q] = o[q];
    } else {                                                                  // a caller's stride that is no multiple of 4: bytes
#pragma unroll
        for (int q = 0; q < 4; ++q) if (g0 + q < groups) { dst[4 * q] = (unsigned char)o[q]; dst[4 * q + 1] = (unsigned char)(o[q] >> 8); dst[4 * q + 2] = (unsigned char)(o[q] >> 16); dst[4 * q + 3] = (unsigned char)(o[q] >> 24); }
    }
}

}  // namespace pngbits
}  // namespace ire
