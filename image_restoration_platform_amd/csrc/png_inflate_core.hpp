// png_inflate_core.hpp -- the device's PNG decoder, written once: the inflate state machine (RFC 1950 / 1951) and the unfilter and colour
// arithmetic of a PNG scanline.  Plain C++17, no HIP header: every function is IRE_HD (__host__ __device__ under hipcc, nothing under
// g++).  csrc/png_dec.hip runs it with one wave per image; tests/native/png_dec_sim.cpp runs the same text with the lanes as a loop,
// under ASan and UBSan.
//
// One stream is one `Inflate` record (LDS in the kernel).  The work is cut into PHASES; between two phases the driver puts a barrier
// (the kernel: __syncthreads, the simulator: the end of its lane loop):
//   begin(S, ...)        lane 0   the zlib header
//   window_load(S, lane) all      in front of each of lane 0's phases: the next kWindow bytes of the input into the record, when lane 0
//                                 is within kWindowNeed bytes of the window's end (a phase reads less than that: see there);
//                                 lane 0 then commits the new window (window_commit) before it reads a bit
//   block_begin(S)       lane 0   the next block's header; a dynamic block's code lengths; both codes in canonical form
//   fill_fast(S, lane)   all      the two lookup tables, entry by entry
//   walk(S)              lane 0   decodes up to kQueue symbols into the queue: positions, distances, literals.  Writes no output.
//   place(S, lane, ...)  all      every output byte of the queue's range, byte p by lane (p - pos0) % kLanes, and its share of Adler-32
//   finish(S)            lane 0   the length, the trailer, the checksum -> the status
// place() resolves a byte through the queue: a literal is its value; a match byte k reads position start - dist + k % dist, which
// lies in front of its own entry, so the chase ends after at most one step per queue entry, in a byte of an earlier ROUND -- read from
// the output, which the barrier behind that round made visible -- or in a literal of this one.  No lane ever reads a byte another lane
// writes in the same phase.
//
// Every loop is bounded and every index is checked before it is used: input is never read at or past in_len, output never written at
// or past out_total, no distance reaches in front of byte 0.  A violation sets a status (first one wins) and ends the walk.
// Status 0 means exactly: zlib decompresses the stream without error, it yields exactly out_total bytes, and (png_dec.hip's second
// kernel) every filter byte is 0..4.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef IRE_HD
#if defined(__HIPCC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif
#endif

namespace ire {
namespace pngdec {

constexpr int kLanes = 64;            // one wave
constexpr int kQueue = 256;           // symbols a walk decodes before the lanes place them
constexpr int kLitFastBits = 10, kDistFastBits = 9;
// The input window: lane 0 reads bits from the record, never from the input itself.  One phase of lane 0 reads at most kWindowNeed
// bytes: a dynamic header 17 + 19 * 3 + 316 * (7 + 7) bits = 563 bytes; a walk kQueue * (15 + 5 + 15 + 13) bits = 1536 bytes; the bit
// buffer reads 8 bytes ahead.
constexpr uint32_t kWindow = 8192, kWindowNeed = 2048;
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kStoredMark = 0xFFFFFFFFu;      // a queue entry that copies from the input (a stored block)

enum Status : int32_t {
    kOk = 0,
    kStTruncated = 1,       // the input ends inside the stream
    kStBlockType = 2,       // block type 3
    kStStoredLen = 3,       // LEN != ~NLEN
    kStCodeLenSet = 4,      // the code-length code is over-subscribed or incomplete
    kStLitSet = 5,          // the literal/length code is over-subscribed or incomplete, or has too many symbols
    kStDistSet = 6,         // the distance code likewise (one code of one bit, or none at all, is allowed)
    kStRepeat = 7,          // a repeat code with nothing before it, or running past the last length
    kStBadCode = 8,         // bits that are no code of the set; literal/length symbol 286 / 287; distance symbol 30 / 31
    kStDistance = 9,        // a distance that reaches in front of the first output byte
    kStTooLong = 10,        // more output than h * (1 + w * bpp) bytes
    kStTooShort = 11,       // the last block ends with less
    kStAdler = 12,          // the trailer is not the output's Adler-32
    kStHeader = 13,         // no deflate stream with a window of at most 32 KiB and no preset dictionary
    kStNoEndCode = 14,      // a dynamic block whose symbol 256 has no code
    kStWindow = 15,         // lane 0 left its input window (not reached: kWindowNeed bounds a phase)
    kStFilter = 16,         // a scanline whose filter byte is not 0..4 (png_dec.hip's unfilter kernel)
};

// one image of a batch as the kernels read it
struct Record {
    uint64_t scan_off;      // its filtered scanlines in the scratch
    uint32_t in_off, in_len;      // its zlib stream in the blob's byte area
    uint32_t h, w, ctype, bpp;
    uint32_t dst, reserved;       // which image of the output, and which status word, is its
    uint8_t pal[768];       // colour type 3: the palette, zeros behind its last entry
    uint32_t depth, interlace;    // 8 and 0: the form the fields above describe alone; else png_adam7_core.hpp's (bpp: the filter unit)
    uint32_t scan_total, pad;     // the stream's expected length: h * (1 + w * bpp) for depth 8 without interlace, else the passes' sum
};

// a prefix code in canonical form: count[l] codes of l bits, their symbols in order
struct Huff {
    uint16_t count[16];
    uint16_t symbol[288];
};

enum : uint32_t { kKindNone = 0, kKindStored = 1, kKindHuff = 2 };

struct Inflate {
    const uint8_t* in;
    uint8_t* out;
    uint32_t in_len, in_i;
    uint32_t win_base, win_len;           // win[k] = in[win_base + k], k < win_len
    uint64_t bitbuf;
    uint32_t bitcnt;
    uint32_t out_total, pos;
    int32_t status;
    uint32_t last, kind, block_end, done;
    uint32_t stored_len;
    Huff lit, dist;
    uint16_t fast_lit[1 << kLitFastBits], fast_dist[1 << kDistFastBits];
    uint8_t lens[320];
    uint32_t qn, qpos[kQueue + 1], qdist[kQueue], qval[kQueue];
    uint64_t s1[kLanes], s2[kLanes];      // the lanes' shares of Adler-32
    uint8_t win[kWindow];
};

IRE_HD void fail(Inflate& S, int32_t st) { if (S.status == 0) S.status = st; }

// ---- bits ---------------------------------------------------------------------------------------------------------------------------
IRE_HD void refill(Inflate& S) {
    while (S.bitcnt <= 56 && S.in_i < S.in_len) {
        const uint32_t k = S.in_i - S.win_base;                 // (in front of the window: wraps, and is caught too)
        if (k >= S.win_len) { fail(S, kStWindow); return; }
        S.bitbuf |= (uint64_t)S.win[k] << S.bitcnt;
        S.bitcnt += 8; S.in_i += 1;
    }
}
// ---- the input window ---------------------------------------------------------------------------------------------------------------
IRE_HD bool window_stale(const Inflate& S) {
    const uint32_t end = S.win_base + S.win_len;
    return S.in_i < S.win_base || S.in_i > end || (end < S.in_len && end - S.in_i < kWindowNeed);
}
IRE_HD uint32_t window_base(const Inflate& S) { return S.in_i & ~3u; }
IRE_HD uint32_t window_len(const Inflate& S) { const uint32_t left = S.in_len - window_base(S); return left < kWindow ? left : kWindow; }      // in_i <= in_len
// all lanes: writes win[] only; nobody reads the window in this phase
IRE_HD void window_load(Inflate& S, int lane) {
    if (!window_stale(S)) return;
    const uint32_t base = window_base(S), len = window_len(S);
    const bool aligned = ((uintptr_t)(S.in + base) & 3u) == 0;
    for (uint32_t k = 4 * (uint32_t)lane; k < len; k += 4 * kLanes) {
        if (aligned && len - k >= 4) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(S.in + base + k);
            S.win[k] = (uint8_t)v; S.win[k + 1] = (uint8_t)(v >> 8); S.win[k + 2] = (uint8_t)(v >> 16); S.win[k + 3] = (uint8_t)(v >> 24);
        } else
            for (uint32_t j = k; j < len && j < k + 4; ++j) S.win[j] = S.in[base + j];
    }
}
// lane 0, behind the barrier that follows window_load
IRE_HD void window_commit(Inflate& S) {
    if (!window_stale(S)) return;
    const uint32_t base = window_base(S), len = window_len(S);
    S.win_base = base; S.win_len = len;
}
// the next bits, zeros behind the end of the input: what is USED of them is checked by drop
IRE_HD uint32_t peek(const Inflate& S, uint32_t k) { return (uint32_t)(S.bitbuf & (((uint64_t)1 << k) - 1)); }
IRE_HD bool drop(Inflate& S, uint32_t k) {
    if (k > S.bitcnt) { fail(S, kStTruncated); return false; }
    S.bitbuf >>= k; S.bitcnt -= k;
    return true;
}
IRE_HD uint32_t bits(Inflate& S, uint32_t k) {      // k <= 16
    refill(S);
    const uint32_t v = peek(S, k);
    return drop(S, k) ? v : 0;
}

// ---- codes --------------------------------------------------------------------------------------------------------------------------
// lens[0 .. n) -> h; returns what is left of the code space: 0 complete, > 0 incomplete, < 0 over-subscribed.  *maxlen: the longest code.
IRE_HD int construct(Huff& h, const uint8_t* lens, int n, int* maxlen) {
    uint16_t offs[16];
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int s = 0; s < n; ++s) h.count[lens[s] & 15] += 1;
    int left = 1, mx = 0;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) { *maxlen = 15; return left; }
        if (h.count[l]) mx = l;
    }
    *maxlen = mx;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s] & 15) h.symbol[offs[lens[s] & 15]++] = (uint16_t)s;       // (at most n <= 288 entries in all)
    h.count[0] = 0;
    return left;
}
// the symbol whose code the bits v start with (first bit of the stream in bit 0), its length to *len; -1: none within nbits bits
IRE_HD int decode_slow(const Huff& h, uint32_t v, int nbits, int* len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= nbits; ++l) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int count = h.count[l];
        if (code - count < first) { *len = l; return h.symbol[index + (code - first)]; }      // index + code - first < sum of counts <= 288
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}
// zlib's rule (inftrees.c) for a literal/length or distance set: over-subscribed never; incomplete only as ONE code of one bit, or none
IRE_HD bool set_ok(int left, int maxlen) { return left == 0 || (left > 0 && maxlen <= 1); }

// the lookup tables: entry i = (length << 9 | symbol) of the code that the bits i start with, 0 where that code is longer than the index
IRE_HD void fill_fast(Inflate& S, int lane) {
    for (int i = lane; i < (1 << kLitFastBits); i += kLanes) {
        int len = 0;
        const int s = decode_slow(S.lit, (uint32_t)i, kLitFastBits, &len);
        S.fast_lit[i] = (uint16_t)(s >= 0 ? (len << 9 | s) : 0);
    }
    for (int i = lane; i < (1 << kDistFastBits); i += kLanes) {
        int len = 0;
        const int s = decode_slow(S.dist, (uint32_t)i, kDistFastBits, &len);
        S.fast_dist[i] = (uint16_t)(s >= 0 ? (len << 9 | s) : 0);
    }
}
// the next symbol of a set; -1 (and a status) when the bits are no code or the input ends
IRE_HD int decode(Inflate& S, const Huff& h, const uint16_t* fast, int fast_bits) {
    refill(S);
    const uint32_t v = peek(S, 15);
    const uint32_t e = fast ? fast[v & ((1u << fast_bits) - 1)] : 0;
    int len = (int)(e >> 9), sym = (int)(e & 511u);
    if (!e) {
        sym = decode_slow(h, v, 15, &len);
        if (sym < 0) { fail(S, S.bitcnt < 15 ? kStTruncated : kStBadCode); return -1; }
    }
    return drop(S, (uint32_t)len) ? sym : -1;
}

// ---- phases -------------------------------------------------------------------------------------------------------------------------
IRE_HD void begin(Inflate& S, const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_total) {
    S.in = in; S.in_len = in_len; S.in_i = 0; S.bitbuf = 0; S.bitcnt = 0;
    S.win_base = 0; S.win_len = 0;
    S.out = out; S.out_total = out_total; S.pos = 0;
    S.status = 0; S.last = 0; S.kind = kKindNone; S.block_end = 1; S.done = 0; S.stored_len = 0; S.qn = 0;
    S.qpos[0] = 0;
    for (int l = 0; l < kLanes; ++l) { S.s1[l] = 0; S.s2[l] = 0; }
    if (in_len < 2) { fail(S, kStTruncated); return; }
    const uint32_t cmf = in[0], flg = in[1];
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8 | flg) % 31u) != 0 || (flg & 0x20u)) { fail(S, kStHeader); return; }
    S.in_i = 2;
}

// the fixed block's two codes (RFC 1951 3.2.6)
IRE_HD void fixed_lens(uint8_t* lens) {
    int s = 0;
    for (; s < 144; ++s) lens[s] = 8;
    for (; s < 256; ++s) lens[s] = 9;
    for (; s < 280; ++s) lens[s] = 7;
    for (; s < 288; ++s) lens[s] = 8;
    for (; s < 320; ++s) lens[s] = 5;       // 288 ..: thirty distance codes (and two that no stream may use)
}

// a dynamic block's header -> S.lens[0 .. nlen + ndist), S.lit, S.dist
IRE_HD void dynamic_header(Inflate& S) {
    const int nlen = (int)bits(S, 5) + 257, ndist = (int)bits(S, 5) + 1, ncode = (int)bits(S, 4) + 4;
    if (S.status) return;
    if (nlen > 286) { fail(S, kStLitSet); return; }
    if (ndist > 30) { fail(S, kStDistSet); return; }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) cl[order[i]] = (uint8_t)bits(S, 3);
    if (S.status) return;
    int mx = 0;
    // (zlib reads an all-zero set as lengths of zero and then misses symbol 256: an error either way)
    if (construct(S.lit, cl, 19, &mx) != 0) { fail(S, kStCodeLenSet); return; }
    int i = 0;
    while (i < nlen + ndist) {             // every turn stores at least one length or ends the walk
        const int sym = decode(S, S.lit, nullptr, 0);
        if (sym < 0) return;
        if (sym < 16) { S.lens[i++] = (uint8_t)sym; continue; }
        int prev = 0, rep = 0;
        if (sym == 16) {
            if (i == 0) { fail(S, kStRepeat); return; }
            prev = S.lens[i - 1];
            rep = 3 + (int)bits(S, 2);
        } else if (sym == 17) rep = 3 + (int)bits(S, 3);
        else rep = 11 + (int)bits(S, 7);
        if (S.status) return;
        if (i + rep > nlen + ndist) { fail(S, kStRepeat); return; }        // (a run may cross from the literal lengths into the distance lengths)
        while (rep--) S.lens[i++] = (uint8_t)prev;
    }
    if (S.lens[256] == 0) { fail(S, kStNoEndCode); return; }
    int left = construct(S.lit, S.lens, nlen, &mx);
    if (!set_ok(left, mx)) { fail(S, kStLitSet); return; }
    left = construct(S.dist, S.lens + nlen, ndist, &mx);
    if (!set_ok(left, mx)) { fail(S, kStDistSet); return; }
}

IRE_HD void block_begin(Inflate& S) {
    S.kind = kKindNone; S.block_end = 0; S.qn = 0;
    if (S.status) { S.done = 1; return; }
    if (S.last) { S.done = 1; return; }
    S.last = bits(S, 1);
    const uint32_t type = bits(S, 2);
    if (S.status) { S.done = 1; return; }
    if (type == 0) {
        (void)drop(S, S.bitcnt & 7u);
        const uint32_t len = bits(S, 16), nlen = bits(S, 16);
        if (!S.status && (len ^ 0xFFFFu) != nlen) fail(S, kStStoredLen);
        if (!S.status) {                   // whole bytes left in the bit buffer go back to the input
            S.in_i -= S.bitcnt >> 3;
            S.bitbuf = 0; S.bitcnt = 0;
            if (len > S.in_len - S.in_i) fail(S, kStTruncated);
        }
        S.stored_len = len;
        S.kind = kKindStored;
    } else if (type == 1) {
        int mx = 0;
        fixed_lens(S.lens);
        (void)construct(S.lit, S.lens, 288, &mx);
        (void)construct(S.dist, S.lens + 288, 32, &mx);
        S.kind = kKindHuff;
    } else if (type == 2) {
        dynamic_header(S);
        S.kind = kKindHuff;
    } else fail(S, kStBlockType);
    if (S.status) { S.done = 1; S.kind = kKindNone; }
}

// one queue entry of `len` bytes at S.pos; false (and a status) when it would pass the end of the output
IRE_HD bool push(Inflate& S, uint32_t len, uint32_t dist, uint32_t val) {
    if (len > S.out_total - S.pos) { fail(S, kStTooLong); return false; }
    S.qdist[S.qn] = dist; S.qval[S.qn] = val;
    S.pos += len;
    S.qpos[++S.qn] = S.pos;
    return true;
}

IRE_HD void walk(Inflate& S) {
    S.qn = 0;
    S.qpos[0] = S.pos;
    if (S.kind == kKindStored) {
        if (S.stored_len && push(S, S.stored_len, kStoredMark, S.in_i)) S.in_i += S.stored_len;       // (block_begin checked the input)
        S.block_end = 1;
        return;
    }
    while (S.qn < (uint32_t)kQueue) {
        const int sym = decode(S, S.lit, S.fast_lit, kLitFastBits);
        if (sym < 0) break;
        if (sym < 256) { if (!push(S, 1, 0, (uint32_t)sym)) break; continue; }
        if (sym == 256) { S.block_end = 1; break; }
        if (sym > 285) { fail(S, kStBadCode); break; }
        const uint32_t i = (uint32_t)sym - 257;
        uint32_t len = 258;
        if (i < 8) len = 3 + i;
        else if (i < 28) { const uint32_t e = (i >> 2) - 1; len = 3 + ((4 + (i & 3u)) << e) + bits(S, e); }
        const int ds = decode(S, S.dist, S.fast_dist, kDistFastBits);
        if (ds < 0) break;
        if (ds > 29) { fail(S, kStBadCode); break; }
        uint32_t dist = 1 + (uint32_t)ds;
        if (ds >= 4) { const uint32_t e = ((uint32_t)ds >> 1) - 1; dist = 1 + ((2 + ((uint32_t)ds & 1u)) << e) + bits(S, e); }
        if (S.status) break;
        if (dist > S.pos) { fail(S, kStDistance); break; }
        if (!push(S, len, dist, 0)) break;
    }
    if (S.status) S.block_end = 1;
}

// the byte at position p of the round [qpos[0], qpos[qn]); prior(q): the output byte at q < qpos[0], final since an earlier round
template <class Prior>
IRE_HD uint32_t resolve(const Inflate& S, uint32_t p, Prior&& prior) {
    uint32_t hi = S.qn;                                        // the entry of p is below hi
    for (int it = 0; it <= kQueue; ++it) {
        if (p < S.qpos[0]) return prior(p);
        uint32_t lo = 0;                                       // the last entry that starts at or before p
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (S.qpos[mid] <= p) lo = mid; else hi = mid; }
        const uint32_t d = S.qdist[lo], k = p - S.qpos[lo];
        if (d == 0) return S.qval[lo];
        if (d == kStoredMark) return S.in[S.qval[lo] + k];   // (walk checked qval + len <= in_len)
        p = S.qpos[lo] - d + k % d;                           // in front of entry lo (walk checked d <= qpos[lo])
        hi = lo;
        if (hi == 0) return prior(p);
    }
    return 0;      // (not reached: hi falls with every turn)
}

// lane's bytes of the round, and their share of Adler-32: a += x, b += (out_total - p) * x
IRE_HD void place(Inflate& S, int lane) {
    const uint32_t p0 = S.qpos[0], p1 = S.qpos[S.qn];
    uint64_t s1 = S.s1[lane], s2 = S.s2[lane];
    const uint8_t* out = S.out;
    for (uint32_t p = p0 + (uint32_t)lane; p < p1; p += kLanes) {      // p1 <= out_total (push)
        const uint32_t x = resolve(S, p, [out](uint32_t q) { return (uint32_t)out[q]; }) & 255u;
        S.out[p] = (uint8_t)x;
        s1 += x;
        s2 += (uint64_t)((S.out_total - p) % kAdlerMod) * x;          // < 2^24 a term, < 2^28 terms
    }
    S.s1[lane] = s1; S.s2[lane] = s2;
}

IRE_HD void finish(Inflate& S) {
    if (S.status) return;
    if (S.pos != S.out_total) { fail(S, kStTooShort); return; }
    (void)drop(S, S.bitcnt & 7u);
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = want << 8 | bits(S, 8);
    if (S.status) return;
    uint64_t a = 1, b = S.out_total;
    for (int l = 0; l < kLanes; ++l) { a += S.s1[l]; b += S.s2[l] % kAdlerMod; }
    const uint32_t got = (uint32_t)(b % kAdlerMod) << 16 | (uint32_t)(a % kAdlerMod);
    if (got != want) fail(S, kStAdler);
}

// ---- scanlines ----------------------------------------------------------------------------------------------------------------------
// One pixel of bpp <= 4 bytes is one uint32, its first byte in bits 0..7.  x: the filtered pixel; a, b, c: the raw pixels to the left,
// above and above left (0 outside the image).  ft: the row's filter type 0..4.
IRE_HD uint32_t unfilter_px(uint32_t ft, uint32_t bpp, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (k >= bpp) break;
        const int xa = (int)(a >> (8 * k) & 255u), xb = (int)(b >> (8 * k) & 255u), xc = (int)(c >> (8 * k) & 255u);
        int pred = 0;
        if (ft == 1) pred = xa;
        else if (ft == 2) pred = xb;
        else if (ft == 3) pred = (xa + xb) >> 1;
        else if (ft == 4) {
            const int pp = xa + xb - xc;
            const int pa = pp > xa ? pp - xa : xa - pp, pb = pp > xb ? pp - xb : xb - pp, pc = pp > xc ? pp - xc : xc - pp;
            pred = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        }
        r |= (((x >> (8 * k)) + (uint32_t)pred) & 255u) << (8 * k);
    }
    return r;
}
// a raw pixel -> R | G << 8 | B << 16: grey replicated, alpha dropped, the palette looked up (what PIL's convert("RGB") gives)
IRE_HD uint32_t rgb_of(uint32_t ctype, uint32_t raw, const uint8_t* pal) {
    if (ctype == 2 || ctype == 6) return raw & 0xFFFFFFu;
    const uint32_t g = raw & 255u;
    if (ctype == 3) return (uint32_t)pal[3 * g] | (uint32_t)pal[3 * g + 1] << 8 | (uint32_t)pal[3 * g + 2] << 16;
    return g | g << 8 | g << 16;
}

}  // namespace pngdec
}  // namespace ire
