// jpeg_dec_core.hpp -- the entropy decoder of a JPEG scan (baseline, and the four scan kinds of a progressive file), written once
// for the device and for the CPU: the records the
// host parser (jpeg_parse.hpp) fills and the kernels (jpeg_dec.hip) read, the two bit readers, the per-symbol step and the
// per-subsequence loop.  Plain C++17, no HIP header: every function is IRE_HD (__host__ __device__ under hipcc, nothing under g++),
// so tests/native/jpeg_dec_sim.cpp runs the very code of the kernels with lanes as a loop, under ASan and UBSan.
//
// The algorithm (Klein & Wiseman 2003; Weissenberger & Schmidt 2018): a Huffman-coded stream re-synchronises by itself, so lanes
// may start decoding at arbitrary bit positions.  A stream (the bytes between two restart markers, byte stuffing removed) is cut
// into subsequences of kSubseqBits bits; kLanes consecutive subsequences are a window.  A lane's state is (bit position, block
// within the MCU, zig-zag position).  In round 0 every lane starts at its own first bit in state (block 0, DC), decodes every
// symbol that BEGINS before its end and records its end state; in every later round lane i restarts from lane i - 1's end state if
// that differs from what it started from.  After round k the first k + 1 lanes are exact, so a loop bounded by kLanes is always
// right and always ends; it stops early when no lane changed.  Then a prefix sum over the lanes' completed-block counts and DC
// sums gives each lane its first block and its DC predictors, and a second pass writes the coefficients.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif

namespace ire {
namespace jpegdec {

constexpr int kLanes = 256;                            // lanes of a window = threads of the workgroup that owns a long stream
constexpr int kSubseqBits = 1024;                      // S: bits per lane and round
constexpr unsigned kWindowBits = (unsigned)kLanes * kSubseqBits;
constexpr unsigned kStageWords = kWindowBits / 32 + 4; // big-endian words staged per window (+ what the last symbol may read ahead)
constexpr unsigned kStagePadded = kStageWords + kStageWords / 32 + 1;      // one pad word per 32: lane i starts at word 33 i (no bank conflict)
constexpr unsigned kShortMaxBytes = 2048;              // a stream of at most this many bytes is decoded by ONE lane, start to end
constexpr unsigned kBadPos = 0xffffffffu;              // the bit position of a state that met an error

// status bits of an image (0 = ok)
constexpr int kStBadCode = 1;                          // a code that no table holds
constexpr int kStBadIndex = 2;                         // a zig-zag index above 63
constexpr int kStBadDc = 4;                            // a DC category above 11
constexpr int kStBadEnd = 8;                           // the stream ended with blocks missing or bytes left over
constexpr int kStBadRange = 16;                        // a dequantised coefficient outside int16, or a sample outside -512..511 before the range limit:
                                                       // no picture gives these, and there libjpeg-turbo's SIMD code (saturating) and its C code (masking) part

// One Huffman table as libjpeg's jdhuff.c decodes it: look[next 9 bits] = length << 8 | symbol for codes of up to 9 bits (0: the
// code is longer), else the first l in 10..16 with code <= maxcode[l] and the symbol vals[valoff[l] + code].
struct DecTable {
    uint16_t look[512];
    int32_t maxcode[18];                               // [l]: the largest code of length l, -1 when there is none
    int32_t valoff[18];                                // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
};
// What the kernels know about one image.  Blocks are counted in SCAN order over the whole image: block g is block g % bpm of MCU
// g / bpm.  Coefficients lie [component][block row][block column][64] (natural order, int16) from coef_off[c] (in blocks).
struct DecImage {
    int32_t h, w, ncomp, sampling;                     // sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, 3 = grey
    uint32_t bpm, mcus_w, mcus_h, nblocks;             // blocks per MCU; MCUs per row / column; nblocks = mcus_w * mcus_h * bpm
    uint8_t comp_of[8], bx[8], by[8];                  // per block of an MCU: its component and its place inside the MCU
    uint8_t hs[4], vs[4], dc_tab[4], ac_tab[4];        // per component: blocks per MCU each way, Huffman table numbers
    uint32_t gridw[4], gridh[4], coef_off[4];          // per component: blocks per row / column of its grid, first block
    uint32_t pw[4], ph[4];                             // per component: the REAL size of its plane in samples
    uint32_t first_long, nlong, first_short, nshort;   // its streams in the batch's stream table: the long ones, then the short ones
    uint16_t quant[4][64];                             // per component, natural order
    // One scan of a progressive file is a record of its own (a "unit"): the frame's geometry, the scan's own MCU (bpm, comp_of, bx,
    // by), its table numbers, and what follows.  A baseline file's one record has all of it 0.
    uint8_t kind, ss, se, al;                          // kScan*; the band in zig-zag positions; the bit position the scan leaves
    uint32_t slot;                                     // the image of the batch whose coefficients and status word this record writes
    uint32_t raster, rw, rh;                           // 1: a scan of ONE component walks the rw x rh blocks of its REAL plane in raster order
    uint32_t walk0;                                    // an AC refinement scan: its first block in the mask and walk-record scratch
};
constexpr int kScanBaseline = 0, kScanDcFirst = 1, kScanAcFirst = 2, kScanDcRefine = 3, kScanAcRefine = 4;
struct DecStream {
    uint32_t off, len;                                 // its bytes (stuffing removed) in the batch's byte area; off is a multiple of 4
    uint32_t mcu0, nmcu;                               // its first MCU and its MCU count
};

struct DecState { uint32_t p, blk, k; };               // bit position | block within the MCU | zig-zag position (0: a DC symbol is next)
struct LaneOut { uint32_t nblk; uint32_t dc[3]; };     // blocks completed and, per component, the sum of the DC differences decoded

IRE_HD uint32_t natural_of(uint32_t k) {               // zig-zag position -> natural (row-major) index
    constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63u];
}

// ---- bit readers: peek(p) = the 32 bits from bit p on, MSB first; past the stream's end every bit is 1, as libjpeg pads ----------
// big-endian word k of a stream (bytes 4 k .. 4 k + 3, clamped to the stream's length); `b` is 4-byte aligned
IRE_HD uint32_t stream_word(const uint8_t* b, uint32_t len, uint32_t k) {
    const uint64_t i = 4ull * k;
    if (i + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(b + i));
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; ++j) v = (v << 8) | (i + j < len ? b[i + j] : 0xffu);
    return v;
}
// over a window staged by stream_word into padded words (kernel: LDS); bit0 = the first staged bit, a multiple of 32
struct WordReader {
    const uint32_t* w;
    uint32_t bit0;
    IRE_HD uint32_t peek(uint32_t p) const {
        const uint32_t i = (p - bit0) >> 5, j = i + 1, s = p & 31u;
        const uint32_t hi = w[i + (i >> 5)], lo = w[j + (j >> 5)];
        return s ? (hi << s) | (lo >> (32u - s)) : hi;
    }
};
// over the stream's bytes where they lie, every read clamped to its length
struct ByteReader {
    const uint8_t* b;
    uint32_t len;
    IRE_HD uint32_t peek(uint32_t p) const {
        const uint32_t i = p >> 3;
        uint64_t v = 0;
        for (uint32_t j = 0; j < 5; ++j) v = (v << 8) | (i + j < len ? b[i + j] : 0xffu);
        return (uint32_t)(v >> (8u - (p & 7u)));
    }
};

// jdhuff's HUFF_EXTEND: the s (0..15) bits behind the first nb (<= 16) bits of w as a signed value.  nb + s <= 31: the peek that
// gave the code gives the value too
IRE_HD int extend_from(uint32_t w, uint32_t nb, uint32_t s) {
    if (s == 0) return 0;
    const int v = (int)((w << nb) >> (32u - s));
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// where block g (scan order) of the image lies in the coefficient scratch, in int16 units
IRE_HD uint32_t block_base(const DecImage& im, uint32_t g) {
    if (im.raster) {
        const uint32_t c = im.comp_of[0] & 3u, y = g / im.rw, x = g - y * im.rw;
        return (im.coef_off[c] + y * im.gridw[c] + x) * 64u;
    }
    const uint32_t mcu = g / im.bpm, j = g - mcu * im.bpm, c = im.comp_of[j];
    const uint32_t my = mcu / im.mcus_w, mx = mcu - my * im.mcus_w;
    return (im.coef_off[c] + (my * im.vs[c] + im.by[j]) * im.gridw[c] + mx * im.hs[c] + im.bx[j]) * 64u;
}

// ---- the per-symbol step.  -> kind | kBlockDone; the value and its zig-zag position for kSymDc / kSymAc; st advanced.
// soft: the synchronising rounds, where a lane that started at a wrong place reads nonsense.  There nothing is an error (an error
// would stop the lane, and a stopped lane hands nothing on, so the lanes behind it could only settle one per round): an unknown code
// costs one bit, a run past position 63 ends the block as it does in libjpeg.  A lane that started at the right place of a
// well-formed stream never takes these branches, so its states are those of the strict step. -----------------------------------------
constexpr int kSymNone = 0, kSymDc = 1, kSymAc = 2, kSymErr = 3, kBlockDone = 4;
// t: the table of this symbol (the block's DC table when st.k == 0, else its AC table); bpm: blocks per MCU
// The first scans of a progressive file take the same step (T.81 G.1.2).  A DC first scan: the block ends behind its DC symbol.  An
// AC first scan: positions ss..se (st.k == 0 stands for ss: every block begins so, in every kind); EOBn ends this block and the next
// `run` - 1, all counted at the moment the symbol is read -- the bit position is never inside a run, so the streams synchronise as
// baseline ones do.  run: blocks completed by this step when kBlockDone is set.
template <class R>
IRE_HD int dec_step_scan(const R& rd, const DecTable& t, uint32_t bpm, int skind, uint32_t ss, uint32_t se, DecState& st, bool soft, int& val, uint32_t& pos,
                         uint32_t& err, uint32_t& run) {
    const uint32_t w = rd.peek(st.p);
    run = 1;
    const uint32_t e = t.look[w >> 23];
    uint32_t nb, sym;
    if (e) { nb = e >> 8; sym = e & 255u; }
    else {
        nb = 10;
        while (nb <= 16 && (int32_t)(w >> (32u - nb)) > t.maxcode[nb]) ++nb;
        if (nb > 16) {
            if (soft) { st.p += 1; return kSymNone; }
            err |= kStBadCode; return kSymErr;
        }
        sym = t.vals[(uint32_t)(t.valoff[nb] + (int32_t)(w >> (32u - nb))) & 255u];
    }
    int kind = kSymNone;
    if (st.k == 0 && skind != kScanAcFirst) {
        if (sym > 11) {
            if (!soft) { err |= kStBadDc; return kSymErr; }
            sym &= 15u;
        }
        val = extend_from(w, nb, sym); pos = 0;
        st.p += nb + sym; st.k = skind == kScanDcFirst ? 64u : 1u; kind = kSymDc;
    } else {
        const uint32_t r = sym >> 4, s = sym & 15u;
        if (st.k == 0) st.k = ss;
        st.p += nb + s;
        if (s == 0) {
            if (r == 15) { st.k += 16; if (st.k > se && !soft) { err |= kStBadIndex; return kSymErr; } }      // ZRL: a coefficient must follow
            else {                                                                                   // end of block, or of `run` blocks
                if (skind == kScanAcFirst && r) { run = (1u << r) + ((w << nb) >> (32u - r)); st.p += r; }
                st.k = 64;
            }
        } else {
            st.k += r;
            if (st.k > se && !soft) { err |= kStBadIndex; return kSymErr; }
            val = extend_from(w, nb, s); pos = st.k & 63u;
            st.k += 1; kind = kSymAc;
        }
        if (st.k > se) st.k = 64;
    }
    if (st.k >= 64) { st.k = 0; st.blk = st.blk + 1 >= bpm ? 0 : st.blk + 1; kind |= kBlockDone; }
    return kind;
}
template <class R>
IRE_HD int dec_step(const R& rd, const DecTable& t, uint32_t bpm, DecState& st, bool soft, int& val, uint32_t& pos, uint32_t& err) {
    uint32_t run;
    return dec_step_scan(rd, t, bpm, kScanBaseline, 0u, 63u, st, soft, val, pos, err, run);
}

// ---- the per-subsequence loop: every symbol that begins before bit `lim`, at most max_blocks completed blocks.  coef == null:
// count only, with the soft step (the synchronising rounds).  Else block `gblk` (scan order in the image) is the one open at st, dcpred
// (4 words) holds the running DC per component, and the coefficients are written.  -> error bits; on an error st.p = kBadPos.  Ends
// after at most lim - st.p steps: every step consumes at least one bit.  What a block needs of the image record (its component, its
// two tables) is read once per block, and the DC sums are updated by selects, not by indexing: they stay in registers. ---------------
template <class R>
IRE_HD uint32_t dec_subseq(const R& rd, const DecTable* tabs, const DecImage& im, DecState& st, uint32_t lim, uint32_t max_blocks, int16_t* coef, uint32_t gblk,
                           uint32_t* dcpred, LaneOut& o) {
    o.nblk = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
    uint32_t err = 0;
    const uint32_t bpm = im.bpm, ss = im.kind == kScanAcFirst ? im.ss : 1u, se = im.kind == kScanAcFirst ? im.se : 63u, al = im.al;
    const int skind = im.kind;
    const bool soft = coef == nullptr;
    uint32_t base = coef && max_blocks ? block_base(im, gblk) : 0;
    uint32_t c = im.comp_of[st.blk & 7u] & 3u;
    const DecTable *tdc = tabs + (im.dc_tab[c] & 3u), *tac = tabs + 4u + (im.ac_tab[c] & 3u);
    while (st.p < lim && o.nblk < max_blocks) {
        int val = 0;
        uint32_t pos = 0;
        uint32_t run;
        const int r = dec_step_scan(rd, st.k == 0 && skind != kScanAcFirst ? *tdc : *tac, bpm, skind, ss, se, st, soft, val, pos, err, run);
        if ((r & 3) == kSymErr) { st.p = kBadPos; break; }
        if (run > max_blocks - o.nblk) { err |= kStBadEnd; st.p = kBadPos; break; }          // an EOB run that overshoots the stream's blocks
        if ((r & 3) == kSymDc) {
            const uint32_t v = (uint32_t)val;
            o.dc[0] += c == 0 ? v : 0u; o.dc[1] += c == 1 ? v : 0u; o.dc[2] += c == 2 ? v : 0u;
            if (coef) {
                dcpred[0] += c == 0 ? v : 0u; dcpred[1] += c == 1 ? v : 0u; dcpred[2] += c == 2 ? v : 0u;
                coef[base] = (int16_t)((c == 0 ? dcpred[0] : c == 1 ? dcpred[1] : dcpred[2]) << al);
            }
        } else if ((r & 3) == kSymAc && coef) coef[base + natural_of(pos)] = (int16_t)((uint32_t)val << al);
        if (r & kBlockDone) {
            o.nblk += run; gblk += run;
            if (coef && o.nblk < max_blocks) base = block_base(im, gblk);
            c = im.comp_of[st.blk & 7u] & 3u;
            tdc = tabs + (im.dc_tab[c] & 3u); tac = tabs + 4u + (im.ac_tab[c] & 3u);
        }
    }
    return err;
}

// what must hold when a stream's last block is done at bit p: its last byte has begun (the rest of it is padding)
IRE_HD bool stream_end_ok(uint32_t p, uint32_t len) { return p != kBadPos && p <= 8u * len && 8u * len - p < 8u; }

// ---- the refinement scans of a progressive file (T.81 G.1.2.3; libjpeg's jdphuff.c) ----------------------------------------------------
// A DC refinement scan has no code at all: bit n of a stream is block n of that stream, OR-ed into coefficient 0 at bit al.
//
// An AC refinement scan: behind every symbol the decoder walks the band and reads one correction bit for each coefficient that was
// non-zero BEFORE this scan (one placed in this scan is never met again in it), so the bits a block takes depend on the blocks in
// front of it and no lane can guess a position.  But they depend on the non-zero PATTERN alone.  So: a mask per block (64 bits in
// zig-zag order, limited to the band: jpeg_dec_mask_kernel); a serial walk per stream over symbols and masks that touches no
// coefficient and records where each block's bits begin (refine_walk_stream); then every block by itself (refine_apply_block).
constexpr uint32_t kRecInRun = 0x80000000u;            // a walk record: the block lies inside an EOB run (bits 0..30: its first bit; kBadPos: none)
struct RefState { uint32_t p, eobrun, k; };            // bit position | blocks the current EOB run still covers | zig-zag position (0: a block begins)

IRE_HD uint64_t band_bits(uint32_t ss, uint32_t se) { return (~0ull << (ss & 63u)) & (~0ull >> (63u - (se & 63u))); }
IRE_HD uint32_t popc64(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
IRE_HD uint32_t ctz64(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }

// the code at the front of w -> its length and symbol; false: no table holds it
IRE_HD bool huff_symbol(const DecTable& t, uint32_t w, uint32_t& nb, uint32_t& sym) {
    const uint32_t e = t.look[w >> 23];
    if (e) { nb = e >> 8; sym = e & 255u; return true; }
    nb = 10;
    while (nb <= 16 && (int32_t)(w >> (32u - nb)) > t.maxcode[nb]) ++nb;
    if (nb > 16) return false;
    sym = t.vals[(uint32_t)(t.valoff[nb] + (int32_t)(w >> (32u - nb))) & 255u];
    return true;
}
// behind a symbol (r, s) read at position k: the (r + 1)-th coefficient at or behind k that is still zero -- where s is placed, or
// the last of the 16 a ZRL skips.  64: the band ends first
IRE_HD uint32_t refine_target(uint64_t mask, uint64_t band, uint32_t k, uint32_t r) {
    uint64_t z = ~mask & band & (~0ull << k);
    for (uint32_t i = 0; i < r; ++i) z &= z - 1;
    return z ? ctz64(z) : 64u;
}

// One step of the walk: a whole block inside an EOB run, or one symbol and what follows it.  done: the block ended.  -> error bits.
// Reads the 32 bits at st.p and no others (the correction bits are only counted).
template <class R>
IRE_HD uint32_t refine_walk_step(const R& rd, const DecTable& t, uint32_t ss, uint32_t se, uint64_t mask, RefState& st, bool& done) {
    done = true;
    if (st.k == 0 && st.eobrun) { st.p += popc64(mask); --st.eobrun; return 0; }
    const uint32_t k = st.k ? st.k : ss;
    const uint32_t w = rd.peek(st.p);
    uint32_t nb, sym;
    if (!huff_symbol(t, w, nb, sym)) return kStBadCode;
    const uint32_t r = sym >> 4, s = sym & 15u;
    st.p += nb;
    st.k = 0;
    if (s) {
        if (s != 1) return kStBadCode;                              // (libjpeg warns and goes on; here the image is flagged)
        st.p += 1;                                                  // the sign
    } else if (r != 15) {                                           // EOBr: the rest of this block, and run - 1 blocks behind it
        uint32_t run = 1u << r;
        if (r) { run += (w << nb) >> (32u - r); st.p += r; }
        st.eobrun = run - 1;
        st.p += popc64(mask & (~0ull << k));
        return 0;
    }
    const uint32_t k2 = refine_target(mask, band_bits(ss, se), k, r);
    if (k2 > se) return kStBadIndex;                                // the run leaves the band
    st.p += popc64(mask & (~0ull << k) & ~(~0ull << k2));
    if (k2 < se) { st.k = k2 + 1; done = false; }
    return 0;
}

// The walk over blocks n .. nend - 1 of a stream while the 32 bits at st.p lie below bit `lim` (what the caller staged; 0xffffffff:
// all of it): masks[j] and recs[j] belong to block first + j.  A block's record is written when it begins.  -> error bits; n, st
// advanced.  total_bits < 2^31: a position beyond the stream's end is an error, so a record never reaches kBadPos.
template <class R>
IRE_HD uint32_t refine_walk_some(const R& rd, const DecTable& t, uint32_t ss, uint32_t se, const uint64_t* masks, uint32_t* recs, uint32_t first, uint32_t nend,
                                 uint32_t lim, uint32_t total_bits, RefState& st, uint32_t& n) {
    while (n < nend && (lim == 0xffffffffu || st.p + 32u <= lim)) {
        if (st.k == 0) recs[n - first] = st.p | (st.eobrun ? kRecInRun : 0u);
        bool done;
        const uint32_t err = refine_walk_step(rd, t, ss, se, masks[n - first], st, done);
        if (err) return err;
        if (st.p > total_bits) return kStBadEnd;
        if (done) ++n;
    }
    return 0;
}
// what must hold behind a stream's last block
IRE_HD uint32_t refine_walk_end(const RefState& st, uint32_t len) { return st.eobrun || !stream_end_ok(st.p, len) ? (uint32_t)kStBadEnd : 0u; }      // (an EOB run that overshoots the stream's blocks)

// a whole stream of nblk blocks by one lane: masks[n] -> recs[n].  -> error bits; behind an error every record is kBadPos.
template <class R>
IRE_HD uint32_t refine_walk_stream(const R& rd, const DecTable& t, uint32_t ss, uint32_t se, const uint64_t* masks, uint32_t* recs, uint32_t nblk, uint32_t len) {
    RefState st{0, 0, 0};
    uint32_t n = 0;
    uint32_t err = refine_walk_some(rd, t, ss, se, masks, recs, 0, nblk, 0xffffffffu, 8u * len, st, n);
    if (err) for (uint32_t j = n + 1; j < nblk; ++j) recs[j] = kBadPos;
    return err ? err : refine_walk_end(st, len);
}
// The same by a wave (jpeg_dec_walk_long_kernel; tests/native/jpeg_prog_sim.cpp as a loop): the walking lane must not wait for a load
// per block or per symbol, so the other lanes stage kWalkBlocks masks and kWalkWords stream words (WordReader's layout) in front of it,
// and the records leave kWalkBlocks at a time.
constexpr unsigned kWalkBlocks = 64;
constexpr unsigned kWalkWords = 256;                   // staged per turn: the walk stops when fewer than 32 bits of them are left
constexpr unsigned kWalkStageWords = kWalkWords + 1;   // (+ WordReader's second word)
constexpr unsigned kWalkStagePadded = kWalkStageWords + kWalkStageWords / 32 + 1;

// the correction bits from bit p on for the coefficients of m (zig-zag bits, all non-zero before this scan) -> the bit behind them
template <class R>
IRE_HD uint32_t refine_correct(const R& rd, uint64_t m, uint32_t p, int p1, int16_t* blk) {
    while (m) {
        const uint32_t k = ctz64(m);
        m &= m - 1;
        if (rd.peek(p) >> 31) {
            int16_t& c = blk[natural_of(k)];
            if (!(c & p1)) c = (int16_t)(c >= 0 ? c + p1 : c - p1);
        }
        ++p;
    }
    return p;
}
// one block from its walk record: its symbols again, the corrections applied, the new coefficients placed.  blk: its 64 coefficients.
// The walk met every error this could meet and turned the record into kBadPos, so a code it cannot read only ends the block.
template <class R>
IRE_HD void refine_apply_block(const R& rd, const DecTable& t, uint32_t ss, uint32_t se, uint32_t al, uint64_t mask, uint32_t rec, int16_t* blk) {
    if (rec == kBadPos) return;
    const int p1 = 1 << al;
    uint32_t p = rec & ~kRecInRun;
    if (rec & kRecInRun) { refine_correct(rd, mask, p, p1, blk); return; }
    const uint64_t band = band_bits(ss, se);
    uint32_t k = ss;
    while (k <= se) {
        const uint32_t w = rd.peek(p);
        uint32_t nb, sym;
        if (!huff_symbol(t, w, nb, sym)) return;
        const uint32_t r = sym >> 4, s = sym & 15u;
        p += nb;
        int v = 0;
        if (s) { v = (rd.peek(p) >> 31) ? p1 : -p1; p += 1; }
        else if (r != 15) { refine_correct(rd, mask & (~0ull << k), p + r, p1, blk); return; }
        const uint32_t k2 = refine_target(mask, band, k, r);
        if (k2 > se) return;
        p = refine_correct(rd, mask & (~0ull << k) & ~(~0ull << k2), p, p1, blk);
        if (s) blk[natural_of(k2)] = (int16_t)v;
        k = k2 + 1;
    }
}

// ---- long streams of several windows, decoded window-parallel in three passes (jpeg_dec.hip: spec / chain / write kernels) ------------
// The only serial link between two windows of a stream is the state at which the second one is entered.  Pass A guesses it -- every
// window's lane 0 starts like any other lane, at its own first bit in state (block 0, DC) -- and settles each window by itself, all
// windows at once; it keeps every lane's start state, end state and counts in a LaneRec.  Pass B walks one stream's windows in order
// with the TRUE entry state: from lane 0 on it decodes a lane again from the end of the lane before until an entry state equals the
// start a lane was settled from -- from there on pass A's records are exact, because a lane's record is a function of its start state
// alone.  A guess that never locks costs a window's kLanes decodes one after the other, never a wrong result.  B also gives every
// window the block count and the DC sums in front of it (WinHead).  Pass C writes every window's coefficients, all windows at once.
struct DecWindow { uint32_t stream, image, win0; };   // a window of a multi-window stream: its stream and image in the batch, its first bit
struct DecChain { uint32_t stream, image, first, nwin; };      // a multi-window stream: its windows are first .. first + nwin - 1 of the window table
struct LaneRec { uint32_t sp, sbk, ep, ebk; LaneOut o; };      // a lane's settled start and end state (bit position; block << 8 | zig-zag position), its counts
struct WinHead { uint32_t done, dc[3]; };                      // in front of a window: completed blocks of its stream, DC sums per component
static_assert(sizeof(LaneRec) == 32 && sizeof(WinHead) == 16 && sizeof(DecWindow) == 12 && sizeof(DecChain) == 16, "as the host lays them out");
constexpr unsigned kChainStageWords = kSubseqBits / 32 + 2;    // what one lane's decode may read: its subsequence and the last symbol's read-ahead
constexpr unsigned kChainStagePadded = kChainStageWords + kChainStageWords / 32 + 1;

IRE_HD uint32_t state_bk(const DecState& s) { return s.blk << 8 | s.k; }
IRE_HD DecState state_of(uint32_t p, uint32_t bk) { return DecState{p, bk >> 8, bk & 255u}; }
// windows of a stream of `len` bytes (len < 2^28: jpeg_parse.hpp refuses larger files)
// Blocks of one image's coefficient scratch at most, whatever its sampling: three components on the 4:2:0 luma grid.  THE extent of
// jpeg_dec.hip's scratch per image (jpeg_dec_blocks) and of what jpeg_dec_launch clears in front of every batch; tests/native's simulators
// take it from here.
inline size_t coef_blocks(int h, int w) { return (size_t)3 * (2 * (((size_t)w + 15) / 16)) * (2 * (((size_t)h + 15) / 16)); }

IRE_HD uint32_t window_count(uint32_t len) { return (8u * len + kWindowBits - 1) / kWindowBits; }
// the lanes of the window at bit win0 whose subsequence begins inside the stream, and the bit behind lane t's subsequence
IRE_HD uint32_t window_lanes(uint32_t total_bits, uint32_t win0) {
    const uint32_t left = (total_bits - win0 + kSubseqBits - 1) / kSubseqBits;
    return left < (uint32_t)kLanes ? left : (uint32_t)kLanes;
}
IRE_HD uint32_t lane_lim(uint32_t total_bits, uint32_t win0, uint32_t t) {
    const uint32_t e = win0 + (t + 1) * kSubseqBits;
    return e < total_bits ? e : total_bits;
}
// pass A: where lane t of the window at bit win0 starts: only the stream's very first lane knows its state, every other start is a
// guess that pass B checks (any state would do: the result does not depend on it)
IRE_HD DecState spec_start(uint32_t win0, uint32_t t) { return DecState{win0 + t * kSubseqBits, 0, 0}; }
// pass B, one lane: `in` is the true state in front of lane t.  true: the lane was settled from exactly that state, so its record and
// all behind it in the window stand.  false: the lane was decoded again (soft, counting only) into its record, and `in` is its end.
// rd must hold the bits from in.p up to `lim` and one symbol's read-ahead
template <class R>
IRE_HD bool chain_lane(const R& rd, const DecTable* tabs, const DecImage& im, uint32_t lim, LaneRec& r, DecState& in) {
    if (r.sp == in.p && r.sbk == state_bk(in)) return true;
    DecState end = in;
    LaneOut lo;
    dec_subseq(rd, tabs, im, end, lim, 0xffffffffu, (int16_t*)nullptr, 0, nullptr, lo);
    r = LaneRec{in.p, state_bk(in), end.p, state_bk(end), lo};
    in = end;
    return false;
}

}  // namespace jpegdec
}  // namespace ire
