// jpeg_progenc_core.hpp -- the entropy coder of a PROGRESSIVE JPEG result (libjpeg's jcphuff.c under jpeg_simple_progression), written
// once for the device and for the CPU: plain C++17, no HIP header, every function IRE_HD, so tests/native/jpeg_progenc_sim.cpp runs
// the very code of jpeg_progenc.hip's count and emit kernels under ASan and UBSan.  tests/jpeg_progenc_model.py restates it and
// equals libjpeg-turbo's file byte for byte.
//
// The file sends one image's quantised coefficients as ten scans (kScans below), each under its own optimal Huffman table, with a
// restart interval of one block row (MCU row) of the scan.  An interval's bits depend on its own blocks alone -- the DC predictors,
// the end-of-band run EOBRUN and the buffered correction bits all restart with it -- so the INTERVAL is the parallel unit, and inside
// it the blocks are walked in order with the state that crosses them (Coder).  walk_interval is that walk; what it produces goes to
// a sink: sym(table slot, symbol) and bits(value, count).  The count pass's sink adds to histograms, the emit pass's packs bits
// MSB-first with byte stuffing (ByteSink).  The same walk under both is what makes the tables fit the symbols.
//
// Coefficient layout (Geom): per image [blocks][64] int16 in zig-zag order, component after component, blocks in raster order.
// 4:4:4: ceil(h/8) x ceil(w/8) blocks per component.  4:2:0: Y on the MCU grid (2 ceil(h/16) x 2 ceil(w/16), dummy blocks included:
// the interleaved DC scans send them), Cb and Cr ceil(h/16) x ceil(w/16); an AC scan of Y walks Y's own ceil(h/8) x ceil(w/8) only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif

namespace ire {
namespace jpegprog {

constexpr int kScans = 10, kTables = 10;
constexpr unsigned kMaxCorrBits = 1000;                 // libjpeg's MAX_CORR_BITS
constexpr unsigned kCorrWords = (kMaxCorrBits + 31) / 32;
constexpr unsigned kFixedHead = 2 + 18 + 69 + 69 + 19;  // SOI APP0 DQT DQT SOF2

struct Scan { uint8_t ncomp, comp, ss, se, ah, al; };
// jpeg_simple_progression for Y Cb Cr (component 0, 1, 2)
IRE_HD Scan scan_of(int s) {
    switch (s) {
        case 0: return Scan{3, 0, 0, 0, 0, 1};
        case 1: return Scan{1, 0, 1, 5, 0, 2};
        case 2: return Scan{1, 2, 1, 63, 0, 1};
        case 3: return Scan{1, 1, 1, 63, 0, 1};
        case 4: return Scan{1, 0, 6, 63, 0, 2};
        case 5: return Scan{1, 0, 1, 63, 2, 1};
        case 6: return Scan{3, 0, 0, 0, 1, 0};
        case 7: return Scan{1, 2, 1, 63, 1, 0};
        case 8: return Scan{1, 1, 1, 63, 1, 0};
        default: return Scan{1, 0, 1, 63, 1, 0};
    }
}
// the ten tables in file order: the scan that defines a table and its DHT class-and-id byte; scan 0 has two, scan 6 none
IRE_HD int table_scan(int t) { return t < 2 ? 0 : t < 7 ? t - 1 : t; }
IRE_HD int table_id(int t) { return t == 0 ? 0x00 : t == 1 ? 0x01 : (t == 2 || t == 5 || t == 6 || t == 9) ? 0x10 : 0x11; }
IRE_HD int first_table(int scan) { return scan == 0 ? 0 : scan < 6 ? scan + 1 : scan; }
IRE_HD int table_count(int scan) { return scan == 0 ? 2 : scan == 6 ? 0 : 1; }
IRE_HD int table_slot(int scan, int comp) { return scan == 0 ? (comp ? 1 : 0) : first_table(scan); }

struct Geom {
    int h, w, sampling;
    unsigned rows[3], cols[3];          // the stored grid of a component, in blocks
    unsigned orows[3], ocols[3];        // its own blocks: what a non-interleaved scan walks
    unsigned off[3], nblocks;           // the component's first block; blocks per image
    unsigned mh, mw;                    // the MCU grid
    unsigned int0[kScans + 1];          // the scan's first interval; [kScans]: intervals per image
};
// Y's value or the chroma components' (Cb and Cr have one grid) by arithmetic: a component-indexed array read, or a select between
// two of its entries, makes the device compiler keep the array in private memory
IRE_HD unsigned y_or_c(unsigned y, unsigned c, int comp) { return c + (y - c) * (unsigned)(comp == 0); }
IRE_HD unsigned comp_off(const Geom& g, int comp) { return (unsigned)(comp != 0) * (g.off[1] + (unsigned)(comp == 2) * (g.off[2] - g.off[1])); }
IRE_HD unsigned scan_rows(const Geom& g, int scan) { const Scan sc = scan_of(scan); return sc.ncomp == 3 ? g.mh : y_or_c(g.orows[0], g.orows[1], sc.comp); }
// the scan's restart interval: its MCUs per MCU row
IRE_HD unsigned scan_interval(const Geom& g, int scan) { const Scan sc = scan_of(scan); return sc.ncomp == 3 ? g.mw : y_or_c(g.ocols[0], g.ocols[1], sc.comp); }
IRE_HD unsigned scan_row_blocks(const Geom& g, int scan) { return scan_of(scan).ncomp == 3 ? g.mw * (g.sampling == 2 ? 6u : 3u) : scan_interval(g, scan); }
IRE_HD Geom geom_of(int h, int w, int sampling) {
    Geom g{};
    g.h = h; g.w = w; g.sampling = sampling;
    const unsigned yh = ((unsigned)h + 7) / 8, yw = ((unsigned)w + 7) / 8;
    if (sampling == 2) {
        g.mh = ((unsigned)h + 15) / 16; g.mw = ((unsigned)w + 15) / 16;
        g.rows[0] = 2 * g.mh; g.cols[0] = 2 * g.mw; g.orows[0] = yh; g.ocols[0] = yw;
        for (int c = 1; c < 3; ++c) { g.rows[c] = g.orows[c] = g.mh; g.cols[c] = g.ocols[c] = g.mw; }
    } else {
        g.mh = yh; g.mw = yw;
        for (int c = 0; c < 3; ++c) { g.rows[c] = g.orows[c] = yh; g.cols[c] = g.ocols[c] = yw; }
    }
    g.off[0] = 0; g.off[1] = g.rows[0] * g.cols[0]; g.off[2] = g.off[1] + g.rows[1] * g.cols[1];
    g.nblocks = g.off[2] + g.rows[2] * g.cols[2];
    g.int0[0] = 0;
    for (int s = 0; s < kScans; ++s) g.int0[s + 1] = g.int0[s] + scan_rows(g, s);
    return g;
}
IRE_HD int scan_of_interval(const Geom& g, unsigned iv) { int s = 0; while (s + 1 < kScans && iv >= g.int0[s + 1]) ++s; return s; }

IRE_HD unsigned bit_length(unsigned v) { unsigned n = 0; while (v) { ++n; v >>= 1; } return n; }

// What happened on the way, for the tests: every rule of jcphuff.c that the walk can get wrong counts itself (the CPU program prints
// them; the kernels pass a null pointer).
struct Events { unsigned eobrun_restart, eobrun_block, eobrun_early, zrl_first, zrl_refine, shifted_to_zero, dc_negative; };

// the state that crosses blocks inside an interval.  corr: kCorrWords words, `cstride` words apart (LDS on the device), bit i of the
// buffer at the top of word i / 32 downwards, so that whole words go out at once.
template <typename Sink>
struct Coder {
    Sink& out;
    uint32_t* corr;
    unsigned cstride;
    Events* ev;
    int slot;
    unsigned eobrun, be;
    IRE_HD void corr_push(unsigned bit) {
        if (be >= kMaxCorrBits) return;                                      // (cannot happen: the early flush keeps be <= 937 + 63)
        uint32_t& w = corr[(be >> 5) * cstride];
        const uint32_t m = bit << (31u - (be & 31u));
        w = (be & 31u) ? (w | m) : m;
        ++be;
    }
    IRE_HD void emit_eobrun() {
        if (!eobrun) return;
        const unsigned n = bit_length(eobrun) - 1u;
        out.sym(slot, (int)(n << 4));
        if (n) out.bits(eobrun & ((1u << n) - 1u), n);
        for (unsigned i = 0; i < be; i += 32) {
            const unsigned l = be - i < 32u ? be - i : 32u;
            out.bits(corr[(i >> 5) * cstride] >> (32u - l), l);
        }
        eobrun = 0; be = 0;
    }
};
IRE_HD void put_bits64(uint64_t& br, unsigned& nbr, unsigned bit) { br = (br << 1) | bit; ++nbr; }

template <typename Sink>
IRE_HD void dc_first(Coder<Sink>& c, int& last_dc, const int16_t* blk, int al) {
    const int v = (int)blk[0] >> al;                                         // the point transform: an arithmetic shift of the signed value
    if (c.ev && blk[0] < 0) ++c.ev->dc_negative;
    const int d = v - last_dc;
    last_dc = v;
    const unsigned s = bit_length((unsigned)(d < 0 ? -d : d));
    c.out.sym(c.slot, (int)s);
    if (s) c.out.bits((unsigned)(d < 0 ? d - 1 : d) & ((1u << s) - 1u), s);
}
// Where the band's coefficients are non-zero after the shift (bit k of nz), where they are exactly 1 (one: the newly non-zero ones of
// a refinement scan) and where the shift zeroed a non-zero value (lost: counted for the tests).  64 independent reads and compares:
// the coders then visit the non-zero positions alone, and a run of zeros is a difference of two positions.
IRE_HD unsigned mag_of(const int16_t* blk, int k, int al) { const int v = blk[k]; return (unsigned)(v < 0 ? -v : v) >> al; }
struct Masks { uint64_t nz, one, lost; };
IRE_HD Masks block_masks(const int16_t* blk, const Scan& sc) {
    uint64_t nz = 0, one = 0, lost = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k < 64; ++k) {
        const unsigned a = mag_of(blk, k, sc.al);
        const uint64_t bit = (k >= sc.ss && k <= sc.se) ? 1ull << k : 0ull;
        if (a != 0) nz |= bit;
        if (a == 1) one |= bit;
        if (a == 0 && blk[k] != 0) lost |= bit;
    }
    return Masks{nz, one, lost};
}
IRE_HD int lowest_bit(uint64_t m) { return __builtin_ctzll(m); }             // (m != 0 wherever these two are called)
IRE_HD int highest_bit(uint64_t m) { return 63 - __builtin_clzll(m); }
IRE_HD unsigned popcount64(uint64_t m) { return (unsigned)__builtin_popcountll(m); }
template <typename Sink>
IRE_HD void ac_first(Coder<Sink>& c, const int16_t* blk, const Scan& sc) {
    const Masks mk = block_masks(blk, sc);
    const uint64_t nz = mk.nz;
    if (c.ev) c.ev->shifted_to_zero += popcount64(mk.lost);
    int prev = sc.ss - 1;
    for (uint64_t m = nz; m; m &= m - 1) {
        const int k = lowest_bit(m);
        unsigned r = (unsigned)(k - prev - 1);
        prev = k;
        const int v = blk[k];
        const unsigned a = (unsigned)(v < 0 ? -v : v) >> sc.al;             // the shift is of the magnitude
        if (c.eobrun) { if (c.ev) ++c.ev->eobrun_block; c.emit_eobrun(); }
        while (r > 15) { if (c.ev) ++c.ev->zrl_first; c.out.sym(c.slot, 0xf0); r -= 16; }
        const unsigned s = bit_length(a);
        c.out.sym(c.slot, (int)((r << 4) | s));
        c.out.bits((v < 0 ? ~a : a) & ((1u << s) - 1u), s);
    }
    if (prev < sc.se) ++c.eobrun;                                            // zeros behind the last one (< 0x7FFF: an interval has at most 1024 blocks)
}
// the block's pending correction bits (nbr <= 63 of them, the first at the top) to the sink
template <typename Sink>
IRE_HD void flush_pending(Sink& out, uint64_t& br, unsigned& nbr) {
    if (nbr > 32) { out.bits((uint32_t)(br >> 32) & ((1u << (nbr - 32)) - 1u), nbr - 32); out.bits((uint32_t)br, 32); }
    else if (nbr) out.bits((uint32_t)br & (nbr == 32 ? ~0u : (1u << nbr) - 1u), nbr);
    br = 0; nbr = 0;
}
template <typename Sink>
IRE_HD void ac_refine(Coder<Sink>& c, const int16_t* blk, const Scan& sc) {
    const Masks mk = block_masks(blk, sc);
    const uint64_t nz = mk.nz, one = mk.one;
    const int eob = one ? highest_bit(one) : 0;                              // the last newly non-zero position
    unsigned r = 0, nbr = 0;                                                 // r: the zeros since the last new coefficient or ZRL
    uint64_t br = 0;                                                         // the block's pending correction bits: at most 63
    int prev = sc.ss - 1;
    for (uint64_t m = nz; m; m &= m - 1) {
        const int k = lowest_bit(m);
        r += (unsigned)(k - prev - 1);
        prev = k;
        const unsigned a = mag_of(blk, k, sc.al);
        while (r > 15 && k <= eob) {
            if (c.eobrun) { if (c.ev) ++c.ev->eobrun_block; c.emit_eobrun(); }
            if (c.ev) ++c.ev->zrl_refine;
            c.out.sym(c.slot, 0xf0);
            r -= 16;
            flush_pending(c.out, br, nbr);
        }
        if (a > 1) { put_bits64(br, nbr, a & 1u); continue; }
        if (c.eobrun) { if (c.ev) ++c.ev->eobrun_block; c.emit_eobrun(); }
        c.out.sym(c.slot, (int)((r << 4) | 1u));
        c.out.bits(blk[k] < 0 ? 0u : 1u, 1);
        flush_pending(c.out, br, nbr);
        r = 0;
    }
    r += (unsigned)(sc.se - prev);
    if (r > 0 || nbr > 0) {
        ++c.eobrun;
        for (unsigned i = 0; i < nbr; ++i) c.corr_push((unsigned)(br >> (nbr - 1 - i)) & 1u);
        if (c.be > kMaxCorrBits - 64 + 1) { if (c.ev) ++c.ev->eobrun_early; c.emit_eobrun(); }
    }
}

// One restart interval: block row `row` of scan `scan` of the image whose coefficients start at coefs.  The sink gets everything up
// to the interval's last bit; padding and the marker are the caller's.  stage(p): where the AC coders read the 64 coefficients at p
// from -- p itself on the CPU (DirectBlocks); on the device a copy in the lane's LDS, fetched with eight wide loads, so that a block
// costs one trip to memory and not one per coefficient.
struct DirectBlocks { IRE_HD const int16_t* operator()(const int16_t* p) const { return p; } };
template <typename Sink, typename Stage>
IRE_HD void walk_interval(const Geom& g, int scan, unsigned row, const int16_t* coefs, Sink& out, uint32_t* corr, unsigned cstride, Events* ev, Stage stage) {
    const Scan sc = scan_of(scan);
    Coder<Sink> c{out, corr, cstride, ev, first_table(scan), 0u, 0u};
    if (sc.ncomp == 3) {
        int dc0 = 0, dc1 = 0, dc2 = 0;                                       // the components' last shifted DC: three variables, not an array
        const unsigned per = g.sampling == 2 ? 6u : 3u;
        for (unsigned m = 0; m < g.mw; ++m)
            for (unsigned j = 0; j < per; ++j) {
                int comp; unsigned by, bx;
                if (g.sampling == 2 && j < 4) { comp = 0; by = 2 * row + (j >> 1); bx = 2 * m + (j & 1u); }
                else { comp = g.sampling == 2 ? (int)j - 3 : (int)j; by = row; bx = m; }
                const int16_t* blk = coefs + ((size_t)comp_off(g, comp) + (size_t)by * y_or_c(g.cols[0], g.cols[1], comp) + bx) * 64;
                if (sc.ah == 0) {
                    c.slot = table_slot(scan, comp);
                    if (comp == 0) dc_first(c, dc0, blk, sc.al); else if (comp == 1) dc_first(c, dc1, blk, sc.al); else dc_first(c, dc2, blk, sc.al);
                }
                else out.bits((unsigned)((int)blk[0] >> sc.al) & 1u, 1);
            }
        return;
    }
    const unsigned nb = y_or_c(g.ocols[0], g.ocols[1], sc.comp);
    const int16_t* const row0 = coefs + ((size_t)comp_off(g, sc.comp) + (size_t)row * y_or_c(g.cols[0], g.cols[1], sc.comp)) * 64;
    for (unsigned b = 0; b < nb; ++b) {
        const int16_t* blk = stage(row0 + (size_t)b * 64);
        if (sc.ah == 0) ac_first(c, blk, sc); else ac_refine(c, blk, sc);
    }
    if (c.eobrun) { if (ev) ++ev->eobrun_restart; c.emit_eobrun(); }
}

template <typename Sink>
IRE_HD void walk_interval(const Geom& g, int scan, unsigned row, const int16_t* coefs, Sink& out, uint32_t* corr, unsigned cstride, Events* ev) {
    walk_interval(g, scan, row, coefs, out, corr, cstride, ev, DirectBlocks{});
}

// the emit pass's sink: MSB-first bits into bytes with stuffing.  The bytes are gathered in a word and stored eight at a time (p is
// 8-byte aligned and cap a multiple of 8; little-endian): nothing is written at or beyond cap.  n counts every byte, stored or not.
typedef uint64_t __attribute__((may_alias)) Word8;
struct ByteSink {
    uint8_t* p;
    unsigned n, cap;
    const uint32_t* codes;              // [tables][256] from table slot0 on: value | length << 16
    int slot0;
    uint64_t acc;
    unsigned nacc;
    uint64_t word;                      // bytes n & ~7 .. n - 1
    IRE_HD void store8(unsigned off) { if (off + 8u <= cap) *reinterpret_cast<Word8*>(p + off) = word; }
    IRE_HD void put(unsigned b) {
        word |= (uint64_t)b << (8u * (n & 7u));
        ++n;
        if ((n & 7u) == 0) { store8(n - 8u); word = 0; }
    }
    IRE_HD void bits(uint32_t v, unsigned l) {                               // l in 0..32, v < 2^l; nacc < 8 on entry
        acc = (acc << l) | v; nacc += l;
        while (nacc >= 8) { const unsigned b = (unsigned)(acc >> (nacc - 8)) & 0xffu; put(b); if (b == 0xffu) put(0); nacc -= 8; }
    }
    IRE_HD void sym(int slot, int s) { const uint32_t c = codes[(slot - slot0) * 256 + s]; bits(c & 0xffffu, c >> 16); }
    IRE_HD void finish(int marker) {                                         // pad with 1-bits; marker: 0xD0..0xD7, or 0 for none
        if (nacc) bits((1u << (8 - nacc)) - 1u, 8 - nacc);
        if (marker) { put(0xff); put((unsigned)marker); }
        if (n & 7u) store8(n & ~7u);
    }
};

// ---- the head pieces -------------------------------------------------------------------------------------------------------------------
// In front of scan s: the DHT segments of its tables, a DRI where the interval differs from the scan's before, the SOS.
IRE_HD bool scan_has_dri(const Geom& g, int scan) { return scan == 0 || scan_interval(g, scan) != scan_interval(g, scan - 1); }
IRE_HD unsigned sos_bytes(int scan) { return 2u + 2u + 1u + 2u * scan_of(scan).ncomp + 3u; }
IRE_HD unsigned scan_head_bytes(const Geom& g, int scan, const int32_t* nvals) {
    unsigned n = (scan_has_dri(g, scan) ? 6u : 0u) + sos_bytes(scan);
    for (int t = first_table(scan); t < first_table(scan) + table_count(scan); ++t) n += 5u + 16u + (unsigned)nvals[t];
    return n;
}
// byte k (< scan_head_bytes) of it; bits_vals[kTables][16 + 256]
IRE_HD uint8_t scan_head_byte(const Geom& g, int scan, unsigned k, const uint8_t* bits_vals, const int32_t* nvals) {
    for (int t = first_table(scan); t < first_table(scan) + table_count(scan); ++t) {
        const unsigned nv = (unsigned)nvals[t], seg = 5u + 16u + nv;
        if (k < seg) {
            if (k == 0) return 0xff;
            if (k == 1) return 0xc4;
            if (k == 2) return (uint8_t)((3u + 16u + nv) >> 8);
            if (k == 3) return (uint8_t)((3u + 16u + nv) & 0xffu);
            if (k == 4) return (uint8_t)table_id(t);
            return bits_vals[t * (16 + 256) + (k - 5u)];
        }
        k -= seg;
    }
    if (scan_has_dri(g, scan)) {
        const unsigned ri = scan_interval(g, scan);
        if (k < 6u) { const uint8_t d[6] = {0xff, 0xdd, 0, 4, (uint8_t)(ri >> 8), (uint8_t)(ri & 0xffu)}; return d[k]; }
        k -= 6u;
    }
    const Scan sc = scan_of(scan);
    const unsigned len = 2u + 1u + 2u * sc.ncomp + 3u;
    if (k == 0) return 0xff;
    if (k == 1) return 0xda;
    if (k == 2) return 0;
    if (k == 3) return (uint8_t)len;
    if (k == 4) return sc.ncomp;
    k -= 5u;
    if (k < 2u * sc.ncomp) {                                                 // (jcmarker.c: a progressive scan names only the table it uses)
        const unsigned comp = sc.ncomp == 3 ? k / 2u : sc.comp, t = comp ? 1u : 0u;
        if ((k & 1u) == 0) return (uint8_t)(comp + 1u);
        return (uint8_t)(sc.ss == 0 ? (sc.ah ? 0u : t << 4) : t);
    }
    k -= 2u * sc.ncomp;
    return k == 0 ? sc.ss : k == 1 ? sc.se : (uint8_t)((sc.ah << 4) | sc.al);
}

}  // namespace jpegprog
}  // namespace ire
