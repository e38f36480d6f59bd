// jpeg_huff_core.hpp -- an image's own Huffman tables from its symbol counts (libjpeg's jpeg_gen_optimal_table, jchuff.c), and the
// file's head with those tables in it, written once for the device and for the CPU: plain C++17, no HIP header, every function
// IRE_HD, so tests/native/jpeg_huffopt_dump.cpp runs the very code of jpeg.hip's table and gather kernels with the lanes as a loop,
// under ASan and UBSan (as jpeg_dec_core.hpp does for the decoder).
//
// One WAVE builds one table.  The 257 entries (256 symbols and libjpeg's pseudo-symbol 256 with count 1, which keeps the all-ones
// code free) are dealt to the 64 lanes, entry i to lane i % 64, five places per lane.  libjpeg merges, up to 256 times, the two
// entries with the smallest non-zero counts -- among equal counts the LARGEST index, as its `<=` scan upward finds it -- and adds 1 to
// the code size of every symbol of both trees, which it finds by walking a linked list (others[]).  Here an entry carries the index
// of its tree's representative instead (root[]: libjpeg's c1 stays the representative of the merged tree), so "every symbol of both
// trees" is a test each lane makes on its own five entries: the same increments, no serial walk, and no lane ever reads another
// lane's entries -- so through the merges a lane's entries are its own variables (Wave::Own: registers on the device, a row per lane
// on the CPU), and shared memory comes in only when the code sizes are counted.  The two smallest of the wave come from one pass:
// every lane keeps its own two smallest as keys (count << 9 | 511 - index: the smaller key is the smaller count, then the larger
// index), a wave-wide minimum gives the first, a second minimum over (own first if it is not the winner, else own second) gives
// the other.  Counts are 64-bit, so no sum of 257 32-bit counts wraps: the tree is always a full binary tree, the lengths satisfy
// Kraft's equality, and libjpeg's length-limiting loop (one lane; it moves a pair of the longest codes up and splits a shorter one)
// always finds the shorter code it looks for.
// The length arrays hold any depth up to 256 (libjpeg's own end at 32, where it aborts) and the loop starts at the longest length
// present: the result is libjpeg's wherever libjpeg gives one, and no input can index out of bounds.  (libjpeg never picks an entry
// whose count exceeds 10^9; an image of 8192 x 8192 has at most 2 * 10^8 symbols per table, so that rule is not restated.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif

namespace ire {
namespace jpeghuff {

constexpr int kLanes = 64;
constexpr int kPerLane = 5;                             // entry i = lane + 64 j; 320 places for 257 entries
constexpr int kPlaces = kLanes * kPerLane;
constexpr int kMaxLen = 256;                            // no code of 257 entries is longer
constexpr int kBitsVals = 16 + 256;                     // a table as the DHT segment carries it: BITS, then HUFFVAL (zero beyond nvals)
constexpr uint64_t kNone = ~0ull;
static_assert(kPlaces >= 257, "every entry has a place");

// the wave's shared memory (LDS on the device)
struct Work {
    int32_t bits[kMaxLen + 4];                          // [l]: codes of length l
    uint16_t codesize[kPlaces];                         // per entry, once the merges are done
};
// a lane's own entries through the merges: place j is entry lane + 64 j
struct Entries {
    uint64_t freq[kPerLane];
    uint64_t k1, k2;                                    // the lane's two smallest keys of the current merge
    uint32_t codesize[kPerLane], root[kPerLane];
};

// The wave: lanes(f) runs f(lane) on every lane; min64(f) is the minimum of f(lane) over the wave, known to every lane; sync()
// makes what the lanes wrote to Work visible to each other; add1(x) adds 1 to a counter in Work that other lanes add to as well;
// Own holds every lane's Entries, own[lane].  On the CPU the lanes are a loop and Own an array; on the device Own is the lane's own
// variable.
struct HostWave {
    struct Own { Entries e[kLanes]; Entries& operator[](unsigned l) { return e[l]; } };
    template <typename F> void lanes(F f) { for (unsigned l = 0; l < (unsigned)kLanes; ++l) f(l); }
    template <typename F> uint64_t min64(F f) { uint64_t m = kNone; for (unsigned l = 0; l < (unsigned)kLanes; ++l) { const uint64_t v = f(l); if (v < m) m = v; } return m; }
    void sync() {}
    void add1(int32_t& x) { ++x; }
};

// counts[256] -> bits_vals[kBitsVals], *nvals and, where codes is not null, codes[256]: value | length << 16 per symbol, 0: no code
// (jpeg_tables.hpp: HuffCodes).  Returns the longest code length before the limit to 16 (uniform over the wave).
template <typename W>
IRE_HD int build_table(W& wv, Work& s, const uint32_t* counts, uint8_t* bits_vals, int32_t* nvals, uint32_t* codes) {
    typename W::Own own;
    wv.lanes([&](unsigned lane) {
        Entries& e = own[lane];
        for (int j = 0; j < kPerLane; ++j) {
            const unsigned i = lane + (unsigned)kLanes * j;
            e.freq[j] = i < 256u ? counts[i] : (i == 256u ? 1u : 0u);
            e.codesize[j] = 0;
            e.root[j] = i;
        }
        for (int k = (int)lane; k < kMaxLen + 4; k += kLanes) s.bits[k] = 0;
        for (int k = (int)lane; k < kBitsVals; k += kLanes) bits_vals[k] = 0;
        if (codes) for (int k = (int)lane; k < 256; k += kLanes) codes[k] = 0;
    });
    // the merges: a lane touches its own entries alone
    for (int merge = 0; merge < 256; ++merge) {
        const uint64_t g1 = wv.min64([&](unsigned lane) {
            Entries& e = own[lane];
            uint64_t k1 = kNone, k2 = kNone;
            for (int j = 0; j < kPerLane; ++j) {
                const unsigned i = lane + (unsigned)kLanes * j;
                const uint64_t f = e.freq[j];
                const uint64_t key = f ? (f << 9) | (511u - i) : kNone;
                if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
            }
            e.k1 = k1; e.k2 = k2;
            return k1;
        });
        const uint64_t g2 = wv.min64([&](unsigned lane) { const Entries& e = own[lane]; return e.k1 == g1 ? e.k2 : e.k1; });
        if (g2 == kNone) break;
        const unsigned c1 = 511u - (unsigned)(g1 & 511u), c2 = 511u - (unsigned)(g2 & 511u);
        wv.lanes([&](unsigned lane) {
            Entries& e = own[lane];
            for (int j = 0; j < kPerLane; ++j) {
                const unsigned i = lane + (unsigned)kLanes * j;
                const unsigned r = e.root[j];      // (an entry without a count is its own root and never c1 or c2)
                if (r == c1 || r == c2) { e.codesize[j] += 1; e.root[j] = c1; }
                if (i == c1) e.freq[j] = (g1 >> 9) + (g2 >> 9);
                if (i == c2) e.freq[j] = 0;
            }
        });
    }
    wv.lanes([&](unsigned lane) {
        for (int j = 0; j < kPerLane; ++j) s.codesize[lane + (unsigned)kLanes * j] = (uint16_t)own[lane].codesize[j];
    });
    wv.sync();
    // bits[l]: every lane counts its own entries' lengths (at most 256: a place of bits[]); the longest of them all
    wv.lanes([&](unsigned lane) {
        for (int j = 0; j < kPerLane; ++j) { const unsigned cs = own[lane].codesize[j]; if (cs) wv.add1(s.bits[cs]); }
    });
    const int longest = 65535 - (int)wv.min64([&](unsigned lane) {
        unsigned m = 0;
        for (int j = 0; j < kPerLane; ++j) if (own[lane].codesize[j] > m) m = own[lane].codesize[j];
        return (uint64_t)(65535u - m);
    });
    wv.sync();
    // one lane: the limit to 16 bits and the pseudo-symbol's leave
    wv.lanes([&](unsigned lane) {
        if (lane != 0) return;
        for (int i = longest; i > 16; --i)
            while (s.bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && s.bits[j] == 0) --j;
                s.bits[i] -= 2; s.bits[i - 1] += 1; s.bits[j + 1] += 2; s.bits[j] -= 1;
            }
        int i = 16;
        while (i > 0 && s.bits[i] == 0) --i;
        if (i > 0) s.bits[i] -= 1;
    });
    wv.sync();
    // HUFFVAL: the real symbols by code size before the limit, then by value; a symbol's place is the number of symbols before it
    wv.lanes([&](unsigned lane) {
        int rank[4] = {0, 0, 0, 0}, mine[4];
        for (int m = 0; m < 4; ++m) mine[m] = s.codesize[lane + (unsigned)kLanes * m];
        for (unsigned j = 0; j < 256u; ++j) {
            const int cs = s.codesize[j];
            if (!cs) continue;
            for (int m = 0; m < 4; ++m) {
                const unsigned i = lane + (unsigned)kLanes * m;
                if (cs < mine[m] || (cs == mine[m] && j < i)) ++rank[m];
            }
        }
        for (int m = 0; m < 4; ++m) if (mine[m]) bits_vals[16 + rank[m]] = (uint8_t)(lane + (unsigned)kLanes * m);
        if (lane < 16u) bits_vals[lane] = (uint8_t)s.bits[lane + 1];
        if (lane == 0) { int n = 0; for (int l = 1; l <= 16; ++l) n += s.bits[l]; *nvals = n; }
    });
    wv.sync();
    // Annex C: the symbols of a length get consecutive codes, shortest first
    if (codes) {
        wv.lanes([&](unsigned lane) {
            for (int m = 0; m < 4; ++m) {
                const int p = (int)lane + kLanes * m;
                unsigned code = 0;
                int idx = 0;
                for (int l = 1; l <= 16; ++l) {
                    const int n = s.bits[l];
                    if (p < idx + n) { codes[bits_vals[16 + p]] = (code + (unsigned)(p - idx)) | ((unsigned)l << 16); break; }
                    code = (code + (unsigned)n) << 1;
                    idx += n;
                }
            }
        });
        wv.sync();
    }
    return longest;
}

// ---- the head of a file with its own tables -------------------------------------------------------------------------------------------
// The fixed-table head (jpeg_tables.hpp: jpeg_header, 629 bytes) is [0, kHeadPre) SOI APP0 DQT DQT SOF0 | four DHT | [kHeadPost0, 629)
// DRI SOS.  Here the four DHT segments, in the same order (0x00, 0x10, 0x01, 0x11), carry the tables given: 5 + 16 + nvals bytes each.
constexpr unsigned kHeadPre = 2 + 18 + 69 + 69 + 19, kHeadPostBytes = 6 + 14, kHeadFixedBytes = 629, kHeadPost0 = kHeadFixedBytes - kHeadPostBytes;
static_assert(kHeadPre + (5 + 16 + 12) * 2 + (5 + 16 + 162) * 2 + kHeadPostBytes == kHeadFixedBytes, "the fixed head's segments");
IRE_HD unsigned opt_head_bytes(const int32_t* nvals) {
    unsigned n = kHeadPre + kHeadPostBytes;
    for (int t = 0; t < 4; ++t) n += 5u + 16u + (unsigned)nvals[t];
    return n;
}
// byte k (< opt_head_bytes) of the head: fixed = the fixed-table head of the same image and settings, bits_vals[4][kBitsVals]
IRE_HD uint8_t opt_head_byte(unsigned k, const uint8_t* fixed, const uint8_t* bits_vals, const int32_t* nvals) {
    if (k < kHeadPre) return fixed[k];
    k -= kHeadPre;
    for (int t = 0; t < 4; ++t) {
        const unsigned nv = (unsigned)nvals[t], seg = 5u + 16u + nv;
        if (k < seg) {
            if (k == 0) return 0xff;
            if (k == 1) return 0xc4;
            if (k == 2) return (uint8_t)((3u + 16u + nv) >> 8);
            if (k == 3) return (uint8_t)((3u + 16u + nv) & 0xffu);
            if (k == 4) return (uint8_t)(((t & 1) << 4) | (t >> 1));
            return bits_vals[t * kBitsVals + (k - 5u)];
        }
        k -= seg;
    }
    return fixed[kHeadPost0 + (k < kHeadPostBytes ? k : kHeadPostBytes - 1u)];
}

}  // namespace jpeghuff
}  // namespace ire
