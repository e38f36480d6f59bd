// jpeg_dec_sim.cpp -- csrc/jpeg_parse.hpp and csrc/jpeg_dec_core.hpp on the CPU: the parser as it is, and the lane algorithm of
// csrc/jpeg_dec.hip with lanes as a loop -- the same windows, the same rounds, the same prefix sums, the same two passes, the same
// per-symbol step and per-subsequence loop (they are the kernel's own, compiled for the host).  Built plain and with
// -fsanitize=address,undefined by tests/test_jpeg_decode_native.py; this is where malformed input is exercised.
//
//   jpeg_dec_sim dump FILE OUT     "ok h w sampling nblocks" | "refused <reason>", then "status S rounds R windows W longest L";
//                                  OUT receives the coefficient scratch: int16 [component][block row][block column][64]
//   jpeg_dec_sim batch PACK        PACK = { u32 length, bytes } ... ; one line per file: "refused <reason>" | "status S rounds R windows W"
//   jpeg_dec_sim consts            the kernel's constants
//   "--poison BYTE" in front of a mode (sim_poison.hpp): the staged words and their padding, the lanes' states and counts, and the staging
//   behind every stream start as that byte; the coefficient scratch stays zero over the extent jpeg_dec_launch clears
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/jpeg_parse.hpp"
#include "sim_poison.hpp"

using simpoison::dirty;

using namespace ire::jpegdec;
using namespace ire::jpegparse;

struct Result { int status = 0; unsigned rounds = 0, windows = 0, longest = 0; };

// one long stream: what one workgroup of jpeg_dec_long_kernel does
static void decode_long(const DecImage& im, const DecTable* tabs, const DecStream& sr, const uint8_t* bytes, int16_t* coef, Result& res) {
    const uint32_t total_bits = 8u * sr.len, total_blocks = sr.nmcu * im.bpm, gblk0 = sr.mcu0 * im.bpm;
    std::vector<uint32_t> words = dirty<uint32_t>(kStagePadded);
    std::vector<DecState> start = dirty<DecState>(kLanes), end = dirty<DecState>(kLanes), prev_end = dirty<DecState>(kLanes);
    std::vector<LaneOut> lo = dirty<LaneOut>(kLanes);
    DecState carry{0, 0, 0};
    uint32_t done_blocks = 0, dc_carry[4] = {0, 0, 0, 0}, final_p = kBadPos;
    uint32_t err = 0;
    bool finished = false;
    for (uint32_t win0 = 0; win0 < total_bits && !finished && !err; win0 += kWindowBits) {
        for (uint32_t k = 0; k < kStageWords; ++k) words[k + (k >> 5)] = stream_word(bytes, sr.len, win0 / 32 + k);
        const WordReader rd{words.data(), win0};
        // the lanes whose subsequence begins inside the stream (a lane behind its end would only hand a state on, one lane per round)
        const int nl = (int)((total_bits - win0 + kSubseqBits - 1) / kSubseqBits < (uint32_t)kLanes ? (total_bits - win0 + kSubseqBits - 1) / kSubseqBits : (uint32_t)kLanes);
        auto lim_of = [&](int t) { const uint64_t e = (uint64_t)win0 + (uint64_t)(t + 1) * kSubseqBits; return e < total_bits ? (uint32_t)e : total_bits; };
        for (int t = 0; t < nl; ++t) {                           // round 0
            start[t] = t == 0 ? carry : DecState{win0 + (uint32_t)t * kSubseqBits, 0, 0};
            end[t] = start[t];
            dec_subseq(rd, tabs, im, end[t], lim_of(t), 0xffffffffu, nullptr, 0, nullptr, lo[t]);
        }
        unsigned rounds = 1;
        for (int round = 1; round <= kLanes; ++round) {          // bounded by the lane count
            prev_end = end;
            bool changed = false;
            for (int t = 1; t < nl; ++t) {
                const DecState& pv = prev_end[t - 1];
                if (pv.p != start[t].p || pv.blk != start[t].blk || pv.k != start[t].k) {
                    start[t] = pv; end[t] = pv;
                    dec_subseq(rd, tabs, im, end[t], lim_of(t), 0xffffffffu, nullptr, 0, nullptr, lo[t]);
                    changed = true;
                }
            }
            if (!changed) break;
            ++rounds;
        }
        res.rounds += rounds; res.windows += 1;
        if (rounds > res.longest) res.longest = rounds;
        // prefix sums, then the writing pass
        uint32_t before = done_blocks, dcb[4] = {dc_carry[0], dc_carry[1], dc_carry[2], 0};
        for (int t = 0; t < nl; ++t) {
            uint32_t dcpred[4] = {dcb[0], dcb[1], dcb[2], 0};
            const uint32_t room = total_blocks > before ? total_blocks - before : 0;
            DecState st = start[t];
            LaneOut w;
            simpoison::soil(&w, 1);
            err |= dec_subseq(rd, tabs, im, st, lim_of(t), room, coef, gblk0 + before, dcpred, w);
            if (w.nblk && before + w.nblk == total_blocks) { final_p = st.p; finished = true; }
            before += lo[t].nblk;
            for (int c = 0; c < 3; ++c) dcb[c] += lo[t].dc[c];
        }
        done_blocks = before;
        for (int c = 0; c < 3; ++c) dc_carry[c] = dcb[c];
        carry = end[nl - 1];
    }
    if (!err && !(finished && stream_end_ok(final_p, sr.len))) err |= kStBadEnd;
    res.status |= (int)err;
}

// one short stream: what one lane of jpeg_dec_short_kernel does
static void decode_short(const DecImage& im, const DecTable* tabs, const DecStream& sr, const uint8_t* bytes, int16_t* coef, Result& res) {
    const ByteReader rd{bytes, sr.len};
    DecState st{0, 0, 0};
    uint32_t dcpred[4] = {0, 0, 0, 0};
    LaneOut o;
    simpoison::soil(&o, 1);
    uint32_t err = dec_subseq(rd, tabs, im, st, 8u * sr.len, sr.nmcu * im.bpm, coef, sr.mcu0 * im.bpm, dcpred, o);
    if (!err && !(o.nblk == sr.nmcu * im.bpm && stream_end_ok(st.p, sr.len))) err |= kStBadEnd;
    res.status |= (int)err;
}

static bool decode_file(const uint8_t* file, size_t bytes, Header& hd, std::vector<int16_t>& coef, Result& res, std::string& why) {
    if (!parse_header(file, bytes, hd, why)) return false;
    const size_t room = scan_room(hd, bytes);
    std::vector<uint8_t> stage = dirty<uint8_t>(room);      // (a pinned blob used before: what lies behind a stream is not zero)
    std::vector<DecStream> streams(hd.nstreams);
    if (!split_scan(hd, file, bytes, stage.data(), room, streams.data(), why)) return false;
    uint32_t nblk = 0;
    for (int c = 0; c < hd.im.ncomp; ++c) nblk += hd.im.gridw[c] * hd.im.gridh[c];
    // the one thing jpeg_dec_launch clears: the status words and, per image, coef_blocks(h, w) blocks of coefficients (jpeg_dec_core.hpp:
    // the launch code's own extent).  The blocks a file really has lie inside that extent, so they start as zero under --poison too; the
    // rest of the extent, and the dirty memory behind it, no block index of this file reaches (dec_subseq writes below the block count).
    const size_t cleared = coef_blocks(hd.im.h, hd.im.w);
    if (nblk > cleared) { why = "simulator: more blocks than jpeg_dec_launch clears"; return false; }
    coef.assign((size_t)nblk * 64, 0);
    for (const DecStream& s : streams) {
        if (s.len > kShortMaxBytes) decode_long(hd.im, hd.tabs, s, stage.data() + s.off, coef.data(), res);
        else decode_short(hd.im, hd.tabs, s, stage.data() + s.off, coef.data(), res);
    }
    return true;
}

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    simpoison::take_poison(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "consts")) {
        std::printf("lanes %d subseq_bits %d window_bits %u short_max_bytes %u\n", kLanes, kSubseqBits, kWindowBits, kShortMaxBytes);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "dump")) {
        const std::vector<uint8_t> file = slurp(argv[2]);
        // an exact-size copy on the heap: a read one byte past the file is a sanitizer report
        std::vector<uint8_t> exact(file.begin(), file.end());
        Header hd;
        std::vector<int16_t> coef;
        Result res;
        std::string why;
        if (!decode_file(exact.data(), exact.size(), hd, coef, res, why)) { std::printf("refused %s\n", why.c_str()); return 0; }
        std::printf("ok %d %d %d %zu\n", hd.im.h, hd.im.w, hd.im.sampling, coef.size() / 64);
        std::printf("status %d rounds %u windows %u longest %u\n", res.status, res.rounds, res.windows, res.longest);
        FILE* f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(coef.data(), 2, coef.size(), f) != coef.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        std::fclose(f);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "batch")) {
        const std::vector<uint8_t> pack = slurp(argv[2]);
        size_t i = 0;
        while (i + 4 <= pack.size()) {
            uint32_t n;
            std::memcpy(&n, pack.data() + i, 4);
            i += 4;
            if (i + n > pack.size()) { std::fprintf(stderr, "bad pack\n"); return 2; }
            uint8_t* exact = static_cast<uint8_t*>(std::malloc(n ? n : 1));      // exactly n bytes: see above
            std::memcpy(exact, pack.data() + i, n);
            i += n;
            Header hd;
            std::vector<int16_t> coef;
            Result res;
            std::string why;
            if (!decode_file(exact, n, hd, coef, res, why)) std::printf("refused %s\n", why.c_str());
            else std::printf("status %d rounds %u windows %u\n", res.status, res.rounds, res.windows);
            std::free(exact);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: jpeg_dec_sim dump FILE OUT | batch PACK | consts\n");
    return 2;
}
