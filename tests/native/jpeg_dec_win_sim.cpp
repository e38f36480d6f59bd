// jpeg_dec_win_sim.cpp -- the window-parallel decode of long streams (csrc/jpeg_dec.hip: the spec, chain and write kernels) on the
// CPU, with windows and lanes as loops.  What the passes share with the kernels BY CODE is csrc/jpeg_dec_core.hpp: the step, the
// subsequence loop, the window arithmetic, spec_start, chain_lane, the records.  The loops round them -- pass A's rounds, pass B's walk,
// pass C's prefix sums -- are written again here as plain loops (the kernels' have barriers, LDS and a shared go flag), as
// jpeg_dec_sim.cpp does for the one-workgroup kernel: a slip in the kernels' own loop structure is the GPU tests' to catch.
// Here EVERY long stream takes the three passes, a single-window one too (the one-workgroup kernel that keeps those on the device
// is tests/native/jpeg_dec_sim.cpp's).  Built plain and with -fsanitize=address,undefined by
// tests/test_jpeg_decode_windows_native.py.
//
//   jpeg_dec_win_sim dump FILE OUT [poison]   "ok h w sampling nblocks" | "refused <reason>", then "status S windows W redecodes a,b,..."
//                                             (per window: the lanes the chain pass decoded again); OUT receives the coefficient scratch.
//                                             poison: every guessed start state of the spec pass is wrong on purpose
//   jpeg_dec_win_sim batch PACK               PACK = { u32 length, bytes } ... ; one line per file: "refused <reason>" | "status S"
//   jpeg_dec_win_sim table LEN                a stream of LEN bytes: "windows W", then per window "win0 lanes last_lim"
//   jpeg_dec_win_sim consts                   the kernels' constants
//   "--poison BYTE" in front of a mode (sim_poison.hpp; not the `poison` word behind dump, which is about guesses): the lane records and
//   window heads (device scratch that nothing clears), the staged words and their padding, the lanes' states and counts and the staging
//   behind the streams start as that byte; the coefficient scratch stays zero over the extent jpeg_dec_launch clears
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

struct Result { int status = 0; std::vector<unsigned> redecodes; };

static void stage(std::vector<uint32_t>& words, unsigned n, const uint8_t* bytes, uint32_t len, uint32_t bit0) {
    for (uint32_t k = 0; k < n; ++k) words[k + (k >> 5)] = stream_word(bytes, len, bit0 / 32 + k);
}

static void decode_long(const DecImage& im, const DecTable* tabs, const DecStream& sr, const uint8_t* bytes, int16_t* coef, bool poison, Result& res) {
    const uint32_t total_bits = 8u * sr.len, total_blocks = sr.nmcu * im.bpm, gblk0 = sr.mcu0 * im.bpm, nwin = window_count(sr.len);
    std::vector<LaneRec> recs = dirty<LaneRec>((size_t)nwin * kLanes);
    std::vector<WinHead> heads = dirty<WinHead>(nwin);
    std::vector<uint32_t> words = dirty<uint32_t>(kStagePadded), lane_words = dirty<uint32_t>(kChainStagePadded);
    uint32_t err = 0;
    // A: every window by itself (jpeg_dec_spec_kernel)
    for (uint32_t wi = 0; wi < nwin; ++wi) {
        const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        stage(words, kStageWords, bytes, sr.len, win0);
        const WordReader rd{words.data(), win0};
        std::vector<DecState> start = dirty<DecState>(nl), end = dirty<DecState>(nl), prev_end = dirty<DecState>(nl);
        std::vector<LaneOut> lo = dirty<LaneOut>(nl);
        for (uint32_t t = 0; t < nl; ++t) {
            start[t] = spec_start(win0, t);
            // poison: every guess (all but the stream's very first lane, whose state is known) wrong on purpose
            if (poison && start[t].p != 0) start[t] = DecState{start[t].p + 7, im.bpm > 1 ? 1u : 0u, 5};
            end[t] = start[t];
            dec_subseq(rd, tabs, im, end[t], lane_lim(total_bits, win0, t), 0xffffffffu, nullptr, 0, nullptr, lo[t]);
        }
        for (int round = 1; round <= kLanes; ++round) {
            prev_end = end;
            bool changed = false;
            for (uint32_t t = 1; t < nl; ++t) {
                const DecState& pv = prev_end[t - 1];
                if (pv.p != start[t].p || state_bk(pv) != state_bk(start[t])) {
                    start[t] = end[t] = pv;
                    dec_subseq(rd, tabs, im, end[t], lane_lim(total_bits, win0, t), 0xffffffffu, nullptr, 0, nullptr, lo[t]);
                    changed = true;
                }
            }
            if (!changed) break;
        }
        for (uint32_t t = 0; t < nl; ++t) recs[(size_t)wi * kLanes + t] = LaneRec{start[t].p, state_bk(start[t]), end[t].p, state_bk(end[t]), lo[t]};
    }
    // B: the stream's windows in order (jpeg_dec_chain_kernel)
    DecState carry{0, 0, 0};
    uint32_t done = 0, dcc[3] = {0, 0, 0};
    for (uint32_t wi = 0; wi < nwin; ++wi) {
        const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        LaneRec* r = recs.data() + (size_t)wi * kLanes;
        heads[wi] = WinHead{done, {dcc[0], dcc[1], dcc[2]}};
        unsigned again = 0;
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t bit0 = win0 + l * kSubseqBits;
            if (r[l].sp == carry.p && r[l].sbk == state_bk(carry)) break;
            if (carry.p < bit0) { err |= kStBadCode; break; }
            stage(lane_words, kChainStageWords, bytes, sr.len, bit0);
            if (chain_lane(WordReader{lane_words.data(), bit0}, tabs, im, lane_lim(total_bits, win0, l), r[l], carry)) break;
            ++again;
        }
        res.redecodes.push_back(again);
        for (uint32_t t = 0; t < nl; ++t) { done += r[t].o.nblk; for (int c = 0; c < 3; ++c) dcc[c] += r[t].o.dc[c]; }
        carry = state_of(r[nl - 1].ep, r[nl - 1].ebk);
    }
    if (done < total_blocks) err |= kStBadEnd;
    // C: every window by itself (jpeg_dec_write_kernel)
    for (uint32_t wi = 0; wi < nwin; ++wi) {
        const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        stage(words, kStageWords, bytes, sr.len, win0);
        const WordReader rd{words.data(), win0};
        uint32_t first = heads[wi].done, dcb[3] = {heads[wi].dc[0], heads[wi].dc[1], heads[wi].dc[2]};
        for (uint32_t t = 0; t < nl; ++t) {
            const LaneRec& r = recs[(size_t)wi * kLanes + t];
            uint32_t dcpred[4] = {dcb[0], dcb[1], dcb[2], 0};
            const uint32_t room = total_blocks > first ? total_blocks - first : 0;
            DecState st = state_of(r.sp, r.sbk);
            LaneOut w;
            simpoison::soil(&w, 1);
            uint32_t e = dec_subseq(rd, tabs, im, st, lane_lim(total_bits, win0, t), room, coef, gblk0 + first, dcpred, w);
            if (!e && w.nblk && first + w.nblk == total_blocks && !stream_end_ok(st.p, sr.len)) e = kStBadEnd;
            err |= e;
            first += r.o.nblk;
            for (int c = 0; c < 3; ++c) dcb[c] += r.o.dc[c];
        }
    }
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

static bool decode_file(const uint8_t* file, size_t bytes, Header& hd, std::vector<int16_t>& coef, bool poison, Result& res, std::string& why) {
    if (!parse_header(file, bytes, hd, why)) return false;
    const size_t room = scan_room(hd, bytes);
    std::vector<uint8_t> stage_bytes = dirty<uint8_t>(room);
    std::vector<DecStream> streams(hd.nstreams);
    if (!split_scan(hd, file, bytes, stage_bytes.data(), room, streams.data(), why)) return false;
    uint32_t nblk = 0;
    for (int c = 0; c < hd.im.ncomp; ++c) nblk += hd.im.gridw[c] * hd.im.gridh[c];
    // the one thing jpeg_dec_launch clears: the status words and, per image, coef_blocks(h, w) blocks of coefficients (jpeg_dec_core.hpp:
    // the launch code's own extent).  The blocks a file really has lie inside that extent, so they start as zero under --poison too; the
    // rest of the extent, and the dirty memory behind it, no block index of this file reaches (dec_subseq writes below the block count).
    const size_t cleared = coef_blocks(hd.im.h, hd.im.w);
    if (nblk > cleared) { why = "simulator: more blocks than jpeg_dec_launch clears"; return false; }
    coef.assign((size_t)nblk * 64, 0);
    for (const DecStream& s : streams) {
        // an exact-size copy of the stream on the heap: a read one byte past it is a sanitizer report
        std::vector<uint8_t> exact(stage_bytes.begin() + s.off, stage_bytes.begin() + s.off + s.len);
        if (s.len > kShortMaxBytes) decode_long(hd.im, hd.tabs, s, exact.data(), coef.data(), poison, res);
        else decode_short(hd.im, hd.tabs, s, exact.data(), coef.data(), res);
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
    if (argc == 3 && !std::strcmp(argv[1], "table")) {
        const uint32_t len = (uint32_t)std::strtoul(argv[2], nullptr, 10), total_bits = 8u * len, nwin = window_count(len);
        std::printf("windows %u\n", nwin);
        for (uint32_t wi = 0; wi < nwin; ++wi) {
            const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
            std::printf("%u %u %u\n", win0, nl, lane_lim(total_bits, win0, nl - 1));
        }
        return 0;
    }
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "dump")) {
        const bool poison = argc == 5 && !std::strcmp(argv[4], "poison");
        const std::vector<uint8_t> file = slurp(argv[2]);
        std::vector<uint8_t> exact(file.begin(), file.end());
        Header hd;
        std::vector<int16_t> coef;
        Result res;
        std::string why;
        if (!decode_file(exact.data(), exact.size(), hd, coef, poison, res, why)) { std::printf("refused %s\n", why.c_str()); return 0; }
        std::printf("ok %d %d %d %zu\n", hd.im.h, hd.im.w, hd.im.sampling, coef.size() / 64);
        std::printf("status %d windows %zu redecodes ", res.status, res.redecodes.size());
        for (size_t k = 0; k < res.redecodes.size(); ++k) std::printf("%s%u", k ? "," : "", res.redecodes[k]);
        std::printf("%s\n", res.redecodes.empty() ? "-" : "");
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
            uint8_t* exact = static_cast<uint8_t*>(std::malloc(n ? n : 1));
            std::memcpy(exact, pack.data() + i, n);
            i += n;
            Header hd;
            std::vector<int16_t> coef;
            Result res;
            std::string why;
            if (!decode_file(exact, n, hd, coef, false, res, why)) std::printf("refused %s\n", why.c_str());
            else std::printf("status %d\n", res.status);
            std::free(exact);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: jpeg_dec_win_sim dump FILE OUT [poison] | batch PACK | table LEN | consts\n");
    return 2;
}
