// jpeg_prog_sim.cpp -- csrc/jpeg_parse.hpp's file entry (plan_file / split_file) and csrc/jpeg_dec_core.hpp's scan kinds on the CPU: a
// progressive file decoded the way csrc/jpeg_dec.hip decodes it, with lanes, windows, waves and launches as loops -- level by level;
// a first scan's long streams through the three passes of the window path (spec / chain / write), its short ones by one lane; a DC
// refinement scan block by block; an AC refinement scan as mask / walk / apply, the walk of a long stream in the wave kernel's turns
// (kWalkBlocks masks and kWalkWords words staged per turn, records flushed per turn).  The steps are the kernels' own, compiled for
// the host.  Built plain and with -fsanitize=address,undefined by tests/test_jpeg_prog_native.py; never loaded into python.
//
//   jpeg_prog_sim dump FILE OUT [poison]   "ok h w sampling nblocks nscans nlevels" | "refused <reason>", then
//                                          "status S windows W maxwin M turns T maxrun R"; OUT receives the coefficient scratch
//                                          (poison: every guessed start state of the window path wrong on purpose)
//   jpeg_prog_sim plan FILE ACCEPT         "ok h w sampling nscans" | "refused <reason>"
//   jpeg_prog_sim batch PACK               PACK = { u32 length, bytes } ... ; one line per file: "refused <reason>" | "status S"
//   jpeg_prog_sim consts                   the kernels' constants
//   "--poison BYTE" in front of a mode (sim_poison.hpp; not the `poison` word behind dump, which is about guesses): the lane records, window
//   heads, masks and walk records (device scratch that nothing clears), the walk's LDS (masks, records, words), the staged words and their
//   padding, the lanes' state and the staging behind the streams start as that byte; the coefficient scratch stays zero over the extent
//   jpeg_dec_launch clears
#include <algorithm>
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

struct Result { int status = 0; unsigned windows = 0, maxwin = 0, turns = 0, maxrun = 0; };

static void stage(std::vector<uint32_t>& words, unsigned n, const uint8_t* bytes, uint32_t len, uint32_t bit0) {
    for (uint32_t k = 0; k < n; ++k) words[k + (k >> 5)] = stream_word(bytes, len, bit0 / 32 + k);
}

// a long stream of a baseline or first scan: jpeg_dec_spec_kernel, jpeg_dec_chain_kernel, jpeg_dec_write_kernel
static void decode_long(const DecImage& im, const DecTable* tabs, const DecStream& sr, const uint8_t* bytes, int16_t* coef, bool poison, Result& res) {
    const uint32_t total_bits = 8u * sr.len, total_blocks = sr.nmcu * im.bpm, gblk0 = sr.mcu0 * im.bpm, nwin = window_count(sr.len);
    std::vector<LaneRec> recs = dirty<LaneRec>((size_t)nwin * kLanes);
    std::vector<WinHead> heads = dirty<WinHead>(nwin);
    std::vector<uint32_t> words = dirty<uint32_t>(kStagePadded), lane_words = dirty<uint32_t>(kChainStagePadded);
    uint32_t err = 0;
    res.windows += nwin; res.maxwin = std::max(res.maxwin, nwin);
    for (uint32_t wi = 0; wi < nwin; ++wi) {
        const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        stage(words, kStageWords, bytes, sr.len, win0);
        const WordReader rd{words.data(), win0};
        std::vector<DecState> start = dirty<DecState>(nl), end = dirty<DecState>(nl), prev_end = dirty<DecState>(nl);
        std::vector<LaneOut> lo = dirty<LaneOut>(nl);
        for (uint32_t t = 0; t < nl; ++t) {
            start[t] = spec_start(win0, t);
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
    DecState carry{0, 0, 0};
    uint32_t done = 0, dcc[3] = {0, 0, 0};
    for (uint32_t wi = 0; wi < nwin; ++wi) {
        const uint32_t win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        LaneRec* r = recs.data() + (size_t)wi * kLanes;
        heads[wi] = WinHead{done, {dcc[0], dcc[1], dcc[2]}};
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t bit0 = win0 + l * kSubseqBits;
            if (r[l].sp == carry.p && r[l].sbk == state_bk(carry)) break;
            if (carry.p < bit0) { err |= kStBadCode; break; }
            stage(lane_words, kChainStageWords, bytes, sr.len, bit0);
            if (chain_lane(WordReader{lane_words.data(), bit0}, tabs, im, lane_lim(total_bits, win0, l), r[l], carry)) break;
        }
        for (uint32_t t = 0; t < nl; ++t) { done += r[t].o.nblk; for (int c = 0; c < 3; ++c) dcc[c] += r[t].o.dc[c]; }
        carry = state_of(r[nl - 1].ep, r[nl - 1].ebk);
    }
    if (done < total_blocks) err |= kStBadEnd;
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

// jpeg_dec_short_kernel's lane
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

// jpeg_dec_dcref_kernel: a thread per block of the scan
static void dc_refine(const DecImage& im, const DecStream* streams, uint32_t nstreams, const uint8_t* stage_bytes, int16_t* coef, Result& res) {
    const uint32_t per = streams[0].nmcu * im.bpm;
    for (uint32_t g = 0; g < im.nblocks; ++g) {
        const uint32_t si = g / per, n = g - si * per;
        if (si >= nstreams) continue;
        const DecStream& sr = streams[si];
        if (n >= sr.nmcu * im.bpm) continue;
        if (n == 0 && !stream_end_ok(sr.nmcu * im.bpm, sr.len)) res.status |= kStBadEnd;
        const uint32_t byte = n >> 3;
        if (byte < sr.len && ((stage_bytes[sr.off + byte] >> (7u - (n & 7u))) & 1u)) {
            int16_t* c = coef + block_base(im, g);
            *c = (int16_t)(*c | (1 << im.al));
        }
    }
}

// jpeg_dec_walk_long_kernel: lane 0's walk between the turns in which the wave stages masks and words and writes the records
static uint32_t walk_long(const DecTable& tab, const DecImage& im, const DecStream& sr, const uint8_t* bytes, const uint64_t* masks, uint32_t* recs, uint32_t nblk, Result& res) {
    std::vector<uint64_t> s_mask = dirty<uint64_t>(kWalkBlocks);
    std::vector<uint32_t> s_rec = dirty<uint32_t>(kWalkBlocks), s_words = dirty<uint32_t>(kWalkStagePadded);
    RefState st{0, 0, 0};
    uint32_t n = 0, mb = 0, err = 0;
    const uint32_t total_bits = 8u * sr.len;
    while (n < nblk && !err) {
        const uint32_t bit0 = st.p & ~31u, nend = std::min(mb + kWalkBlocks, nblk);
        for (uint32_t l = 0; l < kWalkBlocks; ++l) s_mask[l] = mb + l < nblk ? masks[mb + l] : 0;
        stage(s_words, kWalkStageWords, bytes, sr.len, bit0);
        err = refine_walk_some(WordReader{s_words.data(), bit0}, tab, im.ss, im.se, s_mask.data(), s_rec.data(), mb, nend, bit0 + 32u * kWalkWords, total_bits, st, n);
        ++res.turns;
        if (n == nend || err) {
            for (uint32_t l = 0; l < kWalkBlocks; ++l)
                if (mb + l < n || (mb + l == n && n < nblk && err)) recs[mb + l] = s_rec[l];
            if (n == nend) mb = nend;
        }
    }
    if (err) for (uint32_t j = n + 1; j < nblk; ++j) recs[j] = kBadPos;
    return err ? err : refine_walk_end(st, sr.len);
}

// jpeg_dec_mask_kernel, jpeg_dec_walk_kernel / jpeg_dec_walk_long_kernel, jpeg_dec_apply_kernel
static void ac_refine(const DecImage& im, const DecTable* tabs, const DecStream* streams, uint32_t nstreams, const uint8_t* stage_bytes, int16_t* coef, Result& res) {
    std::vector<uint64_t> masks = dirty<uint64_t>(im.nblocks);
    std::vector<uint32_t> recs(im.nblocks, 0x5a5a5a5au);
    simpoison::soil(recs.data(), recs.size());
    for (uint32_t g = 0; g < im.nblocks; ++g) {
        const int16_t* blk = coef + block_base(im, g);
        uint64_t m = 0;
        for (uint32_t j = im.ss; j <= im.se; ++j) if (blk[natural_of(j)] != 0) m |= 1ull << j;
        masks[g] = m;
    }
    const DecTable& tab = tabs[4u + (im.ac_tab[im.comp_of[0] & 3u] & 3u)];
    for (uint32_t si = 0; si < nstreams; ++si) {
        const DecStream& sr = streams[si];
        const uint32_t nblk = sr.mcu0 < im.nblocks ? std::min(sr.nmcu, im.nblocks - sr.mcu0) : 0u;
        const uint8_t* bytes = stage_bytes + sr.off;
        uint32_t err;
        if (sr.len > kShortMaxBytes) err = walk_long(tab, im, sr, bytes, masks.data() + sr.mcu0, recs.data() + sr.mcu0, nblk, res);
        else err = refine_walk_stream(ByteReader{bytes, sr.len}, tab, im.ss, im.se, masks.data() + sr.mcu0, recs.data() + sr.mcu0, nblk, sr.len);
        res.status |= (int)err;
    }
    const uint32_t per = streams[0].nmcu;
    for (uint32_t g = 0; g < im.nblocks; ++g) {
        const uint32_t si = g / per;
        if (si >= nstreams) continue;
        const DecStream& sr = streams[si];
        if (g < sr.mcu0 || g - sr.mcu0 >= sr.nmcu) continue;
        refine_apply_block(ByteReader{stage_bytes + sr.off, sr.len}, tab, im.ss, im.se, im.al, masks[g], recs[g], coef + block_base(im, g));
    }
}

static bool decode_file(const uint8_t* file, size_t bytes, File& f, std::vector<int16_t>& coef, bool poison, Result& res, std::string& why) {
    if (!plan_file(file, bytes, kAcceptProgressive, f, why)) return false;
    const size_t room = file_room(f, bytes);
    std::vector<uint8_t> stage_bytes = dirty<uint8_t>(room);
    std::vector<DecStream> streams(f.nstreams);
    if (!split_file(f, file, bytes, stage_bytes.data(), room, streams.data(), why)) return false;
    const DecImage& fr = f.hd.im;
    uint32_t nblk = 0;
    for (int c = 0; c < fr.ncomp; ++c) nblk += fr.gridw[c] * fr.gridh[c];
    // the one thing jpeg_dec_launch clears: the status words and, per image, coef_blocks(h, w) blocks of coefficients (jpeg_dec_core.hpp:
    // the launch code's own extent).  The blocks a file really has lie inside that extent, so they start as zero under --poison too; the
    // rest of the extent, and the dirty memory behind it, no block index of this file reaches (dec_subseq writes below the block count).
    const size_t cleared = coef_blocks(fr.h, fr.w);
    if (nblk > cleared) { why = "simulator: more blocks than jpeg_dec_launch clears"; return false; }
    coef.assign((size_t)nblk * 64, 0);
    if (!f.progressive) {
        for (const DecStream& s : streams) {
            if (s.len > kShortMaxBytes) decode_long(fr, f.hd.tabs, s, stage_bytes.data() + s.off, coef.data(), poison, res);
            else decode_short(fr, f.hd.tabs, s, stage_bytes.data() + s.off, coef.data(), res);
        }
        return true;
    }
    for (uint32_t level = 0; level < f.nlevels; ++level) {           // one round of launches per level; inside it any order
        uint32_t s0 = 0;
        for (const Scan& sc : f.scans) {
            const DecStream* ss = streams.data() + s0;
            s0 += sc.nstreams;
            if (sc.level != level) continue;
            DecTable tabs[8];
            for (int k = 0; k < 8; ++k) tabs[k] = f.pool[std::min<size_t>(sc.tab[k], f.pool.size() - 1)];
            for (uint32_t k = 0; k < sc.nstreams; ++k) if (sc.im.kind == kScanAcFirst || sc.im.kind == kScanAcRefine) res.maxrun = std::max(res.maxrun, ss[k].nmcu);
            if (sc.im.kind == kScanDcRefine) dc_refine(sc.im, ss, sc.nstreams, stage_bytes.data(), coef.data(), res);
            else if (sc.im.kind == kScanAcRefine) ac_refine(sc.im, tabs, ss, sc.nstreams, stage_bytes.data(), coef.data(), res);
            else
                for (uint32_t k = 0; k < sc.nstreams; ++k) {
                    if (ss[k].len > kShortMaxBytes) decode_long(sc.im, tabs, ss[k], stage_bytes.data() + ss[k].off, coef.data(), poison, res);
                    else decode_short(sc.im, tabs, ss[k], stage_bytes.data() + ss[k].off, coef.data(), res);
                }
        }
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
        std::printf("lanes %d subseq_bits %d window_bits %u short_max_bytes %u walk_blocks %u walk_words %u max_scans %u\n", kLanes, kSubseqBits, kWindowBits, kShortMaxBytes,
                    kWalkBlocks, kWalkWords, kMaxScans);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const std::vector<uint8_t> file = slurp(argv[2]);
        std::vector<uint8_t> exact(file.begin(), file.end());
        File f;
        std::string why;
        if (!plan_file(exact.data(), exact.size(), (uint32_t)std::atoi(argv[3]), f, why)) { std::printf("refused %s\n", why.c_str()); return 0; }
        std::printf("ok %d %d %d %u\n", f.hd.im.h, f.hd.im.w, f.hd.im.sampling, f.nscans());
        return 0;
    }
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "dump")) {
        const std::vector<uint8_t> file = slurp(argv[2]);
        // an exact-size copy on the heap: a read one byte past the file is a sanitizer report
        std::vector<uint8_t> exact(file.begin(), file.end());
        File f;
        std::vector<int16_t> coef;
        Result res;
        std::string why;
        if (!decode_file(exact.data(), exact.size(), f, coef, argc == 5 && !std::strcmp(argv[4], "poison"), res, why)) { std::printf("refused %s\n", why.c_str()); return 0; }
        std::printf("ok %d %d %d %zu %u %u\n", f.hd.im.h, f.hd.im.w, f.hd.im.sampling, coef.size() / 64, f.nscans(), f.nlevels);
        std::printf("status %d windows %u maxwin %u turns %u maxrun %u\n", res.status, res.windows, res.maxwin, res.turns, res.maxrun);
        FILE* o = std::fopen(argv[3], "wb");
        if (!o || std::fwrite(coef.data(), 2, coef.size(), o) != coef.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        std::fclose(o);
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
            File f;
            std::vector<int16_t> coef;
            Result res;
            std::string why;
            if (!decode_file(exact, n, f, coef, false, res, why)) std::printf("refused %s\n", why.c_str());
            else std::printf("status %d\n", res.status);
            std::free(exact);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: jpeg_prog_sim dump FILE OUT [poison] | plan FILE ACCEPT | batch PACK | consts\n");
    return 2;
}
