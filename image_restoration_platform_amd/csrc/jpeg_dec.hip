// jpeg_dec.hip -- baseline and progressive JPEG files -> RGB pixels, on the device, byte for byte what libjpeg-turbo decodes.
//
// The host (jpeg_parse.hpp) reads the markers, refuses what is out of scope, cuts the scan at the restart markers into independent
// streams with the byte stuffing removed, and builds the decode tables; ONE upload carries a whole batch: image records, tables,
// stream table, stream bytes.  Then, per BATCH (image is a grid dimension; nothing below depends on n):
//   memset                    the status words and the coefficient scratch (a block's zero coefficients are never written)
//   K1 jpeg_dec_long_kernel   one workgroup per stream longer than kShortMaxBytes: the self-synchronising lane algorithm of
//                             jpeg_dec_core.hpp, window by window (kLanes x kSubseqBits bits, staged into LDS as big-endian words,
//                             one pad word per 32 so that lane i starts on bank i); the first lane of a window starts from the exact
//                             end state of the window before.  No workgroup waits for another.  It keeps the long streams of ONE window.
//   spec / chain / write      a long stream of two or more windows (the host lists them and their windows in the blob): every window
//                             a workgroup.  jpeg_dec_spec_kernel settles each window from a guessed entry state and records its lanes;
//                             jpeg_dec_chain_kernel, one workgroup per stream, carries the true state through its windows, decoding
//                             again only the lanes up to the one whose recorded start it meets, and sums the windows' block counts and
//                             DC sums; jpeg_dec_write_kernel writes every window's coefficients.  The three launches are the only
//                             ordering between workgroups (jpeg_dec_core.hpp says why the result does not depend on the guess)
//   K2 jpeg_dec_short_kernel  one LANE per short stream in a strided loop (our own encoder's 16-MCU intervals are ~80 bytes): the
//                             same loop, start to end, straight from the stream's bytes
//   K3 jpeg_dec_idct_kernel   dequantise + libjpeg's "islow" inverse DCT (jidctint.c) + range limit: 32 blocks per workgroup,
//                             thread = (block, column) then (block, row) through LDS rows of 9 ints (conflict-free both ways, as
//                             in jpeg.hip); samples to per-component planes on the block grid
//   K4 jpeg_dec_colour_kernel per pixel: "fancy" h2v1 / h2v2 chroma upsampling on the planes' REAL sizes (the blocks' padding is
//                             never read), YCbCr -> RGB in 16-bit fixed point; the image's status word to the caller's array
// A progressive file (jpeg_parse.hpp: parse_progressive) brings a record per SCAN: the frame's DecImage with the scan's own MCU, band and
// bit position.  K1 .. K2 take such a record for an image (its first scans go through the very same lanes: jpeg_dec_core.hpp
// dec_step_scan), once per dependency level; behind them run the level's refinement scans: jpeg_dec_dcref_kernel, and
// jpeg_dec_mask_kernel / jpeg_dec_walk_kernel / jpeg_dec_apply_kernel.  K3 and K4 see the finished coefficients and know no difference.
// Safety: every loop of K1 / K2 is bounded by the stream's bit count and its block count; reads of stream bytes are clamped to
// the stream's length (1-bits behind it, as libjpeg pads); a coefficient is written only to a block index below the image's block
// count; a code no table holds, a zig-zag index above 63, a DC category above 11 or a stream that ends with blocks missing or bytes
// left over sets the image's status word and stops that stream; so does (K3) a dequantised coefficient outside int16 or a sample
// outside -512..511 before the range limit, where libjpeg-turbo's C and SIMD code give different bytes.  tests/native/jpeg_dec_sim.cpp runs the same code on the CPU.
#include "jpeg_dec.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace ire {

namespace {

using namespace jpegdec;

constexpr int kThreads = kLanes;
constexpr int kWaves = kThreads / 64;

struct DecBatch {
    const DecImage* images;
    const DecTable* tabs;          // 8 per image
    const DecStream* streams;
    const unsigned char* bytes;
    int* stat;                     // one word per image
    short* coef;                   // per image coef_stride int16
    unsigned long long coef_stride;
    // the multi-window streams (window_count >= min_windows > 0), decoded by the spec / chain / write kernels and skipped by K1
    const DecWindow* windows;
    const DecChain* chains;
    LaneRec* recs;                 // kLanes per window
    WinHead* heads;                // one per window
    unsigned min_windows;          // 0: K1 decodes every long stream
    // a progressive file has a record per scan; a launch covers the records of ONE dependency level (they lie one behind the other)
    unsigned unit0, win0, chain0;  // the level's first record / window / chain: added to the block index
    uint64_t* masks;               // AC refinement scans: per block its non-zero mask (zig-zag order, the band only) ...
    unsigned* wrecs;               // ... and its walk record, both from the record's walk0 on
};

__device__ __forceinline__ void load_image(const DecBatch& b, unsigned img, DecImage* s_im, DecTable* s_tabs, unsigned t) {
    const unsigned* si = reinterpret_cast<const unsigned*>(b.images + img);
    unsigned* di = reinterpret_cast<unsigned*>(s_im);
    for (unsigned k = t; k < sizeof(DecImage) / 4; k += kThreads) di[k] = si[k];
    const unsigned* st = reinterpret_cast<const unsigned*>(b.tabs + 8ull * img);
    unsigned* dt = reinterpret_cast<unsigned*>(s_tabs);
    for (unsigned k = t; k < 8 * sizeof(DecTable) / 4; k += kThreads) dt[k] = st[k];
    __syncthreads();
}
static_assert(sizeof(DecImage) % 4 == 0 && sizeof(DecTable) % 4 == 0, "copied as dwords");

// K1.  blockIdx.x: the image's long stream, blockIdx.y: the image.
__global__ __launch_bounds__(kThreads) void jpeg_dec_long_kernel(DecBatch b) {
    __shared__ unsigned s_words[kStagePadded];
    __shared__ DecTable s_tabs[8];
    __shared__ DecImage s_im;
    __shared__ unsigned s_endp[2][kLanes], s_endbk[2][kLanes];
    __shared__ unsigned s_scan[4][kWaves];
    __shared__ unsigned s_final, s_err;
    const unsigned t = threadIdx.x, unit = b.unit0 + blockIdx.y, lane = t & 63u, wv = t >> 6;
    if (blockIdx.x >= b.images[unit].nlong) return;
    load_image(b, unit, &s_im, s_tabs, t);
    const unsigned img = s_im.slot;
    const DecStream sr = b.streams[s_im.first_long + blockIdx.x];
    if (b.min_windows && window_count(sr.len) >= b.min_windows) return;          // the window-parallel kernels' stream
    const unsigned char* bytes = b.bytes + sr.off;
    short* coef = b.coef + (unsigned long long)img * b.coef_stride;
    const unsigned total_bits = 8u * sr.len, total_blocks = sr.nmcu * s_im.bpm, gblk0 = sr.mcu0 * s_im.bpm;
    if (t == 0) { s_final = kBadPos; s_err = 0; }
    DecState carry{0, 0, 0};
    unsigned done = 0, dcc[3] = {0, 0, 0};
    for (unsigned win0 = 0; win0 < total_bits; win0 += kWindowBits) {
        __syncthreads();                                            // the window before is read no more
        for (unsigned k = t; k < kStageWords; k += kThreads) s_words[k + (k >> 5)] = stream_word(bytes, sr.len, win0 / 32 + k);
        __syncthreads();
        const WordReader rd{s_words, win0};
        // the lanes whose subsequence begins inside the stream (a lane behind its end would only hand a state on, one lane per round)
        const unsigned left = (total_bits - win0 + kSubseqBits - 1) / kSubseqBits, nl = left < (unsigned)kLanes ? left : (unsigned)kLanes;
        const bool active = t < nl;
        const unsigned e = win0 + (t + 1) * kSubseqBits, lim = e < total_bits ? e : total_bits;
        DecState start = t == 0 ? carry : DecState{win0 + t * kSubseqBits, 0, 0};
        DecState end = start;
        LaneOut lo{0, {0, 0, 0}};
        if (active) dec_subseq(rd, s_tabs, s_im, end, lim, 0xffffffffu, (short*)nullptr, 0, nullptr, lo);
        s_endp[0][t] = end.p; s_endbk[0][t] = end.blk << 8 | end.k;
        unsigned cur = 0;
        __syncthreads();                                            // round 0's end states are written
        for (int round = 1; round <= kLanes; ++round) {             // after round k the first k + 1 lanes are exact; ONE barrier per round:
            int changed = 0;                                        // a round reads buffer `cur` and writes the other one
            if (active && t > 0) {
                const unsigned pp = s_endp[cur][t - 1], pbk = s_endbk[cur][t - 1];
                if (pp != start.p || pbk != (start.blk << 8 | start.k)) {
                    start = DecState{pp, pbk >> 8, pbk & 255u};
                    end = start;
                    dec_subseq(rd, s_tabs, s_im, end, lim, 0xffffffffu, (short*)nullptr, 0, nullptr, lo);
                    changed = 1;
                }
            }
            cur ^= 1u;
            s_endp[cur][t] = end.p; s_endbk[cur][t] = end.blk << 8 | end.k;
            if (!__syncthreads_or(changed)) break;
        }
        // prefix sums over the lanes: completed blocks, and the DC differences per component
        unsigned v[4] = {lo.nblk, lo.dc[0], lo.dc[1], lo.dc[2]}, own[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            own[q] = v[q];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(v[q], off, 64); if ((int)lane >= off) v[q] += o; }
            if (lane == 63) s_scan[q][wv] = v[q];
        }
        __syncthreads();
        unsigned before[4], all[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            before[q] = v[q] - own[q]; all[q] = 0;
#pragma unroll
            for (unsigned k = 0; k < (unsigned)kWaves; ++k) { const unsigned x = s_scan[q][k]; if (k < wv) before[q] += x; all[q] += x; }
        }
        // the writing pass: every lane from its settled start state, its first block and its DC predictors now known
        const unsigned first = done + before[0], room = total_blocks > first ? total_blocks - first : 0;
        unsigned dcpred[4] = {dcc[0] + before[1], dcc[1] + before[2], dcc[2] + before[3], 0};
        unsigned err = 0;
        int fin = 0;
        if (active) {
            DecState st = start;
            LaneOut w;
            err = dec_subseq(rd, s_tabs, s_im, st, lim, room, coef, gblk0 + first, dcpred, w);
            if (w.nblk && first + w.nblk == total_blocks) { s_final = st.p; fin = 1; }
            if (err) atomicOr(&s_err, err);
        }
        done += all[0]; dcc[0] += all[1]; dcc[1] += all[2]; dcc[2] += all[3];
        carry = DecState{s_endp[cur][nl - 1], s_endbk[cur][nl - 1] >> 8, s_endbk[cur][nl - 1] & 255u};
        if (__syncthreads_or((int)err | fin)) break;
    }
    __syncthreads();
    if (t == 0) {
        unsigned err = s_err;
        if (!err && !stream_end_ok(s_final, sr.len)) err = kStBadEnd;
        if (err) atomicOr(&b.stat[img], (int)err);
    }
}

// ---- long streams of several windows: three launches, every window a workgroup (jpeg_dec_core.hpp says why this is exact) ----------

// inclusive scans over the workgroup of four values per thread -> what lies before this thread (before) and the totals (all)
__device__ __forceinline__ void block_scan4(const unsigned (&in)[4], unsigned (*s_scan)[kWaves], unsigned (&before)[4], unsigned (&all)[4]) {
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    unsigned v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = in[q];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(v[q], off, 64); if ((int)lane >= off) v[q] += o; }
        if (lane == 63) s_scan[q][wv] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        before[q] = v[q] - in[q]; all[q] = 0;
#pragma unroll
        for (unsigned k = 0; k < (unsigned)kWaves; ++k) { const unsigned x = s_scan[q][k]; if (k < wv) before[q] += x; all[q] += x; }
    }
}

// A.  blockIdx.x: the window.  K1's rounds on one window whose lane 0 starts from a guess; the settled lanes to the window's records.
__global__ __launch_bounds__(kThreads) void jpeg_dec_spec_kernel(DecBatch b) {
    __shared__ unsigned s_words[kStagePadded];
    __shared__ DecTable s_tabs[8];
    __shared__ DecImage s_im;
    __shared__ unsigned s_endp[2][kLanes], s_endbk[2][kLanes];
    const unsigned t = threadIdx.x, wi = b.win0 + blockIdx.x;
    const DecWindow wn = b.windows[wi];
    load_image(b, wn.image, &s_im, s_tabs, t);
    const DecStream sr = b.streams[wn.stream];
    const unsigned char* bytes = b.bytes + sr.off;
    const unsigned total_bits = 8u * sr.len, win0 = wn.win0;
    for (unsigned k = t; k < kStageWords; k += kThreads) s_words[k + (k >> 5)] = stream_word(bytes, sr.len, win0 / 32 + k);
    __syncthreads();
    const WordReader rd{s_words, win0};
    const unsigned nl = window_lanes(total_bits, win0), lim = lane_lim(total_bits, win0, t);
    const bool active = t < nl;
    DecState start = spec_start(win0, t);
    DecState end = start;
    LaneOut lo{0, {0, 0, 0}};
    if (active) dec_subseq(rd, s_tabs, s_im, end, lim, 0xffffffffu, (short*)nullptr, 0, nullptr, lo);
    s_endp[0][t] = end.p; s_endbk[0][t] = state_bk(end);
    unsigned cur = 0;
    __syncthreads();
    for (int round = 1; round <= kLanes; ++round) {                 // bounded by the lane count, as in K1
        int changed = 0;
        if (active && t > 0) {
            const unsigned pp = s_endp[cur][t - 1], pbk = s_endbk[cur][t - 1];
            if (pp != start.p || pbk != state_bk(start)) {
                start = state_of(pp, pbk);
                end = start;
                dec_subseq(rd, s_tabs, s_im, end, lim, 0xffffffffu, (short*)nullptr, 0, nullptr, lo);
                changed = 1;
            }
        }
        cur ^= 1u;
        s_endp[cur][t] = end.p; s_endbk[cur][t] = state_bk(end);
        if (!__syncthreads_or(changed)) break;
    }
    if (active) b.recs[(unsigned long long)wi * kLanes + t] = LaneRec{start.p, state_bk(start), end.p, state_bk(end), lo};
}

// B.  blockIdx.x: the multi-window stream.  Thread 0 carries the true state through the stream's windows (chain_lane, one lane's bits
// staged into LDS by the workgroup); the workgroup sums each window's settled counts into the head of the next one.
__global__ __launch_bounds__(kThreads) void jpeg_dec_chain_kernel(DecBatch b) {
    __shared__ unsigned s_words[kChainStagePadded];
    __shared__ DecTable s_tabs[8];
    __shared__ DecImage s_im;
    __shared__ unsigned s_scan[4][kWaves];
    __shared__ unsigned s_go, s_bit0;
    const unsigned t = threadIdx.x;
    const DecChain ch = b.chains[b.chain0 + blockIdx.x];
    load_image(b, ch.image, &s_im, s_tabs, t);
    const DecStream sr = b.streams[ch.stream];
    const unsigned char* bytes = b.bytes + sr.off;
    const unsigned total_bits = 8u * sr.len, total_blocks = sr.nmcu * s_im.bpm;
    DecState carry{0, 0, 0};                                        // thread 0's: the true state in front of the next lane
    unsigned done = 0, dcc[3] = {0, 0, 0};
    for (unsigned wi = 0; wi < ch.nwin; ++wi) {                      // nwin = window_count(sr.len): the host built both from the same length
        const unsigned win0 = wi * kWindowBits, nl = window_lanes(total_bits, win0);
        LaneRec* recs = b.recs + (unsigned long long)(ch.first + wi) * kLanes;
        if (t == 0) b.heads[ch.first + wi] = WinHead{done, {dcc[0], dcc[1], dcc[2]}};
        for (unsigned l = 0; l < nl; ++l) {                         // until a lane's recorded start is the true one; all of them at the worst
            if (t == 0) {
                const bool same = recs[l].sp == carry.p && recs[l].sbk == state_bk(carry);
                // (carry.p is never in front of lane l's first bit, where the staged words begin: the soft loop of the lane before
                // ended at or behind its own last bit)
                s_bit0 = win0 + l * kSubseqBits;
                s_go = !same && carry.p >= s_bit0;
                if (carry.p < s_bit0) atomicOr(&b.stat[s_im.slot], kStBadCode);          // never: flagged, not guessed
            }
            __syncthreads();
            if (!s_go) break;
            if (t < kChainStageWords) s_words[t + (t >> 5)] = stream_word(bytes, sr.len, s_bit0 / 32 + t);
            __syncthreads();
            if (t == 0) chain_lane(WordReader{s_words, s_bit0}, s_tabs, s_im, lane_lim(total_bits, win0, l), recs[l], carry);
            __syncthreads();                                        // s_go, s_words and recs[l] are read no more / written
        }
        __syncthreads();                                            // thread 0's records are written
        unsigned v[4] = {0, 0, 0, 0}, before[4], all[4];
        if (t < nl) { const LaneOut o = recs[t].o; v[0] = o.nblk; v[1] = o.dc[0]; v[2] = o.dc[1]; v[3] = o.dc[2]; }
        block_scan4(v, s_scan, before, all);
        done += all[0]; dcc[0] += all[1]; dcc[1] += all[2]; dcc[2] += all[3];
        if (t == 0) carry = state_of(recs[nl - 1].ep, recs[nl - 1].ebk);
        __syncthreads();                                            // s_scan is read no more
    }
    if (t == 0 && done < total_blocks) atomicOr(&b.stat[s_im.slot], kStBadEnd);      // blocks missing
}

// C.  blockIdx.x: the window.  K1's writing pass from every lane's settled start.
__global__ __launch_bounds__(kThreads) void jpeg_dec_write_kernel(DecBatch b) {
    __shared__ unsigned s_words[kStagePadded];
    __shared__ DecTable s_tabs[8];
    __shared__ DecImage s_im;
    __shared__ unsigned s_scan[4][kWaves];
    const unsigned t = threadIdx.x, wi = b.win0 + blockIdx.x;
    const DecWindow wn = b.windows[wi];
    load_image(b, wn.image, &s_im, s_tabs, t);
    const DecStream sr = b.streams[wn.stream];
    const unsigned char* bytes = b.bytes + sr.off;
    short* coef = b.coef + (unsigned long long)s_im.slot * b.coef_stride;
    const unsigned total_bits = 8u * sr.len, total_blocks = sr.nmcu * s_im.bpm, gblk0 = sr.mcu0 * s_im.bpm, win0 = wn.win0;
    for (unsigned k = t; k < kStageWords; k += kThreads) s_words[k + (k >> 5)] = stream_word(bytes, sr.len, win0 / 32 + k);
    const unsigned nl = window_lanes(total_bits, win0), lim = lane_lim(total_bits, win0, t);
    const bool active = t < nl;
    LaneRec r{0, 0, 0, 0, {0, {0, 0, 0}}};
    if (active) r = b.recs[(unsigned long long)wi * kLanes + t];
    const WinHead hd = b.heads[wi];
    const unsigned v[4] = {r.o.nblk, r.o.dc[0], r.o.dc[1], r.o.dc[2]};
    unsigned before[4], all[4];
    block_scan4(v, s_scan, before, all);                            // (its barrier also ends the staging)
    const WordReader rd{s_words, win0};
    const unsigned first = hd.done + before[0], room = total_blocks > first ? total_blocks - first : 0;
    unsigned dcpred[4] = {hd.dc[0] + before[1], hd.dc[1] + before[2], hd.dc[2] + before[3], 0};
    if (active) {
        DecState st = state_of(r.sp, r.sbk);
        LaneOut w;
        unsigned err = dec_subseq(rd, s_tabs, s_im, st, lim, room, coef, gblk0 + first, dcpred, w);
        if (!err && w.nblk && first + w.nblk == total_blocks && !stream_end_ok(st.p, sr.len)) err = kStBadEnd;     // bytes left over
        if (err) atomicOr(&b.stat[s_im.slot], (int)err);
    }
}

// K2.  one lane per short stream of image blockIdx.y, in a strided loop
__global__ __launch_bounds__(kThreads) void jpeg_dec_short_kernel(DecBatch b) {
    __shared__ DecTable s_tabs[8];
    __shared__ DecImage s_im;
    const unsigned t = threadIdx.x, unit = b.unit0 + blockIdx.y;
    if (b.images[unit].kind >= kScanDcRefine || blockIdx.x * kThreads >= b.images[unit].nshort) return;       // (a refinement scan's streams are no lanes' work)
    load_image(b, unit, &s_im, s_tabs, t);
    const unsigned img = s_im.slot;
    short* coef = b.coef + (unsigned long long)img * b.coef_stride;
    unsigned err = 0;
    for (unsigned s = blockIdx.x * kThreads + t; s < s_im.nshort; s += gridDim.x * kThreads) {
        const DecStream sr = b.streams[s_im.first_short + s];
        const ByteReader rd{b.bytes + sr.off, sr.len};
        DecState st{0, 0, 0};
        unsigned dcpred[4] = {0, 0, 0, 0};
        LaneOut o;
        unsigned e = dec_subseq(rd, s_tabs, s_im, st, 8u * sr.len, sr.nmcu * s_im.bpm, coef, sr.mcu0 * s_im.bpm, dcpred, o);
        if (!e && !(o.nblk == sr.nmcu * s_im.bpm && stream_end_ok(st.p, sr.len))) e = kStBadEnd;
        err |= e;
    }
    if (err) atomicOr(&b.stat[img], (int)err);
}

// ---- the refinement scans of a progressive file (jpeg_dec_core.hpp says how an AC refinement scan is split) -------------------------
// A refinement scan's streams lie in scan order from first_short on (none is "long"); restart intervals count the scan's own MCUs,
// so block g of the scan belongs to stream g / (interval's blocks), and the interval is stream 0's own block count.

// DC refinement: one thread per block of the scan; bit n of a stream is its block n.  blockIdx.y: the record within the level.
__global__ __launch_bounds__(kThreads) void jpeg_dec_dcref_kernel(DecBatch b) {
    const DecImage& im = b.images[b.unit0 + blockIdx.y];
    if (im.kind != kScanDcRefine) return;
    const unsigned g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= im.nblocks) return;
    const unsigned per = b.streams[im.first_short].nmcu * im.bpm, si = g / per, n = g - si * per;
    if (si >= im.nshort) return;
    const DecStream sr = b.streams[im.first_short + si];
    if (n >= sr.nmcu * im.bpm) return;
    if (n == 0 && !stream_end_ok(sr.nmcu * im.bpm, sr.len)) atomicOr(&b.stat[im.slot], kStBadEnd);
    const unsigned byte = n >> 3;
    if (byte < sr.len && ((b.bytes[sr.off + byte] >> (7u - (n & 7u))) & 1u)) {
        short* c = b.coef + (unsigned long long)im.slot * b.coef_stride + block_base(im, g);
        *c = (short)(*c | (1 << im.al));
    }
}

// AC refinement, the masks: one wave per block of the scan's plane, lane j looks at zig-zag position j.
__global__ __launch_bounds__(kThreads) void jpeg_dec_mask_kernel(DecBatch b) {
    const DecImage& im = b.images[b.unit0 + blockIdx.y];
    if (im.kind != kScanAcRefine) return;
    const unsigned lane = threadIdx.x & 63u, g = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g >= im.nblocks) return;                                    // (the whole wave)
    const short* blk = b.coef + (unsigned long long)im.slot * b.coef_stride + block_base(im, g);
    const bool nz = lane >= im.ss && lane <= im.se && blk[natural_of(lane)] != 0;
    const uint64_t m = __ballot(nz);
    if (lane == 0) b.masks[im.walk0 + g] = m;
}

// AC refinement, the walk of the short streams (at most kShortMaxBytes, as K2's): one lane per stream, over symbols and masks alone;
// a record per block.
__global__ __launch_bounds__(kThreads) void jpeg_dec_walk_kernel(DecBatch b) {
    const DecImage& im = b.images[b.unit0 + blockIdx.y];
    if (im.kind != kScanAcRefine) return;
    const unsigned si = blockIdx.x * kThreads + threadIdx.x;
    if (si >= im.nshort) return;
    const DecStream sr = b.streams[im.first_short + si];
    if (sr.len > kShortMaxBytes) return;                            // jpeg_dec_walk_long_kernel's
    const unsigned c = im.comp_of[0] & 3u, g0 = sr.mcu0, nblk = sr.mcu0 < im.nblocks ? min(sr.nmcu, im.nblocks - sr.mcu0) : 0u;
    const DecTable& tab = b.tabs[8ull * (b.unit0 + blockIdx.y) + 4u + (im.ac_tab[c] & 3u)];
    const ByteReader rd{b.bytes + sr.off, sr.len};
    const unsigned err = refine_walk_stream(rd, tab, im.ss, im.se, b.masks + im.walk0 + g0, b.wrecs + im.walk0 + g0, nblk, sr.len);
    if (err) atomicOr(&b.stat[im.slot], (int)err);
}

// The walk of a longer stream: one WAVE (a workgroup of 64) per stream.  Lane 0 walks; in turns all 64 lanes stage the next
// kWalkBlocks masks (lane i block i's: 512 bytes in one go) and the next kWalkWords stream words into LDS, so that the walking lane
// never waits for a load of its own, and write the turn's records.  blockIdx.x: the stream of the scan, blockIdx.y: the record.
__global__ __launch_bounds__(64) void jpeg_dec_walk_long_kernel(DecBatch b) {
    __shared__ uint64_t s_mask[kWalkBlocks];
    __shared__ unsigned s_rec[kWalkBlocks];
    __shared__ unsigned s_words[kWalkStagePadded];
    __shared__ DecTable s_tab;
    __shared__ unsigned s_n, s_p, s_err;
    const DecImage& im = b.images[b.unit0 + blockIdx.y];
    if (im.kind != kScanAcRefine || blockIdx.x >= im.nshort) return;
    const DecStream sr = b.streams[im.first_short + blockIdx.x];
    if (sr.len <= kShortMaxBytes) return;
    const unsigned lane = threadIdx.x, c = im.comp_of[0] & 3u, ss = im.ss, se = im.se;
    const unsigned nblk = sr.mcu0 < im.nblocks ? min(sr.nmcu, im.nblocks - sr.mcu0) : 0u, total_bits = 8u * sr.len;
    const uint64_t* masks = b.masks + im.walk0 + sr.mcu0;
    unsigned* recs = b.wrecs + im.walk0 + sr.mcu0;
    const unsigned char* bytes = b.bytes + sr.off;
    {
        const unsigned* st = reinterpret_cast<const unsigned*>(b.tabs + 8ull * (b.unit0 + blockIdx.y) + 4u + (im.ac_tab[c] & 3u));
        unsigned* dt = reinterpret_cast<unsigned*>(&s_tab);
        for (unsigned k = lane; k < sizeof(DecTable) / 4; k += 64) dt[k] = st[k];
    }
    RefState st{0, 0, 0};                                           // lane 0's
    unsigned n = 0, mb = 0, p = 0, err = 0;                         // the next block | the staged masks' first block | st.p and the error, known to all
    while (n < nblk && !err) {                                      // (uniform: n, p and err come out of LDS)
        const unsigned bit0 = p & ~31u, nend = min(mb + kWalkBlocks, nblk);
        __syncthreads();                                            // the turn before is read no more
        s_mask[lane] = mb + lane < nblk ? masks[mb + lane] : 0ull;
        for (unsigned k = lane; k < kWalkStageWords; k += 64) s_words[k + (k >> 5)] = stream_word(bytes, sr.len, bit0 / 32 + k);
        __syncthreads();
        if (lane == 0) {
            unsigned nn = n;
            const unsigned e = refine_walk_some(WordReader{s_words, bit0}, s_tab, ss, se, s_mask, s_rec, mb, nend, bit0 + 32u * kWalkWords, total_bits, st, nn);
            s_n = nn; s_p = st.p; s_err = e;
        }
        __syncthreads();
        n = s_n; p = s_p; err = s_err;
        // every record of this turn's blocks that has begun: up to block n, and block n itself when the walk stopped inside it (an
        // error, or the staged words ran out: its record was written when it began, in this turn or in one before -- then again the same)
        if (n == nend || err) {
            if (mb + lane < n || (mb + lane == n && n < nblk && err)) recs[mb + lane] = s_rec[lane];
            if (n == nend) mb = nend;
        }
    }
    if (err) for (unsigned j = n + 1 + lane; j < nblk; j += 64) recs[j] = kBadPos;
    if (lane == 0) {
        if (!err) err = refine_walk_end(st, sr.len);
        if (err) atomicOr(&b.stat[im.slot], (int)err);
    }
}

// AC refinement, every block by itself from its record: one thread per block.
__global__ __launch_bounds__(kThreads) void jpeg_dec_apply_kernel(DecBatch b) {
    const DecImage& im = b.images[b.unit0 + blockIdx.y];
    if (im.kind != kScanAcRefine) return;
    const unsigned g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= im.nblocks) return;
    const unsigned per = b.streams[im.first_short].nmcu, si = g / per;
    if (si >= im.nshort) return;
    const DecStream sr = b.streams[im.first_short + si];
    if (g < sr.mcu0 || g - sr.mcu0 >= sr.nmcu) return;
    const unsigned c = im.comp_of[0] & 3u;
    const DecTable& tab = b.tabs[8ull * (b.unit0 + blockIdx.y) + 4u + (im.ac_tab[c] & 3u)];
    const ByteReader rd{b.bytes + sr.off, sr.len};
    short* blk = b.coef + (unsigned long long)im.slot * b.coef_stride + block_base(im, g);
    refine_apply_block(rd, tab, im.ss, im.se, im.al, b.masks[im.walk0 + g], b.wrecs[im.walk0 + g], blk);
}

// ---- libjpeg's "islow" inverse DCT (jidctint.c): 13-bit constants, 2 extra bits kept between the passes -----------------------------
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633;
constexpr int F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

// In 64 bit, as jidctint.c's JLONG is: any int16 coefficient times any 8-bit table entry stays exact (< 2^47), so a well-formed
// stream with absurd values has defined results; what passes between the passes fits 32 bits (< 2^29).
template <int kShift>
__device__ __forceinline__ void idct_1d(long long* d) {
    long long z1 = (d[2] + d[6]) * F_0_541196100;
    const long long e2 = z1 - d[6] * F_1_847759065, e3 = z1 + d[2] * F_0_765366865;
    const long long e0 = (d[0] + d[4]) * (1 << 13), e1 = (d[0] - d[4]) * (1 << 13);
    const long long t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    long long t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    long long z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const long long z5 = (z3 + z4) * F_1_175875602;
    t0 *= F_0_298631336; t1 *= F_2_053119869; t2 *= F_3_072711026; t3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr long long r = 1ll << (kShift - 1);
    d[0] = (t10 + t3 + r) >> kShift; d[7] = (t10 - t3 + r) >> kShift;
    d[1] = (t11 + t2 + r) >> kShift; d[6] = (t11 - t2 + r) >> kShift;
    d[2] = (t12 + t1 + r) >> kShift; d[5] = (t12 - t1 + r) >> kShift;
    d[3] = (t13 + t0 + r) >> kShift; d[4] = (t13 - t0 + r) >> kShift;
}

constexpr int kIdctBlocks = kThreads / 8;     // blocks per workgroup
constexpr int kPlane = 72;                    // ints per block in LDS: rows of 9

// K3.  blockIdx.x: 32 blocks of the image's coefficient scratch (all components, in its order), blockIdx.y: the image.
// A component's plane lies at 64 x its coef_off bytes, gridw * 8 samples per row.
__global__ __launch_bounds__(kThreads) void jpeg_dec_idct_kernel(DecBatch b, unsigned char* __restrict__ planes, unsigned long long plane_stride) {
    __shared__ int s_ws[kIdctBlocks * kPlane];
    const unsigned t = threadIdx.x, img = blockIdx.y, lb = t >> 3, q = t & 7u;
    const DecImage& im = b.images[img];
    const unsigned nc = (unsigned)im.ncomp, nb = im.coef_off[nc - 1] + im.gridw[nc - 1] * im.gridh[nc - 1];
    const unsigned g = blockIdx.x * kIdctBlocks + lb;
    if (blockIdx.x * kIdctBlocks >= nb) return;
    const bool valid = g < nb;
    unsigned c = 0;
    for (unsigned k = 1; k < nc; ++k) if (g >= im.coef_off[k]) c = k;
    long long d[8];
    bool odd = false;                                             // kStBadRange
    if (valid) {                                                  // columns: coefficient x table entry, (x + 2^10) >> 11
        const short* in = b.coef + (unsigned long long)img * b.coef_stride + (unsigned long long)g * 64 + q;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int v = (int)in[8 * r] * (int)im.quant[c][8 * r + q];
            odd |= v < -32768 || v > 32767;
            d[r] = v;
        }
        idct_1d<11>(d);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[lb * kPlane + r * 9 + q] = (int)d[r];
    }
    __syncthreads();
    if (!valid) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = s_ws[lb * kPlane + q * 9 + k];
    idct_1d<18>(d);                                               // rows: (x + 2^17) >> 18, then libjpeg's range limit
    unsigned long long out = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        odd |= d[k] < -512 || d[k] > 511;
        int v = (int)(d[k] & 1023);
        if (v >= 512) v -= 1024;
        v += 128;
        v = v < 0 ? 0 : v > 255 ? 255 : v;
        out |= (unsigned long long)v << (8 * k);
    }
    if (odd) atomicOr(&b.stat[img], kStBadRange);
    const unsigned l = g - im.coef_off[c], brow = l / im.gridw[c], bcol = l - brow * im.gridw[c];
    unsigned char* p = planes + (unsigned long long)img * plane_stride + 64ull * im.coef_off[c] + (unsigned long long)(brow * 8 + q) * (im.gridw[c] * 8) + bcol * 8;
    *reinterpret_cast<unsigned long long*>(p) = out;              // (8-byte aligned: every term is a multiple of 8)
}

// which image of the output, and which status word, file i of the batch becomes (the batcher's slots: a file's place in its slot)
struct DecDst { unsigned char at[64]; };
// K4.  one thread per pixel
__global__ __launch_bounds__(kThreads) void jpeg_dec_colour_kernel(DecBatch b, const unsigned char* __restrict__ planes, unsigned long long plane_stride,
                                                                   unsigned char* __restrict__ rgb, unsigned long long image_pitch, int h, int w, int* __restrict__ d_status,
                                                                   DecDst dst) {
    const unsigned img = blockIdx.y, out = dst.at[img];
    const unsigned long long idx = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx == 0) d_status[out] = b.stat[img];
    if (idx >= (unsigned long long)h * w) return;
    const DecImage& im = b.images[img];
    const unsigned y = (unsigned)(idx / (unsigned)w), x = (unsigned)(idx - (unsigned long long)y * (unsigned)w);
    const unsigned char* base = planes + (unsigned long long)img * plane_stride;
    const int Y = base[(unsigned long long)y * (im.gridw[0] * 8) + x];
    unsigned char* o = rgb + (unsigned long long)out * image_pitch + idx * 3;
    if (im.sampling == 3) { o[0] = o[1] = o[2] = (unsigned char)Y; return; }
    int cc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned char* P = base + 64ull * im.coef_off[k + 1];
        const unsigned pitch = im.gridw[k + 1] * 8, cw = im.pw[k + 1], ch = im.ph[k + 1];
        if (im.sampling == 0) cc[k] = P[(unsigned long long)y * pitch + x];
        else if (im.sampling == 1) {                              // jdsample.c h2v1_fancy_upsample
            const unsigned char* row = P + (unsigned long long)y * pitch;
            const unsigned i = x >> 1;
            const int a = row[i];
            if (x & 1u) cc[k] = i + 1 < cw ? (3 * a + row[i + 1] + 2) >> 2 : a;
            else cc[k] = i > 0 ? (3 * a + row[i - 1] + 1) >> 2 : a;
        } else {                                                  // h2v2_fancy_upsample
            const unsigned r = y >> 1, nr = (y & 1u) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
            const unsigned char *r0 = P + (unsigned long long)r * pitch, *r1 = P + (unsigned long long)nr * pitch;
            const unsigned j = x >> 1, jn = (x & 1u) ? (j + 1 < cw ? j + 1 : j) : (j > 0 ? j - 1 : j);
            const int cs = 3 * r0[j] + r1[j], cn = 3 * r0[jn] + r1[jn];
            cc[k] = (3 * cs + cn + ((x & 1u) ? 7 : 8)) >> 4;
        }
    }
    const int cb = cc[0] - 128, cr = cc[1] - 128;                 // jdcolor.c: F(x) = floor(x * 65536 + 0.5)
    const int R = Y + ((91881 * cr + 32768) >> 16), B = Y + ((116130 * cb + 32768) >> 16), G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    o[0] = (unsigned char)(R < 0 ? 0 : R > 255 ? 255 : R);
    o[1] = (unsigned char)(G < 0 ? 0 : G > 255 ? 255 : G);
    o[2] = (unsigned char)(B < 0 ? 0 : B > 255 ? 255 : B);
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// blocks of one image's coefficient scratch at most, whatever its sampling: three components on the 4:2:0 luma grid
size_t jpeg_dec_blocks(int h, int w) { return jpegdec::coef_blocks(h, w); }
size_t jpeg_dec_coef_bytes(int n, int h, int w) { return up256(4 * (size_t)n) + (size_t)n * jpeg_dec_blocks(h, w) * 128; }
size_t jpeg_dec_plane_bytes(int n, int h, int w) { return (size_t)n * jpeg_dec_blocks(h, w) * 64; }
size_t jpeg_dec_lane_bytes(size_t nwin) { return nwin * (sizeof(LaneRec) * kLanes + sizeof(WinHead)); }

size_t jpeg_dec_walk_bytes(size_t blocks) { return up256(8 * blocks) + 4 * blocks; }

// rooms[i]: the bytes image i's streams take at most in the blob's byte area; nstreams[i], nscans[i]: over all its scans
JpegDecLayout jpeg_dec_layout_rooms(const uint32_t* nstreams, const uint32_t* nscans, const size_t* rooms, int n) {
    JpegDecLayout L;
    size_t ns = 0, nu = 0;
    for (int i = 0; i < n; ++i) { ns += nstreams[i]; nu += nscans[i]; }
    L.images = 0;
    L.tabs = up256(sizeof(DecImage) * nu);
    L.streams = up256(L.tabs + sizeof(DecTable) * 8 * nu);
    // multi-window streams are longer than a window, so a file has at most 8 * stream bytes / kWindowBits of them and twice as many windows
    size_t nc = 0;
    for (int i = 0; i < n; ++i) nc += 8 * rooms[i] / kWindowBits;
    L.chains = up256(L.streams + sizeof(DecStream) * ns);
    L.windows = up256(L.chains + sizeof(DecChain) * nc);
    L.bytes = up256(L.windows + sizeof(DecWindow) * 2 * nc);
    L.total = L.bytes;
    for (int i = 0; i < n; ++i) L.total += up256(rooms[i]);
    L.total += 256;                                               // (what an aligned dword load behind the last stream may touch)
    return L;
}

JpegDecLayout jpeg_dec_layout(const jpegparse::File* f, const size_t* bytes, int n) {
    std::vector<size_t> rooms((size_t)n);
    std::vector<uint32_t> ns((size_t)n), nu((size_t)n);
    for (int i = 0; i < n; ++i) { rooms[(size_t)i] = jpegparse::file_room(f[i], bytes[i]); ns[(size_t)i] = f[i].nstreams; nu[(size_t)i] = f[i].nscans(); }
    return jpeg_dec_layout_rooms(ns.data(), nu.data(), rooms.data(), n);
}

namespace {
// One record ("unit": a baseline file, or one scan of a progressive one) into the blob as record u: its streams (cut already: `first`,
// stream s0 of the batch's table, their offsets moved into the batch's byte area before) with the long ones in front where lanes
// decode them, its image record and tables, the chains and windows of its multi-window streams, and its share of its level's grids.
void pack_unit(uint32_t u, uint32_t slot, DecImage im, const DecTable* const* tabs8, DecStream* first, uint32_t nstreams, uint32_t s0, const JpegDecLayout& L, uint8_t* blob,
               JpegDecLayout& out, JpegDecLevel& lv) {
    DecImage* images = reinterpret_cast<DecImage*>(blob + L.images);
    DecTable* tabs = reinterpret_cast<DecTable*>(blob + L.tabs);
    DecChain* chains = reinterpret_cast<DecChain*>(blob + L.chains);
    DecWindow* windows = reinterpret_cast<DecWindow*>(blob + L.windows);
    const size_t chain_room = (L.windows - L.chains) / sizeof(DecChain), window_room = (L.bytes - L.windows) / sizeof(DecWindow);
    const uint32_t min_windows = out.min_windows;
    im.slot = slot;
    im.first_long = s0;
    if (im.kind >= kScanDcRefine) {                               // no lanes: the streams stay in scan order
        im.nlong = 0;
        if (im.kind == kScanDcRefine) lv.dcref_blocks = std::max(lv.dcref_blocks, im.nblocks);
        else {
            im.walk0 = lv.walk_blocks; lv.walk_blocks += im.nblocks;
            lv.ac_blocks = std::max(lv.ac_blocks, im.nblocks); lv.ac_streams = std::max(lv.ac_streams, nstreams);
            for (uint32_t k = 0; k < nstreams; ++k) (first[k].len > kShortMaxBytes ? lv.ac_long : lv.ac_short) = 1;
        }
    } else {
        DecStream* mid = std::stable_partition(first, first + nstreams, [](const DecStream& s) { return s.len > kShortMaxBytes; });
        im.nlong = (uint32_t)(mid - first);
    }
    im.first_short = im.first_long + im.nlong; im.nshort = nstreams - im.nlong;
    uint32_t k1 = 0;                                              // the last of its long streams that K1 keeps, + 1
    for (uint32_t k = 0; k < im.nlong; ++k) {
        const uint32_t nw = window_count(first[k].len);
        if (!min_windows || nw < std::max(min_windows, 2u)) { k1 = k + 1; continue; }
        if (out.nchain + 1 > chain_room || out.nwin + (size_t)nw > window_room) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's window table overflows");
        chains[out.nchain++] = DecChain{im.first_long + k, u, out.nwin, nw};
        for (uint32_t j = 0; j < nw; ++j) windows[out.nwin++] = DecWindow{im.first_long + k, u, j * kWindowBits};
    }
    lv.max_long = std::max(lv.max_long, k1);
    if (im.kind < kScanDcRefine) lv.max_short = std::max(lv.max_short, im.nshort);
    images[u] = im;
    for (int k = 0; k < 8; ++k) std::memcpy(tabs + 8 * (size_t)u + k, tabs8[k], sizeof(DecTable));
}

// the records of n files whose streams lie in the blob's table in file order (image i's from s_img[i] on, their offsets inside the image's
// own bytes, which begin b_img[i] bytes into the byte area): the first scan of every file in front (records 0 .. n - 1 are the images'
// own: K3 and K4 read the geometry there), then the other scans by dependency level
void pack_units(const jpegparse::File* const* f, int n, const uint32_t* s_img, const size_t* b_img, const JpegDecLayout& L, uint8_t* blob, JpegDecLayout& out) {
    DecStream* streams = reinterpret_cast<DecStream*>(blob + L.streams);
    struct Ref { uint32_t level, img, scan, s0; };
    std::vector<Ref> order;
    uint32_t nlevels = 1;
    for (int i = 0; i < n; ++i) {
        order.push_back(Ref{0, (uint32_t)i, 0, s_img[i]});
        for (uint32_t k = 0; k < f[i]->nstreams; ++k) streams[s_img[i] + k].off += (uint32_t)b_img[i];
    }
    for (int i = 0; i < n; ++i) {
        uint32_t s0 = s_img[i];
        for (uint32_t k = 0; k < f[i]->nscans(); ++k) {
            if (k) order.push_back(Ref{f[i]->scans[k].level, (uint32_t)i, k, s0});
            if (f[i]->progressive) { s0 += f[i]->scans[k].nstreams; nlevels = std::max(nlevels, f[i]->scans[k].level + 1); }
        }
    }
    std::stable_sort(order.begin() + n, order.end(), [](const Ref& a, const Ref& b) { return a.level < b.level; });
    out.levels.assign(nlevels, JpegDecLevel{});
    out.nunits = (uint32_t)order.size();
    out.walk_blocks = 0;
    if ((size_t)out.nunits * sizeof(DecImage) > L.tabs) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's record table overflows");
    for (uint32_t u = 0; u < out.nunits; ++u) {
        const Ref& r = order[u];
        const jpegparse::File& fi = *f[r.img];
        JpegDecLevel& lv = out.levels[r.level];
        if (!lv.nunits) { lv.unit0 = u; lv.win0 = out.nwin; lv.chain0 = out.nchain; }
        ++lv.nunits;
        const DecTable* t8[8];
        if (fi.progressive) {
            const jpegparse::Scan& sc = fi.scans[r.scan];
            if (fi.pool.empty()) fail(IRE_ERR_INTERNAL, "internal: a progressive file without Huffman tables");
            for (int k = 0; k < 8; ++k) t8[k] = &fi.pool[std::min<size_t>(sc.tab[k], fi.pool.size() - 1)];
            pack_unit(u, r.img, sc.im, t8, streams + r.s0, sc.nstreams, r.s0, L, blob, out, lv);
        } else {
            for (int k = 0; k < 8; ++k) t8[k] = &fi.hd.tabs[k];
            pack_unit(u, r.img, fi.hd.im, t8, streams + r.s0, fi.hd.nstreams, r.s0, L, blob, out, lv);
        }
        lv.nwin = out.nwin - lv.win0; lv.nchain = out.nchain - lv.chain0;
        out.walk_blocks = std::max<size_t>(out.walk_blocks, lv.walk_blocks);
    }
}
}  // namespace

// the batch's blob into `blob` (pinned): records, tables, the streams cut and unstuffed.  A file whose scan is refused: Error.
void jpeg_dec_pack(const uint8_t* const* files, const size_t* bytes, const jpegparse::File* f, int n, const JpegDecLayout& L, uint8_t* blob, JpegDecLayout& out,
                   uint32_t min_windows) {
    out = L;
    out.nwin = out.nchain = 0;
    out.min_windows = min_windows;
    DecStream* streams = reinterpret_cast<DecStream*>(blob + L.streams);
    std::vector<uint32_t> s_img((size_t)n);
    std::vector<size_t> b_img((size_t)n);
    std::vector<const jpegparse::File*> fp((size_t)n);
    size_t s0 = 0, b0 = 0;
    for (int i = 0; i < n; ++i) {
        const size_t room = jpegparse::file_room(f[i], bytes[i]);
        std::string why;
        if (!jpegparse::split_file(f[i], files[i], bytes[i], blob + L.bytes + b0, room, streams + s0, why)) fail(IRE_ERR_INVALID_INPUT, why);
        s_img[(size_t)i] = (uint32_t)s0; b_img[(size_t)i] = b0; fp[(size_t)i] = f + i;
        s0 += f[i].nstreams; b0 += up256(room);
    }
    pack_units(fp.data(), n, s_img.data(), b_img.data(), L, blob, out);
}

// the same for files whose scans were cut before (jpegparse::split_file into the caller's own memory): only the records, up to
// L.bytes; byte_off[i] says where image i's bytes belong in the byte area (the caller copies them there, rooms[i] at most)
void jpeg_dec_pack_streams(const jpegparse::File* const* f, const DecStream* const* streams_in, const size_t* rooms, int n, const JpegDecLayout& L, uint8_t* blob,
                           JpegDecLayout& out, size_t* byte_off, uint32_t min_windows) {
    out = L;
    out.nwin = out.nchain = 0;
    out.min_windows = min_windows;
    DecStream* streams = reinterpret_cast<DecStream*>(blob + L.streams);
    std::vector<uint32_t> s_img((size_t)n);
    size_t s0 = 0, b0 = 0;
    for (int i = 0; i < n; ++i) {
        std::copy(streams_in[i], streams_in[i] + f[i]->nstreams, streams + s0);
        s_img[(size_t)i] = (uint32_t)s0; byte_off[i] = b0;
        s0 += f[i]->nstreams; b0 += up256(rooms[i]);
    }
    pack_units(f, n, s_img.data(), byte_off, L, blob, out);
}

void jpeg_dec_launch(const uint8_t* d_blob, const JpegDecLayout& L, int n, int h, int w, uint8_t* d_coef, uint8_t* d_planes, uint8_t* d_lanes, uint8_t* d_walk, uint8_t* d_rgb,
                     size_t image_pitch, int32_t* d_status, hipStream_t s, hipEvent_t* marks, const int* dst) {
    if (n < 1 || n > 64) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's batch is outside 1..64");
    DecDst where;
    for (int i = 0; i < 64; ++i) where.at[i] = (unsigned char)(i < n && dst ? dst[i] : i);
    for (int i = 0; dst && i < n; ++i) if (dst[i] < 0 || dst[i] > 63) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's output index is outside 0..63");
    auto mark = [&](int k) { if (marks) IRE_HIP(hipEventRecord(marks[k], s)); };
    DecBatch b;
    b.images = reinterpret_cast<const DecImage*>(d_blob + L.images);
    b.tabs = reinterpret_cast<const DecTable*>(d_blob + L.tabs);
    b.streams = reinterpret_cast<const DecStream*>(d_blob + L.streams);
    b.bytes = d_blob + L.bytes;
    b.stat = reinterpret_cast<int*>(d_coef);
    b.coef = reinterpret_cast<short*>(d_coef + up256(4 * (size_t)n));
    const size_t blocks = jpeg_dec_blocks(h, w);
    b.coef_stride = blocks * 64;
    b.chains = reinterpret_cast<const DecChain*>(d_blob + L.chains);
    b.windows = reinterpret_cast<const DecWindow*>(d_blob + L.windows);
    b.recs = reinterpret_cast<LaneRec*>(d_lanes);
    b.heads = reinterpret_cast<WinHead*>(d_lanes + sizeof(LaneRec) * kLanes * (size_t)L.nwin);
    b.min_windows = L.nwin ? std::max(L.min_windows, 2u) : 0;
    b.masks = reinterpret_cast<uint64_t*>(d_walk);
    b.wrecs = reinterpret_cast<unsigned*>(d_walk + up256(8 * L.walk_blocks));
    if (L.nwin && !d_lanes) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's lane records are missing");
    if (L.walk_blocks && !d_walk) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's walk records are missing");
    if (L.levels.empty() || L.levels[0].unit0 != 0 || L.levels[0].nunits < (uint32_t)n) fail(IRE_ERR_INTERNAL, "internal: the JPEG decoder's records are out of order");
    mark(0);
    IRE_HIP(hipMemsetAsync(d_coef, 0, jpeg_dec_coef_bytes(n, h, w), s));
    mark(1);
    // One round of launches per dependency level: the scans of a level touch disjoint coefficients.  A batch of baseline files has
    // one level and in it what lanes decode; the marks between the lanes' launches are those of level 0.
    for (size_t li = 0; li < L.levels.size(); ++li) {
        const JpegDecLevel& lv = L.levels[li];
        if (!lv.nunits) continue;
        b.unit0 = lv.unit0; b.win0 = lv.win0; b.chain0 = lv.chain0;
        if (lv.max_long) hipLaunchKernelGGL(jpeg_dec_long_kernel, dim3(lv.max_long, lv.nunits), dim3(kThreads), 0, s, b);
        if (!li) mark(2);
        if (lv.nwin) {
            hipLaunchKernelGGL(jpeg_dec_spec_kernel, dim3(lv.nwin), dim3(kThreads), 0, s, b);
            if (!li) mark(3);
            hipLaunchKernelGGL(jpeg_dec_chain_kernel, dim3(lv.nchain), dim3(kThreads), 0, s, b);
            if (!li) mark(4);
            hipLaunchKernelGGL(jpeg_dec_write_kernel, dim3(lv.nwin), dim3(kThreads), 0, s, b);
        } else if (!li) { mark(3); mark(4); }
        if (!li) mark(5);
        if (lv.max_short) hipLaunchKernelGGL(jpeg_dec_short_kernel, dim3(std::min<uint32_t>((lv.max_short + kThreads - 1) / kThreads, 1024u), lv.nunits), dim3(kThreads), 0, s, b);
        if (!li) mark(6);
        if (lv.dcref_blocks) hipLaunchKernelGGL(jpeg_dec_dcref_kernel, dim3((lv.dcref_blocks + kThreads - 1) / kThreads, lv.nunits), dim3(kThreads), 0, s, b);
        if (lv.ac_blocks) {
            hipLaunchKernelGGL(jpeg_dec_mask_kernel, dim3((lv.ac_blocks + kWaves - 1) / kWaves, lv.nunits), dim3(kThreads), 0, s, b);
            if (lv.ac_short) hipLaunchKernelGGL(jpeg_dec_walk_kernel, dim3((lv.ac_streams + kThreads - 1) / kThreads, lv.nunits), dim3(kThreads), 0, s, b);
            if (lv.ac_long) hipLaunchKernelGGL(jpeg_dec_walk_long_kernel, dim3(lv.ac_streams, lv.nunits), dim3(64), 0, s, b);
            hipLaunchKernelGGL(jpeg_dec_apply_kernel, dim3((lv.ac_blocks + kThreads - 1) / kThreads, lv.nunits), dim3(kThreads), 0, s, b);
        }
    }
    mark(7);                                                       // (6 .. 7: every level behind the first, all of a progressive file's refinement)
    hipLaunchKernelGGL(jpeg_dec_idct_kernel, dim3((unsigned)((blocks + kIdctBlocks - 1) / kIdctBlocks), n), dim3(kThreads), 0, s, b, d_planes, (unsigned long long)(blocks * 64));
    mark(8);
    hipLaunchKernelGGL(jpeg_dec_colour_kernel, dim3((unsigned)(((size_t)h * w + kThreads - 1) / kThreads), n), dim3(kThreads), 0, s, b, d_planes, (unsigned long long)(blocks * 64),
                       d_rgb, (unsigned long long)image_pitch, h, w, d_status, where);
    mark(9);
    IRE_HIP(hipGetLastError());
}

}  // namespace ire
