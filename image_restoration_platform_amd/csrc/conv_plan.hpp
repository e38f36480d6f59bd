// conv_plan.hpp -- the rule book of the convolution launches, on the host; no HIP, no device code.  plan_conv() decides for one
// launch site which of the convolution kernels takes it and with which slabs, chunk counts, tile grid, strip window and
// GroupNorm-partials layout; Engine::exec_conv binds the pointers the plan names and launches.  Everything here is a pure function of
// (switches, convolution, site): tests/native/conv_plan_dump.cpp walks the whole network with plain g++ under the sanitizers.
//
// Three invariants the kernels and the tests lean on:
//   * a result must not depend on the batch around it or on the strip decomposition, so every choice that changes the fp32 order of the
//     GroupNorm partials (64- or 128-cout items, which kernel family) is a function of the IMAGE's shape at that level alone;
//   * conv_pk / conv_pc get only the launches their LDS coefficient table can hold (coef_table_fits);
//   * a strip's tiles land at their GLOBAL tile offset (ty0), so the finalize sees exactly the whole-image partials layout.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "conv_kind.hpp"

namespace ire {

enum Family { FAM_CLASSIFIER = 0, FAM_CONV3 = 1, FAM_CONV1 = 2, FAM_STEM = 3, FAM_HEAD = 4, FAM_GN = 5,
              FAM_FUSION = 6, FAM_COUNT = 7 };

// ---- the A/B switches, each with its default (tests/test_restore_gpu.py and tests/test_layers_gpu.py run every one) ----
struct ConvSwitches {
    int w4_split = 1;            // IRE_W4_SPLIT=0: never use the 64-cout items
    int use_dnq = 1;             // the stride-2 convs with cout >= 128 as all-DMA 128-cout items on conv_dnq.hip (IRE_DNQ=0: conv_down.hip)
    int use_upq = 1;             // the level-2 `up` + `fuse` (cout = 128) as parity-major 128-cout items on conv_upq.hip (IRE_UPQ=0: conv_up.hip)
    int use_pk = 2;              // C >= 128 ResBlock convs (128-cout items, fused activation) on conv_pk.hip's producer / consumer workgroups: 2 = all, 1 = the convs without a residual (IRE_PK=0: conv_w4.hip)
    int use_w4 = 1;              // C >= 128 ResBlock convs on conv_w4.hip (IRE_W4=0: conv_rb.hip)
    int fp8_mx = 1;              // fp8: the block-scaled K = 64 MFMA (conv_f8.hip); IRE_FP8_MX=0: the same-rate 32x32x16 fp8 form in conv_w4.hip
    int down_rb = 1;             // stride-2 `down` convs on conv_down.hip's pipelined phase kernel (IRE_DOWN_RB=0: the v1 kernel)
    int head_rb = 1;             // the 32 -> 3 head conv on conv_rb.hip's pipelined kernel (IRE_HEAD_RB=0: the v1 kernel)
    int pc_split = 3;            // producer / consumer workgroups (conv_pc.hip): bit 0 = C = 32 ResBlock convs + head, bit 1 = C = 64; IRE_PC=0: conv_rb.hip
    int gn_fold = 1;             // GroupNorm finalize inside the consuming conv's prologue (gn_fold.hpp); IRE_GN_FOLD=0: 33 gn_finalize launches per step
    int stem_rb = 1;             // the stem on its own kernel (conv_stem.hip); IRE_STEM_RB=0: the v1 template
    int up_fuse = 1;             // `up` + 1x1 `fuse` as ONE composed convolution with the skip term in conv_up.hip's epilogue (IRE_UP_FUSE=0: two kernels)
    int up_subpixel = 1;         // `up` convs as sub-pixel convolutions on the low-res grid (IRE_UP_SUBPIX=0: nearest x2 + 3x3 on conv_rb.hip)
    int up_rb_min_c = 32;        // `up` convs with cout >= this run on conv_rb.hip (IRE_UP_RB_MINC), the rest on the v1 kernel
    int prio_young = 0;          // static s_setprio for waves 4-7 of conv_rb (A/B'd: it only swaps which half waits)
    int rb_tile_h = kRbTileH;    // 16: persistent pipelined conv_rb.hip; 8: conv_mfma.hip (IRE_CONV_V1=1)

    static ConvSwitches from_env() {
        ConvSwitches s;
        if (const char* v = std::getenv("IRE_CONV_V1")) s.rb_tile_h = (v[0] == '1') ? 8 : kRbTileH;
        if (const char* v = std::getenv("IRE_RB_PRIO")) s.prio_young = std::atoi(v);
        if (const char* v = std::getenv("IRE_W4")) s.use_w4 = std::atoi(v);
        if (const char* v = std::getenv("IRE_W4_SPLIT")) s.w4_split = std::atoi(v);
        if (const char* v = std::getenv("IRE_UP_RB_MINC")) s.up_rb_min_c = std::atoi(v);
        if (const char* v = std::getenv("IRE_UP_SUBPIX")) s.up_subpixel = std::atoi(v);
        if (const char* v = std::getenv("IRE_UP_FUSE")) s.up_fuse = std::atoi(v);
        if (const char* v = std::getenv("IRE_GN_FOLD")) s.gn_fold = std::atoi(v);
        if (const char* v = std::getenv("IRE_PC")) s.pc_split = std::atoi(v);
        if (const char* v = std::getenv("IRE_PK")) s.use_pk = std::atoi(v);
        if (const char* v = std::getenv("IRE_UPQ")) s.use_upq = std::atoi(v);
        if (const char* v = std::getenv("IRE_DNQ")) s.use_dnq = std::atoi(v);
        if (const char* v = std::getenv("IRE_HEAD_RB")) s.head_rb = std::atoi(v);
        if (const char* v = std::getenv("IRE_DOWN_RB")) s.down_rb = std::atoi(v);
        if (const char* v = std::getenv("IRE_STEM_RB")) s.stem_rb = std::atoi(v);
        if (const char* v = std::getenv("IRE_FP8_MX")) s.fp8_mx = std::atoi(v);
        return s;
    }
};

// ---- one convolution: its scalars and which packed arrays exist (weight_pack.hpp::conv_desc; names: PackedConv / ConvW) ----
struct ConvDesc {
    ConvKind kind = CONV_RB1;
    int cin = 0, cout = 0;       // logical channel counts (FLOP accounting)
    int cin0 = 0, cin1 = 0;      // channels per pixel of the two sources
    int nkc = 0, nblocks = 0, kc_split = 0;      // of the v1 slabs (d_w)
    bool w = false, wp = false, w4 = false, w4h = false, wstem = false, wd = false, wu = false, wuf = false, wdq = false, wuq = false,
         wsq = false, wsk = false, bias_uf = false, w8x = false, w8 = false, oscale = false, bias8 = false, bias = false;
};

// ---- one launch site: the op (engine.hpp Op), the piece it runs on (Geo) and the device ----
struct ConvSite {
    int lin = 0, lout = 0;       // levels of in0 / out
    bool use_ab = false;         // GroupNorm+FiLM+SiLU applied while staging in0
    bool has_in1 = false;        // a second source: the skip tensor of `fuse`, or of an `up` composed with it
    bool stats_out = false;      // the conv writes GroupNorm partials of its output
    int nimg = 1, h = 0, w = 0;  // rows / columns of THIS piece at level 0
    int H = 0;                   // global image height (level 0)
    int halo = 0;                // 1: a row strip (one halo row above and below in every buffer)
    bool has_up = false, has_down = false;
    int y0 = 0;                  // first global row of the piece
    int cus = 256;               // persistent_grid_cus(), read once per engine
};

// one value per launch call of Engine::exec_conv
enum ConvKernel { K_V1, K_F8, K_PK, K_W4, K_PC, K_RB, K_PC_HEAD, K_RB_HEAD, K_DNQ, K_DOWN, K_STEM, K_UPQ, K_UP_FUSED, K_UP_SUB, K_UP_RB };
enum WeightArr { W_NONE, W_W, W_WP, W_W4, W_W4H, W_WSTEM, W_WD, W_WU, W_WUF, W_WDQ, W_WUQ, W_WSQ, W_WSK, W_W8X, W_W8 };
enum BiasArr { B_BIAS, B_BIAS_UF, B_BIAS8 };

struct ConvPlan {
    ConvKernel kernel = K_V1;
    bool resid = false;          // CONV_RB2: the launch's `resid` argument
    bool fused_act = false;      // the activation is applied while staging (a.ab bound; conv_rb_launch's `fused_act`)
    const char* kname = "conv_mfma";     // what the profiler reports
    WeightArr w = W_W, w1 = W_NONE;
    BiasArr bias = B_BIAS;
    // ConvArgs scalars
    int nkc = 0, nblocks = 0, w4_nt = 0, fp8 = 0, cin1 = 0, cout = 0, group_size = 1;
    bool zeros = false;          // bind the engine's zero page (conv_upq / conv_dnq: what a DMA lane outside the image fetches)
    bool in1_first_row = false;  // in1 is read at output pixels only: bound at its first real row, not at the buffer start
    // grid and strip window
    int tile_h = 8, tiles_x = 0, tiles_y = 0, iy_lo = 0, iy_span = 0, in_rows = 0, in_row_off = 0;
    // GroupNorm partials of the output (stats_out): [image][global tile][8][2], parts_mul rows per tile
    int parts_mul = 1, stats_level = -1, ty0 = 0, stat_parts = 0;
    bool folds_gn = false;       // this kernel finalizes its input's GroupNorm in its prologue (gn_fold.hpp)
    // profiler
    int fam = FAM_CONV3;
    char key[12] = "conv";       // layer group: "stem", "L2.rb1", "down0", "up1", "fuse0", "head"
    double flops = 0, flops_exec = 0, bytes = 0;

    long long stats_offset() const { return (long long)ty0 * tiles_x * 16 * parts_mul; }     // floats in front of this piece's partials
};

// ---- the producer / consumer kernels' coefficient tables: images whose (A, B) the LDS table of a workgroup holds ----
constexpr int PK_IMGS = 4;                                               // conv_pk.hip
constexpr int pc_coef_imgs(int C) { return C == 32 ? 64 : 8; }          // conv_pc.hip
// Every workgroup's items must stay within imgs_cap images: the workgroups of XCD group x walk items [items x / X, items (x + 1) / X)
// (persist.hpp); a range may not span more images than the table holds.
inline bool coef_table_fits(int imgs_cap, long long items_per_img, int nimg, int cus) {
    if (nimg <= imgs_cap) return true;
    const long long ipi = items_per_img, items = ipi * nimg;
    const long long G = items < cus ? items : cus, X = G < 8 ? G : 8;
    for (long long x = 0; x < X; ++x) {
        const long long lo = items * x / X, hi = items * (x + 1) / X;
        if (hi > lo && (hi - 1) / ipi - lo / ipi + 1 > imgs_cap) return false;
    }
    return true;
}

// ---- the address rule: what 32-bit byte offsets reach (DESIGN.md "Address arithmetic at the largest shapes") ----
// A convolution addresses ONE image's tensor -- of a row strip: the strip's rows and its two halo rows -- with a 64-bit base and an unsigned
// 32-bit byte offset per lane, and range-checks the offset against a buffer resource whose size is 32 bits too; the offset 0xffffffff is how
// a chunk outside the image asks for its zero padding.  Images of a batch lie a 64-bit stride apart: the batch size is no part of the rule.
// So a piece runs iff every tensor of it is smaller than 2^32 bytes.  The largest is level 0 (32 channels of bf16: 64 bytes a pixel): among
// whole images of at most 8192 a side the rule refuses 8192 x 8192 alone (2^26 pixels = 2^32 bytes exactly), which still runs in row strips.
constexpr unsigned long long kTensorBytesEnd = 1ull << 32;
inline unsigned long long piece_tensor_bytes(int rows, int w, int halo, int level) {      // rows, w: of the piece at level 0, halo rows excluded
    return (unsigned long long)((rows >> level) + 2 * halo) * (unsigned long long)(w >> level) * (unsigned long long)(kWidths[level] * 2);
}
// (level 0 decides: the bytes halve from level to level, the halo rows do not make up for it)
inline bool piece_addressable(int rows, int w, int halo) { return piece_tensor_bytes(rows, w, halo, 0) < kTensorBytesEnd; }
// h x w: the image as it runs -- for the any-size entries the size padded to multiples of 8, which is what the message names
inline std::string not_addressable(int h, int w) {
    char m[256];
    std::snprintf(m, sizeof m, "invalid image size: a level-0 tensor of the image (height x width x 64 bytes, sides padded to multiples of 8) must stay "
                  "below 2^32 bytes, which %d x %d (%llu bytes) is not; restore it in row strips", h, w, piece_tensor_bytes(h, w, 0, 0));
    return m;
}

// `up` composed with the level's 1x1 `fuse` into one convolution (weight_pack.hpp::pack_up_fused): the schedule then has no `fuse`
// op and the `up` op carries the skip tensor as its second source (Engine::build_program), and the launch is a fused form below.
inline bool up_is_composed(const ConvSwitches& sw, const ConvDesc& d) {
    return d.kind == CONV_UP && sw.rb_tile_h == kRbTileH && sw.up_fuse && sw.up_subpixel && d.wu && d.wuf && d.cout >= sw.up_rb_min_c;
}
// a plain `up` feeds the 1x1 fuse only and the head writes pixels; every other output is read by a 3x3 convolution (strips exchange its
// boundary rows) and by a GroupNorm (its producer writes the partials)
inline bool conv_feeds_gn(ConvKind kind, bool composed) { return (kind != CONV_UP || composed) && kind != CONV_HEAD; }

// (runs on every launch: the layer group is spelled by hand, a formatted print would cost more than the rest of the plan)
inline void plan_key(char* k, const char* head, int digit, const char* tail) {
    while (*head) *k++ = *head++;
    if (digit >= 0) *k++ = (char)('0' + digit);
    while (*tail) *k++ = *tail++;
    *k = 0;
}

inline ConvPlan plan_conv(const ConvSwitches& sw, const ConvDesc& d, const ConvSite& s, bool fp8_engine) {
    auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    const int Hin = s.h >> s.lin, Win = s.w >> s.lin, Hout = s.h >> s.lout, Wout = s.w >> s.lout;
    const bool v2 = sw.rb_tile_h == kRbTileH;        // the pipelined kernels; IRE_CONV_V1=1: everything on the v1 template
    const bool ab = s.use_ab;
    ConvPlan p;
    // what every branch starts from: the v1 template (conv_mfma.hip) on the v1 slabs
    p.resid = d.kind == CONV_RB2; p.fused_act = ab;
    p.nkc = d.nkc; p.nblocks = d.nblocks; p.cin1 = d.cin1;
    p.cout = d.kind == CONV_HEAD ? 32 : d.cout;
    p.group_size = std::max(1, p.cout / 8);
    p.in_rows = Hin + 2 * s.halo; p.in_row_off = s.halo;
    // the readable (virtual) input rows of a strip: the halo row of a neighbouring strip is data, a row outside the image is padding
    auto window = [&](int rows) {
        p.iy_lo = (s.halo && s.has_up) ? -1 : 0;
        p.iy_span = rows + ((s.halo && s.has_down) ? 1 : 0) - p.iy_lo;
    };
    auto grid = [&](int rows, int cols, int th) { p.tile_h = th; p.tiles_x = cdiv(cols, 32); p.tiles_y = cdiv(rows, th); };
    window(d.kind == CONV_UP ? 2 * Hin : Hin);       // nearest x2 folded into the staging
    grid(Hout, Wout, conv_tile_h(d.kind));
    int stats_level = s.lout;

    switch (d.kind) {
    // ---- stem: u8 RGB -> 32 ----
    case CONV_STEM:
        p.fam = FAM_STEM;
        plan_key(p.key, "stem", -1, "");
        if (v2 && sw.stem_rb && d.wstem && s.stats_out) { p.kernel = K_STEM; p.kname = "conv_stem"; p.w = W_WSTEM; grid(Hout, Wout, sw.rb_tile_h); }
        break;

    // ---- ResBlock convs: C -> C, activation fused into the staging ----
    case CONV_RB1:
    case CONV_RB2: {
        plan_key(p.key, "L", s.lout, d.kind == CONV_RB1 ? ".rb1" : ".rb2");
        grid(Hout, Wout, sw.rb_tile_h);
        if (!v2) break;
        p.folds_gn = ab;
        const int tiles = p.tiles_x * p.tiles_y;
        if (sw.use_w4 && d.w4 && ab && d.cout >= 128) {
            // C >= 128: one-wave-per-SIMD items on 16-channel stages (conv_w4.hip) and what shares their slabs
            if (fp8_engine && sw.fp8_mx && d.w8x) {          // the 2x-rate block-scaled fp8 MFMA
                p.kernel = K_F8; p.kname = "conv_f8"; p.fp8 = 1; p.w = W_W8X; p.bias = B_BIAS8; p.nkc = d.cin / 32; p.nblocks = d.cout / 128;
                break;
            }
            p.w = W_W4; p.nkc = d.cin / 16; p.nblocks = d.cout / 128;
            // 64-cout items where 128-cout ones would leave CUs idle (512^2 at level 3): twice the items, each half the MFMAs.  The two
            // forms add the GroupNorm partials of a tile in different fp32 orders, so the choice looks at the IMAGE's shape at this level
            // only -- never at the batch size or the strip.  Rule: a batch of 8 such images would not fill the CUs.
            const int tiles_img = cdiv(s.H >> s.lout, kRbTileH) * cdiv(s.w >> s.lout, 32);
            const bool f8 = fp8_engine && d.w8;              // e4m3 operands on conv_w4.hip (IRE_FP8_MX=0)
            if (sw.w4_split && d.w4h && !f8 && tiles_img * p.nblocks * 8 < 256) { p.w = W_W4H; p.nblocks = d.cout / 64; p.w4_nt = 64; }
            if (f8) { p.fp8 = 1; p.w = W_W8; p.bias = B_BIAS8; }
            // the producer / consumer form (conv_pk.hip) takes the 128-cout bf16 launches whose workgroups stay within its coefficient
            // table, with and without the residual; same slabs, bit-identical results.  conv_w4 keeps fp8, the 64-cout items and the
            // batches the table cannot hold.  (use_pk 1: only the convs without a residual: profiles/r05_experiments.md)
            const bool pk = sw.use_pk && (sw.use_pk >= 2 || d.kind != CONV_RB2) && !p.fp8 && p.w4_nt != 64 && d.cin == d.cout &&
                            (d.cout == 128 || d.cout == 256) && coef_table_fits(PK_IMGS, (long long)tiles * (d.cout / 128), s.nimg, s.cus);
            if (pk) { p.kernel = K_PK; p.kname = "conv_pk"; }
            else { p.kernel = K_W4; p.kname = "conv_w4"; }
            break;
        }
        // C = 32 / 64 (and C >= 128 behind IRE_W4=0): the persistent pipelined kernel (conv_rb.hip), or its producer / consumer form
        // (conv_pc.hip) where the activation is fused and the launch fits the coefficient table
        if (d.wp) p.w = W_WP;
        const bool pc = ab && d.wp && d.cin == d.cout && ((d.cout == 32 && (sw.pc_split & 1)) || (d.cout == 64 && (sw.pc_split & 2))) &&
                        coef_table_fits(pc_coef_imgs(d.cout), tiles, s.nimg, s.cus);
        if (pc) { p.kernel = K_PC; p.kname = "conv_pc"; }
        else { p.kernel = K_RB; p.kname = "conv_rb"; }
        break;
    }

    // ---- down: C -> 2C, stride 2, by pixel phase ----
    case CONV_DOWN:
        plan_key(p.key, "down", s.lin, "");
        if (!(v2 && sw.down_rb && d.wd)) break;
        grid(Hout, Wout, sw.rb_tile_h);
        p.nkc = d.cin / 32;
        if (sw.use_dnq && d.wdq) { p.kernel = K_DNQ; p.kname = "conv_dnq"; p.w = W_WDQ; p.nblocks = d.cout / 128; p.zeros = true; }
        else { p.kernel = K_DOWN; p.kname = "conv_down"; p.w = W_WD; p.nblocks = d.cout / 64; }
        break;

    // ---- up: nearest x2 then 2C -> C, alone or composed with the level's 1x1 `fuse` ----
    case CONV_UP: {
        plan_key(p.key, "up", s.lout, "");
        if (!(v2 && d.cout >= sw.up_rb_min_c)) break;
        if (!(sw.up_subpixel && d.wu)) {                      // nearest x2 + 3x3 on conv_rb.hip
            p.kernel = K_UP_RB; p.kname = "conv_rb"; if (d.wp) p.w = W_WP;
            grid(Hout, Wout, sw.rb_tile_h);
            break;
        }
        // sub-pixel form (conv_up.hip): tiles and halo rows on the LOW-res grid
        grid(Hin, Win, 16);
        window(Hin);
        p.nkc = d.cin / 32; p.nblocks = d.cout / 32;
        if (!(s.has_in1 && up_is_composed(sw, d))) { p.kernel = K_UP_SUB; p.kname = "conv_up"; p.w = W_WU; break; }
        // composed with `fuse`: the skip tensor is read at output pixels only, one partial per LOW-res tile (items of 32 x 64 output pixels)
        p.kernel = K_UP_FUSED; p.kname = "conv_up"; p.w = W_WUF; p.w1 = W_WSK; p.bias = B_BIAS_UF; p.in1_first_row = true; p.cin1 = d.cout;
        stats_level = s.lin;
        // cout = 128: parity-major items with all 128 couts (conv_upq.hip), four partial rows per low-res tile (fp8 engines too: their `up`
        // and `down` convs stay bf16).  The cout = 64 level stays on conv_up.hip: its row-parity form of this kernel measured 278 us
        // against 241 (profiles/r04_experiments.md).  A function of the layer only: batch / strip invariance holds.
        if (sw.use_upq && d.wuq && d.cout == 128 && d.cin % 32 == 0) {
            p.kernel = K_UPQ; p.kname = "conv_upq"; p.w = W_WUQ; p.w1 = W_WSQ; p.zeros = true; p.parts_mul = 4; p.nblocks = p.parts_mul;
        }
        break;
    }

    // ---- fuse: 1x1 over concat(up, skip), when `up` is not composed with it ----
    case CONV_FUSE:
        p.fam = FAM_CONV1;
        plan_key(p.key, "fuse", s.lout, "");
        break;

    // ---- head: 32 -> 3, + input, to u8 ----
    case CONV_HEAD:
        p.fam = FAM_HEAD;
        plan_key(p.key, "head", -1, "");
        if (!(v2 && sw.head_rb && d.wp)) break;
        p.w = W_WP; p.folds_gn = ab;
        grid(Hout, Wout, sw.rb_tile_h);
        if (sw.pc_split & 1) { p.kernel = K_PC_HEAD; p.kname = "conv_pc"; }
        else { p.kernel = K_RB_HEAD; p.kname = "conv_rb"; }
        break;
    }

    if (s.stats_out) {
        // partials are indexed by the GLOBAL tile: a strip writes its tiles at its offset (strip starts are multiples of the tile height
        // at every level: checked by the strip planner), so the finalize sees exactly the whole-image layout
        p.stats_level = stats_level;
        p.ty0 = (s.y0 >> stats_level) / p.tile_h;
        p.stat_parts = p.tiles_x * cdiv(s.H >> stats_level, p.tile_h) * p.parts_mul;
    }

    // what the profiler reports: the algorithmic work, and the flops the kernel really issues -- the sub-pixel `up` form runs 4 of the 9
    // taps, its composed `fuse` only the skip half of the 1x1 (the up half is folded into the weights)
    const int taps = d.kind == CONV_FUSE ? 1 : 9;
    const double px = (double)s.nimg * Hout * Wout, in_px = (double)s.nimg * Hin * Win;
    p.flops = 2.0 * taps * d.cin * d.cout * px;
    p.bytes = in_px * d.cin * (d.kind == CONV_STEM ? 1 : 2) + px * d.cout * (d.kind == CONV_HEAD ? 1 : 2);
    const bool fused = p.kernel == K_UP_FUSED || p.kernel == K_UPQ;
    if (fused) { p.flops += 2.0 * 2 * d.cout * d.cout * px; p.bytes += px * d.cout * 2; }      // `fuse` rides along: 1x1 over 2C channels, the skip tensor read
    if (d.kind == CONV_RB2) p.bytes += px * d.cout * 2;
    if (d.kind == CONV_HEAD) p.bytes += px * 3;
    p.flops_exec = p.flops;
    if (fused) p.flops_exec = 2.0 * 4 * d.cin * d.cout * px + 2.0 * d.cout * d.cout * px;
    else if (p.kernel == K_UP_SUB) p.flops_exec = 2.0 * 4 * d.cin * d.cout * px;
    return p;
}

// What one planned launch asks of the kernels' index types, in 64 bits (tests/test_conv_plan.py holds every field against the type the
// kernels form it in): the bytes of one image of each tensor (32-bit resource sizes and byte offsets), of the whole batch (64-bit bases),
// and the counts persist.hpp's cursor and the partials layout keep in `int`.
struct ConvExtents {
    unsigned long long in0_bytes = 0, in1_bytes = 0, out_bytes = 0;      // one image; in0 with the piece's halo rows
    unsigned long long batch_bytes = 0;                                  // the largest tensor of the launch, all images
    long long items = 0, stages = 0, stat_floats = 0;
};
inline ConvExtents conv_extents(const ConvPlan& p, const ConvDesc& d, const ConvSite& s) {
    typedef unsigned long long u64;
    ConvExtents e;
    const u64 Win = (u64)(s.w >> s.lin), Hout = (u64)(s.h >> s.lout), Wout = (u64)(s.w >> s.lout);
    e.in0_bytes = (u64)p.in_rows * Win * (d.kind == CONV_STEM ? 3u : (u64)d.cin0 * 2);
    e.in1_bytes = s.has_in1 ? (Hout + 2 * (u64)s.halo) * Wout * (u64)p.cin1 * 2 : 0;
    e.out_bytes = Hout * Wout * (d.kind == CONV_HEAD ? 3u : (u64)d.cout * 2);
    e.batch_bytes = (u64)s.nimg * std::max({e.in0_bytes, e.in1_bytes, e.out_bytes});
    e.items = (long long)p.tiles_x * p.tiles_y * s.nimg * std::max(1, p.nblocks);
    e.stages = e.items * std::max(1, p.nkc);
    e.stat_floats = s.stats_out ? (long long)s.nimg * p.stat_parts * 16 : 0;
    return e;
}

}  // namespace ire
