// weight_pack.hpp -- the weight file parser and every weight layout of the convolution kernels, on the host; no HIP, no device
// code: engine.cpp uploads what comes back, tests/native/weight_pack_dump.cpp builds it with plain g++ under the sanitizers.
//
// Every kernel reads its weights from a slab that is the exact LDS image of one of its stages.  Three layout families cover
// them all: stage slabs (pack_stages), sub-pixel parity slabs (pack_subpixel) and the stem's A fragments (pack_stem).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "conv_kind.hpp"
#include "conv_plan.hpp"
#include "errors.hpp"

namespace ire {

struct Tensor {
    std::vector<int> dims;
    std::vector<float> data;
};
using TensorMap = std::map<std::string, Tensor>;

// "IREW" | u32 version = 1 | u32 count | count x (u32 name length | name | u32 rank | rank x u32 dim | fp32 data)
inline TensorMap parse_weights(const void* blob, size_t bytes) {
    const unsigned char* p = (const unsigned char*)blob;
    size_t off = 0;                                      // <= bytes at all times
    auto take = [&](size_t n) {                          // the next n bytes, or the error; no sum that could wrap
        if (n > bytes - off) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: truncated");
        const unsigned char* q = p + off;
        off += n;
        return q;
    };
    auto u32 = [&] { uint32_t v; std::memcpy(&v, take(4), 4); return v; };
    if (bytes < 12) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: truncated");
    if (std::memcmp(take(4), "IREW", 4) != 0) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: bad magic");
    const uint32_t ver = u32(), nt = u32();
    if (ver != 1 || nt > 4096) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: version");
    TensorMap m;
    for (uint32_t i = 0; i < nt; ++i) {
        const uint32_t ln = u32();
        if (ln > 256) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: name");
        std::string name((const char*)take(ln), ln);
        while (!name.empty() && name.back() == '\0') name.pop_back();
        const uint32_t nd = u32();
        if (nd > 4) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: ndim");
        Tensor t;
        t.dims.resize(nd);
        size_t cnt = 1;                                  // saturates: a product past SIZE_MAX is past the file's size too
        for (uint32_t d = 0; d < nd; ++d) {
            const uint32_t v = u32();
            t.dims[d] = (int)v;
            cnt = (v == 0) ? 0 : (cnt > SIZE_MAX / v ? SIZE_MAX : cnt * v);
        }
        if (cnt > (bytes - off) / 4) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: truncated");
        t.data.resize(cnt);
        if (cnt) std::memcpy(t.data.data(), take(cnt * 4), cnt * 4);
        m[name] = std::move(t);
    }
    return m;
}

inline unsigned short f32_to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;  // weights are finite: no NaN handling needed
    return (unsigned short)u;
}

// fp32 -> OCP e4m3fn (1-4-3, bias 7, no infinities, max 448), round to nearest even, saturating.
inline unsigned char f32_to_e4m3(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const unsigned char sign = (u >> 31) ? 0x80 : 0;
    float a = std::fabs(f);
    if (!(a == a)) return sign | 0x7f;
    if (a >= 448.0f) return sign | 0x7e;
    if (a < 0.0009765625f) return sign;                         // < 2^-10 = half the smallest subnormal (2^-9): rounds to zero
    int e;
    std::frexp(a, &e);                                          // a = m * 2^e, m in [0.5, 1)
    int E = e - 1;                                              // a = 1.xxx * 2^E
    if (E < -6) E = -6;                                         // subnormal range: fixed exponent, step 2^-9
    const float step = std::ldexp(1.0f, E - 3);
    float q = std::nearbyint(a / step);                         // default rounding mode: to nearest even
    if (E == -6 && q < 8.0f) return sign | (unsigned char)q;    // subnormal: mantissa only
    if (q >= 16.0f) { q = 8.0f; E += 1; }
    if (E > 8) return sign | 0x7e;
    return sign | (unsigned char)(((E + 7) << 3) | ((int)q - 8));
}

// Direct epilogues (conv_rb.hip, conv_w4.hip and every kernel after them): slab row n of a 32-row MFMA tile carries cout
// perm_row(n) = n with bits 2 and 3 swapped, so that the 16 accumulators of a lane-half are two runs of 8 CONTIGUOUS couts (one
// 16-B store each, no v_permlane32_swap pairing).  The other bits stay: the same map serves 64- and 128-row blocks.
inline int perm_row(int n) { return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1); }

// What every stage slab is made of: the fragment of 8 consecutive input channels of one (cout, tap), quantised -- 16 bytes of bf16,
// 8 of fp8.  [cout][group of 8 cin][tap][8], zero beyond cin; quant(cout, w) is the element.
template <class T, class Quant>
std::vector<T> to_fragments(const float* W, int cout, int cin, int taps, Quant quant) {
    const int cin8 = (cin + 7) / 8;
    std::vector<T> f((size_t)cout * cin8 * taps * 8, 0);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < taps; ++tap)
                f[((((size_t)co * cin8 + ci / 8) * taps + tap) * 8) + ci % 8] = quant(co, W[((size_t)co * cin + ci) * taps + tap]);
    return f;
}
inline unsigned short bf16_of(int, float w) { return f32_to_bf16(w); }

// Stage slabs [cout block of nt][K-chunk of cs channels][kk = t * (cs / E) + c][nt rows][E], gathered from the fragments f (rows
// row_stride elements apart, cin8 groups each): row n of block nb = cout nb * nt + n (or perm_row(n)), its E channels = chunk * cs +
// c * E + (0..E-1) at tap order[t] -- zero where cout or cin lie outside the tensor and in the kk rows that pad taps * cs / E up to nkk.
struct StageShape {
    int nt;                      // couts per block
    int cs;                      // channels per stage
    int E = 8;                   // channels per row: 8, or 16 (conv_f8.hip: 16 fp8 = 16 bytes)
    int taps = 9;
    const int* order = nullptr;  // tap of slot t; null: t
    bool permute = true;         // rows in perm_row order
    int nkk = 0;                 // kk rows per stage; 0: taps * cs / E
};
template <class T>
std::vector<T> pack_stages(const StageShape& s, const T* f, size_t row_stride, int cout, int cin8, int cout_pad, int cin_pad) {
    const int nt = s.nt, E = s.E, taps = s.taps, g = s.cs / E, nkk = s.nkk ? s.nkk : taps * g, nblocks = cout_pad / nt, nkc = cin_pad / s.cs;
    std::vector<T> a((size_t)nblocks * nkc * nkk * nt * E, 0);
    for (int nb = 0; nb < nblocks; ++nb)
        for (int kc = 0; kc < nkc; ++kc)
            for (int kk = 0; kk < taps * g; ++kk) {
                const int t = kk / g, tap = s.order ? s.order[t] : t, cg0 = (kc * s.cs + kk % g * E) / 8;
                T* dst = &a[(((size_t)nb * nkc + kc) * nkk + kk) * nt * E];
                for (int n = 0; n < nt; ++n, dst += E) {
                    const int co = nb * nt + (s.permute ? perm_row(n) : n);
                    if (co >= cout) continue;
                    for (int u = 0; u < E / 8 && cg0 + u < cin8; ++u)
                        std::memcpy(dst + u * 8, f + (size_t)co * row_stride + ((size_t)(cg0 + u) * taps + tap) * 8, 8 * sizeof(T));
                }
            }
    return a;
}

// conv_down.hip / conv_dnq.hip: the stride-2 conv as a unit-stride conv over the four pixel phases P_ab[Y][X] = in[2Y+a][2X+b]:
// phase (a, b) carries the taps ky in (a ? {0, 2} : {1}) x kx in (b ? {0, 2} : {1}), in that order (1 + 2 + 2 + 4 taps)
constexpr int kPhaseTapOrder[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};

// conv_up.hip / conv_upq.hip: nearest x2 -> 3x3 == four 2x2 convolutions on the low-res grid, one per output parity (pa, pb); the
// taps that land on the same low-res pixel are summed here in Acc, then rounded to bf16 once:
//   pa = 0: window row 0 <- ky 0, row 1 <- ky 1 + ky 2;   pa = 1: row 0 <- ky 0 + ky 1, row 1 <- ky 2   (columns alike)
// [cout block of nt][kc32][parity][kk = tap4 * 4 + c8][nt permuted rows][8], or parity outermost (one cout block)
template <class Acc>
std::vector<unsigned short> pack_subpixel(const Acc* W, int cout, int cin, int nt, bool parity_outer) {
    const int nb_n = cout / nt, nkc = cin / 32;
    std::vector<unsigned short> a((size_t)nb_n * nkc * 4 * 16 * nt * 8, 0);
    auto lo_of = [](int par, int d) { return par == 0 ? (d == 0 ? 0 : 1) : (d == 0 ? 0 : 2); };
    auto hi_of = [](int par, int d) { return par == 0 ? (d == 0 ? 0 : 2) : (d == 0 ? 1 : 2); };
    for (int nb = 0; nb < nb_n; ++nb)
        for (int kc = 0; kc < nkc; ++kc)
            for (int par = 0; par < 4; ++par) {
                const size_t stage = parity_outer ? (size_t)par * nkc + kc : ((size_t)nb * nkc + kc) * 4 + par;
                for (int kk = 0; kk < 16; ++kk) {
                    const int pa = par >> 1, pb = par & 1, tap4 = kk >> 2, c8 = kk & 3, dy = tap4 >> 1, dx = tap4 & 1;
                    for (int n = 0; n < nt; ++n)
                        for (int e = 0; e < 8; ++e) {
                            const int co = nb * nt + perm_row(n), ci = kc * 32 + c8 * 8 + e;
                            Acc sum = 0;
                            for (int ky = lo_of(pa, dy); ky <= hi_of(pa, dy); ++ky)
                                for (int kx = lo_of(pb, dx); kx <= hi_of(pb, dx); ++kx) sum += W[((size_t)co * cin + ci) * 9 + ky * 3 + kx];
                            a[((stage * 16 + kk) * nt + n) * 8 + e] = f32_to_bf16((float)sum);
                        }
                }
            }
    return a;
}

// conv_stem.hip (3 -> 32): k-step ky is one tile row; lane (row rho, half h) holds W[perm_row(rho)] at k = 16 ky + 8 h + e, i.e.
// kx = 2 h + (e >> 2), c = e & 3 -- zero for the pad positions kx = 3 and c = 3 (the LDS tile holds a pixel as four bf16: R, G, B, 0)
inline std::vector<unsigned short> pack_stem(const float* W) {
    std::vector<unsigned short> a(3 * 2 * 32 * 8, 0);
    for (int ky = 0; ky < 3; ++ky)
        for (int hh = 0; hh < 2; ++hh)
            for (int rho = 0; rho < 32; ++rho)
                for (int e = 0; e < 8; ++e) {
                    const int kx = 2 * hh + (e >> 2), ch = e & 3;
                    if (kx >= 3 || ch >= 3) continue;
                    a[(((size_t)ky * 2 + hh) * 32 + rho) * 8 + e] = f32_to_bf16(W[((size_t)perm_row(rho) * 3 + ch) * 9 + ky * 3 + kx]);
                }
    return a;
}

// The packed arrays of one convolution (an empty vector = the array does not exist: conv_plan.hpp picks kernels by that) and the
// scalars the launches need.  Field names and layouts: ConvW in engine.hpp.
struct PackedConv {
    ConvKind kind = CONV_RB1;
    int cin = 0, cout = 0, cin0 = 0, cin1 = 0;
    int nt = 0, nblocks = 0, nkc = 0, kc_split = 0;
    std::vector<unsigned short> w, wp, w4, w4h, wstem, wd, wu, wuf, wdq, wuq, wsq, wsk;
    std::vector<float> bias_uf;
    std::vector<unsigned char> w8x, w8;
    std::vector<float> oscale, bias8, bias;
};

inline PackedConv pack_conv(const TensorMap& tm, ConvKind kind, const std::string& wname, const std::string& bname, int cin, int cout,
                            bool fp8) {
    auto wi = tm.find(wname), bi = tm.find(bname);
    if (wi == tm.end() || bi == tm.end()) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: missing " + wname);
    const auto& dims = wi->second.dims;
    const int taps = (kind == CONV_FUSE) ? 1 : 9, ks = (kind == CONV_FUSE) ? 1 : 3;
    if (dims.size() != 4 || dims[0] != cout || dims[1] != cin || dims[2] != ks || dims[3] != ks || (int)bi->second.data.size() != cout)
        fail(IRE_ERR_INVALID_INPUT, "invalid weight file: shape of " + wname);
    const float* W = wi->second.data.data();
    const float* B = bi->second.data.data();
    PackedConv c;
    c.kind = kind; c.cin = cin; c.cout = cout;
    const int cs = (kind == CONV_STEM) ? 8 : 32;
    const int cin_pad = (kind == CONV_STEM) ? 8 : cin;
    const int cout_pad = (kind == CONV_HEAD) ? 32 : cout;
    c.nt = conv_nt(kind, cout_pad);
    if (cin_pad % cs || cout_pad % c.nt) fail(IRE_ERR_INTERNAL, "internal: conv channel counts");
    c.nkc = cin_pad / cs;
    c.nblocks = cout_pad / c.nt;
    if (kind == CONV_FUSE) { c.cin0 = cin / 2; c.cin1 = cin / 2; c.kc_split = c.nkc / 2; }
    else { c.cin0 = cin_pad; c.cin1 = 0; c.kc_split = c.nkc; }
    const int cin8 = (cin + 7) / 8;
    const size_t row = (size_t)cin8 * taps * 8;
    const std::vector<unsigned short> F = to_fragments<unsigned short>(W, cout, cin, taps, bf16_of);
    auto stages = [&](StageShape s) { return pack_stages(s, F.data(), row, cout, cin8, cout_pad, cin_pad); };
    // the v1 template (conv_mfma.hip) keeps the natural row order; conv_rb.hip / conv_pc.hip read the same slabs with permuted rows
    StageShape v1{c.nt, cs};
    v1.taps = taps; v1.nkk = conv_nsteps(kind) * 2; v1.permute = false;
    c.w = stages(v1);
    v1.permute = true;
    if (kind == CONV_RB1 || kind == CONV_RB2 || kind == CONV_UP || kind == CONV_HEAD) c.wp = stages(v1);
    if (kind == CONV_STEM && cin == 3 && cout == 32) c.wstem = pack_stem(W);
    if (kind == CONV_DOWN && cin % 32 == 0 && cout % 64 == 0) {
        StageShape ph{64, 32};
        ph.order = kPhaseTapOrder;
        c.wd = stages(ph);
        ph.nt = 128;                                                // conv_dnq.hip: the same taps in the same order as 128-cout slabs
        if (cout % 128 == 0) c.wdq = stages(ph);
    }
    if (kind == CONV_UP && cin % 64 == 0 && cout % 32 == 0) c.wu = pack_subpixel(W, cout, cin, 32, false);
    if ((kind == CONV_RB1 || kind == CONV_RB2) && cout >= 128 && cin % 16 == 0 && cout % 128 == 0) {
        c.w4 = stages({128, 16});                                   // conv_w4.hip / conv_pk.hip: 16-channel stages, 128-cout blocks
        c.w4h = stages({64, 16});                                   // the same in 64-cout blocks
        if (fp8) {
            // the same slabs as OCP e4m3 with one scale per OUTPUT channel: w_q = e4m3(w / s_w[co]), s_w[co] = max|w[co]| / 448
            // (the whole e4m3 range per channel); activations are scaled by kActScale = 16 while staging (conv_w4.hip), so the
            // kernel's accumulator times oscale = s_w / 16 is the conv output and its accumulators start at bias / oscale
            const float kActScale = 16.0f;
            std::vector<float> sw(cout);
            c.oscale.resize(cout); c.bias8.resize(cout);
            for (int co = 0; co < cout; ++co) {
                float m = 0.f;
                for (size_t k = 0; k < (size_t)cin * 9; ++k) m = std::max(m, std::fabs(W[(size_t)co * cin * 9 + k]));
                sw[co] = m > 0.f ? m / 448.0f : 1.0f;
                c.oscale[co] = sw[co] / kActScale;
                c.bias8[co] = B[co] / c.oscale[co];
            }
            const std::vector<unsigned char> F8 = to_fragments<unsigned char>(W, cout, cin, 9, [&](int co, float w) { return f32_to_e4m3(w / sw[co]); });
            c.w8 = pack_stages({128, 16}, F8.data(), row, cout, cin8, cout, cin);
            // the K = 64 form (conv_f8.hip): 32-channel stages, [tap][16-channel half][128 rows][16 bytes]
            if (cin % 32 == 0) c.w8x = pack_stages({128, 32, 16}, F8.data(), row, cout, cin8, cout, cin);
        }
    }
    c.bias.assign(cout_pad, 0.f);
    std::copy(B, B + cout, c.bias.begin());
    return c;
}

// what conv_plan.hpp needs to know of a packed convolution: its scalars and which arrays exist
inline ConvDesc conv_desc(const PackedConv& p) {
    ConvDesc d;
    d.kind = p.kind; d.cin = p.cin; d.cout = p.cout; d.cin0 = p.cin0; d.cin1 = p.cin1; d.nkc = p.nkc; d.nblocks = p.nblocks; d.kc_split = p.kc_split;
    d.w = !p.w.empty(); d.wp = !p.wp.empty(); d.w4 = !p.w4.empty(); d.w4h = !p.w4h.empty(); d.wstem = !p.wstem.empty(); d.wd = !p.wd.empty();
    d.wu = !p.wu.empty(); d.wuf = !p.wuf.empty(); d.wdq = !p.wdq.empty(); d.wuq = !p.wuq.empty(); d.wsq = !p.wsq.empty(); d.wsk = !p.wsk.empty();
    d.bias_uf = !p.bias_uf.empty(); d.w8x = !p.w8x.empty(); d.w8 = !p.w8.empty(); d.oscale = !p.oscale.empty(); d.bias8 = !p.bias8.empty();
    d.bias = !p.bias.empty();
    return d;
}

// `up` (nearest x2 -> 3x3, 2C -> C) followed by `fuse` (1x1 over concat(up, skip), 2C -> C) with nothing non-linear between
// them is ONE convolution plus a 1x1 over the skip tensor:
//   fuse(concat(up(x), skip)) = (Wf_up . Wup) * x_up  +  Wf_skip . skip  +  (Wf_up . b_up + b_f),   Wf = [Wf_up | Wf_skip].
// The composition is done once here in double, then the sub-pixel pre-sums, then ONE rounding to bf16.  Adds wuf, wsk, bias_uf
// (and, for C = 128, conv_upq.hip's wuq, wsq) to the packed `up` of level `sl`; nothing where the composed form does not apply.
inline void pack_up_fused(const TensorMap& tm, PackedConv& up, const std::string& sl) {
    const int C = up.cout, cin = up.cin;
    if (up.kind != CONV_UP || up.wu.empty() || (C != 32 && C != 64 && C != 128)) return;
    auto wu = tm.find("up" + sl + ".w"), bu = tm.find("up" + sl + ".b"), wf = tm.find("fuse" + sl + ".w"), bf = tm.find("fuse" + sl + ".b");
    if (wu == tm.end() || bu == tm.end() || wf == tm.end() || bf == tm.end()) return;
    const float* Wu = wu->second.data.data();        // [C][cin][3][3]
    const float* Wf = wf->second.data.data();        // [C][2C]
    if ((int)wf->second.data.size() != C * 2 * C) return;
    std::vector<double> Wc((size_t)C * cin * 9, 0.0);
    for (int co = 0; co < C; ++co)
        for (int m = 0; m < C; ++m) {
            const double f = Wf[(size_t)co * 2 * C + m];
            const float* src = Wu + (size_t)m * cin * 9;
            double* dst = Wc.data() + (size_t)co * cin * 9;
            for (int k = 0; k < cin * 9; ++k) dst[k] += f * (double)src[k];
        }
    up.bias_uf.resize(C);
    for (int co = 0; co < C; ++co) {
        double b = bf->second.data[co];
        for (int m = 0; m < C; ++m) b += (double)Wf[(size_t)co * 2 * C + m] * (double)bu->second.data[m];
        up.bias_uf[co] = (float)b;
    }
    // the skip half of the fuse weights as one-tap stage slabs: [nblock32][ks16][h][32][8] (conv_up.hip's A fragments)
    const std::vector<unsigned short> Ff = to_fragments<unsigned short>(Wf, C, 2 * C, 1, bf16_of);
    const unsigned short* skip = Ff.data() + C;      // [C][2C] (one tap: the fragments are the rows), second half of every row
    StageShape sk{32, 16};
    sk.taps = 1;
    up.wuf = pack_subpixel(Wc.data(), C, cin, 32, false);
    up.wsk = pack_stages(sk, skip, 2 * C, C, C / 8, C, C);
    if (C == 128) {
        // conv_upq.hip: the same composed, pre-summed weights (the same single rounding) as 128-cout slabs per output parity, and the
        // skip half as four 32-channel stages [ks32][c8][128][8]
        sk.nt = 128; sk.cs = 32;
        up.wuq = pack_subpixel(Wc.data(), C, cin, 128, true);
        up.wsq = pack_stages(sk, skip, 2 * C, C, C / 8, C, C);
    }
}

}  // namespace ire
