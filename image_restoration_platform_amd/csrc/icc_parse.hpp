// icc_parse.hpp -- the host side of the device's ICC conversion (icc.hip): collects the ICC profile of a JPEG upload from its APP2
// segments, parses a matrix/TRC or grey-TRC profile and builds the ALL-INTEGER transform to sRGB that the device applies.  Host-only,
// header-only, plain C++17, no HIP: libire.so uses it in front of icc.hip, tests/native/icc_fuzz.cpp compiles it alone under ASan and
// UBSan.  No read goes past `bytes`, whatever the profile says: every access goes through Cursor (jpeg_parse.hpp's, with 32-bit
// reads) or is checked against the end beside it; offsets and sizes are compared by subtraction, never summed.
//
// The transform (DESIGN.md "Upload jobs", stated once): tables built here in double precision,
//   lin[c][v] = rint(65535 * TRC_c(v / 255))                     u16, clamped; 3 x 256 (grey: row 0)
//   m         = rint(16384 * inv(M_sRGB) * M_profile)            nine int32, Q14; M_profile's columns are the profile's colorants
//   y_c       = clamp((sum_k m[c][k] * lin[k][v_k] + 8192) >> 14, 0, 65535)      arithmetic shift, 64-bit sum
//   out_c     = enc8(y_c),  enc8(x) = rint(255 * sRGB_OETF(x / 65535))           exact for all 65536 x
//   grey:       out = enc8(lin[0][v]) on all three bytes
// plan_profile reports kNone (no usable profile: structurally broken bytes, or a colour space that is not the file's), kIdentity (the
// integer transform changes no byte: the sRGB profile), kMatrix / kGrey (a transform to apply), or REFUSES with a reason ("invalid: ICC
// profile ..."): a well-formed profile this transform cannot stand for -- A2B0/1/2 tags (littlecms would use the LUT), a data colour
// space other than RGB / GRAY, a PCS other than XYZ, a curve of a kind or length not offered, a matrix coefficient outside (-4, 4).
// Such an upload stays with the host codec.  A broken profile is never a refusal (the reference's failOnError: false).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ire {
namespace icc {

constexpr int kNone = 0, kIdentity = 1, kMatrix = 2, kGrey = 3;      // ire.h: IRE_ICC_*
constexpr size_t kMaxProfile = (size_t)1 << 20;                      // an assembled profile larger than this is no profile
constexpr uint32_t kMaxCurve = 4096;                                 // entries of a `curv` table

struct Transform {               // ire.h: ire_icc_transform
    int32_t kind;
    int32_t m[9];
    uint16_t lin[3][256];
};

// the D50 sRGB colorants (columns r, g, b), each rounded to s15Fixed16 as a profile stores them
constexpr double s15(double v) { return (double)(long long)(v * 65536.0 + (v < 0 ? -0.5 : 0.5)) / 65536.0; }
constexpr double M_sRGB[3][3] = {{s15(0.43607), s15(0.38515), s15(0.14307)},
                                 {s15(0.22249), s15(0.71687), s15(0.06061)},
                                 {s15(0.01392), s15(0.09708), s15(0.71410)}};

struct Cursor {
    const uint8_t* p;
    size_t n, i = 0;
    bool ok = true;
    Cursor(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
    void seek(size_t o) { if (o > n) { ok = false; i = n; } else i = o; }
    unsigned u8() { if (i >= n) { ok = false; return 0; } return p[i++]; }
    uint32_t u16() { const uint32_t a = u8(), b = u8(); return a << 8 | b; }
    uint32_t u32() { const uint32_t a = u16(), b = u16(); return a << 16 | b; }
    double s15f16() { return (double)(int32_t)u32() / 65536.0; }
};
constexpr uint32_t sig(char a, char b, char c, char d) { return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint8_t)d; }

inline bool refuse(std::string& why, const char* reason) { why = std::string("invalid: ICC profile ") + reason; return false; }

// ---- the exact sRGB encode and its device form ----------------------------------------------------------------------------------------
inline int enc8(uint32_t x) {
    const double l = (double)x / 65535.0;
    const double e = l <= 0.0031308 ? 12.92 * l : 1.055 * std::pow(l, 1.0 / 2.4) - 0.055;
    const double r = std::rint(255.0 * e);
    return r < 0 ? 0 : r > 255 ? 255 : (int)r;
}
// o = coarse[x >> 4]; o += (x > last[o]): coarse[b] = enc8(16 b), last[o] = the largest x with enc8(x) <= o.  A bucket of 16 holds at
// most one step of enc8 (its steepest slope is 12.92 * 255 / 65535 = 0.05 levels per unit, 0.8 per bucket), so one correction gives
// the exact table; the constructor verifies that for all 65536 inputs (`verified`, which IccConverter::setup insists on).
struct EncTables {
    uint8_t coarse[4096];
    uint16_t last[256];
    std::vector<uint8_t> exact;       // enc8 of every x
    bool verified = false;
    EncTables() : exact(65536) {
        for (uint32_t x = 0; x < 65536; ++x) exact[x] = (uint8_t)enc8(x);
        for (uint32_t b = 0; b < 4096; ++b) coarse[b] = exact[16 * b];
        for (int o = 0; o < 256; ++o) last[o] = 65535;
        for (uint32_t x = 0; x + 1 < 65536; ++x) if (exact[x + 1] != exact[x]) last[exact[x]] = (uint16_t)x;
        verified = true;
        for (uint32_t x = 0; x < 65536; ++x) { int o = coarse[x >> 4]; o += x > last[o]; if (o != exact[x]) verified = false; }
    }
};
inline const EncTables& enc_tables() { static const EncTables t; return t; }

// ---- curves ----------------------------------------------------------------------------------------------------------------------------
inline uint16_t to_u16(double y) {       // rint(65535 y), clamped; NaN is 0
    if (!(y > 0.0)) return 0;
    if (y >= 1.0) return 65535;
    return (uint16_t)std::rint(65535.0 * y);
}
inline double pow_pos(double base, double g) { return base > 0.0 ? std::pow(base, g) : 0.0; }      // (a base <= 0 gives 0, as littlecms does)
// the tag at [off, off + size) of the profile -> one row of lin.  0: ok, 1: broken (no profile), 2: a curve that is not offered
inline int read_curve(const uint8_t* p, size_t off, size_t size, uint16_t lin[256]) {
    Cursor s(p + off, size);
    const uint32_t type = s.u32();
    (void)s.u32();
    if (!s.ok) return 1;
    if (type == sig('c', 'u', 'r', 'v')) {
        const uint32_t count = s.u32();
        if (!s.ok) return 1;
        if (count > kMaxCurve) return 2;
        if (count == 0) { for (int v = 0; v < 256; ++v) lin[v] = (uint16_t)(v * 257); return 0; }
        if (count == 1) {
            const double g = (double)s.u16() / 256.0;
            if (!s.ok) return 1;
            for (int v = 0; v < 256; ++v) lin[v] = to_u16(pow_pos((double)v / 255.0, g));
            return 0;
        }
        if ((size - s.i) / 2 < count) return 1;
        const uint8_t* t = p + off + s.i;
        for (int v = 0; v < 256; ++v) {
            const double x = (double)v / 255.0 * (double)(count - 1);
            uint32_t k = (uint32_t)x;
            if (k > count - 2) k = count - 2;
            const double f = x - (double)k;
            const double a = (double)((uint32_t)t[2 * k] << 8 | t[2 * k + 1]), b = (double)((uint32_t)t[2 * k + 2] << 8 | t[2 * k + 3]);
            lin[v] = to_u16((a + (b - a) * f) / 65535.0);
        }
        return 0;
    }
    if (type == sig('p', 'a', 'r', 'a')) {
        const uint32_t fn = s.u16();
        (void)s.u16();
        if (!s.ok) return 1;
        if (fn > 4) return 2;
        static const int kParams[5] = {1, 3, 4, 5, 7};
        double q[7] = {0, 0, 0, 0, 0, 0, 0};       // g a b c d e f
        for (int k = 0; k < kParams[fn]; ++k) q[k] = s.s15f16();
        if (!s.ok) return 1;
        const double g = q[0], a = q[1], b = q[2], c = q[3], d = q[4], e = q[5], f = q[6];
        for (int v = 0; v < 256; ++v) {
            const double x = (double)v / 255.0;
            double y;
            if (fn == 0) y = pow_pos(x, g);
            else if (fn == 1) y = a != 0.0 && x >= -b / a ? pow_pos(a * x + b, g) : 0.0;
            else if (fn == 2) y = a != 0.0 && x >= -b / a ? pow_pos(a * x + b, g) + c : c;
            else if (fn == 3) y = x >= d ? pow_pos(a * x + b, g) : c * x;
            else y = x >= d ? pow_pos(a * x + b, g) + e : c * x + f;
            lin[v] = to_u16(y);
        }
        return 0;
    }
    return 2;
}

inline void inv3(const double a[3][3], double r[3][3]) {
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
    r[0][0] = c00 / det; r[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det; r[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    r[1][0] = c01 / det; r[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det; r[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    r[2][0] = c02 / det; r[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det; r[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
}

// ---- the profile -----------------------------------------------------------------------------------------------------------------------
// true: t.kind says what to do (kNone included).  false: refused, `why` says why.  components: of the image the profile came with, 1 or 3.
inline bool plan_profile(const uint8_t* p, size_t n, int components, Transform& t, std::string& why) {
    std::memset(&t, 0, sizeof(t));
    t.kind = kNone;
    if (!p || n < 132 || n > kMaxProfile) return true;
    Cursor hd(p, n);
    const size_t size = hd.u32();
    if (size > n || size < 132) return true;
    hd.seek(36);
    if (hd.u32() != sig('a', 'c', 's', 'p')) return true;
    hd.seek(16);
    const uint32_t space = hd.u32(), pcs = hd.u32();
    if (space != sig('R', 'G', 'B', ' ') && space != sig('G', 'R', 'A', 'Y')) return refuse(why, "of a colour space other than RGB or GRAY (convert with the host codec)");
    if (pcs != sig('X', 'Y', 'Z', ' ')) return refuse(why, "with a connection space other than XYZ (convert with the host codec)");
    // the tag table: every entry inside the profile
    Cursor tt(p, size);
    tt.seek(128);
    const uint32_t ntags = tt.u32();
    if (ntags > (size - 132) / 12) return true;
    struct Tag { uint32_t off = 0, size = 0; bool have = false; };
    Tag xyz[3], trc[3], ktrc;
    bool lut = false;
    for (uint32_t k = 0; k < ntags; ++k) {
        const uint32_t s = tt.u32(), off = tt.u32(), sz = tt.u32();
        if (!tt.ok || off > size || sz > size - off) return true;
        Tag* dst = s == sig('r', 'X', 'Y', 'Z') ? &xyz[0] : s == sig('g', 'X', 'Y', 'Z') ? &xyz[1] : s == sig('b', 'X', 'Y', 'Z') ? &xyz[2]
                 : s == sig('r', 'T', 'R', 'C') ? &trc[0] : s == sig('g', 'T', 'R', 'C') ? &trc[1] : s == sig('b', 'T', 'R', 'C') ? &trc[2]
                 : s == sig('k', 'T', 'R', 'C') ? &ktrc : nullptr;
        if (dst && !dst->have) { dst->off = off; dst->size = sz; dst->have = true; }
        if (s == sig('A', '2', 'B', '0') || s == sig('A', '2', 'B', '1') || s == sig('A', '2', 'B', '2')) lut = true;
    }
    if (lut) return refuse(why, "with A2B lookup tables (convert with the host codec)");
    const EncTables& E = enc_tables();
    if (space == sig('G', 'R', 'A', 'Y')) {
        if (components != 1 || !ktrc.have) return true;
        const int rc = read_curve(p, ktrc.off, ktrc.size, t.lin[0]);
        if (rc == 2) return refuse(why, "with a tone curve that is not offered (convert with the host codec)");
        if (rc) { std::memset(&t, 0, sizeof(t)); return true; }
        bool same = true;
        for (int v = 0; v < 256; ++v) same = same && E.exact[t.lin[0][v]] == v;
        t.kind = same ? kIdentity : kGrey;
        return true;
    }
    if (components != 3) return true;
    double M[3][3];
    for (int c = 0; c < 3; ++c) {
        if (!xyz[c].have || !trc[c].have) return true;
        Cursor s(p + xyz[c].off, xyz[c].size);
        const uint32_t type = s.u32();
        (void)s.u32();
        const double X = s.s15f16(), Y = s.s15f16(), Z = s.s15f16();
        if (!s.ok || type != sig('X', 'Y', 'Z', ' ')) return true;
        M[0][c] = X; M[1][c] = Y; M[2][c] = Z;
    }
    for (int c = 0; c < 3; ++c) {
        const int rc = read_curve(p, trc[c].off, trc[c].size, t.lin[c]);
        if (rc == 2) return refuse(why, "with a tone curve that is not offered (convert with the host codec)");
        if (rc) { std::memset(&t, 0, sizeof(t)); return true; }
    }
    double inv[3][3];
    inv3(M_sRGB, inv);
    bool unit = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double v = inv[r][0] * M[0][c] + inv[r][1] * M[1][c] + inv[r][2] * M[2][c];
            if (!(v > -4.0 && v < 4.0)) { std::memset(&t, 0, sizeof(t)); return refuse(why, "with a matrix coefficient outside (-4, 4) (convert with the host codec)"); }
            t.m[3 * r + c] = (int32_t)std::rint(16384.0 * v);
            unit = unit && t.m[3 * r + c] == (r == c ? 16384 : 0);
        }
    for (int c = 0; c < 3 && unit; ++c)
        for (int v = 0; v < 256; ++v) unit = unit && E.exact[t.lin[c][v]] == v;
    t.kind = unit ? kIdentity : kMatrix;
    return true;
}

// ---- the profile of a JPEG file ---------------------------------------------------------------------------------------------------------
// Walks the markers in front of the first scan: the APP2 segments whose payload starts "ICC_PROFILE\0" seq count, in any order, and the
// frame header's component count.  false: no profile -- none there, or a chunk set that breaks the rules (chunks that state different
// counts, a sequence number outside 1..count or seen twice or missing, more than 1 MiB in all).
inline bool collect_file(const uint8_t* file, size_t bytes, std::vector<uint8_t>& profile, int& components) {
    profile.clear();
    components = 0;
    if (!file || bytes < 4 || file[0] != 0xFF || file[1] != 0xD8) return false;
    struct Chunk { size_t off = 0, len = 0; bool have = false; };
    std::vector<Chunk> ch;
    unsigned count = 0;
    bool bad = false;
    size_t total = 0;
    size_t i = 2;
    while (i + 4 <= bytes) {
        if (file[i] != 0xFF) break;
        while (i < bytes && file[i] == 0xFF) ++i;
        if (i + 2 >= bytes) break;
        const unsigned b = file[i++];
        if (b == 0xDA || b == 0xD9 || b == 0xD8 || b == 0x00 || b == 0x01 || (b >= 0xD0 && b <= 0xD7)) break;
        const size_t len = (size_t)file[i] << 8 | file[i + 1];
        if (len < 2 || len > bytes - i) break;
        if (b >= 0xC0 && b <= 0xCF && b != 0xC4 && b != 0xC8 && b != 0xCC && !components && len >= 8) components = file[i + 7];
        if (b == 0xE2 && len >= 16 && std::memcmp(file + i + 2, "ICC_PROFILE\0", 12) == 0) {
            const unsigned seq = file[i + 14], cnt = file[i + 15];
            if (!count && cnt) { count = cnt; ch.assign(cnt, Chunk{}); }
            if (!cnt || cnt != count || seq < 1 || seq > count || ch[seq - 1].have) bad = true;
            else {
                ch[seq - 1].off = i + 16; ch[seq - 1].len = len - 16; ch[seq - 1].have = true;
                total += len - 16;
            }
        }
        i += len;
    }
    if (!count || bad || total > kMaxProfile) return false;
    for (const Chunk& c : ch) if (!c.have) return false;
    profile.reserve(total);
    for (const Chunk& c : ch) profile.insert(profile.end(), file + c.off, file + c.off + c.len);
    return true;
}
// plan_profile of the file's own profile and component count; a file without a (whole) profile, or of another component count than 1 or 3, is kNone
inline bool plan_file(const uint8_t* file, size_t bytes, Transform& t, std::string& why) {
    std::memset(&t, 0, sizeof(t));
    std::vector<uint8_t> profile;
    int components = 0;
    if (!collect_file(file, bytes, profile, components)) return true;
    if (components != 1 && components != 3) return true;
    return plan_profile(profile.data(), profile.size(), components, t, why);
}

// ---- the transform on the host: what the device computes, for the tables that are composed here --------------------------------------
inline void grey_lut(const Transform& t, uint8_t lut[256]) {
    const EncTables& E = enc_tables();
    for (int v = 0; v < 256; ++v) lut[v] = E.exact[t.lin[0][v]];
}

}  // namespace icc
}  // namespace ire
