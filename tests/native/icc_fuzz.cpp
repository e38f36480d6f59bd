// icc_fuzz.cpp -- the ICC planner of upload jobs (image_restoration_platform_amd/csrc/icc_parse.hpp) alone on the CPU, built with
// AddressSanitizer + UBSan by tests/test_icc_native.py.  Valid matrix/TRC and grey profiles of every curve form, and a JPEG head with
// a profile in three APP2 chunks: every truncation and every single-byte mutation (all 255 other values of every byte) of each.  Every outcome must be a valid
// kind or a refusal with a reason, the matrix of a transform inside (-4, 4) in Q14, kNone all zeros -- and the sanitizers silent.
// Test infrastructure: libire.so never contains it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/icc_parse.hpp"

using namespace ire;
typedef std::vector<uint8_t> Bytes;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); ++g_fail; } } while (0)

static void be32(Bytes& b, uint32_t v) { for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)(v >> s)); }
static void be16(Bytes& b, uint32_t v) { b.push_back((uint8_t)(v >> 8)); b.push_back((uint8_t)v); }
static void s15(Bytes& b, double v) { be32(b, (uint32_t)(int32_t)(v * 65536.0 + (v < 0 ? -0.5 : 0.5))); }
static void tag4(Bytes& b, const char* s) { b.insert(b.end(), s, s + 4); }

static Bytes xyz(double x, double y, double z) { Bytes b; tag4(b, "XYZ "); be32(b, 0); s15(b, x); s15(b, y); s15(b, z); return b; }
static Bytes curv(const std::vector<uint32_t>& v) { Bytes b; tag4(b, "curv"); be32(b, 0); be32(b, (uint32_t)v.size()); for (uint32_t x : v) be16(b, x); return b; }
static Bytes para(int fn, const std::vector<double>& p) { Bytes b; tag4(b, "para"); be32(b, 0); be16(b, (uint32_t)fn); be16(b, 0); for (double x : p) s15(b, x); return b; }

struct Tag { const char* sig; Bytes data; };
static Bytes profile(const std::vector<Tag>& tags, const char* space, int version) {
    Bytes body, table;
    const uint32_t off = 128 + 4 + 12 * (uint32_t)tags.size();
    for (const Tag& t : tags) {
        tag4(table, t.sig); be32(table, off + (uint32_t)body.size()); be32(table, (uint32_t)t.data.size());
        body.insert(body.end(), t.data.begin(), t.data.end());
        while (body.size() % 4) body.push_back(0);
    }
    Bytes p;
    be32(p, off + (uint32_t)body.size()); be32(p, 0); be32(p, version >= 4 ? 0x04300000u : 0x02400000u);
    tag4(p, "mntr"); tag4(p, space); tag4(p, "XYZ ");
    p.resize(36, 0);
    tag4(p, "acsp");
    p.resize(128, 0);
    be32(p, (uint32_t)tags.size());
    p.insert(p.end(), table.begin(), table.end());
    p.insert(p.end(), body.begin(), body.end());
    return p;
}
static Bytes rgb_profile(const double c[3][3], const Bytes& r, const Bytes& g, const Bytes& b, int version) {
    return profile({{"rXYZ", xyz(c[0][0], c[0][1], c[0][2])}, {"gXYZ", xyz(c[1][0], c[1][1], c[1][2])}, {"bXYZ", xyz(c[2][0], c[2][1], c[2][2])},
                    {"rTRC", r}, {"gTRC", g}, {"bTRC", b}}, "RGB ", version);
}

static const double kP3[3][3] = {{0.51512, 0.24120, -0.00105}, {0.29198, 0.69225, 0.04189}, {0.15710, 0.06657, 0.78407}};
static const double kAdobe[3][3] = {{0.60974, 0.31111, 0.01947}, {0.20528, 0.62567, 0.06087}, {0.14919, 0.06322, 0.74457}};
static const double kSrgb[3][3] = {{0.43607, 0.22249, 0.01392}, {0.38515, 0.71687, 0.09708}, {0.14307, 0.06061, 0.71410}};

static long g_runs = 0, g_kinds[4] = {0, 0, 0, 0}, g_refused = 0;
static void outcome(bool ok, const icc::Transform& t, const std::string& why) {
    ++g_runs;
    if (!ok) { ++g_refused; CHECK(why.rfind("invalid: ICC profile ", 0) == 0); return; }
    CHECK(t.kind >= icc::kNone && t.kind <= icc::kGrey);
    if (t.kind < icc::kNone || t.kind > icc::kGrey) return;
    ++g_kinds[t.kind];
    if (t.kind == icc::kNone) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(&t);
        bool zero = true;
        for (size_t i = 0; i < sizeof(t); ++i) zero = zero && p[i] == 0;
        CHECK(zero);
    }
    for (int k = 0; k < 9; ++k) CHECK(t.m[k] > -65536 && t.m[k] < 65536);      // (lin is u16: 0..65535 by its type)
}
static void run_profile(const uint8_t* p, size_t n, int components) {
    // (an exact-size heap copy: a read past the end is ASan's to find)
    Bytes copy(p, p + n);
    icc::Transform t;
    std::string why;
    const bool ok = icc::plan_profile(copy.data(), copy.size(), components, t, why);
    outcome(ok, t, why);
}
static void run_file(const uint8_t* p, size_t n) {
    Bytes copy(p, p + n);
    icc::Transform t;
    std::string why;
    const bool ok = icc::plan_file(copy.data(), copy.size(), t, why);
    outcome(ok, t, why);
}

template <typename F>
static void torture(const Bytes& valid, F&& run) {
    for (size_t n = 0; n <= valid.size(); ++n) run(valid.data(), n);
    Bytes m = valid;
    for (size_t i = 0; i < m.size(); ++i) {
        const uint8_t keep = m[i];
        for (int v = 0; v < 256; ++v) {
            if (v == keep) continue;
            m[i] = (uint8_t)v;
            run(m.data(), m.size());
        }
        m[i] = keep;
    }
}

int main() {
    const Bytes srgb_para = para(3, {2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045});
    std::vector<uint32_t> table;
    for (int i = 0; i < 64; ++i) table.push_back((uint32_t)(65535.0 * (i / 63.0) * (i / 63.0)));
    std::vector<std::pair<Bytes, int>> profiles = {
        {rgb_profile(kP3, srgb_para, srgb_para, srgb_para, 4), 3},
        {rgb_profile(kAdobe, curv({563}), curv({563}), curv({563}), 2), 3},
        {rgb_profile(kSrgb, srgb_para, srgb_para, srgb_para, 2), 3},
        {rgb_profile(kP3, curv({}), curv(table), para(0, {2.2}), 2), 3},
        {rgb_profile(kAdobe, para(1, {2.2, 0.95, 0.05}), para(2, {2.0, 0.9, 0.05, 0.02}), para(4, {2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, 0.01, 0.0}), 4), 3},
        {profile({{"kTRC", curv({563})}}, "GRAY", 2), 1},
        {profile({{"kTRC", curv(table)}}, "GRAY", 4), 1},
    };
    // the valid ones first: what they must be
    {
        icc::Transform t; std::string why;
        CHECK(icc::plan_profile(profiles[0].first.data(), profiles[0].first.size(), 3, t, why) && t.kind == icc::kMatrix);
        CHECK(icc::plan_profile(profiles[2].first.data(), profiles[2].first.size(), 3, t, why) && t.kind == icc::kIdentity);
        CHECK(icc::plan_profile(profiles[5].first.data(), profiles[5].first.size(), 1, t, why) && t.kind == icc::kGrey);
        CHECK(icc::plan_profile(profiles[0].first.data(), profiles[0].first.size(), 1, t, why) && t.kind == icc::kNone);
        CHECK(icc::enc_tables().verified);
    }
    for (const auto& p : profiles) {
        const int comp = p.second;
        torture(p.first, [&](const uint8_t* d, size_t n) { run_profile(d, n, comp); });
    }
    // a JPEG head: SOI, APP0, the first profile in three APP2 chunks out of order, a frame header of three components, SOS
    Bytes file = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    const Bytes& pr = profiles[0].first;
    const size_t step = (pr.size() + 2) / 3;
    for (int k : {1, 2, 0}) {
        const size_t a = step * (size_t)k, b = std::min(pr.size(), a + step);
        file.push_back(0xFF); file.push_back(0xE2);
        be16(file, (uint32_t)(2 + 14 + (b - a)));
        const char* id = "ICC_PROFILE";
        file.insert(file.end(), id, id + 12);
        file.push_back((uint8_t)(k + 1)); file.push_back(3);
        file.insert(file.end(), pr.begin() + (long)a, pr.begin() + (long)b);
    }
    const uint8_t sof[] = {0xFF, 0xC0, 0x00, 0x11, 8, 0, 24, 0, 40, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
    file.insert(file.end(), sof, sof + sizeof(sof));
    const uint8_t sos[] = {0xFF, 0xDA, 0x00, 0x0C, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0, 0x12, 0x34};
    file.insert(file.end(), sos, sos + sizeof(sos));
    {
        icc::Transform t, want; std::string why;
        CHECK(icc::plan_file(file.data(), file.size(), t, why) && t.kind == icc::kMatrix);
        CHECK(icc::plan_profile(pr.data(), pr.size(), 3, want, why) && std::memcmp(&t, &want, sizeof(t)) == 0);
    }
    torture(file, [&](const uint8_t* d, size_t n) { run_file(d, n); });

    std::printf("%ld runs: none %ld, identity %ld, matrix %ld, grey %ld, refused %ld\n", g_runs, g_kinds[0], g_kinds[1], g_kinds[2], g_kinds[3], g_refused);
    CHECK(g_kinds[0] > 0 && g_kinds[2] > 0 && g_kinds[3] > 0 && g_refused > 0);
    if (g_fail) { std::fprintf(stderr, "icc_fuzz: %d check(s) failed\n", g_fail); return 1; }
    std::printf("icc_fuzz ok\n");
    return 0;
}
