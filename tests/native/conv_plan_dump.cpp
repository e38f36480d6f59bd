// conv_plan_dump.cpp -- csrc/conv_plan.hpp on the host alone (test infrastructure; libire.so includes the same header): walks the
// network's convolutions in schedule order for a list of cases and prints, per case and layer group (the profiler key), one line with
// every field of the launch plan, in the order of the header line; two ops of one group that plan differently print both lines.  The ConvDesc of a layer is what
// weight_pack.hpp's packer produces for zero weights of the layer's shape: which arrays exist depends on shapes and precision only.
// usage: conv_plan_dump fixture | props | fp8 | strips | items | large | rule
//   fixture: the recorded cases
//   props:   the cases behind the separately asserted invariants
//   fp8:     an fp8 engine under every combination of the switches that decide its C >= 128 ResBlock convolutions
//   strips:  the strips of tests/test_strips_layers_gpu.py's shapes
//   items:   the cases of tests/test_items_gpu.py at its two shapes, and the (3, 200, 328) batch under IRE_PK 0 / 1 / 2
//   large:   conv_extents -- bytes, items, stages, partials -- of every launch of tests/test_large_shapes_gpu.py's shapes and strip plans
//   rule:    piece_addressable on both sides of its boundary
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/weight_pack.hpp"

using namespace ire;

struct Case {
    std::string name;
    std::vector<std::pair<const char*, const char*>> env;
    bool fp8 = false;
    int n = 1, h = 0, w = 0;      // whole batches: h x w images.  Strips: the whole image is h x w, cut into nstrips, this is strip `strip`
    int nstrips = 0, strip = 0;
};

static std::string env_name(const std::vector<std::pair<const char*, const char*>>& env) {
    std::string s;
    for (auto& kv : env) s += (s.empty() ? "" : ",") + std::string(kv.first) + "=" + kv.second;
    return s.empty() ? "default" : s;
}

static Case whole(const std::vector<std::pair<const char*, const char*>>& env, bool fp8, int n, int h, int w) {
    Case c;
    c.env = env; c.fp8 = fp8; c.n = n; c.h = h; c.w = w;
    c.name = env_name(env) + (fp8 ? ":fp8:" : ":bf16:") + std::to_string(n) + "x" + std::to_string(h) + "x" + std::to_string(w);
    return c;
}
static Case strip_of(int H, int W, int nstrips, int s) {
    Case c;
    c.h = H; c.w = W; c.nstrips = nstrips; c.strip = s;
    c.name = "default:bf16:strip" + std::to_string(s) + "of" + std::to_string(nstrips) + ":" + std::to_string(H) + "x" + std::to_string(W);
    return c;
}

static const int kShapes[12][3] = {{1, 16, 16}, {1, 72, 136}, {2, 64, 96}, {3, 200, 328}, {12, 32, 48}, {1, 512, 512}, {8, 512, 512},
                                   {2, 1024, 1024}, {8, 1024, 1024}, {5, 1024, 1024}, {64, 64, 64}, {1, 8192, 8192}};
static const int kStripPlans[3][3] = {{1024, 1024, 2}, {1024, 1024, 8}, {2048, 1024, 4}};      // H, W, strips

// the recorded cases: 12 + 1 default + 18 switch sets x 2 + 2 x 3 fp8 + 8 strips = 63
static std::vector<Case> fixture_cases() {
    std::vector<Case> cs;
    for (auto& s : kShapes) cs.push_back(whole({}, false, s[0], s[1], s[2]));
    cs.push_back(whole({}, false, 64, 512, 512));      // 128-cout items at level 2 whose XCD ranges span 8 images: conv_pk's table refuses
    // tests/test_layers_gpu.py SWITCHES and tests/test_restore_gpu.py test_alternate_kernel_schedules_agree, and IRE_PK=1
    const std::vector<std::vector<std::pair<const char*, const char*>>> sets = {
        {{"IRE_W4", "0"}}, {{"IRE_CONV_V1", "1"}}, {{"IRE_UP_RB_MINC", "64"}}, {{"IRE_UP_SUBPIX", "0"}}, {{"IRE_UP_FUSE", "0"}},
        {{"IRE_GN_FOLD", "0"}}, {{"IRE_PC", "0"}}, {{"IRE_PC", "1"}}, {{"IRE_PC", "3"}}, {{"IRE_PC", "0"}, {"IRE_GN_FOLD", "0"}},
        {{"IRE_DOWN_RB", "0"}, {"IRE_HEAD_RB", "0"}}, {{"IRE_STEM_RB", "0"}}, {{"IRE_W4_SPLIT", "0"}}, {{"IRE_PK", "0"}}, {{"IRE_PK", "1"}},
        {{"IRE_PK", "2"}}, {{"IRE_UPQ", "0"}}, {{"IRE_DNQ", "0"}}};
    for (auto& e : sets) { cs.push_back(whole(e, false, 1, 72, 136)); cs.push_back(whole(e, false, 8, 1024, 1024)); }
    for (const char* mx : {"1", "0"})
        for (auto& s : {std::vector<int>{1, 72, 136}, {2, 128, 160}, {8, 1024, 1024}}) cs.push_back(whole({{"IRE_FP8_MX", mx}}, true, s[0], s[1], s[2]));
    for (auto& p : kStripPlans)       // the first, a middle and the last strip (two strips: first and last)
        for (int s : {0, p[2] / 2 - (p[2] > 2 ? 1 : 0), p[2] - 1})
            if (cs.back().nstrips != p[2] || cs.back().strip != s || cs.back().h != p[0]) cs.push_back(strip_of(p[0], p[1], p[2], s));
    return cs;
}

// the cases behind the separately asserted invariants: every shape of the list with n = 1..8, and every strip of the three strip
// plans next to its whole image
static std::vector<Case> property_cases() {
    std::vector<Case> cs;
    for (auto& s : kShapes)
        for (int n = 1; n <= 8; ++n) {
            const Case c = whole({}, false, n, s[1], s[2]);
            bool seen = false;
            for (auto& o : cs) seen = seen || o.name == c.name;      // the list has 512^2 twice and 1024^2 three times
            if (!seen) cs.push_back(c);
        }
    for (auto& p : kStripPlans) {
        if (p[0] != 1024) cs.push_back(whole({}, false, 1, p[0], p[1]));      // (1 x 1024 x 1024 is in the list above)
        for (int s = 0; s < p[2]; ++s) cs.push_back(strip_of(p[0], p[1], p[2], s));
    }
    return cs;
}

// an fp8 engine under IRE_FP8_MX x IRE_W4 x IRE_PK, at the shapes tests/test_layers_gpu.py gives it
static std::vector<Case> fp8_cases() {
    std::vector<Case> cs;
    for (const char* mx : {"1", "0"})
        for (const char* w4 : {"1", "0"})
            for (const char* pk : {"2", "0"})
                for (auto& s : {std::vector<int>{1, 16, 16}, {2, 200, 328}, {12, 32, 48}, {3, 72, 136}})
                    cs.push_back(whole({{"IRE_FP8_MX", mx}, {"IRE_W4", w4}, {"IRE_PK", pk}}, true, s[0], s[1], s[2]));
    return cs;
}

// the shapes tests/test_strips_layers_gpu.py runs as strips (first, a middle and the last strip of each), under the switches that decide
// which kernel and which item form the C >= 128 ResBlock convolutions get there
static std::vector<Case> strip_layer_cases() {
    std::vector<Case> cs;
    auto add = [&](const std::vector<std::pair<const char*, const char*>>& env, bool fp8, int H, int W, int n) {
        for (int s : {0, n / 2, n - 1}) {
            if (!cs.empty() && cs.back().strip == s && cs.back().nstrips == n && cs.back().h == H && cs.back().fp8 == fp8 && env_name(cs.back().env) == env_name(env)) continue;      // (two strips: first and last)
            Case c = strip_of(H, W, n, s);
            c.env = env; c.fp8 = fp8;
            c.name = env_name(env) + (fp8 ? ":fp8:" : ":bf16:") + c.name.substr(c.name.find("strip"));
            cs.push_back(c);
        }
    };
    for (auto& p : {std::vector<int>{384, 264, 3}, {1024, 264, 8}, {256, 72, 2}, {512, 264, 4}}) add({}, false, p[0], p[1], p[2]);
    add({{"IRE_PK", "0"}}, false, 1024, 264, 8);
    for (const char* mx : {"1", "0"})
        for (auto& p : {std::vector<int>{384, 264, 3}, {1024, 264, 8}}) add({{"IRE_FP8_MX", mx}}, true, p[0], p[1], p[2]);
    return cs;
}

// the cases of tests/test_items_gpu.py at its two shapes (default switches in bf16, the 128-cout items under IRE_W4_SPLIT=0 with IRE_PK 2 / 0 / 1,
// the fp8 engine in both forms, every switch set of tests/test_layers_gpu.py SWITCHES), and the batch of
// tests/test_restore_gpu.py::test_producer_consumer_c128_equals_conv_w4_bit_for_bit under IRE_PK 0 / 1 / 2 with and without IRE_W4_SPLIT=0
static std::vector<Case> item_cases() {
    std::vector<Case> cs;
    const std::vector<std::vector<std::pair<const char*, const char*>>> sets = {
        {}, {{"IRE_W4_SPLIT", "0"}}, {{"IRE_W4_SPLIT", "0"}, {"IRE_PK", "0"}}, {{"IRE_W4_SPLIT", "0"}, {"IRE_PK", "1"}},
        {{"IRE_PK", "0"}}, {{"IRE_PC", "0"}}, {{"IRE_PC", "1"}}, {{"IRE_W4", "0"}}, {{"IRE_UPQ", "0"}}, {{"IRE_DNQ", "0"}}, {{"IRE_UP_FUSE", "0"}},
        {{"IRE_UP_SUBPIX", "0"}}, {{"IRE_GN_FOLD", "0"}}, {{"IRE_DOWN_RB", "0"}, {"IRE_HEAD_RB", "0"}}, {{"IRE_STEM_RB", "0"}}};
    for (auto& s : {std::vector<int>{3, 136, 136}, {3, 72, 264}}) {
        for (auto& e : sets) cs.push_back(whole(e, false, s[0], s[1], s[2]));
        for (const char* mx : {"1", "0"}) cs.push_back(whole({{"IRE_FP8_MX", mx}}, true, s[0], s[1], s[2]));
    }
    for (const char* pk : {"0", "1", "2"}) {
        cs.push_back(whole({{"IRE_PK", pk}}, false, 3, 200, 328));
        cs.push_back(whole({{"IRE_W4_SPLIT", "0"}, {"IRE_PK", pk}}, false, 3, 200, 328));
    }
    return cs;
}

// the shapes of tests/test_large_shapes_gpu.py, whole and in the strip plans it runs (every strip), plus the shapes the issue named that
// the strip planner refuses (4224 in 8, 8128 in 8: rows per strip no multiple of 128) as whole images, and 8192 x 8192 whole: the one
// image the address rule refuses, printed so that the test sees WHY
static const int kLargeWhole[8][3] = {{1, 4224, 8192}, {1, 8064, 8192}, {1, 8128, 8192}, {1, 8184, 8192}, {1, 8192, 8184}, {1, 8192, 8192}, {1, 8192, 4224}, {64, 1024, 1024}};
static const int kLargeStrips[6][3] = {{4224, 8192, 11}, {8064, 8192, 7}, {8192, 8184, 8}, {8192, 8184, 16}, {8192, 8192, 16}, {8192, 4224, 8}};
static std::vector<Case> large_cases() {
    std::vector<Case> cs;
    for (auto& s : kLargeWhole) cs.push_back(whole({}, false, s[0], s[1], s[2]));
    cs.push_back(whole({}, true, 1, 4224, 8192));
    cs.push_back(whole({}, true, 1, 8192, 8184));
    for (auto& p : kLargeStrips)
        for (int s = 0; s < p[2]; ++s) cs.push_back(strip_of(p[0], p[1], p[2], s));
    return cs;
}

// ---- the network's convolutions as weight_pack.hpp packs them (zero weights: existence of an array is a matter of shape) ----
static const int kW[4] = {32, 64, 128, 256};
struct NetDesc {
    ConvDesc stem, head, rb1[4], rb2[4], down[3], up[3], fuse[3];      // every ResBlock of a level packs alike
};
static void zeros(TensorMap& tm, const std::string& nm, std::vector<int> dims) {
    Tensor t;
    size_t n = 1;
    for (int d : dims) n *= (size_t)d;
    t.dims = std::move(dims);
    t.data.assign(n, 0.f);
    tm[nm] = std::move(t);
}
static ConvDesc desc_of(ConvKind kind, int cin, int cout, bool fp8) {
    TensorMap tm;
    const int ks = kind == CONV_FUSE ? 1 : 3;
    zeros(tm, "c.w", {cout, cin, ks, ks});
    zeros(tm, "c.b", {cout});
    return conv_desc(pack_conv(tm, kind, "c.w", "c.b", cin, cout, fp8));
}
static NetDesc net_desc(bool fp8) {
    NetDesc n;
    n.stem = desc_of(CONV_STEM, 3, 32, fp8);
    n.head = desc_of(CONV_HEAD, 32, 3, fp8);
    for (int l = 0; l < 4; ++l) { n.rb1[l] = desc_of(CONV_RB1, kW[l], kW[l], fp8); n.rb2[l] = desc_of(CONV_RB2, kW[l], kW[l], fp8); }
    for (int l = 0; l < 3; ++l) {
        n.down[l] = desc_of(CONV_DOWN, kW[l], kW[l + 1], fp8);
        n.fuse[l] = desc_of(CONV_FUSE, 2 * kW[l], kW[l], fp8);
        const std::string s = std::to_string(l);
        TensorMap tm;
        zeros(tm, "up" + s + ".w", {kW[l], kW[l + 1], 3, 3}); zeros(tm, "up" + s + ".b", {kW[l]});
        zeros(tm, "fuse" + s + ".w", {kW[l], 2 * kW[l], 1, 1}); zeros(tm, "fuse" + s + ".b", {kW[l]});
        PackedConv up = pack_conv(tm, CONV_UP, "up" + s + ".w", "up" + s + ".b", kW[l + 1], kW[l], fp8);
        pack_up_fused(tm, up, s);
        n.up[l] = conv_desc(up);
    }
    return n;
}

static const char* kKernel[] = {"V1", "F8", "PK", "W4", "PC", "RB", "PC_HEAD", "RB_HEAD", "DNQ", "DOWN", "STEM", "UPQ", "UP_FUSED", "UP_SUB", "UP_RB"};
static const char* kSlab[] = {"none", "w", "wp", "w4", "w4h", "wstem", "wd", "wu", "wuf", "wdq", "wuq", "wsq", "wsk", "w8x", "w8"};
static const char* kBias[] = {"bias", "bias_uf", "bias8"};

static bool g_extents = false;      // mode `large`: conv_extents of every launch instead of the plan's fields

static void run_case(const Case& c, const NetDesc& net) {
    static const char* vars[] = {"IRE_CONV_V1", "IRE_RB_PRIO", "IRE_W4", "IRE_W4_SPLIT", "IRE_UP_RB_MINC", "IRE_UP_SUBPIX", "IRE_UP_FUSE", "IRE_GN_FOLD", "IRE_PC",
                                 "IRE_PK", "IRE_UPQ", "IRE_DNQ", "IRE_HEAD_RB", "IRE_DOWN_RB", "IRE_STEM_RB", "IRE_FP8_MX"};
    for (const char* v : vars) unsetenv(v);
    for (auto& kv : c.env) setenv(kv.first, kv.second, 1);
    const ConvSwitches sw = ConvSwitches::from_env();
    ConvSite geo;          // Engine::geo_of_lane, or StripSession's strips
    geo.cus = 256;         // MI355X
    if (c.nstrips) {
        const int hr = c.h / c.nstrips;
        geo.nimg = 1; geo.h = hr; geo.w = c.w; geo.halo = 1; geo.H = c.h; geo.y0 = c.strip * hr;
        geo.has_up = c.strip > 0; geo.has_down = c.strip + 1 < c.nstrips;
    } else { geo.nimg = c.n; geo.h = c.h; geo.w = c.w; geo.H = c.h; }
    std::vector<std::pair<std::string, std::string>> lines;      // (group, line) in schedule order, one per distinct line of a group
    auto conv = [&](const ConvDesc& d, int lin, int lout, bool use_ab, bool has_in1) {
        ConvSite s = geo;
        s.lin = lin; s.lout = lout; s.use_ab = use_ab; s.has_in1 = has_in1;
        s.stats_out = conv_feeds_gn(d.kind, d.kind == CONV_UP && has_in1);
        const ConvPlan p = plan_conv(sw, d, s, c.fp8);
        const long long in1_off = !has_in1 ? -1 : p.in1_first_row ? (long long)s.halo * (s.w >> lout) * d.cout : 0;
        char buf[1024];
        if (g_extents) {
            const ConvExtents e = conv_extents(p, d, s);
            std::snprintf(buf, sizeof buf, "%s %s %llu %llu %llu %llu %lld %lld %lld %d %d %d %d", kKernel[p.kernel], p.kname, e.in0_bytes, e.in1_bytes, e.out_bytes,
                          e.batch_bytes, e.items, e.stages, e.stat_floats, p.tiles_x, p.tiles_y, p.nblocks, p.nkc);
            for (auto& gl : lines) if (gl.first == p.key && gl.second == buf) return;
            lines.emplace_back(p.key, buf);
            return;
        }
        std::snprintf(buf, sizeof buf, "%s %d %d %s %s %s %s %d %d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %lld %d %d %d %.0f %.0f %.0f",
                      kKernel[p.kernel], (int)p.resid, (int)p.fused_act, p.kname, kSlab[p.w], kSlab[p.w1], kBias[p.bias], p.zeros ? 1 : 0, p.cin1, p.nkc,
                      p.nblocks, p.w4_nt, p.fp8, p.cout, p.group_size, in1_off, p.tile_h, p.tiles_x, p.tiles_y, p.iy_lo, p.iy_span, p.in_rows,
                      p.in_row_off, p.parts_mul, p.stats_level, p.ty0, s.stats_out ? p.stats_offset() : -1, p.stat_parts, (int)p.folds_gn, p.fam,
                      p.flops, p.flops_exec, p.bytes);
        for (auto& gl : lines) if (gl.first == p.key && gl.second == buf) return;
        lines.emplace_back(p.key, buf);
    };
    // Engine::build_program
    auto resblock = [&](int l) { conv(net.rb1[l], l, l, true, false); conv(net.rb2[l], l, l, true, false); };
    conv(net.stem, 0, 0, false, false);
    for (int l = 0; l < 4; ++l) {
        resblock(l); resblock(l);
        if (l < 3) conv(net.down[l], l, l + 1, false, false);
    }
    resblock(3); resblock(3);
    for (int l = 2; l >= 0; --l) {
        if (up_is_composed(sw, net.up[l])) conv(net.up[l], l + 1, l, false, true);
        else { conv(net.up[l], l + 1, l, false, false); conv(net.fuse[l], l, l, false, true); }
        resblock(l); resblock(l);
    }
    conv(net.head, 0, 0, true, false);
    for (auto& gl : lines) std::printf("%s %s %s\n", c.name.c_str(), gl.first.c_str(), gl.second.c_str());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string mode = argv[1];
    if (mode == "rule") {
        // the address rule (piece_addressable) on both sides of its boundary: `rule ROWS W HALO answer level-0-bytes`
        static const int q[][3] = {{8192, 8192, 0}, {8184, 8192, 0}, {8192, 8184, 0}, {8128, 8192, 0}, {8064, 8192, 0}, {4224, 8192, 0}, {4096, 8192, 0},
                                   {8192, 4224, 0}, {1024, 1024, 0}, {16, 16, 0}, {8192, 8192, 1}, {8190, 8192, 1}, {8189, 8192, 1}, {8184, 8192, 1},
                                   {4096, 8192, 1}, {1152, 8192, 1}, {512, 8192, 1}, {384, 8192, 1}, {1024, 4224, 1}};
        for (auto& r : q) std::printf("rule %d %d %d %d %llu\n", r[0], r[1], r[2], piece_addressable(r[0], r[1], r[2]) ? 1 : 0, piece_tensor_bytes(r[0], r[1], r[2], 0));
        std::printf("end %llu\n", kTensorBytesEnd);
        return 0;
    }
    if (mode != "fixture" && mode != "props" && mode != "fp8" && mode != "strips" && mode != "items" && mode != "large") return 2;
    const NetDesc bf16 = net_desc(false), fp8 = net_desc(true);
    if (mode == "large") {
        g_extents = true;
        std::printf("# case group kernel kname in0_bytes in1_bytes out_bytes batch_bytes items stages stat_floats tiles_x tiles_y nblocks nkc\n");
        for (const Case& c : large_cases()) run_case(c, c.fp8 ? fp8 : bf16);
        return 0;
    }
    std::printf("# case group kernel resid fused_act kname w w1 bias zeros cin1 nkc nblocks w4_nt fp8 cout group_size in1_off tile_h tiles_x tiles_y iy_lo iy_span in_rows in_row_off parts_mul stats_level ty0 stats_off stat_parts folds_gn fam flops flops_exec bytes\n");
    for (const Case& c : mode == "props" ? property_cases() : mode == "fp8" ? fp8_cases() : mode == "strips" ? strip_layer_cases() : mode == "items" ? item_cases() : fixture_cases()) run_case(c, c.fp8 ? fp8 : bf16);
    return 0;
}
