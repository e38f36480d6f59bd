// weight_pack_dump.cpp -- csrc/weight_pack.hpp on the host alone (test infrastructure; libire.so includes the same header):
// parses a weight file, packs the whole network in the order Engine::load_weights does, and prints per convolution its
// scalars and per packed array `<layer>.<field> <bytes> <FNV-1a-64 of the bytes>`.  A blob the parser refuses prints
// `error <code> <text>` and exits 3.      usage: weight_pack_dump <weights.bin> <0 = bf16 | 1 = fp8>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "../../image_restoration_platform_amd/csrc/weight_pack.hpp"

using namespace ire;

template <class T>
static void dump(const std::string& layer, const char* field, const std::vector<T>& v) {
    if (v.empty()) return;
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)v.data();
    const size_t n = v.size() * sizeof(T);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    std::printf("%s.%s %zu %016llx\n", layer.c_str(), field, n, h);
}

static void dump(const std::string& name, const PackedConv& c) {
    std::printf("%s meta nt=%d nblocks=%d nkc=%d kc_split=%d cin0=%d cin1=%d\n", name.c_str(), c.nt, c.nblocks, c.nkc, c.kc_split, c.cin0, c.cin1);
#define DUMP(f) dump(name, "d_" #f, c.f);
    DUMP(w) DUMP(wp) DUMP(w4) DUMP(w4h) DUMP(wstem) DUMP(wd) DUMP(wu) DUMP(wuf) DUMP(wdq) DUMP(wuq) DUMP(wsq) DUMP(wsk)
    DUMP(bias_uf) DUMP(w8x) DUMP(w8) DUMP(oscale) DUMP(bias8) DUMP(bias)
#undef DUMP
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
    if (!f) return 2;
    std::vector<char> blob((size_t)f.tellg());
    f.seekg(0);
    f.read(blob.data(), (std::streamsize)blob.size());
    const bool fp8 = std::atoi(argv[2]) != 0;
    const int W[4] = {32, 64, 128, 256};
    try {
        const TensorMap tm = parse_weights(blob.data(), blob.size());
        auto conv = [&](ConvKind kind, const std::string& nm, int cin, int cout) { dump(nm, pack_conv(tm, kind, nm + ".w", nm + ".b", cin, cout, fp8)); };
        auto rb = [&](const std::string& p, int C) { conv(CONV_RB1, p + ".conv1", C, C); conv(CONV_RB2, p + ".conv2", C, C); };
        conv(CONV_STEM, "stem", 3, 32);
        for (int l = 0; l < 4; ++l) {
            const std::string s = std::to_string(l);
            for (int i = 0; i < 2; ++i) rb("enc" + s + ".rb" + std::to_string(i), W[l]);
            if (l < 3) conv(CONV_DOWN, "down" + s, W[l], W[l + 1]);
        }
        for (int i = 0; i < 2; ++i) rb("mid.rb" + std::to_string(i), 256);
        for (int l = 2; l >= 0; --l) {
            const std::string s = std::to_string(l);
            PackedConv up = pack_conv(tm, CONV_UP, "up" + s + ".w", "up" + s + ".b", W[l + 1], W[l], fp8);
            pack_up_fused(tm, up, s);
            dump("up" + s, up);
            conv(CONV_FUSE, "fuse" + s, 2 * W[l], W[l]);
            for (int i = 0; i < 2; ++i) rb("dec" + s + ".rb" + std::to_string(i), W[l]);
        }
        conv(CONV_HEAD, "head", 32, 3);
    } catch (const Error& e) {
        std::printf("error %d %s\n", e.code, e.msg.c_str());
        return 3;
    }
    return 0;
}
