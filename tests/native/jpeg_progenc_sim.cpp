// jpeg_progenc_sim.cpp -- csrc/jpeg_progenc_core.hpp on the CPU: the walk of jpeg_progenc.hip's count and emit kernels, the table
// builder between them (jpeg_huff_core.hpp, lanes as a loop) and the gather's head pieces, for comparison with
// tests/jpeg_progenc_model.py (tests/test_jpeg_progenc_native.py compiles this with -fsanitize=address,undefined).  Commands on
// standard input:
//   F h w q s          "F h w q s: file_bound base64_bound"
//   C name h w q s     and on the next line the image's coefficients ([blocks][64], the core's layout):
//                      "C name: length hex | the seven event counts"
// Every interval is emitted into a heap buffer of exactly its bound (rounded up to the sink's 8-byte words), so ASan sees a store
// beyond it.
//   "--poison BYTE" as the program's arguments (sim_poison.hpp): the correction words and the table builder's work area (LDS), the codes,
//   tables and symbol counts (device scratch the table kernel writes) and every interval's buffer start as that byte; the histograms
//   stay zero: jpeg_progenc.hip clears exactly n * kTables * 256 words of them in front of the count pass.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/jpeg_tables.hpp"
#include "sim_poison.hpp"

using simpoison::dirty;

using namespace ire;
using namespace ire::jpegprog;

struct CountSink {
    uint32_t* hist;
    void sym(int slot, int s) { ++hist[slot * 256 + s]; }
    void bits(uint32_t, unsigned) {}
};

int main(int argc, char** argv) {
    simpoison::take_poison(argc, argv);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "F") {
            int h, w, q, s;
            in >> h >> w >> q >> s;
            std::printf("F %d %d %d %d: %zu %zu\n", h, w, q, s, jpegtab::jpeg_prog_file_bound(h, w, q, s), jpegtab::jpeg_prog_base64_bound(h, w, q, s));
        } else if (cmd == "C") {
            std::string name;
            int h, w, q, s;
            in >> name >> h >> w >> q >> s;
            const Geom g = geom_of(h, w, s);
            std::vector<int16_t> coefs((size_t)g.nblocks * 64);
            std::string data;
            std::getline(std::cin, data);
            std::istringstream din(data);
            for (auto& c : coefs) { int v; din >> v; c = (int16_t)v; }
            if (!din) { std::fprintf(stderr, "bad coefficient line\n"); return 2; }
            Events ev{};
            std::vector<uint32_t> corr = dirty<uint32_t>(kCorrWords);
            std::vector<uint32_t> hist(kTables * 256, 0u), codes = dirty<uint32_t>(kTables * 256);
            CountSink cs{hist.data()};
            for (int sc = 0; sc < kScans; ++sc)
                for (unsigned r = 0; r < scan_rows(g, sc); ++r) walk_interval(g, sc, r, coefs.data(), cs, corr.data(), 1u, &ev);
            std::vector<unsigned char> bv = dirty<unsigned char>(kTables * jpeghuff::kBitsVals);
            std::vector<int32_t> nv = dirty<int32_t>(kTables);
            for (int t = 0; t < kTables; ++t) {
                jpeghuff::HostWave wv;
                jpeghuff::Work* work = new jpeghuff::Work();
                simpoison::soil(work, 1);
                jpeghuff::build_table(wv, *work, hist.data() + t * 256, bv.data() + t * jpeghuff::kBitsVals, &nv[t], codes.data() + t * 256);
                delete work;
            }
            const jpegtab::JpegHeader fixed = jpegtab::jpeg_header(h, w, q, s);
            std::vector<unsigned char> file(fixed.b, fixed.b + kFixedHead);
            file[2 + 18 + 69 + 69 + 1] = 0xc2;
            const size_t bound = jpegtab::jpeg_prog_file_bound(h, w, q, s);
            for (int sc = 0; sc < kScans; ++sc) {
                const unsigned hb = scan_head_bytes(g, sc, nv.data());
                if (hb > jpegtab::kProgScanHeadMax) { std::fprintf(stderr, "scan head of %u bytes\n", hb); return 3; }
                for (unsigned k = 0; k < hb; ++k) file.push_back(scan_head_byte(g, sc, k, bv.data(), nv.data()));
                const size_t ibound = jpegtab::prog_interval_bound(g, q, sc), cap = (ibound + 7) / 8 * 8;      // (the sink stores words of 8 bytes)
                for (unsigned r = 0; r < scan_rows(g, sc); ++r) {
                    std::vector<unsigned char>* buf = new std::vector<unsigned char>(dirty<unsigned char>(cap));
                    ByteSink bs{buf->data(), 0u, (unsigned)cap, codes.data(), 0, 0ull, 0u, 0ull};
                    walk_interval(g, sc, r, coefs.data(), bs, corr.data(), 1u, nullptr);
                    bs.finish(r + 1 == scan_rows(g, sc) ? 0 : 0xd0 + (int)(r & 7u));
                    if (bs.n > ibound) { std::fprintf(stderr, "C %s: scan %d row %u: %u bytes, bound %zu\n", name.c_str(), sc, r, bs.n, ibound); return 3; }
                    file.insert(file.end(), buf->begin(), buf->begin() + bs.n);
                    delete buf;
                }
            }
            file.push_back(0xff); file.push_back(0xd9);
            if (file.size() > bound) { std::fprintf(stderr, "C %s: %zu bytes, bound %zu\n", name.c_str(), file.size(), bound); return 3; }
            std::printf("C %s: %zu ", name.c_str(), file.size());
            for (unsigned char b : file) std::printf("%02x", b);
            std::printf(" | %u %u %u %u %u %u %u\n", ev.eobrun_restart, ev.eobrun_block, ev.eobrun_early, ev.zrl_first, ev.zrl_refine, ev.shifted_to_zero, ev.dc_negative);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
