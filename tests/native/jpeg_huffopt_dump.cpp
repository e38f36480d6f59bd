// jpeg_huffopt_dump.cpp -- csrc/jpeg_huff_core.hpp and the any-table part of csrc/jpeg_tables.hpp on the CPU, for comparison with
// tests/jpeg_huffopt_model.py (tests/test_jpeg_huffopt_model.py compiles this with -fsanitize=address,undefined).  The table builder
// is the kernel's own code with the 64 lanes as a loop (jpeghuff::HostWave).  Commands, one per line of standard input:
//   B                      every (quality, sampling): "B q s: mcu_bits_any raw_bytes fits_any_class"
//   F h w q s              "F h w q s: file_bound base64_bound"
//   T name c0 .. c255      a table from 256 counts: "T name: longest nvals | bits x 16 | vals x nvals"; the code array is checked
//                          against jpegtab::huff_codes of the same bits and vals
//   H h w q s              the head with the last four tables of T commands (in DHT order): "H h w q s: length hex"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/jpeg_tables.hpp"

using namespace ire;

int main() {
    std::vector<std::vector<unsigned char>> tabs;       // each kBitsVals bytes
    std::vector<int32_t> nv;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "B") {
            for (int q = 1; q <= 100; ++q)
                for (int s : {0, 2}) {
                    const unsigned mb = jpegtab::mcu_bits_any(q, s);
                    std::printf("B %d %d: %u %u %d\n", q, s, mb, jpegtab::raw_bound_of(s, mb), jpegtab::fits_any_class(s, mb) ? 1 : 0);
                }
        } else if (cmd == "F") {
            int h, w, q, s;
            in >> h >> w >> q >> s;
            std::printf("F %d %d %d %d: %zu %zu\n", h, w, q, s, jpegtab::jpeg_opt_file_bound(h, w, q, s), jpegtab::jpeg_opt_base64_bound(h, w, q, s));
        } else if (cmd == "T") {
            std::string name;
            in >> name;
            std::vector<uint32_t> counts(256);
            for (auto& c : counts) in >> c;
            if (!in) { std::fprintf(stderr, "bad T line\n"); return 2; }
            std::vector<unsigned char> bv(jpeghuff::kBitsVals);
            std::vector<uint32_t> codes(256);
            int32_t n = -1;
            jpeghuff::HostWave wv;
            jpeghuff::Work* work = new jpeghuff::Work;      // (on the heap: ASan sees its ends)
            const int longest = jpeghuff::build_table(wv, *work, counts.data(), bv.data(), &n, codes.data());
            delete work;
            const jpegtab::HuffCodes ref = jpegtab::huff_codes(bv.data(), bv.data() + 16);
            for (int k = 0; k < 256; ++k)
                if (ref.code[k] != codes[k]) { std::fprintf(stderr, "code of symbol %d: %x, Annex C gives %x\n", k, codes[k], ref.code[k]); return 3; }
            std::printf("T %s: %d %d |", name.c_str(), longest, n);
            for (int k = 0; k < 16; ++k) std::printf(" %d", bv[k]);
            std::printf(" |");
            for (int k = 0; k < n; ++k) std::printf(" %d", bv[16 + k]);
            std::printf("\n");
            tabs.push_back(bv);
            nv.push_back(n);
        } else if (cmd == "H") {
            int h, w, q, s;
            in >> h >> w >> q >> s;
            if (tabs.size() < 4) { std::fprintf(stderr, "H needs four tables\n"); return 2; }
            std::vector<unsigned char> bv;
            for (size_t t = tabs.size() - 4; t < tabs.size(); ++t) bv.insert(bv.end(), tabs[t].begin(), tabs[t].end());
            std::vector<unsigned char> out(jpegtab::kHeaderBytes);
            const size_t n = jpegtab::jpeg_header_opt(h, w, q, s, bv.data(), nv.data() + nv.size() - 4, out.data());
            if (n > out.size()) { std::fprintf(stderr, "head of %zu bytes\n", n); return 3; }
            std::printf("H %d %d %d %d: %zu ", h, w, q, s, n);
            for (size_t k = 0; k < n; ++k) std::printf("%02x", out[k]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
