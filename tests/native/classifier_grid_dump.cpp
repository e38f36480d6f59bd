// classifier_grid_dump.cpp -- test infrastructure: csrc/classifier_grid.hpp (the header classifier.hpp and classifier.hip include)
// compiled for the host alone and printed.  tests/test_classifier_grid.py checks the lines against the rule's stated properties and
// against its own restatement (tests/classifier_cases.py::classifier_grid).
//
//   C CT_H CT_W CLS_MAX_WG CLS_TICKET_CAP                 the constants
//   T v tiles_x tiles_y                                   cls_tiles(v, v) for every side v in 1..8192
//   G n ntiles per_img                                    cls_workgroups_per_image for every n in 1..64 and every tile count an
//                                                         image of at most 8192 x 8192 can have (a product tiles_x * tiles_y)
#include <cstdio>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/classifier_grid.hpp"

int main() {
    std::printf("C %d %d %d %d\n", ire::CT_H, ire::CT_W, ire::CLS_MAX_WG, ire::CLS_TICKET_CAP);
    const int kMaxSide = 8192;
    for (int v = 1; v <= kMaxSide; ++v) {
        const ire::ClsTiles t = ire::cls_tiles(v, v);
        std::printf("T %d %d %d\n", v, t.tiles_x, t.tiles_y);
    }
    const ire::ClsTiles top = ire::cls_tiles(kMaxSide, kMaxSide);
    std::vector<char> has((size_t)top.tiles_x * top.tiles_y + 1, 0);
    for (int tx = 1; tx <= top.tiles_x; ++tx)
        for (int ty = 1; ty <= top.tiles_y; ++ty) has[(size_t)tx * ty] = 1;
    for (int n = 1; n <= ire::CLS_TICKET_CAP; ++n)
        for (int nt = 1; nt <= top.tiles_x * top.tiles_y; ++nt)
            if (has[(size_t)nt]) std::printf("G %d %d %d\n", n, nt, ire::cls_workgroups_per_image(n, nt));
    return 0;
}
