// persist_walk.cpp -- test infrastructure: csrc/persist.hpp (the header every persistent conv kernel includes) compiled for the
// host, walked with next() by every workgroup of a list of geometries in both directions, and printed.  tests/test_persist_walk.py
// checks the lines against its own from-scratch decode.
//
// One line per (geometry, grid size G, direction, workgroup):
//   tiles_x tiles_y nimg nblocks nkc G reverse block S my_items first_img last_img | img,ty,tx,nb,tile,kc ... | img,ty,tx,nb,tile,kc x3
// the first list holds the S stages in the order the cursor hands them out (`cur`, then next() S - 1 times), the second what three
// further next() calls return (the clamp past the last stage).
#include <cstdio>

#include "../../image_restoration_platform_amd/csrc/persist.hpp"

namespace {

struct Geo { int tiles_x, tiles_y, nimg, nblocks, nkc; };
const Geo kGeos[] = {{1, 1, 1, 1, 1}, {3, 2, 3, 2, 4}, {11, 13, 3, 1, 2}, {32, 64, 8, 1, 1}, {4, 8, 8, 2, 16}, {2, 1, 5, 4, 8},
                     {5, 3, 2, 3, 1}, {64, 32, 1, 2, 2}};
const int kGrids[] = {1, 3, 8, 12, 256, 5, 512};

void put(const ire::PersistStage& st) {
    std::printf(" %d,%d,%d,%d,%d,%d", st.it.img, st.it.ty, st.it.tx, st.it.nb, st.it.tile, st.kc);
}

}  // namespace

int main() {
    for (const Geo& g : kGeos)
        for (int G : kGrids)
            for (int rev = 0; rev < 2; ++rev)
                for (int b = 0; b < G; ++b) {
                    ire::PersistCursor c(g.tiles_x, g.tiles_y, g.nimg, g.nblocks, g.nkc, G, b, rev != 0);
                    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d |", g.tiles_x, g.tiles_y, g.nimg, g.nblocks, g.nkc, G, rev, b, c.S, c.my_items,
                                c.first_img, c.last_img);
                    if (c.S > 0) put(c.cur);
                    for (int s = 1; s < c.S; ++s) put(c.next());
                    std::printf(" |");
                    for (int k = 0; k < 3; ++k) put(c.next());
                    std::printf("\n");
                }
    return 0;
}
