// classifier_grid.hpp -- the launch geometry of the classifier scan (classifier.hip), on the host; no HIP, no device code.  The tile
// size, the extents of the scan's scratch block and the rule that gives an image its workgroups: pure integer functions that
// tests/native/classifier_grid_dump.cpp sweeps with plain g++ under the sanitizers, and that tests/classifier_grid.py restates so that
// every GPU case can assert which geometry it reaches.
#pragma once
#include <algorithm>

namespace ire {

constexpr int CT_H = 16, CT_W = 256;            // output tile: 16 rows x 64 four-pixel groups
constexpr int CLS_MAX_WG = 768;              // three workgroups per CU (42 KB of LDS, 142 VGPRs each)
constexpr int CLS_TICKET_CAP = 64;              // >= max_batch of any engine (ire_config: 1..64)

struct ClsTiles { int tiles_x, tiles_y; };
inline ClsTiles cls_tiles(int h, int w) { return {(w + CT_W - 1) / CT_W, (h + CT_H - 1) / CT_H}; }

// Workgroups per image (gridDim.x) of a launch of `n` images with `ntiles` tiles each: three workgroups per CU chip-wide, an equal
// number of tiles each where the counts allow; every workgroup amortises its 9 KB table load over its tiles.  n * result <= CLS_MAX_WG
// (the rows of `parts`), and balancing never adds a round to the ceil(ntiles / min(ntiles, CLS_MAX_WG / n)) of the unbalanced split.
inline int cls_workgroups_per_image(int n, int ntiles) {
    int per_img = std::max(1, std::min(ntiles, CLS_MAX_WG / std::max(1, n)));
    const int rounds = (ntiles + per_img - 1) / per_img;
    return (ntiles + rounds - 1) / rounds;
}

}  // namespace ire
