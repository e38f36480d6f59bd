// conv_kind.hpp -- the seven convolution kinds, the integers of their v1 weight slabs and the network's fixed sizes; no HIP, no device
// code: shared by the launch interface (conv_mfma.hpp), by the host-only weight packer (weight_pack.hpp), by the launch rule book
// (conv_plan.hpp) and by the buffer tables (device_buf.hpp).
#pragma once
#include <cstddef>

namespace ire {

// RestoreNet-v0's fixed sizes: channels per level, and the FiLM vector (a scale and a shift per channel of every level, level l at kFilmOff[l])
constexpr int kWidths[4] = {32, 64, 128, 256}, kFilmOff[4] = {0, 64, 192, 448}, kFilmDim = 960;
// floats of GroupNorm partials one h x w image needs at most: [8 groups][2] per 4 x 32-pixel tile of level 0, the smallest tile any producer uses
inline size_t gn_partials(int h, int w) { return (size_t)((h + 3) / 4) * ((w + 31) / 32) * 16; }

// The seven ways RestoreNet-v0 uses a convolution (DESIGN.md "RestoreNet-v0").
enum ConvKind {
    CONV_STEM,  // u8 RGB (padded to 8 ch) -> 32, 3x3, GroupNorm stats out
    CONV_RB1,   // C->C 3x3, GN+FiLM+SiLU prologue, stats out
    CONV_RB2,   // C->C 3x3, GN+FiLM+SiLU prologue, + residual, stats out
    CONV_DOWN,  // C->2C 3x3 stride 2, stats out
    CONV_UP,    // nearest x2 then 2C->C 3x3
    CONV_FUSE,  // concat(up, skip) 2C->C 1x1, stats out
    CONV_HEAD   // GN+SiLU prologue, 32->3 3x3, out = clamp(round(input + y)) u8
};

// output channels per workgroup
inline int conv_nt(ConvKind kind, int cout) {
    if (kind == CONV_STEM || kind == CONV_HEAD) return 32;
    return cout >= 64 ? 64 : 32;
}
// MFMA k-steps per K-chunk (weight slab = nsteps*2*NT*16 B)
inline int conv_nsteps(ConvKind kind) {
    switch (kind) {
        case CONV_STEM: return 5;   // 9 taps x 1 chunk, padded to 10 kk
        case CONV_FUSE: return 2;   // 1 tap x 4 chunks
        default: return 18;         // 9 taps x 4 chunks
    }
}
// output rows per workgroup tile (columns: 32): the v1 template (conv_mfma.hip) ...
inline int conv_tile_h(ConvKind kind) { return kind == CONV_DOWN ? 4 : 8; }
// ... and the persistent pipelined kernels (conv_rb.hip and every kernel after it)
constexpr int kRbTileH = 16;

}  // namespace ire
