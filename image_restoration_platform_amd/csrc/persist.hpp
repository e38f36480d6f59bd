// persist.hpp -- work distribution of the persistent convolution kernels (conv_pc, conv_pk, conv_w4, conv_stem, ...): which (image, tile,
// n-block, k-chunk) a workgroup runs in its s-th pipeline stage.
//
// Items L = ((img * tiles_per_img + ty * tiles_x + tx) * nblocks + nb) are dealt XCD-aware: the workgroups that share an XCD
// (blockIdx % 8: a label, not an id) walk one contiguous eighth [lo, hi) of the item range, workgroup jx of the group taking
// L = lo + jx, lo + jx + nwx, ...  (halo rows and the n-blocks of a tile are then served by that XCD's L2; speed only).
// A workgroup's stages are consecutive (item k, k-chunk kc), so the cursor advances by additions and carries: the integer
// divisions of a from-scratch decode (4 per stage, ~100 scalar instructions) run once, in the constructor.
#pragma once

// The cursor is integer arithmetic only: a kernel passes gridDim.x / blockIdx.x in, and a host build (plain g++, tests/native/
// persist_walk.cpp) compiles the same code with the qualifier empty.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define IRE_HD __host__ __device__ __forceinline__
#else
#define IRE_HD inline
#endif

namespace ire {

struct PersistItem { int img, ty, tx, nb, tile; };
struct PersistStage { PersistItem it; int kc; };

// Walk direction (ConvArgs::walk_rev): a workgroup's SET of items is the same either way; reverse hands them out last item
// first -- L = lo + jx + (my_items - 1 - k) * nwx -- so that a launch starts on the rows the launch before it touched last, which the
// Infinity Cache still holds.  The k-chunks of an item count up in both directions.
struct PersistCursor {
    int S;                      // stages this workgroup runs (items x nkc); 0: nothing to do
    int my_items;
    // geometry
    int nkc, nblocks, tiles_x, tiles_y;
    // the stride decomposed: nwx = ((d_img * tiles_y + d_ty) * tiles_x + d_tx) * nblocks + d_nb.  Reverse: the digits of -nwx in the same
    // mixed radix, as a complement -- d_nb, d_tx, d_ty within their radix as ever, the borrows gathered in a negative d_img -- so that
    // next() steps backwards with the additions and carries it steps forwards with
    int d_img, d_ty, d_tx, d_nb;
    int s;                      // stage the cursor points at
    PersistStage cur;
    int first_img, last_img;    // lowest and highest image among this workgroup's items (gn_fold.hpp, the coefficient tables)

    IRE_HD PersistCursor(int tiles_x_, int tiles_y_, int nimg, int nblocks_, int nkc_, int G, int block, bool reverse) {
        tiles_x = tiles_x_; tiles_y = tiles_y_; nblocks = nblocks_; nkc = nkc_;
        const int tiles_per_img = tiles_x * tiles_y;
        const int items = tiles_per_img * nimg * nblocks;
        const int X = G < 8 ? G : 8;
        const int xcd = block % X, jx = block / X;
        const int nwx = (G - xcd + X - 1) / X;                        // workgroups in this XCD group
        const int lo = (int)((long long)items * xcd / X), hi = (int)((long long)items * (xcd + 1) / X);
        my_items = (lo + jx < hi) ? (hi - lo - jx + nwx - 1) / nwx : 0;
        S = my_items * nkc;
        auto split = [&](int L, int& img, int& ty, int& tx, int& nb) {
            nb = L % nblocks;
            const int t = L / nblocks;
            img = t / tiles_per_img;
            const int tile = t - img * tiles_per_img;
            ty = tile / tiles_x;
            tx = tile - ty * tiles_x;
        };
        split(nwx, d_img, d_ty, d_tx, d_nb);
        const int L_lo = lo + jx, span = my_items > 0 ? (my_items - 1) * nwx : 0;      // first item, and how far the last lies behind it
        split(reverse ? L_lo + span : L_lo, cur.it.img, cur.it.ty, cur.it.tx, cur.it.nb);
        cur.it.tile = cur.it.ty * tiles_x + cur.it.tx;
        cur.kc = 0;
        s = 0;
        // selects, not a branch: with the digits defined on two paths hipcc spills them on both
        const int t_tx = d_tx + (d_nb ? 1 : 0), t_ty = d_ty + (t_tx ? 1 : 0);
        d_img = reverse ? -d_img - (t_ty ? 1 : 0) : d_img;
        d_ty = reverse && t_ty ? tiles_y - t_ty : reverse ? 0 : d_ty;
        d_tx = reverse && t_tx ? tiles_x - t_tx : reverse ? 0 : d_tx;
        d_nb = reverse && d_nb ? nblocks - d_nb : d_nb;
        const int other_img = (reverse ? L_lo : L_lo + span) / nblocks / tiles_per_img;      // the image at the walk's far end
        first_img = reverse ? other_img : cur.it.img;
        last_img = reverse ? cur.it.img : other_img;
    }
    // the stage after `cur` (clamped: past the last stage the cursor stays on it, as the pipelines' harmless over-fetch expects)
    IRE_HD PersistStage next() {
        if (s + 1 < S) {
            ++s;
            if (++cur.kc == nkc) {
                cur.kc = 0;
                PersistItem& it = cur.it;
                it.nb += d_nb;
                int c = 0;
                if (it.nb >= nblocks) { it.nb -= nblocks; c = 1; }
                it.tx += d_tx + c; c = 0;
                if (it.tx >= tiles_x) { it.tx -= tiles_x; c = 1; }
                it.ty += d_ty + c; c = 0;
                if (it.ty >= tiles_y) { it.ty -= tiles_y; c = 1; }
                it.img += d_img + c;
                it.tile = it.ty * tiles_x + it.tx;
            }
        }
        return cur;
    }
};

}  // namespace ire
