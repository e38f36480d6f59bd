"""The images the JPEG encoder is tested on, shared by the CPU tests of the model (test_jpeg_model.py) and the GPU tests of the
device against it (test_jpeg_gpu.py).  Everything is seeded; nothing is read from disk.  Shapes are h x w and small: each case
names a way to go wrong."""
import numpy as np

import jpeg_model as model
from png_deflate_cases import noise, smooth      # noqa: F401

R = model.R

# noise(8, 8, seed): file lengths 0, 1 and 2 mod 3 (found by searching seeds with the model; the test checks that they still are)
MOD3_SEEDS = {0: 1, 1: 2, 2: 0}


def checkerboard(h, w, period, lo=0, hi=255):
    y, x = np.mgrid[:h, :w]
    v = np.where(((y // period) + (x // period)) % 2 == 0, hi, lo).astype(np.uint8)
    return np.repeat(v[:, :, None], 3, axis=2)


def impulses(h, w, seed):
    """single full-scale pixels, one per 8 x 8 block at a seeded place, white on black in even blocks and black on white in odd"""
    r = np.random.default_rng(seed)
    px = np.zeros((h, w, 3), np.uint8)
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            inv = ((by + bx) // 8) % 2
            px[by:by + 8, bx:bx + 8] = 255 * inv
            px[min(h - 1, by + int(r.integers(8))), min(w - 1, bx + int(r.integers(8)))] = 255 * (1 - inv)
    return px


def saturated_colours(h, w):
    """8 x 8 blocks of saturated colours, horizontal neighbours complementary: full-scale DC swings of Cb and Cr from block to block"""
    cols = np.array([[255, 0, 0], [0, 255, 255], [0, 0, 255], [255, 255, 0], [0, 255, 0], [255, 0, 255]], np.uint8)
    y, x = np.mgrid[:h, :w]
    return cols[(2 * ((y // 8) % 3) + (x // 8) % 2) % 6]


def ramp_with_one_high_term(h, w):
    """a gentle horizontal ramp plus the highest vertical frequency at a small amplitude: in zig-zag order a few low coefficients,
    then a run of at least 16 zeros before the (7, 0) term -- the ZRL symbol 0xF0"""
    y, x = np.mgrid[:h, :w]
    v = 100 + 1.5 * (x % 8) + 40 * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    return np.repeat(np.clip(np.rint(v), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def all_cases():
    """name -> pixels"""
    d = {
        "1x1": noise(1, 1, 11), "7x5": noise(7, 5, 12), "8x8": smooth(8, 8, 13), "9x17": smooth(9, 17, 14),      # partial MCUs each way
        "wrap40x88": smooth(40, 88, 15),          # 11 MCUs per row, 5 rows: intervals of 16 wrap across rows; 55 MCUs: a last interval of 7
        "wrap24x136": noise(24, 136, 16),         # 17 MCUs per row: every interval but the first straddles a row
        "rst_wraps": smooth(96, 128, 17),         # 192 MCUs: 12 intervals, RST0..RST7, RST0..RST2
        "black": np.zeros((19, 33, 3), np.uint8), "white": np.full((19, 33, 3), 255, np.uint8),      # DC and EOB only
        "checker1": checkerboard(16, 24, 1), "checker1_inv": checkerboard(16, 24, 1, 255, 0),          # the highest frequency at full scale
        "checker8": checkerboard(24, 40, 8),      # full-scale DC differences, both signs
        "checker4": checkerboard(16, 16, 4),
        "impulses": impulses(24, 40, 18),
        "saturated": saturated_colours(24, 40),
        "ramp_high": ramp_with_one_high_term(16, 24),
        "noise160": noise(160, 160, 21),
    }
    for r, seed in MOD3_SEEDS.items():
        d["mod3_%d" % r] = noise(8, 8, seed)
    return d
