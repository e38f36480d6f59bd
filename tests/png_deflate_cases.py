"""The images the compressing PNG encoder is tested on, shared by the CPU tests of the model (test_png_deflate_model.py) and the
GPU tests of the device against it (test_png_deflate_gpu.py).  Everything is seeded; nothing is read from disk."""
import numpy as np

import png_deflate_model as model


def smooth(h, w, seed):
    """a random walk in both directions: neighbouring pixels correlate, as in an image (small Paeth residuals)"""
    r = np.random.default_rng(seed)
    x = r.normal(size=(h, w, 3)).cumsum(0).cumsum(1)
    x = (x - x.min()) / (x.max() - x.min() + 1e-9) * 255
    return x.astype(np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def from_histogram(h, w, counts, seed):
    """An image whose filtered stream has exactly `counts` ({byte value: count}, summing to h * (1 + 3 w); the h filter-type bytes
    are part of the count of value 4): the residuals in seeded random order, un-filtered (the filter is a bijection)."""
    assert sum(counts.values()) == h * (1 + 3 * w) and counts.get(4, 0) >= h
    rest = dict(counts)
    rest[4] -= h
    res = np.concatenate([np.full(c, v, np.uint8) for v, c in sorted(rest.items())])
    np.random.default_rng(seed).shuffle(res)
    rows = np.empty((h, 1 + 3 * w), np.uint8)
    rows[:, 0] = 4
    rows[:, 1:] = res.reshape(h, 3 * w)
    px = model.paeth_unfilter(rows.tobytes(), h, w)
    assert model.paeth_filter(px) == rows.tobytes()
    return px


# Fibonacci counts over 21 byte values, 28 656 bytes = 144 rows of 1 + 3 * 66: value 4 (the filter-type bytes) has the count 144
FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946]
FIB_VALUES = [200, 201, 202, 203, 204, 205, 206, 207, 208, 209, 210, 4, 212, 213, 214, 215, 216, 217, 218, 219, 0]
# c(k) = c(k-1) + c(k-2) + 1 from (end-of-block's 1, 2): no two partial sums tie, every merge of a Huffman construction takes the
# running sum and the next count, and the unlimited tree is 18 deep: the 15-bit limit BINDS.  28 634 bytes = 278 rows of 1 + 3 * 34;
# value 4 has the count 376 (278 filter-type bytes and 98 residuals).
SKEW = [2, 4, 7, 12, 20, 33, 54, 88, 143, 232, 376, 609, 986, 1596, 2583, 4180, 6764, 10945]
SKEW_VALUES = [100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 4, 111, 112, 113, 114, 115, 116, 0]


def fibonacci_image():
    return from_histogram(144, 66, dict(zip(FIB_VALUES, FIB)), 5)


def skewed_image():
    return from_histogram(278, 34, dict(zip(SKEW_VALUES, SKEW)), 6)


# noise(6, 5, seed): file lengths 0, 1 and 2 mod 3 (found by searching seeds with the model; the test checks that they still are)
MOD3_SEEDS = {0: 4, 1: 2, 2: 0}


def shape_cases():
    """name -> pixels: the shapes of the issue's first test (h x w)."""
    flat = np.empty((120, 100, 3), np.uint8)
    flat[:] = (77, 130, 9)
    return {
        "1x1": noise(1, 1, 11), "1x7": noise(1, 7, 12), "5x1": noise(5, 1, 13),
        "120x100": smooth(120, 100, 14),          # 36 120 filtered bytes: two blocks, a scanline across the boundary
        "8192x1": smooth(8192, 1, 15),            # exactly one full block, no tail
        "4096x5": smooth(4096, 5, 16),            # exactly two
        "flat": flat,                             # two-symbol histograms
        "random264x200": noise(264, 200, 17),
    }
