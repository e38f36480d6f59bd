"""The pixel cases and histograms that tests/test_jpeg_huffopt_model.py (CPU) and tests/test_jpeg_huffopt_gpu.py (GPU) share.  Fixed
seeds; every image is a pure function of its name."""
import functools

import numpy as np

QUALITIES = [1, 25, 49, 50, 51, 75, 85, 95, 100]
SAMPLINGS = [0, 2]


def flat(h=16, w=24):
    return np.full((h, w, 3), 180, np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp_noise(h, w, power, seed, gain=128.0):
    """a smooth sinusoid plus noise whose amplitude grows as (x / w) ** power: the left of the image gives the short, frequent
    symbols, the right the long, rare ones, so the symbol counts span many orders of magnitude"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = 128 + 60 * np.sin(x / 23.0) * np.cos(y / 17.0)
    amp = gain * (x / max(w - 1, 1)) ** power
    v = smooth[..., None] + amp[..., None] * rng.standard_normal((h, w, 3))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(name):
    return {
        "1x1": lambda: noise(1, 1, 11),
        "5x7": lambda: noise(5, 7, 12),
        "flat": lambda: flat(),
        "noise": lambda: noise(45, 37, 13),
        "ramp": lambda: ramp_noise(160, 200, 3, 14),       # 32 intervals at 4:4:4: RSTm wraps
        "deep": lambda: ramp_noise(256, 384, 4, 15),       # at q100 4:4:4 the unlimited code lengths pass 16: the limiting loop runs
    }[name]()


SMALL = ["1x1", "5x7", "flat", "noise"]
LARGE = ["ramp", "deep"]
DEEP = ("deep", 100, 0)
# (name, quality, sampling): every quality at both samplings on the small cases, q85 / q100 at both on the two larger ones
CASES = [(n, q, s) for n in SMALL for q in QUALITIES for s in SAMPLINGS] + [(n, q, s) for n in LARGE for q in (85, 100) for s in SAMPLINGS]
# what the GPU tests run through all three entries: every image, every path of the kernels (both samplings, a quality of each end)
GPU_CASES = [(n, q, s) for n in SMALL for q, s in ((1, 0), (50, 2), (85, 0), (85, 2), (100, 2))] + [(n, q, s) for n in LARGE for q in (85, 100) for s in SAMPLINGS]


def synthetic_histograms():
    """{name: [256] counts}: the table builder's own edge cases"""
    fib = [1, 2]                                           # distinct counts: every merge takes the running sum and the next term
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    ac_symbols = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    out = {}
    out["one"] = {0x05: 7}
    out["tie2"] = {0x03: 9, 0x21: 9}
    out["ac162"] = {s: 5 for s in ac_symbols}
    out["fib30"] = {i: fib[i] for i in range(30)}          # a depth far above 16
    out["all256"] = {i: 1 + (i * 37) % 11 for i in range(256)}
    res = {}
    for k, d in out.items():
        h = np.zeros(256, np.int64)
        for s, c in d.items():
            h[s] = c
        res[k] = h
    return res
