"""The images that carry the JPEG encoder's settings to their edges, shared by the CPU test of the cases (test_jpeg_opt_cases.py) and
the GPU test of the device against the model (test_jpeg_opt_cases_gpu.py).  Everything is seeded and small.  Every case exists for a
condition -- a symbol, a chain of symbols, a dummy block behind a full DC swing, an interval's last byte -- and `census` counts those
conditions from the model (tests/jpeg_opt_model.py) alone, so that `assert_conditions` can hold them before an engine sees a case: a
case that stops meeting its condition fails on the CPU instead of silently testing less.

    shapes (h x w)   (33, 130)  h % 16 == 1, w % 16 == 2: dummy Y rows and columns at 4:2:0 plus replication; 5 x 17 = 85 MCUs at 4:4:4,
                                3 x 9 = 27 at 4:2:0, so intervals straddle MCU rows at both samplings
                     (41, 139)  replication only; 6 x 18 = 108 MCUs at 4:4:4 (6 full intervals and 12), 3 x 9 = 27 at 4:2:0
                     (8, 136)   17 MCUs at 4:4:4, 9 at 4:2:0: a last interval of ONE MCU at either sampling, and at 4:2:0 every lower Y
                                block is a dummy
    settings         quality 100 (the categories only it reaches), 86 | 87 at 4:4:4 and 85 | 86 at 4:2:0 (the two sides of the size-class
                     switch of csrc/jpeg.hip's interval kernel), 50 and 25 (the chains of ZRL codes), 1 (every divisor 255)

The model's texts and the census are computed once per process (lru_cache) and shared by both test files."""
import base64
import functools

import numpy as np

import jpeg_cases as cases
import jpeg_opt_model as model

SETTINGS = [(100, 0), (100, 2), (86, 0), (87, 0), (85, 2), (86, 2), (50, 2), (25, 2), (1, 0), (1, 2)]
SHAPES = [(33, 130), (41, 139), (8, 136)]
RAW_SMALL, RAW_BIG = 5034, 9448          # an interval's bytes before stuffing, at most, in the two size classes of csrc/jpeg.hip


def big_class(quality, sampling):
    """csrc/jpeg_tables.hpp::big_class restated: the interval kernel's size class is "small" while the interval's raw bound fits 5034 bytes"""
    return not (model.R_OF[sampling] * model.mcu_bits_max(quality, sampling) + 7) // 8 <= RAW_SMALL


# ---- content ------------------------------------------------------------------------------------------------------------------------
def cells2(h, w, seed):
    """random 0 / 255 per channel on 2 x 2 cells: full-scale swings of every DC and large amplitudes in every band, which survive the
    4:2:0 downsample; at quality 100 DC category 11 and AC category 10 in both tables, and hundreds of stuffed 0xFF bytes"""
    v = np.random.default_rng(seed).integers(0, 2, ((h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)[:h, :w])


def noise01(h, w, seed):
    """independent 0 / 255 per channel and pixel: the fullest intervals an image gives (about half the bound)"""
    return np.random.default_rng(seed).integers(0, 2, (h, w, 3), dtype=np.uint8) * 255


def saturated(h, w, period):
    """jpeg_cases.saturated_colours on cells of `period` pixels; 16 keeps the chroma DC swing at full scale behind the 4:2:0 downsample"""
    k = period // 8
    small = cases.saturated_colours(-(-h // k), -(-w // k))
    return np.ascontiguousarray(np.repeat(np.repeat(small, k, axis=0), k, axis=1)[:h, :w])


def _zrl_plane(h, w, scale):
    """per 8 x 8 block (pixel-doubled for scale 2) 60 cos((2y+1) 7 pi / 16) cos((2x+1) 7 pi / 16): the (7, 7) term alone, zig-zag position 63"""
    y, x = np.mgrid[:h, :w]
    y, x = (y // scale) % 8, (x // scale) % 8
    return 60.0 * np.cos((2 * y + 1) * 7 * np.pi / 16) * np.cos((2 * x + 1) * 7 * np.pi / 16)


def zrl_luma(h, w):
    """the pattern in Y: only position 63 survives the quantiser, a run of 62 = three ZRL codes and a run of 14, luminance table"""
    return np.repeat(np.clip(np.rint(128 + _zrl_plane(h, w, 1)), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def zrl_chroma(h, w, scale=1):
    """the pattern in Cb and minus the pattern in Cr over Y = 128, by the inverse colour transform rounded to u8.  scale 2: pixel-doubled
    to 16 x 16, which the h2v2 downsample turns back into the 8 x 8 pattern: the chain in chroma at 4:2:0."""
    p = _zrl_plane(h, w, scale)
    cb, cr = p, -p
    rgb = np.stack([128 + 1.402 * cr, 128 - 0.344136 * cb - 0.714136 * cr, 128 + 1.772 * cb], axis=2)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


# name -> (generator of (h, w, seed), what the case is for)
CONTENT = {
    "cells2": (cells2, "DC category 11, AC category 10 in both tables at quality 100; a dummy block behind a full DC swing; stuffed bytes"),
    "noise01": (noise01, "the fullest intervals"),
    "checker8": (lambda h, w, seed: cases.checkerboard(h, w, 8), "full-scale luminance DC differences of both signs, DC + EOB blocks"),
    "sat8": (lambda h, w, seed: saturated(h, w, 8), "full-scale chroma DC differences at 4:4:4"),
    "sat16": (lambda h, w, seed: saturated(h, w, 16), "full-scale chroma DC differences behind the 4:2:0 downsample"),
    "black": (lambda h, w, seed: np.zeros((h, w, 3), np.uint8), "the shortest text: one DC difference per chain, then zeros and EOBs"),
    "white": (lambda h, w, seed: np.full((h, w, 3), 255, np.uint8), "the same at the other end of the DC range"),
    "impulses": (cases.impulses, "every AC position at a small amplitude beside a full DC swing"),
    "ramp_high": (lambda h, w, seed: cases.ramp_with_one_high_term(h, w), "one ZRL code at quality 85, two at 50, luminance"),
    "zrl_y": (lambda h, w, seed: zrl_luma(h, w), "three ZRL codes in one symbol, luminance table"),
    "zrl_c": (lambda h, w, seed: zrl_chroma(h, w), "three ZRL codes in one symbol, chrominance table at 4:4:4"),
    "zrl_c16": (lambda h, w, seed: zrl_chroma(h, w, 2), "three ZRL codes in one symbol, chrominance table at 4:2:0"),
}
# One batch per shape: the images of one device call, in this order (black beside cells2: neighbours whose lengths differ by two orders
# of magnitude).  Every content occurs; at most 8 images, the session engine's max_batch.
BATCHES = {
    (33, 130): ["black", "cells2", "noise01", "checker8", "sat16", "zrl_c16", "impulses", "white"],
    (41, 139): ["cells2", "black", "noise01", "sat8", "zrl_y", "zrl_c", "ramp_high", "checker8"],
    (8, 136): ["noise01", "white", "cells2", "zrl_y", "sat16", "impulses", "zrl_c16", "ramp_high"],
}


def seed_of(name, shape):
    """The seeded contents' seed.  With these the matrix holds, at either sampling, intervals whose bit total is a multiple of 8 (no
    padding: 73 and 116 of them) and intervals whose padded last byte is 0xFF (4 and 8); no seed had to be searched for, and
    assert_conditions checks that both still occur."""
    return 1000 * SHAPES.index(shape) + sorted(CONTENT).index(name)


@functools.lru_cache(maxsize=None)
def pixels(name, shape):
    px = np.ascontiguousarray(CONTENT[name][0](shape[0], shape[1], seed_of(name, shape)), np.uint8)
    assert px.shape == (shape[0], shape[1], 3), (name, shape, px.shape)
    px.setflags(write=False)
    return px


def batch(shape):
    """[n][h][w][3] of the shape's cases, in BATCHES' order"""
    return np.stack([pixels(name, shape) for name in BATCHES[shape]])


def all_cases():
    return [(name, shape) for shape in SHAPES for name in BATCHES[shape]]


# ---- the census -----------------------------------------------------------------------------------------------------------------------
def _cat(v):
    return int(abs(int(v))).bit_length()


def census(px, quality, sampling):
    """What the file of `px` at (quality, sampling) holds, from model.mcus and model.interval_bytes:
         dc_cat[t], ac_cat[t]   the largest category of a DC DIFFERENCE and of an AC coefficient, per Huffman table t (0 luminance, 1 chrominance)
         zrl[t][k], k = 1..3    the number of AC symbols with k ZRL codes in front (a run of 16 k .. 16 k + 15 zeros)
         dc_eob                 real (not dummy) blocks that are a DC difference and an EOB
         dummies                dummy Y blocks (4:2:0)
         dummy_own_dc           of those, the ones whose copied DC differs from 0 and from the DC of the MCU's first block: a copy from the
                                wrong block, or no copy, changes the bytes
         dummy_after_swing      dummy blocks of an MCU in which a real Y block before them has a DC difference of category 10 or more
         intervals              per interval (MCUs, bit total, raw bytes, stuffed 0xFF bytes, whether the padded last byte is 0xFF)"""
    h, w, _ = px.shape
    ms = model.mcus(px, quality, sampling)
    r, ny = model.R_OF[sampling], 4 if sampling == 2 else 1
    mw = (w + 15) // 16
    out = {"dc_cat": [0, 0], "ac_cat": [0, 0], "zrl": [[0] * 4, [0] * 4], "dc_eob": 0, "dummies": 0, "dummy_own_dc": 0, "dummy_after_swing": 0, "intervals": []}
    for i0 in range(0, len(ms), r):
        part = ms[i0:i0 + r]
        pred = [0, 0, 0]
        bits = 0
        for mi, m in enumerate(part):
            my, mx = divmod(i0 + mi, mw)
            swing = False
            for k, (t, zz) in enumerate(m):
                c = 0 if k < ny else k - ny + 1
                dummy = sampling == 2 and k < 4 and ((2 * mx + (k & 1)) * 8 >= w or (2 * my + (k >> 1)) * 8 >= h)
                dcat = _cat(int(zz[0]) - pred[c])
                out["dc_cat"][t] = max(out["dc_cat"][t], dcat)
                nz = np.flatnonzero(zz[1:]) + 1
                if dummy:
                    assert not len(nz) and dcat == 0
                    out["dummies"] += 1
                    out["dummy_own_dc"] += int(zz[0]) not in (0, int(m[0][1][0]))
                    out["dummy_after_swing"] += swing
                else:
                    out["dc_eob"] += not len(nz)
                    swing = swing or (k < ny and dcat >= 10)
                if len(nz):
                    out["ac_cat"][t] = max(out["ac_cat"][t], _cat(np.abs(zz[nz]).max()))
                    for n in (np.diff(np.concatenate([[0], nz])) - 1) >> 4:
                        out["zrl"][t][n] += 1
                bits += sum(l for _, l in model.base.block_symbols(zz, pred[c], t))
                pred[c] = int(zz[0])
        data = model.interval_bytes(part, sampling)
        raw = (bits + 7) // 8
        out["intervals"].append((len(part), bits, raw, len(data) - raw, data.endswith(b"\xff\x00")))
    return out


@functools.lru_cache(maxsize=None)
def encoded(name, shape, quality, sampling):
    """(the model's file, its census), once per process"""
    px = pixels(name, shape)
    return model.jpeg_file(px, quality, sampling), census(px, quality, sampling)


def text(name, shape, quality, sampling):
    return base64.b64encode(encoded(name, shape, quality, sampling)[0])


@functools.lru_cache(maxsize=None)
def summary():
    """the census of the whole matrix, folded: per sampling the conditions of the module's head; per setting the fullest interval"""
    out = {}
    for s in (0, 2):
        o = {"dc_cat_q100": [0, 0], "ac_cat_q100": [0, 0], "zrl": [[0] * 4, [0] * 4], "dc_eob": 0, "dummies": 0, "dummy_own_dc": 0, "dummy_after_swing": 0,
             "one_mcu_last": 0, "no_padding": 0, "ends_stuffed": 0, "stuffed": 0}
        for q, s2 in SETTINGS:
            if s2 != s:
                continue
            fullest = 0
            for name, shape in all_cases():
                c = encoded(name, shape, q, s)[1]
                for t in (0, 1):
                    if q == 100:
                        o["dc_cat_q100"][t] = max(o["dc_cat_q100"][t], c["dc_cat"][t])
                        o["ac_cat_q100"][t] = max(o["ac_cat_q100"][t], c["ac_cat"][t])
                    for k in range(1, 4):
                        o["zrl"][t][k] += c["zrl"][t][k]
                for key in ("dc_eob", "dummies", "dummy_own_dc", "dummy_after_swing"):
                    o[key] += c[key]
                o["one_mcu_last"] += c["intervals"][-1][0] == 1
                for nm, bits, raw, ff, ends in c["intervals"]:
                    o["no_padding"] += bits % 8 == 0 and bits > 0
                    o["ends_stuffed"] += ends
                    o["stuffed"] += ff
                    fullest = max(fullest, raw)
            out[(q, s)] = fullest
        out[s] = o
    return out


def assert_conditions():
    """The conditions the cases exist for, from the model alone.  Both test files call this before they use a case."""
    sm = summary()
    for s in (0, 2):
        o = sm[s]
        assert o["dc_cat_q100"] == [11, 11] and o["ac_cat_q100"] == [10, 10], (s, o)      # the last entries of the DC and AC tables
        for t in (0, 1):
            assert all(o["zrl"][t][k] > 0 for k in (1, 2, 3)), (s, t, o["zrl"])              # one, two and three ZRL codes in either table
        assert o["dc_eob"] > 0 and o["one_mcu_last"] > 0 and o["no_padding"] > 0 and o["ends_stuffed"] > 0, (s, o)
    assert sm[0]["dummies"] == 0                                                              # 4:4:4 has no dummy blocks
    assert sm[2]["dummy_after_swing"] > 0 and sm[2]["dummy_own_dc"] > 0, sm[2]
    # the fullest interval: what an image can give of a class's bytes (no image comes near the bound itself)
    assert sm[(100, 0)] >= 0.45 * RAW_BIG and sm[(100, 2)] >= 0.45 * RAW_BIG, (sm[(100, 0)], sm[(100, 2)])
    assert sm[(86, 0)] >= 0.35 * RAW_SMALL and sm[(85, 2)] >= 0.35 * RAW_SMALL, (sm[(86, 0)], sm[(85, 2)])
    assert [big_class(q, s) for q, s in ((86, 0), (87, 0), (85, 2), (86, 2))] == [False, True, False, True]
    return sm
