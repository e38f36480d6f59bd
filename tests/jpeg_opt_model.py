"""The device's JPEG result for any (quality, sampling), as a Python model: tests/jpeg_model.py generalised.  What carries over
unchanged is imported from there (colour transform, islow DCT, quantiser, symbol coder, stuffing, the Annex K tables); this file
restates only what the two settings change.

    quality  1..100: the Annex K tables scaled the IJG way ((q * scale + 50) / 100, scale = 5000 / quality below 50 and
             200 - 2 * quality from 50 on), every entry clamped to 1..255 (baseline)
    sampling 0 = 4:4:4 (an MCU is 8 x 8 pixels: Y Cb Cr), 2 = 4:2:0 (an MCU is 16 x 16 pixels: Y00 Y01 Y10 Y11 Cb Cr), numbered as
             ire_decode_jpeg_plan numbers them
    restart  every R_OF[sampling] MCUs: 16 at 4:4:4, 8 at 4:2:0 -- 48 blocks either way

4:2:0 as libjpeg writes it (jcprepct.c, jcsample.c h2v2_downsample, jccoefct.c):
  * Y is completed by edge replication to ceil(w / 8) x ceil(h / 8) blocks ONLY.  A Y block of a partial MCU beyond that is a dummy
    block: every AC coefficient 0, the quantised DC that of the block before it in the MCU's order (so it codes as a DC difference of
    0 and an EOB).
  * Cb and Cr at full resolution are completed to the right by replicating the last real column out to the MCU grid, and an odd
    number of rows is made even by repeating the last row; then every 2 x 2 cell is averaged as (a + b + c + d + bias) >> 2 with
    bias 1 in even output columns and 2 in odd ones; then the last DOWNSAMPLED row is replicated down to the MCU grid (which is not
    what averaging replicated pixels would give when h is even)."""
import base64
import functools
import struct

import numpy as np

import jpeg_model as base

R_OF = {0: 16, 2: 8}                     # MCUs per restart interval, per sampling
QUALITIES = [1, 25, 49, 50, 51, 75, 85, 95, 100]
SAMPLINGS = [0, 2]
ZIGZAG = base.ZIGZAG
HEADER_BYTES = base.HEADER_BYTES


def check(quality, sampling):
    assert 1 <= quality <= 100 and sampling in R_OF, (quality, sampling)


def quant_tables(quality):
    """(luminance, chrominance), natural order"""
    return base.quant_table(base.K1_LUMINANCE, quality), base.quant_table(base.K2_CHROMINANCE, quality)


def header(h, w, quality, sampling):
    check(quality, sampling)
    out = b"\xff\xd8" + base._seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(quant_tables(quality)):
        out += base._seg(0xDB, bytes([i]) + bytes(q[ZIGZAG[k]] for k in range(64)))
    out += base._seg(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22 if sampling == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, base.DC_LUM_BITS, base.DC_VALS), (0x10, base.AC_LUM_BITS, base.AC_LUM_VALS), (0x01, base.DC_CHR_BITS, base.DC_VALS),
                              (0x11, base.AC_CHR_BITS, base.AC_CHR_VALS)):
        out += base._seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += base._seg(0xDD, struct.pack(">H", R_OF[sampling]))
    out += base._seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ---- pixels -> MCUs of quantised blocks ---------------------------------------------------------------------------------------------
def _blocks(plane, q):
    """[8 a][8 b] samples in 0..255 -> [a][b][64] quantised coefficients in zig-zag order"""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    blk = (plane - 128).reshape(a, 8, b, 8).transpose(0, 2, 1, 3)
    return base.quantise(base.fdct_islow(blk).reshape(a, b, 64), q)[..., ZIGZAG]


def _clamped(plane, rows, cols):
    h, w = plane.shape
    return plane[np.minimum(np.arange(rows), h - 1)][:, np.minimum(np.arange(cols), w - 1)]


def downsample_h2v2(plane, rows, cols):
    """one full-resolution chroma plane [h][w] -> [rows][cols] (the MCU grid's share), as the module's head says"""
    h, w = plane.shape
    x = _clamped(plane, (h + 1) // 2 * 2, 2 * cols)
    bias = np.where(np.arange(cols) % 2 == 0, 1, 2)
    d = (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + bias) >> 2
    return d[np.minimum(np.arange(rows), d.shape[0] - 1)]


def mcus(px, quality, sampling):
    """[h][w][3] uint8 -> [MCU][block] of (table, [64] zig-zag quantised coefficients) in raster order of MCUs, scan order of blocks"""
    check(quality, sampling)
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    ql, qc = quant_tables(quality)
    y, cb, cr = base.rgb_to_ycc(px)
    if sampling == 0:
        H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
        by, bb, br = (_blocks(_clamped(p, H, W), q) for p, q in ((y, ql), (cb, qc), (cr, qc)))
        return [[(0, by[i, j]), (1, bb[i, j]), (1, br[i, j])] for i in range(H // 8) for j in range(W // 8)]
    mh, mw = (h + 15) // 16, (w + 15) // 16
    yh, yw = (h + 7) // 8, (w + 7) // 8              # the Y blocks that exist
    by = _blocks(_clamped(y, 8 * yh, 8 * yw), ql)
    bb, br = (_blocks(downsample_h2v2(p, 8 * mh, 8 * mw), qc) for p in (cb, cr))
    out = []
    for i in range(mh):
        for j in range(mw):
            m = []
            for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if 2 * i + a < yh and 2 * j + b < yw:
                    m.append((0, by[2 * i + a, 2 * j + b]))
                else:                                # a dummy block
                    zz = np.zeros(64, np.int64)
                    zz[0] = m[-1][1][0]
                    m.append((0, zz))
            out.append(m + [(1, bb[i, j]), (1, br[i, j])])
    return out


# ---- entropy coding ----------------------------------------------------------------------------------------------------------------
def interval_bytes(ms, sampling):
    """the MCUs of one interval -> its entropy-coded bytes, stuffed, without the marker.  Three DC predictor chains; at 4:2:0 Y's runs
    through the four blocks of every MCU."""
    ny = 4 if sampling == 2 else 1
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    for m in ms:
        for k, (table, zz) in enumerate(m):
            c = 0 if k < ny else k - ny + 1
            for v, l in base.block_symbols(zz, pred[c], table):
                acc = (acc << l) | v
                nbits += l
            pred[c] = int(zz[0])
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def jpeg_file(px, quality=85, sampling=0):
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    assert 1 <= h <= 8192 and 1 <= w <= 8192
    ms = mcus(px, quality, sampling)
    r = R_OF[sampling]
    parts = [header(h, w, quality, sampling)]
    n = (len(ms) + r - 1) // r
    for m in range(n):
        parts.append(interval_bytes(ms[m * r:(m + 1) * r], sampling))
        parts.append(b"\xff\xd9" if m == n - 1 else bytes([0xFF, 0xD0 + (m & 7)]))
    return b"".join(parts)


def jpeg_base64(px, quality=85, sampling=0):
    return base64.b64encode(jpeg_file(px, quality, sampling))


# ---- the worst case ------------------------------------------------------------------------------------------------------------------
# The DC of islow is exact: the first pass leaves 4 * (the row's sum), the second descales the sum of eight of those by 2 bits.  So
# the DC (scaled by 8) is the sum of 64 samples in -128..127: -8192..8128, and the quantised DC lies in
# -(8192 + 4 q) // (8 q) .. (8128 + 4 q) // (8 q).  A DC difference is at most the sum of the two: 2040 at q = 1, category 11, the
# largest the DC tables have.  The three AC terms with both frequencies in {0, 4} are exact in the same way (islow forms them with
# shifts alone): a sum of 32 samples minus a sum of 32 others, at most 32 * 128 + 32 * 127 = 8160, where COEF_MAX allows 8208 and at
# q = 1 that would be a category 11 no AC table has.  Every other AC amplitude is at most (7584 + 4 q) // (8 q) <= 948.  So an AC
# coefficient is at most category 10, the largest the AC tables have (libjpeg's own MAX_COEF_BITS).
DC_MIN, DC_MAX, EXACT_AC_MAX = 8192, 8128, 8160
EXACT_AC = (4, 32, 36)                   # natural indices (0, 4), (4, 0), (4, 4)


def coef_bound(natural):
    return EXACT_AC_MAX if natural in EXACT_AC else base.COEF_MAX[natural]


def size_max(table, quality):
    q = quant_tables(quality)[table]
    out = [((DC_MIN + 4 * q[0]) // (8 * q[0]) + (DC_MAX + 4 * q[0]) // (8 * q[0])).bit_length()]
    for k in range(1, 64):
        n = ZIGZAG[k]
        out.append(((coef_bound(n) + 4 * q[n]) // (8 * q[n])).bit_length())
    return out


@functools.lru_cache(maxsize=None)
def block_bits_max(table, quality):
    """jpeg_model.block_bits_max with the categories of this quality; a category without a code is an error, not zero bits"""
    smax = size_max(table, quality)
    dc, ac = base.DC_CODES[table], base.AC_CODES[table]
    assert smax[0] <= 11 and max(smax[1:]) <= 10
    best = [max(dc[s][1] + s for s in range(smax[0] + 1))] + [0] * 63
    zrl = ac[0xF0][1]
    for p in range(1, 64):
        cand = []
        for prev in range(p):
            run = p - prev - 1
            sym = max(ac[((run & 15) << 4) | s][1] + s for s in range(1, smax[p] + 1))
            cand.append(best[prev] + (run >> 4) * zrl + sym)
        best[p] = max(cand)
    return max(best[63], max(best[p] for p in range(63)) + ac[0x00][1])


def mcu_bits_max(quality, sampling):
    check(quality, sampling)
    ny = 4 if sampling == 2 else 1
    return ny * block_bits_max(0, quality) + 2 * block_bits_max(1, quality)


def interval_bound(nmcu, quality, sampling):
    return 2 * ((nmcu * mcu_bits_max(quality, sampling) + 7) // 8) + 2


def file_bound(h, w, quality, sampling):
    p = 16 if sampling == 2 else 8
    nmcu = ((h + p - 1) // p) * ((w + p - 1) // p)
    full, tail = divmod(nmcu, R_OF[sampling])
    return HEADER_BYTES + full * interval_bound(R_OF[sampling], quality, sampling) + (interval_bound(tail, quality, sampling) if tail else 0)


def base64_bound(h, w, quality, sampling):
    if not (1 <= h <= 8192 and 1 <= w <= 8192 and 1 <= quality <= 100 and sampling in R_OF):
        return 0
    return (file_bound(h, w, quality, sampling) + 2) // 3 * 4
