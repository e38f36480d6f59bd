"""The specification of the device's JPEG encoder (csrc/jpeg.hip) as a Python model: stdlib + numpy, no product code.

    file   = SOI | JFIF APP0 (1.01, density 1:1, no thumbnail) | DQT luminance | DQT chrominance | SOF0 | DHT DC lum | DHT AC lum |
             DHT DC chr | DHT AC chr | DRI | SOS | entropy-coded data | EOI
    frame  = baseline sequential DCT, 8 bit, Y Cb Cr, every component sampled 1 x 1 (4:4:4), one interleaved scan: an MCU is one
             8 x 8 block of Y, of Cb and of Cr; h, w in 1..8192; a partial MCU is completed by edge replication
    tables = the standard's Annex K quantisation tables at IJG quality 85 ((q * 30 + 50) / 100, clamped to 1..255) and its Annex K
             Huffman tables, fixed
    steps  = libjpeg's published integer algorithms: RGB -> YCbCr in 16-bit fixed point, level shift by 128, the "islow" forward
             DCT (13-bit constants, 2 pass bits, output scaled by 8), a quantiser that divides the magnitude by 8 q rounding half
             up, zig-zag, differential DC, (run, size) AC symbols with ZRL and EOB
    restart= every R = 16 MCUs in raster order (an interval may wrap from one MCU row into the next): the DC predictors start at 0,
             the last byte is padded with 1-bits, a 0x00 follows every 0xFF byte, RST(m mod 8) follows every interval but the last

The restart interval is what makes the entropy coder parallel: an interval's bits depend on its own 16 MCUs alone.  The model is
held to the published format by an independent decoder and to libjpeg-turbo's own file (tests/test_jpeg_model.py); the device is
held to the model byte for byte (tests/test_jpeg_gpu.py)."""
import base64
import math
import struct

import numpy as np

R = 16                                   # MCUs per restart interval
QUALITY = 85

# ---- Annex K ---------------------------------------------------------------------------------------------------------------------
K1_LUMINANCE = [
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2_CHROMINANCE = [
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99]
ZIGZAG = [                               # ZIGZAG[k]: the natural (row-major) index of the k-th coefficient in zig-zag order
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def quant_table(base, quality=QUALITY):
    """IJG quality scaling, baseline (8-bit entries); natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(255, max(1, (q * scale + 50) // 100)) for q in base]


Q_LUM = quant_table(K1_LUMINANCE)
Q_CHR = quant_table(K2_CHROMINANCE)
QTABLES = (Q_LUM, Q_CHR, Q_CHR)          # per component


def huffman_codes(bits, vals):
    """Annex C: BITS / HUFFVAL -> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


DC_CODES = (huffman_codes(DC_LUM_BITS, DC_VALS), huffman_codes(DC_CHR_BITS, DC_VALS))
AC_CODES = (huffman_codes(AC_LUM_BITS, AC_LUM_VALS), huffman_codes(AC_CHR_BITS, AC_CHR_VALS))
TABLE_OF = (0, 1, 1)                     # component -> table


# ---- the file's head ---------------------------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def header(h, w):
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate((Q_LUM, Q_CHR)):
        out += _seg(0xDB, bytes([i]) + bytes(q[ZIGZAG[k]] for k in range(64)))
    out += _seg(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS), (0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS)):
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, struct.pack(">H", R))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


HEADER_BYTES = len(header(1, 1))         # 629


# ---- pixels -> quantised coefficients ----------------------------------------------------------------------------------------------
def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(px):
    """[h][w][3] uint8 -> [3][h][w] int64 in 0..255 (libjpeg jccolor.c: 16-bit fixed point, +32768 to round; chroma +128)"""
    r, g, b = (px[..., k].astype(np.int64) for k in range(3))
    half, off = 1 << 15, 128 << 16
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off + half - 1) >> 16
    return np.stack([y, cb, cr])


CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """libjpeg jfdctint.c, one pass over the last axis of d ([..., 8] int64)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        o[0], o[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541196100
    o[2] = _descale(z1 + t13 * F_0_765366865, n)
    o[6] = _descale(z1 - t12 * F_1_847759065, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175875602
    t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_islow(blocks):
    """[..., 8, 8] level-shifted samples -> the DCT coefficients scaled by 8: rows first, then columns"""
    x = _fdct_1d(blocks.astype(np.int64), True)
    return np.swapaxes(_fdct_1d(np.swapaxes(x, -1, -2), False), -1, -2)


def quantise(coef, q):
    """[..., 64] natural order, q [64]: the magnitude plus half the divisor, divided by 8 q, the sign put back"""
    d = np.asarray(q, np.int64) * 8
    m = (np.abs(coef) + (d >> 1)) // d
    return np.where(coef < 0, -m, m)


def quantised_blocks(px):
    """[h][w][3] uint8 -> [MCU rows][MCU columns][3][64] quantised coefficients in ZIG-ZAG order"""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    ycc = rgb_to_ycc(px)
    ycc = ycc[:, np.minimum(np.arange(H), h - 1)][:, :, np.minimum(np.arange(W), w - 1)] - 128        # edge replication, level shift
    blocks = ycc.reshape(3, H // 8, 8, W // 8, 8).transpose(1, 3, 0, 2, 4)                            # [my][mx][c][8][8]
    coef = fdct_islow(blocks).reshape(H // 8, W // 8, 3, 64)
    out = np.empty_like(coef)
    for c in range(3):
        out[:, :, c] = quantise(coef[:, :, c], QTABLES[c])[..., ZIGZAG]
    return out


# ---- entropy coding ----------------------------------------------------------------------------------------------------------------
def _size(v):
    return int(abs(v)).bit_length()


def block_symbols(zz, pred, table):
    """one block (64 zig-zag coefficients) -> [(bits, length)] ; a negative value is sent as v - 1 in `size` bits"""
    out = []
    diff = int(zz[0]) - pred
    s = _size(diff)
    out.append(DC_CODES[table][s])
    if s:
        out.append(((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s))
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(AC_CODES[table][0xF0])
            run -= 16
        s = _size(v)
        out.append(AC_CODES[table][(run << 4) | s])
        out.append(((v if v >= 0 else v - 1) & ((1 << s) - 1), s))
        run = 0
    if run:
        out.append(AC_CODES[table][0x00])
    return out


def interval_bytes(mcus):
    """[n][3][64] -> the interval's entropy-coded bytes: padded with 1-bits, a 0x00 behind every 0xFF (no marker)"""
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    for m in mcus:
        for c in range(3):
            for v, l in block_symbols(m[c], pred[c], TABLE_OF[c]):
                acc = (acc << l) | v
                nbits += l
            pred[c] = int(m[c][0])
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00")


def intervals(px):
    q = quantised_blocks(px)
    flat = q.reshape(-1, 3, 64)          # raster order of MCUs
    return [flat[o:o + R] for o in range(0, len(flat), R)]


def jpeg_file(px):
    """[h][w][3] uint8 -> the bytes of the JPEG file the device writes"""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    assert 1 <= h <= 8192 and 1 <= w <= 8192
    parts = [header(h, w)]
    ivs = intervals(px)
    for m, iv in enumerate(ivs):
        parts.append(interval_bytes(iv))
        parts.append(b"\xff\xd9" if m == len(ivs) - 1 else bytes([0xFF, 0xD0 + (m & 7)]))
    return b"".join(parts)


def jpeg_base64(px):
    return base64.b64encode(jpeg_file(px))


# ---- the worst case, from the tables ------------------------------------------------------------------------------------------------
# |coefficient| <= COEF_MAX[natural index]: the exact DCT of samples in -128..127, scaled by 8 as islow's output is, is at most
# 8 * 128 * (C(u)/2 * sum_x |cos((2x+1) u pi / 16)|) * (the same in v); islow's own error (13-bit constants, two roundings per pass)
# is a few units of that scale, and 16 units are allowed for it.
def _abs_sum(u):
    return (math.sqrt(0.5) if u == 0 else 1.0) / 2 * sum(abs(math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8))


COEF_MAX = [int(math.floor(8 * 128 * _abs_sum(k // 8) * _abs_sum(k % 8) + 0.5)) + 16 for k in range(64)]      # (rounded: no product lies within 0.07 of a half)


def size_max(table):
    """per ZIG-ZAG position: the largest magnitude category the quantised coefficient can have (position 0: of the DC DIFFERENCE)"""
    q = (Q_LUM, Q_CHR)[table]
    out = []
    for k in range(64):
        n = ZIGZAG[k]
        m = (COEF_MAX[n] + 4 * q[n]) // (8 * q[n])
        out.append(_size(2 * m if k == 0 else m))
    return out


def block_bits_max(table):
    """The most bits one block can take: the exact maximum over every sequence of (run, size) symbols whose sizes respect size_max,
    by dynamic programming over the position of the last non-zero coefficient.  best[p]: the most bits of DC and positions 1..p when
    position p is non-zero (best[0]: the DC alone)."""
    smax = size_max(table)
    dc, ac = DC_CODES[table], AC_CODES[table]
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


MCU_BITS_MAX = block_bits_max(0) + 2 * block_bits_max(1)


def interval_bound(nmcu):
    """bytes of one interval of nmcu MCUs at most: its bits padded to a byte, every byte doubled by stuffing, the marker"""
    return 2 * ((nmcu * MCU_BITS_MAX + 7) // 8) + 2


def file_bound(h, w):
    nmcu = ((h + 7) // 8) * ((w + 7) // 8)
    full, tail = divmod(nmcu, R)
    return HEADER_BYTES + full * interval_bound(R) + (interval_bound(tail) if tail else 0)


def base64_bound(h, w):
    if not (1 <= h <= 8192 and 1 <= w <= 8192):
        return 0
    return (file_bound(h, w) + 2) // 3 * 4
