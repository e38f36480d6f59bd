"""The specification of the device's JPEG decoder (csrc/jpeg_parse.hpp, csrc/jpeg_dec_core.hpp, csrc/jpeg_dec.hip) as a Python
model: stdlib + numpy, no product code.  Every step is libjpeg's published integer algorithm, so the model's pixels equal
`PIL.Image.open(f).convert("RGB")` (libjpeg-turbo) byte for byte (tests/test_jpeg_decode_model.py); the CPU build of the lane
algorithm is held to the model's coefficients (tests/test_jpeg_decode_native.py) and the device to its pixels
(tests/test_jpeg_decode_gpu.py).

    plan     = which files the device takes: SOF0 / SOF1, 8 bit, one interleaved scan, 8-bit quantisers, Y Cb Cr at 4:4:4 / 4:2:2 /
               4:2:0 (width >= 5 when subsampled) or grey, 1..8192 per side; everything else is Refused with a reason
    streams  = the scan cut at RSTn, `FF 00` -> `FF`; a stream's DC predictors start at 0
    entropy  = Huffman codes from the file's own DHT, (run, size) symbols, ZRL, EOB, differential DC
    pixels   = dequantise, the "islow" inverse DCT (13-bit constants, 2 pass bits), libjpeg's range limit, "fancy" (triangle)
               chroma upsampling on the REAL plane sizes, YCbCr -> RGB in 16-bit fixed point
"""
import struct

import numpy as np

from jpeg_model import ZIGZAG

SAMPLING_NAMES = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0", 3: "grey"}


class Refused(Exception):
    """the device does not decode this file; .reason says why (the C side's message is "invalid: " + reason)"""

    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


class Plan:
    pass


def _huff_lookup(counts, vals):
    """{(length, code): symbol}; Refused when the counts are no prefix code"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        if code + counts[length - 1] > (1 << length):
            raise Refused("corrupt JPEG header (DHT is no prefix code)")
        for _ in range(counts[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def plan(data):
    """bytes -> Plan (h, w, sampling, tables, where the scan begins); raises Refused"""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Refused("not a JPEG file (no SOI)")
    p = Plan()
    p.restart = 0
    qt, huff = {}, {}
    jfif = adobe = False
    sof = None
    i = 2
    trunc = Refused("truncated JPEG header")
    while True:
        if i >= n:
            raise trunc
        if data[i] != 0xFF:
            raise Refused("corrupt JPEG header (no marker where one must be)")
        while i < n and data[i] == 0xFF:
            i += 1
        if i >= n:
            raise trunc
        m = data[i]
        i += 1
        if m in (0xD8, 0x01, 0x00) or 0xD0 <= m <= 0xD7:
            raise Refused("corrupt JPEG header (stray marker)")
        if m == 0xD9:
            raise Refused("JPEG file without a scan")
        if i + 2 > n:
            raise trunc
        ln = struct.unpack(">H", data[i:i + 2])[0]
        if ln < 2 or i + ln > n:
            raise trunc
        seg = data[i + 2:i + ln]
        i += ln
        if m == 0xC2:
            raise Refused("progressive JPEG (SOF2): not decoded on the device")
        if m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Refused("arithmetic-coded JPEG")
        if m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise Refused("lossless or hierarchical JPEG")
        if m == 0xDC:
            raise Refused("JPEG with a DNL marker")
        if m in (0xC0, 0xC1):
            if sof is not None:
                raise Refused("JPEG with two frames")
            if len(seg) < 6:
                raise trunc
            prec, h, w, nc = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise Refused("JPEG with 12-bit samples")
            if h == 0:
                raise Refused("JPEG with a DNL marker")
            if h > 8192 or not 1 <= w <= 8192:
                raise Refused("JPEG size outside 1..8192")
            if nc == 4:
                raise Refused("JPEG with 4 components (CMYK / YCCK)")
            if nc not in (1, 3):
                raise Refused("JPEG with an unsupported number of components")
            if len(seg) < 6 + 3 * nc:
                raise trunc
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nc)]
            if any(c[3] > 3 for c in comps):
                raise Refused("corrupt JPEG header (quantiser table number)")
            bad = Refused("unsupported sampling factors")
            if nc == 1:
                if comps[0][1:3] != (1, 1):
                    raise bad
                p.sampling = 3
            else:
                if comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
                    raise bad
                p.sampling = {(1, 1): 0, (2, 1): 1, (2, 2): 2}.get(comps[0][1:3])
                if p.sampling is None:
                    raise bad
                if p.sampling and w < 5:
                    raise Refused("subsampled chroma needs a width of at least 5")
            p.h, p.w, p.ncomp, sof = h, w, nc, comps
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                if seg[j] >> 4:
                    raise Refused("JPEG with 16-bit quantiser tables")
                if (seg[j] & 15) > 3 or len(seg) - j - 1 < 64:
                    raise Refused("corrupt JPEG header (DQT)")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = seg[j + 1 + k]
                qt[seg[j] & 15] = t
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                tc = seg[j]
                if (tc >> 4) > 1 or (tc & 15) > 3 or len(seg) - j - 1 < 16:
                    raise Refused("corrupt JPEG header (DHT)")
                counts = list(seg[j + 1:j + 17])
                total = sum(counts)
                if total > 256 or total > len(seg) - j - 17:
                    raise Refused("corrupt JPEG header (DHT counts overrun the segment)")
                huff[((tc >> 4), tc & 15)] = _huff_lookup(counts, list(seg[j + 17:j + 17 + total]))
                j += 17 + total
        elif m == 0xDD:
            if len(seg) < 2:
                raise trunc
            p.restart = struct.unpack(">H", seg[:2])[0]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            adobe = adobe or seg[:5] == b"Adobe"
        elif m == 0xDA:
            if sof is None:
                raise Refused("corrupt JPEG header (SOS before SOF)")
            if len(seg) < 1:
                raise trunc
            if seg[0] != p.ncomp:
                raise Refused("multi-scan JPEG")
            if len(seg) < 1 + 2 * p.ncomp + 3:
                raise trunc
            p.dc, p.ac, p.quant = [], [], []
            for k in range(p.ncomp):
                cid, tt = seg[1 + 2 * k], seg[2 + 2 * k]
                if cid != sof[k][0]:
                    raise Refused("multi-scan JPEG (components out of frame order)")
                if (tt >> 4) > 3 or (tt & 15) > 3:
                    raise Refused("corrupt JPEG header (Huffman table number)")
                if (0, tt >> 4) not in huff or (1, tt & 15) not in huff:
                    raise Refused("corrupt JPEG header (scan names a missing Huffman table)")
                if sof[k][3] not in qt:
                    raise Refused("corrupt JPEG header (frame names a missing quantiser table)")
                p.dc.append(huff[(0, tt >> 4)])
                p.ac.append(huff[(1, tt & 15)])
                p.quant.append(qt[sof[k][3]])
            if tuple(seg[1 + 2 * p.ncomp:4 + 2 * p.ncomp]) != (0, 63, 0):
                raise Refused("progressive JPEG scan parameters")
            if p.ncomp == 3:
                if adobe:
                    raise Refused("JPEG with an Adobe marker (RGB / YCCK colour)")
                if not jfif and [c[0] for c in sof] != [1, 2, 3]:
                    raise Refused("JPEG whose colour space is not Y Cb Cr")
            p.hs = [c[1] for c in sof]
            p.vs = [c[2] for c in sof]
            hmax, vmax = p.hs[0], p.vs[0]
            p.mcus_w, p.mcus_h = -(-p.w // (8 * hmax)), -(-p.h // (8 * vmax))
            p.nmcu = p.mcus_w * p.mcus_h
            p.plane = [(-(-p.h * p.vs[c] // vmax), -(-p.w * p.hs[c] // hmax)) for c in range(p.ncomp)]      # real (rows, columns)
            p.scan_off = i
            p.nstreams = -(-p.nmcu // p.restart) if p.restart else 1
            p.streams = _split(p, data)
            return p


def _split(p, data):
    """the scan -> [(bytes without stuffing, first MCU, MCU count)]"""
    out, cur, i, n = [], bytearray(), p.scan_off, len(data)

    def finish():
        m0 = len(out) * p.restart if p.restart else 0
        out.append((bytes(cur), m0, min(p.restart, p.nmcu - m0) if p.restart else p.nmcu))
        cur.clear()
    while True:
        q = data.find(b"\xff", i)
        cur += data[i:q if q >= 0 else n]
        if q < 0 or q + 1 >= n:
            raise Refused("truncated JPEG scan (no EOI)")
        m = data[q + 1]
        if m == 0x00:
            cur.append(0xFF)
            i = q + 2
        elif m == 0xFF:
            i = q + 1
        elif 0xD0 <= m <= 0xD7:
            if not p.restart or len(out) + 1 >= p.nstreams or m != 0xD0 + (len(out) & 7):
                raise Refused("corrupt JPEG data (restart markers out of order)")
            finish()
            i = q + 2
        elif m == 0xD9:
            if len(out) + 1 != p.nstreams:
                raise Refused("corrupt JPEG data (restart markers missing)")
            finish()
            return out
        elif m == 0xDC:
            raise Refused("JPEG with a DNL marker")
        else:
            raise Refused("multi-scan JPEG (a marker follows the first scan)")


class Corrupt(Exception):
    """what the device reports as a non-zero status word"""


class _Bits:
    def __init__(self, b):
        self.b, self.i, self.acc, self.n = b, 0, 0, 0

    def _fill(self, need):
        while self.n < need:
            self.acc = (self.acc << 8) | (self.b[self.i] if self.i < len(self.b) else 0xFF)      # libjpeg pads with 1-bits
            self.i += 1
            self.n += 8

    def symbol(self, table):
        self._fill(16)
        for length in range(1, 17):
            s = table.get((length, (self.acc >> (self.n - length)) & ((1 << length) - 1)))
            if s is not None:
                self.n -= length
                self.acc &= (1 << self.n) - 1
                return s
        raise Corrupt("a code that no table holds")

    def value(self, s):
        if s == 0:
            return 0
        self._fill(s)
        self.n -= s
        v = (self.acc >> self.n) & ((1 << s) - 1)
        self.acc &= (1 << self.n) - 1
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    def position(self):
        return 8 * self.i - self.n


def coefficients(p):
    """Plan -> per component [block rows][block columns][64] int64, natural order, DC absolute (not yet dequantised)"""
    grids = [np.zeros((p.mcus_h * p.vs[c], p.mcus_w * p.hs[c], 64), np.int64) for c in range(p.ncomp)]
    for data, mcu0, nmcu in p.streams:
        bits = _Bits(data)
        pred = [0] * p.ncomp
        for mcu in range(mcu0, mcu0 + nmcu):
            my, mx = divmod(mcu, p.mcus_w)
            for c in range(p.ncomp):
                for by in range(p.vs[c]):
                    for bx in range(p.hs[c]):
                        blk = grids[c][my * p.vs[c] + by, mx * p.hs[c] + bx]
                        s = bits.symbol(p.dc[c])
                        if s > 11:
                            raise Corrupt("a DC category above 11")
                        pred[c] += bits.value(s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(p.ac[c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 63:
                                    raise Corrupt("a zig-zag index above 63")
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt("a zig-zag index above 63")
                            blk[ZIGZAG[k]] = bits.value(s)
                            k += 1
        pos = bits.position()
        if not (pos <= 8 * len(data) and 8 * len(data) - pos < 8):
            raise Corrupt("a stream that ends with blocks missing or bytes left over")
    return grids


# ---- libjpeg's jidctint.c "islow" --------------------------------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(d, shift):
    """one pass over the last axis of d ([..., 8] int64): -> (x + 2^(shift-1)) >> shift"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    z1 = (d2 + d6) * F_0_541196100
    t2 = z1 - d6 * F_1_847759065
    t3 = z1 + d2 * F_0_765366865
    t0 = (d0 + d4) << CONST_BITS
    t1 = (d0 - d4) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175875602
    t0, t1, t2, t3 = t0 * F_0_298631336, t1 * F_2_053119869, t2 * F_3_072711026, t3 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return (np.stack(o, axis=-1) + (1 << (shift - 1))) >> shift


def idct_islow_raw(coef):
    """[..., 8, 8] dequantised coefficients -> level-shifted samples before the range limit: columns ((x + 2^10) >> 11), rows ((x + 2^17) >> 18)"""
    ws = np.swapaxes(_idct_1d(np.swapaxes(coef.astype(np.int64), -1, -2), CONST_BITS - PASS1_BITS), -1, -2)
    return _idct_1d(ws, CONST_BITS + PASS1_BITS + 3)


def idct_islow(coef):
    """-> samples 0..255 by libjpeg's range limit (its C code: a table indexed by x & 1023)"""
    x = idct_islow_raw(coef)
    v = x & 1023
    v = np.where(v >= 512, v - 1024, v)
    return np.clip(v + 128, 0, 255)


def planes(p, grids=None):
    """-> per component its REAL plane [rows][columns] int64 (the blocks' padding cut off)"""
    grids = coefficients(p) if grids is None else grids
    out = []
    for c in range(p.ncomp):
        g = grids[c] * np.asarray(p.quant[c], np.int64)
        bh, bw, _ = g.shape
        # No picture gives these, and there libjpeg-turbo's SIMD code (16-bit products, saturating packs) and its C code (the
        # masking table above) give different bytes: the device flags the image (status bit 16) instead of choosing one.
        raw = idct_islow_raw(g.reshape(bh, bw, 8, 8))
        if np.abs(g).max() > 32767 or raw.min() < -512 or raw.max() > 511:
            raise Corrupt("a dequantised coefficient outside int16 or a sample outside -512..511 before the range limit")
        s = idct_islow(g.reshape(bh, bw, 8, 8)).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(s[:p.plane[c][0], :p.plane[c][1]])
    return out


def upsample_h2v1(rows, w):
    """jdsample.c h2v1_fancy_upsample on [r][cw] -> [r][w]"""
    cw = rows.shape[1]
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    out = np.empty((rows.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * rows + left + 1) >> 2
    out[:, 1::2] = (3 * rows + right + 2) >> 2
    out[:, 0] = rows[:, 0]
    out[:, 2 * cw - 1] = rows[:, cw - 1]
    return out[:, :w]


def upsample_h2v2(pl, h, w):
    """jdsample.c h2v2_fancy_upsample on [ch][cw] -> [h][w]"""
    ch, cw = pl.shape
    above = np.concatenate([pl[:1], pl[:-1]], axis=0)
    below = np.concatenate([pl[1:], pl[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for par, nb in ((0, above), (1, below)):
        cs = 3 * pl + nb
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * cs + left + 8) >> 4
        out[par::2, 1::2] = (3 * cs + right + 7) >> 4
    return out[:h, :w]


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(p, grids=None):
    pl = planes(p, grids)
    if p.sampling == 3:
        return np.repeat(pl[0].astype(np.uint8)[:, :, None], 3, axis=2)
    y, cb, cr = pl
    if p.sampling == 1:
        cb, cr = upsample_h2v1(cb, p.w), upsample_h2v1(cr, p.w)
    elif p.sampling == 2:
        cb, cr = upsample_h2v2(cb, p.h, p.w), upsample_h2v2(cr, p.h, p.w)
    return ycc_to_rgb(y, cb, cr)


def decode(data):
    """bytes of a JPEG file -> [h][w][3] uint8; raises Refused (not the device's file) or Corrupt (the device's status word)"""
    return pixels(plan(data))
