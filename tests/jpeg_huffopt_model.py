"""The device's JPEG result with OPTIMISED Huffman tables, as a Python model: tests/jpeg_opt_model.py with libjpeg's two-pass scheme
(jchuff.c: encode_mcu_gather, jpeg_gen_optimal_table) in place of the fixed Annex K tables.  The colour transform, DCT, quantiser,
mcus(), the restart rule and huffman_codes are imported; this file restates only what the feature changes.

    statistics  four histograms per image, over the whole image: DC and AC of table 0 (Y) and of table 1 (Cb and Cr together).  The
                symbols are the coder's own: the size category of the DC difference; (run << 4) | size; 0xF0 per run of 16 zeros;
                0x00 when the block ends in zeros.  The DC predictors restart at every restart interval in this pass too.
    tables      gen_optimal_table below, libjpeg's steps in libjpeg's order
    file        as jpeg_opt_model.jpeg_file, except that the four DHT segments (0x00, 0x10, 0x01, 0x11) carry the image's own tables,
                so the head's length varies (never above the fixed 629 bytes: a DC table has at most 12 symbols, an AC table 162)

Held to libjpeg-turbo's file (Pillow, optimize=True) byte for byte by tests/test_jpeg_huffopt_model.py."""
import base64
import struct

import numpy as np

import jpeg_model as base
import jpeg_opt_model as opt

R_OF = opt.R_OF
HIST_ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))      # (is AC, table) of histogram / DHT segment 0..3: 0x00, 0x10, 0x01, 0x11


def _coded(v):
    s = int(abs(v)).bit_length()
    return s, ((v if v >= 0 else v - 1) & ((1 << s) - 1))


def block_symbols(zz, pred):
    """one block -> [(is AC, symbol, value bits, number of value bits)], in the order the coder sends them"""
    out = []
    s, bits = _coded(int(zz[0]) - pred)
    out.append((0, s, bits, s))
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        s, bits = _coded(v)
        out.append((1, (run << 4) | s, bits, s))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def interval_symbols(ms, sampling):
    """the MCUs of one interval -> [(table, is AC, symbol, value bits, nbits)]: three DC chains, all starting at 0"""
    ny = 4 if sampling == 2 else 1
    pred = [0, 0, 0]
    out = []
    for m in ms:
        for k, (table, zz) in enumerate(m):
            c = 0 if k < ny else k - ny + 1
            out += [(table,) + sym for sym in block_symbols(zz, pred[c])]
            pred[c] = int(zz[0])
    return out


def intervals_of(ms, sampling):
    r = R_OF[sampling]
    return [ms[o:o + r] for o in range(0, len(ms), r)]


def histograms(ms, sampling):
    """[4][256] counts in HIST_ORDER"""
    h = np.zeros((4, 256), np.int64)
    for iv in intervals_of(ms, sampling):
        for table, is_ac, sym, _, _ in interval_symbols(iv, sampling):
            h[HIST_ORDER.index((is_ac, table)), sym] += 1
    return h


def gen_optimal_table(counts):
    """libjpeg's jpeg_gen_optimal_table: [256] counts -> (bits[16], vals, the longest code length BEFORE the limit to 16).
    The length arrays are sized for any depth up to 256 and the limiting loop starts at the longest length present (libjpeg's own
    arrays end at 32, where it aborts; the result is libjpeg's wherever libjpeg gives one)."""
    freq = [int(c) for c in counts] + [1]                # 1. the pseudo-symbol 256: no real symbol gets the all-ones code
    codesize = [0] * 257
    others = [-1] * 257
    while True:

        def smallest(skip):                              # 2. the smallest non-zero count; among equals the LARGEST index
            c, v = -1, None
            for i in range(257):
                if freq[i] and i != skip and (v is None or freq[i] <= v):
                    c, v = i, freq[i]
            return c

        c1 = smallest(-1)
        c2 = smallest(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]                             # 3. merge
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    bits = [0] * (max(longest, 16) + 1)                  # 4.
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(longest, 16, -1):                     # 5. limit the lengths to 16
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16                                               # 6. the pseudo-symbol leaves
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for i in range(1, longest + 1) for j in range(256) if codesize[j] == i]      # 7.
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals, longest


def tables_of(hist):
    """[4][256] -> [(bits, vals)] in HIST_ORDER"""
    return [gen_optimal_table(h)[:2] for h in hist]


def header(h, w, quality, sampling, tabs):
    opt.check(quality, sampling)
    out = b"\xff\xd8" + base._seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(opt.quant_tables(quality)):
        out += base._seg(0xDB, bytes([i]) + bytes(q[opt.ZIGZAG[k]] for k in range(64)))
    out += base._seg(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22 if sampling == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (is_ac, table), (bits, vals) in zip(HIST_ORDER, tabs):
        out += base._seg(0xC4, bytes([(is_ac << 4) | table]) + bytes(bits) + bytes(vals))
    out += base._seg(0xDD, struct.pack(">H", R_OF[sampling]))
    out += base._seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def interval_bytes(ms, sampling, codes):
    """codes[is AC][table]: {symbol: (code, length)}"""
    acc, nbits = 0, 0
    for table, is_ac, sym, vbits, nv in interval_symbols(ms, sampling):
        code, length = codes[is_ac][table][sym]
        acc = (((acc << length) | code) << nv) | vbits
        nbits += length + nv
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def jpeg_file(px, quality=85, sampling=0):
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    assert 1 <= h <= 8192 and 1 <= w <= 8192
    ms = opt.mcus(px, quality, sampling)
    tabs = tables_of(histograms(ms, sampling))
    codes = [[None, None], [None, None]]
    for (is_ac, table), (bits, vals) in zip(HIST_ORDER, tabs):
        codes[is_ac][table] = base.huffman_codes(bits, vals)
    parts = [header(h, w, quality, sampling, tabs)]
    ivs = intervals_of(ms, sampling)
    for m, iv in enumerate(ivs):
        parts.append(interval_bytes(iv, sampling, codes))
        parts.append(b"\xff\xd9" if m == len(ivs) - 1 else bytes([0xFF, 0xD0 + (m & 7)]))
    return b"".join(parts)


def jpeg_base64(px, quality=85, sampling=0):
    return base64.b64encode(jpeg_file(px, quality, sampling))


def image_histograms(px, quality, sampling):
    return histograms(opt.mcus(np.ascontiguousarray(px, np.uint8), quality, sampling), sampling)


# ---- the worst case under ANY table -------------------------------------------------------------------------------------------------
# A code has at most 16 bits.  Price every one of a block's 64 positions at 16 bits plus the largest size category it can have
# (jpeg_opt_model.size_max): a coded coefficient costs that at most; a ZRL code (at most 16 bits) stands for 16 zero positions and the
# EOB (at most 16 bits) for at least one, and each of those positions is priced at 16 bits or more.
def block_bits_any(table, quality):
    return sum(16 + s for s in opt.size_max(table, quality))


def mcu_bits_any(quality, sampling):
    opt.check(quality, sampling)
    return (4 if sampling == 2 else 1) * block_bits_any(0, quality) + 2 * block_bits_any(1, quality)


RAW_ANY = max((R_OF[s] * mcu_bits_any(100, s) + 7) // 8 for s in R_OF)      # bytes of an interval before stuffing: the one size class


def interval_bound(nmcu, quality, sampling):
    return 2 * ((nmcu * mcu_bits_any(quality, sampling) + 7) // 8) + 2


def file_bound(h, w, quality, sampling):
    p = 16 if sampling == 2 else 8
    nmcu = ((h + p - 1) // p) * ((w + p - 1) // p)
    full, tail = divmod(nmcu, R_OF[sampling])
    return opt.HEADER_BYTES + full * interval_bound(R_OF[sampling], quality, sampling) + (interval_bound(tail, quality, sampling) if tail else 0)


def base64_bound(h, w, quality, sampling):
    if not (1 <= h <= 8192 and 1 <= w <= 8192 and 1 <= quality <= 100 and sampling in R_OF):
        return 0
    return (file_bound(h, w, quality, sampling) + 2) // 3 * 4
