"""A numpy restatement of the PROGRESSIVE side of the device's JPEG decoder (csrc/jpeg_parse.hpp parse_progressive, csrc/jpeg_dec_core.hpp's
scan kinds): the multi-scan parser with its refusals and dependency levels, and the four Huffman scan decoders written straight from
T.81 Annex G (figures G.3 - G.7; one block after the other, one bit after the other -- no lanes, no masks, no records).  The pixels
come from jpeg_decode_model's own inverse DCT, upsampling and colour transform, imported and not edited.  Reasons are the C side's
without their "invalid: "."""
import struct

import numpy as np

import jpeg_decode_model as base
from jpeg_decode_model import Corrupt, Refused, ZIGZAG, _Bits, _huff_lookup      # noqa: F401

MAX_SCANS = 64
DC_FIRST, AC_FIRST, DC_REFINE, AC_REFINE = 1, 2, 3, 4


class Scan:
    pass


def _cut(data, i, restart, nstreams):
    """entropy-coded data from data[i] on -> ([stream bytes without stuffing], the place of the marker behind it)"""
    out, cur, n = [], bytearray(), len(data)
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
            if not restart or len(out) + 1 >= nstreams or m != 0xD0 + (len(out) & 7):
                raise Refused("corrupt JPEG data (restart markers out of order)")
            out.append(bytes(cur))
            cur.clear()
            i = q + 2
        elif m == 0xDC:
            raise Refused("JPEG with a DNL marker")
        else:
            if len(out) + 1 != nstreams:
                raise Refused("corrupt JPEG data (restart markers missing)")
            out.append(bytes(cur))
            return out, q


def plan(data):
    """bytes of a progressive file -> Plan (the frame as jpeg_decode_model's, and .scans); raises Refused"""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Refused("not a JPEG file (no SOI)")
    p = base.Plan()
    p.scans, p.nlevels = [], 1
    restart = 0
    qt, huff = {}, {}
    jfif = adobe = False
    sof = None
    coef_bits, coef_level = None, None
    i = 2
    while True:
        trunc = Refused("truncated JPEG header" if not p.scans else "truncated JPEG scan (no EOI)")
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
            if not p.scans:
                raise Refused("JPEG file without a scan")
            if any(b != 0 for c in range(p.ncomp) for b in coef_bits[c]):
                raise Refused("progressive JPEG with an incomplete scan script (it would be smoothed)")
            return p
        trunc = Refused("truncated JPEG header")
        if i + 2 > n:
            raise trunc
        ln = struct.unpack(">H", data[i:i + 2])[0]
        if ln < 2 or i + ln > n:
            raise trunc
        seg = data[i + 2:i + ln]
        i += ln
        if m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Refused("arithmetic-coded JPEG")
        if m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise Refused("lossless or hierarchical JPEG")
        if m == 0xDC:
            raise Refused("JPEG with a DNL marker")
        if m in (0xC0, 0xC1, 0xC2):
            if sof is not None or m != 0xC2:
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
            p.hs = [c[1] for c in sof]
            p.vs = [c[2] for c in sof]
            hmax, vmax = p.hs[0], p.vs[0]
            p.mcus_w, p.mcus_h = -(-p.w // (8 * hmax)), -(-p.h // (8 * vmax))
            p.plane = [(-(-p.h * p.vs[c] // vmax), -(-p.w * p.hs[c] // hmax)) for c in range(p.ncomp)]      # real (rows, columns)
            coef_bits = [[-1] * 64 for _ in range(nc)]
            coef_level = [[0] * 64 for _ in range(nc)]
        elif m == 0xDB:
            if p.scans:
                raise Refused("progressive JPEG with a DQT behind the first scan")
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
            restart = struct.unpack(">H", seg[:2])[0]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            adobe = adobe or seg[:5] == b"Adobe"
        elif m == 0xDA:
            if sof is None:
                raise Refused("corrupt JPEG header (SOS before SOF)")
            if len(p.scans) >= MAX_SCANS:
                raise Refused("progressive JPEG with more than 64 scans")
            if not p.scans:
                if p.ncomp == 3:
                    if adobe:
                        raise Refused("JPEG with an Adobe marker (RGB / YCCK colour)")
                    if not jfif and [c[0] for c in sof] != [1, 2, 3]:
                        raise Refused("JPEG whose colour space is not Y Cb Cr")
                if any(c[3] not in qt for c in sof):
                    raise Refused("corrupt JPEG header (frame names a missing quantiser table)")
                p.quant = [qt[c[3]] for c in sof]
            if len(seg) < 1:
                raise trunc
            ns = seg[0]
            if not 1 <= ns <= p.ncomp:
                raise Refused("progressive JPEG scan with a wrong number of components")
            sc = Scan()
            sc.comps, sc.dc, sc.ac = [], {}, {}
            sel = []
            for k in range(ns):
                if len(seg) < 3 + 2 * k:
                    raise trunc
                cid, tt = seg[1 + 2 * k], seg[2 + 2 * k]
                ci = next((j for j in range(p.ncomp) if sof[j][0] == cid), None)
                if ci is None or (sc.comps and ci <= sc.comps[-1]):
                    raise Refused("progressive JPEG scan (components unknown or out of frame order)")
                if (tt >> 4) > 3 or (tt & 15) > 3:
                    raise Refused("corrupt JPEG header (Huffman table number)")
                sc.comps.append(ci)
                sel.append((tt >> 4, tt & 15))
            if len(seg) < 1 + 2 * ns + 3:
                raise trunc
            ss, se, ahl = seg[1 + 2 * ns:4 + 2 * ns]
            ah, al = ahl >> 4, ahl & 15
            if (se != 0) if ss == 0 else (se < ss or se > 63):
                raise Refused("progressive JPEG scan with a wrong band (Ss, Se)")
            if ss != 0 and ns != 1:
                raise Refused("progressive JPEG with an AC scan of more than one component")
            if al > 13 or (ah != 0 and al + 1 != ah):
                raise Refused("progressive JPEG scan with a wrong bit position (Ah, Al)")
            sc.ss, sc.se, sc.ah, sc.al = ss, se, ah, al
            sc.kind = (DC_REFINE if ah else DC_FIRST) if ss == 0 else (AC_REFINE if ah else AC_FIRST)
            sc.level = 0
            for ci, (td, ta) in zip(sc.comps, sel):
                if ss != 0 and coef_bits[ci][0] < 0:
                    raise Refused("progressive JPEG with an AC scan before the component's DC scan")
                for z in range(ss, se + 1):
                    prev = coef_bits[ci][z]
                    if (ah != 0) if prev < 0 else (ah == 0 or prev != ah):
                        raise Refused("progressive JPEG scan whose Ah is not the Al of the coefficient's last scan")
                    coef_bits[ci][z] = al
                    sc.level = max(sc.level, coef_level[ci][z] + (0 if prev < 0 else 1))
                if sc.kind == DC_FIRST and (0, td) not in huff:
                    raise Refused("corrupt JPEG header (scan names a missing Huffman table)")
                if ss != 0 and (1, ta) not in huff:
                    raise Refused("corrupt JPEG header (scan names a missing Huffman table)")
                sc.dc[ci], sc.ac[ci] = huff.get((0, td)), huff.get((1, ta))
            for ci in sc.comps:
                for z in range(ss, se + 1):
                    coef_level[ci][z] = sc.level
            if ns == 1:          # not interleaved: the blocks of the component's REAL plane, row by row
                c = sc.comps[0]
                sc.rw, sc.rh = -(-p.plane[c][1] // 8), -(-p.plane[c][0] // 8)
                sc.nmcu = sc.rw * sc.rh
            else:
                sc.nmcu = p.mcus_w * p.mcus_h
            sc.restart = restart
            sc.nstreams = -(-sc.nmcu // restart) if restart else 1
            sc.streams, i = _cut(data, i, restart, sc.nstreams)
            p.nlevels = max(p.nlevels, sc.level + 1)
            p.scans.append(sc)


def _blocks(p, sc, grids, mcu):
    """the blocks of MCU `mcu` of the scan, in its order: (component, its 64 coefficients)"""
    if len(sc.comps) == 1:
        c = sc.comps[0]
        y, x = divmod(mcu, sc.rw)
        return [(c, grids[c][y, x])]
    my, mx = divmod(mcu, p.mcus_w)
    return [(c, grids[c][my * p.vs[c] + by, mx * p.hs[c] + bx]) for c in sc.comps for by in range(p.vs[c]) for bx in range(p.hs[c])]


def _bit(bits):
    bits._fill(1)
    bits.n -= 1
    v = (bits.acc >> bits.n) & 1
    bits.acc &= (1 << bits.n) - 1
    return v


def _uint(bits, s):
    v = 0
    for _ in range(s):
        v = (v << 1) | _bit(bits)
    return v


def _refine_nonzero(bits, blk, z, p1):
    """G.1.2.3: a correction bit for a coefficient with a non-zero history"""
    if _bit(bits) and not (int(blk[z]) & p1):
        blk[z] += p1 if blk[z] >= 0 else -p1


def _decode_stream(p, sc, grids, data, mcu0, nmcu):
    bits = _Bits(data)
    pred = {c: 0 for c in sc.comps}
    eobrun = 0
    p1 = 1 << sc.al
    for mcu in range(mcu0, mcu0 + nmcu):
        for c, blk in _blocks(p, sc, grids, mcu):
            if sc.kind == DC_FIRST:
                s = bits.symbol(sc.dc[c])
                if s > 11:
                    raise Corrupt("a DC category above 11")
                pred[c] += bits.value(s)
                blk[0] = pred[c] * p1
            elif sc.kind == DC_REFINE:
                if _bit(bits):
                    blk[0] = int(blk[0]) | p1
            elif sc.kind == AC_FIRST:
                if eobrun:
                    eobrun -= 1
                    continue
                k = sc.ss
                while k <= sc.se:
                    rs = bits.symbol(sc.ac[c])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            eobrun = (1 << r) + _uint(bits, r) - 1
                            break
                        k += 16
                        if k > sc.se:
                            raise Corrupt("a run that leaves the band")
                        continue
                    k += r
                    if k > sc.se:
                        raise Corrupt("a run that leaves the band")
                    blk[ZIGZAG[k]] = bits.value(s) * p1
                    k += 1
            else:
                k = sc.ss
                if not eobrun:
                    while k <= sc.se:
                        rs = bits.symbol(sc.ac[c])
                        r, s = rs >> 4, rs & 15
                        if s:
                            if s != 1:
                                raise Corrupt("a refinement symbol of size above 1")
                            s = p1 if _bit(bits) else -p1
                        elif r != 15:
                            eobrun = (1 << r) + _uint(bits, r)
                            break
                        while True:                      # over the non-zero ones, and r zero ones
                            if k > sc.se:
                                raise Corrupt("a run that leaves the band")
                            z = ZIGZAG[k]
                            if blk[z] != 0:
                                _refine_nonzero(bits, blk, z, p1)
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            k += 1
                        if s:
                            blk[ZIGZAG[k]] = s
                        k += 1
                if eobrun:
                    while k <= sc.se:
                        if blk[ZIGZAG[k]] != 0:
                            _refine_nonzero(bits, blk, ZIGZAG[k], p1)
                        k += 1
                    eobrun -= 1
    if eobrun:
        raise Corrupt("an EOB run that overshoots the stream's blocks")
    pos = bits.position()
    if not (pos <= 8 * len(data) and 8 * len(data) - pos < 8):
        raise Corrupt("a stream that ends with blocks missing or bytes left over")


def coefficients(p):
    """Plan -> per component [block rows][block columns][64] int64, natural order: the scans in file order"""
    grids = [np.zeros((p.mcus_h * p.vs[c], p.mcus_w * p.hs[c], 64), np.int64) for c in range(p.ncomp)]
    for sc in p.scans:
        for k, data in enumerate(sc.streams):
            m0 = k * sc.restart if sc.restart else 0
            _decode_stream(p, sc, grids, data, m0, min(sc.restart, sc.nmcu - m0) if sc.restart else sc.nmcu)
    return grids


def levels(p):
    return [sc.level for sc in p.scans]


def decode(data):
    """bytes of a progressive JPEG file -> [h][w][3] uint8; raises Refused or Corrupt"""
    p = plan(data)
    return base.pixels(p, coefficients(p))
