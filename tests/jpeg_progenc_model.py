"""The device's PROGRESSIVE JPEG result, as a Python model: the quantised coefficients of tests/jpeg_opt_model.py sent as libjpeg's
ten jpeg_simple_progression scans (jcphuff.c), every scan with its own optimal Huffman table (jpeg_gen_optimal_table, restated in
tests/jpeg_huffopt_model.py) and a restart interval of one MCU row of the scan.  Held to libjpeg-turbo's file

    Image.fromarray(px).save(f, "JPEG", quality=q, subsampling=s, progressive=True, restart_marker_rows=1)

byte for byte by tests/test_jpeg_progenc_model.py.

    planes      the coefficients per component, blocks in raster order, 64 zig-zag values each.  4:4:4: ceil(h/8) x ceil(w/8) blocks
                per component.  4:2:0: Y on the MCU grid, 2 ceil(h/16) x 2 ceil(w/16) blocks, dummy blocks included (all AC 0, the DC
                the encoder gives them today); Cb and Cr ceil(h/16) x ceil(w/16).
    scans       SCANS below: (components, Ss, Se, Ah, Al).  A DC scan is interleaved and walks the MCUs; an AC scan walks the
                component's OWN blocks, ceil(h_c/8) rows of ceil(w_c/8) -- no dummy blocks.
    intervals   one block row (MCU row) of the scan: the restart interval is the scan's MCUs per row, written as a DRI whenever it
                changes from the scan before.  RSTm stands between intervals, m counting from 0 in every scan; none behind the last.
    coders      the four of jcphuff.c, below, as a walk over the interval's blocks with the state that crosses blocks: the DC
                predictors; EOBRUN; in a refinement scan the buffered correction bits (BE).  A coder yields ('sym', table, symbol) and
                ('bits', value, count); the statistics pass counts the first, the emit pass sends both.
    tables      TABLES: ten per image, in file order; (scan, DHT class-and-id byte).

EVENTS counts what the walk did, so that tests/jpeg_progenc_cases.py can show that every rule fired."""
import base64
import collections
import struct

import numpy as np

import jpeg_huffopt_model as huff
import jpeg_model as base
import jpeg_opt_model as opt

SCANS = (((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
         ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))
# the ten tables in file order: (scan, Tc << 4 | Th)
TABLES = ((0, 0x00), (0, 0x01), (1, 0x10), (2, 0x11), (3, 0x11), (4, 0x10), (5, 0x10), (7, 0x11), (8, 0x11), (9, 0x10))
MAX_CORR_BITS = 1000
EVENTS = collections.Counter()


def table_slot(scan, comp):
    """the index into TABLES of the table a component's blocks use in a scan; None: the DC refinement scan has none"""
    if scan == 0:
        return 0 if comp == 0 else 1
    return {1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 7: 7, 8: 8, 9: 9}.get(scan)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def geometry(h, w, sampling):
    """per component: (stored rows, stored cols, own rows, own cols) in blocks; and the MCU grid (rows, cols)"""
    yh, yw = (h + 7) // 8, (w + 7) // 8
    if sampling == 0:
        return [(yh, yw, yh, yw)] * 3, (yh, yw)
    mh, mw = (h + 15) // 16, (w + 15) // 16
    return [(2 * mh, 2 * mw, yh, yw), (mh, mw, mh, mw), (mh, mw, mh, mw)], (mh, mw)


def planes_of(px, quality, sampling):
    """pixels -> [3] arrays [rows][cols][64] int64, through today's front end (jpeg_opt_model.mcus)"""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    geo, (mh, mw) = geometry(h, w, sampling)
    out = [np.zeros((g[0], g[1], 64), np.int64) for g in geo]
    for m, blocks in enumerate(opt.mcus(px, quality, sampling)):
        i, j = divmod(m, mw)
        if sampling == 0:
            for c in range(3):
                out[c][i, j] = blocks[c][1]
        else:
            for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                out[0][2 * i + a, 2 * j + b] = blocks[k][1]
            out[1][i, j] = blocks[4][1]
            out[2][i, j] = blocks[5][1]
    return out


def flat_coefs(planes):
    """the layout of ire_debug_jpeg_progressive_from_coefs: [blocks][64] int16, component after component"""
    return np.concatenate([p.reshape(-1, 64) for p in planes]).astype(np.int16)


def planes_from_flat(flat, h, w, sampling):
    geo, _ = geometry(h, w, sampling)
    out, o = [], 0
    for g in geo:
        out.append(np.asarray(flat[o:o + g[0] * g[1]], np.int64).reshape(g[0], g[1], 64))
        o += g[0] * g[1]
    assert o == len(flat)
    return out


def intervals(planes, h, w, sampling, scan):
    """the scan's restart intervals: each a list of (component, [64] coefficients) in coding order"""
    comps = SCANS[scan][0]
    geo, (mh, mw) = geometry(h, w, sampling)
    out = []
    if len(comps) == 3:
        for i in range(mh):
            iv = []
            for j in range(mw):
                if sampling == 0:
                    iv += [(c, planes[c][i, j]) for c in range(3)]
                else:
                    iv += [(0, planes[0][2 * i + a, 2 * j + b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
                    iv += [(1, planes[1][i, j]), (2, planes[2][i, j])]
            out.append(iv)
        return out
    c = comps[0]
    rows, cols = geo[c][2], geo[c][3]
    return [[(c, planes[c][i, j]) for j in range(cols)] for i in range(rows)]


def restart_interval(h, w, sampling, scan):
    geo, (mh, mw) = geometry(h, w, sampling)
    comps = SCANS[scan][0]
    return mw if len(comps) == 3 else geo[comps[0]][3]


# ---- the four coders (jcphuff.c) -------------------------------------------------------------------------------------------------------
def _size_bits(v):
    s = int(abs(v)).bit_length()
    return s, ((v if v >= 0 else v - 1) & ((1 << s) - 1))


def walk(scan, blocks):
    """one restart interval of one scan -> the coder's output in order: ('sym', table slot, symbol) | ('bits', value, count)"""
    comps, ss, se, ah, al = SCANS[scan]
    out = []
    if ss == 0 and ah == 0:                                  # DC first: the arithmetic shift of the signed value
        last = [0, 0, 0]
        for c, zz in blocks:
            v = int(zz[0]) >> al
            if int(zz[0]) < 0:
                EVENTS["dc_negative_shift"] += 1
            s, bits = _size_bits(v - last[c])
            last[c] = v
            EVENTS["dc_size_%d" % s] += 1
            out.append(("sym", table_slot(scan, c), s))
            if s:
                out.append(("bits", bits, s))
        return out
    if ss == 0:                                              # DC refinement: one bit per block
        return [("bits", (int(zz[0]) >> al) & 1, 1) for _, zz in blocks]
    assert len(blocks) <= 1024                               # so EOBRUN never reaches 0x7FFF
    slot = table_slot(scan, comps[0])
    eobrun, be = 0, []                                       # be: the correction bits that travel with EOBRUN

    def emit_eobrun(why):
        nonlocal eobrun, be
        if eobrun:
            n = eobrun.bit_length() - 1
            EVENTS["eobrun_" + why] += 1
            if eobrun >= len(blocks) and why == "restart":
                EVENTS["eobrun_whole_interval"] += 1
            out.append(("sym", slot, n << 4))
            if n:
                out.append(("bits", eobrun & ((1 << n) - 1), n))
            out.extend(("bits", b, 1) for b in be)
            eobrun, be = 0, []

    for bi, (_, zz) in enumerate(blocks):
        if ah == 0:                                          # AC first: the shift is of the magnitude
            r = 0
            for k in range(ss, se + 1):
                v = int(zz[k])
                a = abs(v) >> al
                if a == 0:
                    if v:
                        EVENTS["ac_shifted_to_zero"] += 1
                    r += 1
                    continue
                if eobrun:
                    if bi == len(blocks) - 1 and sum(1 for x in zz[ss:se + 1] if abs(int(x)) >> al) == 1:
                        EVENTS["run_broken_in_last_block"] += 1
                    emit_eobrun("block")
                while r > 15:
                    EVENTS["zrl_first"] += 1
                    out.append(("sym", slot, 0xF0))
                    r -= 16
                s = a.bit_length()
                EVENTS["ac_size_%d_al%d" % (s, al)] += 1
                out.append(("sym", slot, (r << 4) | s))
                out.append(("bits", (a if v > 0 else ~a) & ((1 << s) - 1), s))
                r = 0
            if r:
                eobrun += 1
                assert eobrun < 0x7FFF
            continue
        av = [abs(int(zz[k])) >> al for k in range(64)]      # AC refinement
        eob = max([k for k in range(ss, se + 1) if av[k] == 1], default=0)
        r, br = 0, []
        for k in range(ss, se + 1):
            if av[k] == 0:
                r += 1
                continue
            if r > 15 and k > eob:
                EVENTS["refine_zrl_suppressed"] += 1
            while r > 15 and k <= eob:
                emit_eobrun("block")
                EVENTS["zrl_refine"] += 1
                out.append(("sym", slot, 0xF0))
                r -= 16
                out.extend(("bits", b, 1) for b in br)
                br = []
            if av[k] > 1:
                br.append(av[k] & 1)
                continue
            emit_eobrun("block")
            out.append(("sym", slot, (r << 4) | 1))
            out.append(("bits", 0 if int(zz[k]) < 0 else 1, 1))
            out.extend(("bits", b, 1) for b in br)
            br = []
            r = 0
        if r > 15 and eob:
            EVENTS["refine_trailing_zeros_no_zrl"] += 1
        if r > 0 or br:
            eobrun += 1
            be += br
            assert eobrun < 0x7FFF
            if len(be) > MAX_CORR_BITS - 64 + 1:
                EVENTS["corr_bits_early_flush"] += 1
                emit_eobrun("early")
    emit_eobrun("restart")
    return out


# ---- the file --------------------------------------------------------------------------------------------------------------------------
def histograms(planes, h, w, sampling):
    """[10][256] counts, in TABLES order"""
    hist = np.zeros((len(TABLES), 256), np.int64)
    for scan in range(len(SCANS)):
        for iv in intervals(planes, h, w, sampling, scan):
            for item in walk(scan, iv):
                if item[0] == "sym":
                    hist[item[1], item[2]] += 1
    return hist


def fixed_head(h, w, quality, sampling):
    opt.check(quality, sampling)
    out = b"\xff\xd8" + base._seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(opt.quant_tables(quality)):
        out += base._seg(0xDB, bytes([i]) + bytes(q[opt.ZIGZAG[k]] for k in range(64)))
    return out + base._seg(0xC2, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22 if sampling == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))


FIXED_HEAD_BYTES = 2 + 18 + 69 + 69 + 19


def sos(scan):
    comps, ss, se, ah, al = SCANS[scan]
    body = bytes([len(comps)])
    for c in comps:                                          # (jcmarker.c: a progressive scan names only the table it uses)
        t = 0 if c == 0 else 1
        body += bytes([c + 1, (0 if ah else t << 4) if ss == 0 else t])
    return base._seg(0xDA, body + bytes([ss, se, (ah << 4) | al]))


def scan_head(scan, tabs, h, w, sampling, prev_interval):
    """the DHT segments of the scan's tables, the DRI where the interval changes, the SOS; and the interval now in force"""
    out = b""
    for t, (sc, tc_th) in enumerate(TABLES):
        if sc == scan:
            out += base._seg(0xC4, bytes([tc_th]) + bytes(tabs[t][0]) + bytes(tabs[t][1]))
    ri = restart_interval(h, w, sampling, scan)
    if ri != prev_interval:
        out += base._seg(0xDD, struct.pack(">H", ri))
    return out + sos(scan), ri


def interval_bytes(items, codes):
    acc, nbits = 0, 0
    for item in items:
        if item[0] == "sym":
            v, l = codes[item[1]][item[2]]
        else:
            _, v, l = item
        acc = (acc << l) | v
        nbits += l
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def file_from_planes(planes, h, w, quality, sampling):
    assert 1 <= h <= 8192 and 1 <= w <= 8192
    tabs = [huff.gen_optimal_table(c)[:2] for c in histograms(planes, h, w, sampling)]
    codes = [base.huffman_codes(b, v) for b, v in tabs]
    once = dict(EVENTS)                                      # (the emit pass walks again: an event counts once)
    parts = [fixed_head(h, w, quality, sampling)]
    ri = 0
    for scan in range(len(SCANS)):
        head, ri = scan_head(scan, tabs, h, w, sampling, ri)
        parts.append(head)
        ivs = intervals(planes, h, w, sampling, scan)
        for m, iv in enumerate(ivs):
            parts.append(interval_bytes(walk(scan, iv), codes))
            if m != len(ivs) - 1:
                parts.append(bytes([0xFF, 0xD0 + (m & 7)]))
    EVENTS.clear()
    EVENTS.update(once)
    return b"".join(parts) + b"\xff\xd9"


def jpeg_file(px, quality=85, sampling=0):
    px = np.ascontiguousarray(px, np.uint8)
    return file_from_planes(planes_of(px, quality, sampling), px.shape[0], px.shape[1], quality, sampling)


def jpeg_base64(px, quality=85, sampling=0):
    return base64.b64encode(jpeg_file(px, quality, sampling))


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
# Any table: a code has at most 16 bits.  Per scan and block:
#   DC first        16 + the largest category of a difference of two shifted DCs: the quantised DC lies in -A..B (jpeg_opt_model), the
#                   shifted one in -ceil(A / 2)..floor(B / 2)
#   DC refinement   1 bit
#   AC first        every position of the band at 16 + the largest category of its magnitude after the shift (a ZRL stands for 16
#                   zero positions, each priced at 16 or more), and one EOBn symbol with 14 extra bits
#   AC refinement   every position at 16 + 1 (the sign) + 1 (a correction bit), and one EOBn symbol with 14 extra bits
# An interval is its blocks' bits rounded up to bytes, doubled for the stuffing, and 2 bytes of marker.  A scan's head is at most two
# DHT segments of 16 + 256 entries, a DRI and a three-component SOS.
SCAN_HEAD_MAX = 2 * (5 + 16 + 256) + 6 + 14
EOBN_BITS = 16 + 14


def block_bits(scan, comp, quality):
    comps, ss, se, ah, al = SCANS[scan]
    table = 0 if comp == 0 else 1
    q = opt.quant_tables(quality)[table]
    if ss == 0:
        if ah:
            return 1
        a, b = (opt.DC_MIN + 4 * q[0]) // (8 * q[0]), (opt.DC_MAX + 4 * q[0]) // (8 * q[0])
        return 16 + ((b >> al) + -(-a >> al)).bit_length()
    if ah:
        return (se - ss + 1) * 18 + EOBN_BITS
    bits = EOBN_BITS
    for k in range(ss, se + 1):
        n = opt.ZIGZAG[k]
        bits += 16 + (((opt.coef_bound(n) + 4 * q[n]) // (8 * q[n])) >> al).bit_length()
    return bits


def interval_bound(h, w, quality, sampling, scan):
    """bytes of one interval of the scan, marker included"""
    geo, (mh, mw) = geometry(h, w, sampling)
    comps = SCANS[scan][0]
    if len(comps) == 3:
        bits = mw * ((4 if sampling == 2 else 1) * block_bits(scan, 0, quality) + 2 * block_bits(scan, 1, quality))
    else:
        bits = geo[comps[0]][3] * block_bits(scan, comps[0], quality)
    return 2 * ((bits + 7) // 8) + 2


def scan_intervals(h, w, sampling, scan):
    geo, (mh, mw) = geometry(h, w, sampling)
    comps = SCANS[scan][0]
    return mh if len(comps) == 3 else geo[comps[0]][2]


def file_bound(h, w, quality, sampling):
    opt.check(quality, sampling)
    n = FIXED_HEAD_BYTES + 2
    for scan in range(len(SCANS)):
        n += SCAN_HEAD_MAX + scan_intervals(h, w, sampling, scan) * interval_bound(h, w, quality, sampling, scan)
    return n


def base64_bound(h, w, quality, sampling):
    if not (1 <= h <= 8192 and 1 <= w <= 8192 and 1 <= quality <= 100 and sampling in opt.R_OF):
        return 0
    return (file_bound(h, w, quality, sampling) + 2) // 3 * 4
