"""The JPEG encoder without a GPU: the Python model of the format (tests/jpeg_model.py) held to the published format by an independent
decoder (Pillow / libjpeg-turbo), by a marker walk and by an entropy decoder written here from the standard; the model's bytes against
libjpeg-turbo's own file for the same settings; the worst-case bound; csrc/jpeg_tables.hpp against the model's constants (a
stand-alone program under the address and undefined-behaviour sanitizers); the C ABI's new symbols and flag."""
import base64
import ctypes
import io
import os
import struct
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as cases      # noqa: E402
import jpeg_model as model      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = model.R
SIZES = [(1, 1), (5, 7), (64, 64), (750, 1000), (1024, 1024), (1365, 2048), (8192, 8192)]
OUT_OF_RANGE = [(0, 8), (8, 0), (-1, 8), (8, -8), (8193, 8), (8, 8193), (0, 0)]


@pytest.fixture(scope="module")
def all_cases():
    return {k: (px, model.jpeg_file(px)) for k, px in cases.all_cases().items()}


def pillow_file(px):
    """libjpeg-turbo through Pillow with the model's settings"""
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=85, subsampling=0, optimize=False, restart_marker_blocks=R)
    return bio.getvalue()


def pillow_decode(f):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # a truncated or corrupt scan is a warning in libjpeg, an exception here
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.format == "JPEG" and im.mode == "RGB"
        return np.asarray(im)


# ---- a marker walk and an entropy decoder, from the standard (not from the model's encoder) ------------------------------------------
def segments(f):
    """-> ([(marker, payload)] up to and including SOS, [(interval bytes still stuffed, the marker behind it)])"""
    assert f[:2] == b"\xff\xd8"
    segs, o = [], 2
    while True:
        assert f[o] == 0xFF
        marker = f[o + 1]
        n, = struct.unpack(">H", f[o + 2:o + 4])
        segs.append((marker, f[o + 4:o + 2 + n]))
        o += 2 + n
        if marker == 0xDA:
            break
    ivs, start = [], o
    while o < len(f):
        if f[o] == 0xFF:
            nxt = f[o + 1]
            assert nxt == 0x00 or 0xD0 <= nxt <= 0xD7 or nxt == 0xD9, "an unstuffed 0xFF inside entropy data at %d" % o      # (also: o + 1 exists)
            if nxt != 0x00:
                ivs.append((f[start:o], nxt))
                start = o + 2
            o += 2
        else:
            o += 1
    assert start == len(f) and ivs[-1][1] == 0xD9
    return segs, ivs


def dht_tables(segs):
    """{(class, id): {(length, code): symbol}} from the file's own DHT segments"""
    out = {}
    for marker, p in segs:
        if marker != 0xC4:
            continue
        tc_th, bits, vals = p[0], p[1:17], p[17:]
        assert sum(bits) == len(vals)
        t, code, k = {}, 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                t[(length, code)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        out[(tc_th >> 4, tc_th & 15)] = t
    return out


def decode_interval(stuffed, tables):
    """one restart interval -> ([block: 64 zig-zag coefficients, DC as the DIFFERENCE], [AC symbols seen])"""
    raw = stuffed.replace(b"\xff\x00", b"\xff")
    bits = "".join(format(b, "08b") for b in raw)
    pos, blocks, syms = 0, [], []

    def symbol(t):
        nonlocal pos
        code, length = 0, 0
        while True:
            code = (code << 1) | int(bits[pos]); pos += 1; length += 1
            if (length, code) in t:
                return t[(length, code)]
            assert length < 16

    def value(s):
        nonlocal pos
        if s == 0:
            return 0
        v = int(bits[pos:pos + s], 2); pos += s
        return v if v >> (s - 1) else v - (1 << s) + 1

    while len(bits) - pos >= 8 or (pos < len(bits) and "0" in bits[pos:]):
        c = len(blocks) % 3
        tb = 0 if c == 0 else 1
        zz = [0] * 64
        zz[0] = value(symbol(tables[(0, tb)]))
        k = 1
        while k < 64:
            rs = symbol(tables[(1, tb)])
            syms.append(rs)
            if rs == 0x00:
                break
            if rs == 0xF0:
                k += 16
                continue
            k += rs >> 4
            zz[k] = value(rs & 15)
            k += 1
        assert k <= 64
        blocks.append(zz)
    assert set(bits[pos:]) <= {"1"} and len(bits) - pos < 8          # padded with 1-bits to the byte
    return blocks, syms


@pytest.fixture(scope="module")
def decoded(all_cases):
    """name -> (segments, [(blocks, symbols, marker) per interval])"""
    out = {}
    for name, (px, f) in all_cases.items():
        segs, ivs = segments(f)
        t = dht_tables(segs)
        out[name] = (segs, [decode_interval(b, t) + (m,) for b, m in ivs])
    return out


def test_pillow_decodes_the_model_files(all_cases):
    for name, (px, f) in all_cases.items():
        got = pillow_decode(f)
        assert got.shape == px.shape, name
    # flat images keep only their DCs: the DC quantiser's step is 5 * 8 on a DC of 8 * 64 samples / 8 (under a grey level), the two
    # colour transforms round once each
    for name in ("black", "white"):
        px, f = all_cases[name]
        assert np.abs(pillow_decode(f).astype(int) - px.astype(int)).max() <= 2, name


def test_marker_walk_and_interval_structure(all_cases, decoded):
    for name, (px, f) in all_cases.items():
        h, w, _ = px.shape
        segs, ivs = decoded[name]
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA], name
        assert segs[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert [p[0] for m, p in segs if m == 0xDB] == [0, 1] and [p[0] for m, p in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
        sof = segs[3][1]
        assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, 3) and sof[6:] == bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert struct.unpack(">H", segs[8][1]) == (R,)
        assert len(f) == model.HEADER_BYTES + sum(len(b) + 2 for b, _ in segments(f)[1])
        nmcu = ((h + 7) // 8) * ((w + 7) // 8)
        assert len(ivs) == (nmcu + R - 1) // R, name
        for m, (blocks, _, marker) in enumerate(ivs):
            last = m == len(ivs) - 1
            assert marker == (0xD9 if last else 0xD0 + m % 8), (name, m)                     # RST0..RST7 and round again
            assert len(blocks) == 3 * (nmcu - R * (len(ivs) - 1) if last else R), (name, m)   # every interval but the last holds R MCUs
        # the decoded coefficients are the model's own: differential DC from 0 in every interval
        q = model.quantised_blocks(px).reshape(-1, 3, 64)
        for m, (blocks, _, _) in enumerate(ivs):
            pred = [0, 0, 0]
            for k, zz in enumerate(blocks):
                want = q[m * R + k // 3][k % 3]
                assert zz[0] + pred[k % 3] == want[0] and zz[1:] == want[1:].tolist(), (name, m, k)
                pred[k % 3] = int(want[0])


def test_the_cases_reach_what_they_name(all_cases, decoded):
    n = {k: len(v[1]) for k, v in decoded.items()}
    assert n["1x1"] == n["7x5"] == n["8x8"] == 1 and n["9x17"] == 1 and n["rst_wraps"] == 12 > 8
    assert (88 // 8) % R != 0 and n["wrap40x88"] == 4 and (136 // 8) % R != 0 and n["wrap24x136"] == 4      # intervals wrap across MCU rows
    for name in ("black", "white"):                                                           # DC and EOB only
        assert all(set(syms) == {0x00} for _, syms, _ in decoded[name][1])
    assert any(0xF0 in syms for _, syms, _ in decoded["ramp_high"][1])                        # a zero run of at least 16: ZRL
    px, f = all_cases["noise160"]
    assert b"\xff\x00" in f[model.HEADER_BYTES:]                                              # a stuffed byte
    # the largest categories the bound allows for are reached: the DC difference of full-scale block swings, the highest frequency
    smax = (model.size_max(0), model.size_max(1))
    dc = max(abs(zz[0]) for _, ivs in [decoded["checker8"]] for blocks, _, _ in ivs for zz in blocks[0::3])
    assert int(dc).bit_length() == smax[0][0]
    hf = max(abs(zz[63]) for _, ivs in [decoded["checker1"]] for blocks, _, _ in ivs for zz in blocks[0::3])
    assert int(hf).bit_length() == smax[0][63]
    cdc = max(abs(zz[0]) for _, ivs in [decoded["saturated"]] for blocks, _, _ in ivs for k, zz in enumerate(blocks) if k % 3)
    assert int(cdc).bit_length() == smax[1][0]
    for name, (px, f) in all_cases.items():
        _, ivs = decoded[name]
        for blocks, _, _ in ivs:
            for k, zz in enumerate(blocks):
                sm = smax[1 if k % 3 else 0]
                assert all(int(abs(v)).bit_length() <= sm[p] for p, v in enumerate(zz)), name


def test_model_equals_libjpeg_turbo(all_cases):
    """The pin against the reference's codec family: byte equality with Pillow's file (libjpeg-turbo; quality 85, 4:4:4, fixed tables,
    the same restart interval) on every case.  profiles/jpeg_device.md records it."""
    for name, (px, f) in all_cases.items():
        p = pillow_file(px)
        first = next((i for i, (a, b) in enumerate(zip(f, p)) if a != b), None)
        print("%-14s model %6d  libjpeg-turbo %6d  first difference %s" % (name, len(f), len(p), first))
        assert f == p, (name, first)


def test_file_length_mod_3_seeds(all_cases):
    for r in (0, 1, 2):
        px, f = all_cases["mod3_%d" % r]
        assert len(f) % 3 == r
        assert model.jpeg_base64(px) == base64.b64encode(f) and model.jpeg_base64(px).count(b"=") == (3 - r) % 3


def _argmax_block(table):
    """A coefficient block (zig-zag, the DC as a difference from 0) that takes model.block_bits_max(table) bits: the same dynamic
    programme with back pointers, restated here."""
    smax = model.size_max(table)
    dc, ac = model.DC_CODES[table], model.AC_CODES[table]
    best, back = [0] * 64, [None] * 64
    s0 = max(range(smax[0] + 1), key=lambda s: dc[s][1] + s)
    best[0] = dc[s0][1] + s0
    for p in range(1, 64):
        for prev in range(p):
            run = p - prev - 1
            s = max(range(1, smax[p] + 1), key=lambda s: ac[((run & 15) << 4) | s][1] + s)
            v = best[prev] + (run >> 4) * ac[0xF0][1] + ac[((run & 15) << 4) | s][1] + s
            if v > best[p]:
                best[p], back[p] = v, (prev, s)
    end = max(range(64), key=lambda p: best[p] + (ac[0x00][1] if p < 63 else 0))
    zz = [0] * 64
    p = end
    while p:
        prev, s = back[p]
        zz[p] = (1 << s) - 1
        p = prev
    zz[0] = (1 << s0) - 1
    return zz


def test_bound(all_cases):
    lib = _lib.load()
    assert R <= 64 and model.MCU_BITS_MAX == 2343
    for table in (0, 1):                      # the bound of a block is reached by a real symbol sequence, and by nothing longer
        zz = _argmax_block(table)
        assert sum(l for _, l in model.block_symbols(zz, 0, table)) == model.block_bits_max(table)
        rng = np.random.default_rng(table)
        smax = np.array(model.size_max(table))
        for _ in range(200):
            mag = rng.integers(0, 1 << smax) * (rng.random(64) < rng.random())
            zz = (mag * rng.choice([-1, 1], 64)).tolist()
            assert sum(l for _, l in model.block_symbols(zz, 0, table)) <= model.block_bits_max(table)
    # the amplitude table behind the categories: no quantised coefficient of full-scale patterns (every sample at +-full scale with
    # the sign of one basis function) exceeds it
    y, x = np.mgrid[:8, :8]
    worst = np.zeros(64, np.int64)
    for u in range(8):
        for v in range(8):
            basis = np.cos((2 * y + 1) * u * np.pi / 16) * np.cos((2 * x + 1) * v * np.pi / 16)
            for sign in (1, -1):
                blk = np.where(sign * basis >= 0, 127, -128)
                worst = np.maximum(worst, np.abs(model.fdct_islow(blk[None])[0].reshape(64)))
    assert (worst <= np.array(model.COEF_MAX)).all() and (worst >= np.array(model.COEF_MAX) - 16 - 8 * 8).all()      # (-128 / +127: up to 64 units short)
    for name, (px, f) in all_cases.items():
        h, w, _ = px.shape
        assert len(f) <= model.file_bound(h, w), name
        assert lib.ire_jpeg_base64_bound(h, w) == model.base64_bound(h, w) >= len(model.jpeg_base64(px))
    for h, w in SIZES:
        assert lib.ire_jpeg_base64_bound(h, w) == model.base64_bound(h, w) > 0
    for h, w in OUT_OF_RANGE:
        assert lib.ire_jpeg_base64_bound(h, w) == 0 == model.base64_bound(h, w), (h, w)


def test_tables_header_against_the_model(tmp_path):
    """csrc/jpeg_tables.hpp, compiled alone with -fsanitize=address,undefined: its tables, heads and bounds are the model's."""
    exe = str(tmp_path / "jpeg_tables_dump")
    src = os.path.join(ROOT, "tests", "native", "jpeg_tables_dump.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    args = [str(v) for hw in SIZES + [(8192, 1), (1, 8192)] for v in hw]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())

    def ints(key):
        return [int(v) for v in got[key].split()]

    def codes(key):
        return {int(a): (int(b), int(c)) for a, b, c in (item.split("/") for item in got[key].split())}

    assert ints("R") == [R] and ints("header_bytes") == [model.HEADER_BYTES] and ints("mcu_bits_max") == [model.MCU_BITS_MAX]
    assert ints("zigzag") == model.ZIGZAG and ints("coef_max") == model.COEF_MAX
    for t, q in enumerate((model.Q_LUM, model.Q_CHR)):
        assert ints("quant%d" % t) == q and ints("size_max%d" % t) == model.size_max(t) and ints("block_bits_max%d" % t) == [model.block_bits_max(t)]
        assert codes("dc%d" % t) == model.DC_CODES[t] and codes("ac%d" % t) == model.AC_CODES[t]
    for h, w in SIZES + [(8192, 1), (1, 8192)]:
        assert bytes.fromhex(got["header %d %d" % (h, w)]) == model.header(h, w)
        assert ints("bound %d %d" % (h, w)) == [model.file_bound(h, w), model.base64_bound(h, w)]
    assert ints("recip_checked") == [2 * 64 * 65536]


def test_abi_symbols_and_flag():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ire_jpeg_base64_bound", "ire_encode_jpeg_base64_fit_device", "ire_encode_jpeg_base64_fit", "ire_poll_text"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert _lib.IRE_FLAG_RESULT_JPEG == 8
    import torch
    h = ctypes.c_void_p()
    cfg = _lib.IreConfig()
    cfg.struct_size = ctypes.sizeof(_lib.IreConfig)
    cfg.max_batch = 2
    for bad in (9, 12, 10, 16, 24):          # JPEG with either PNG result; 2 is no flag; nor is any higher bit
        cfg.flags = bad
        assert lib.ire_init(ctypes.byref(cfg), ctypes.byref(h)) == _lib.IRE_ERR_INVALID_INPUT
        assert b"flags" in lib.ire_last_error()
    cfg.flags = 8                            # accepted as far as the device check
    st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
    if torch.cuda.is_available():
        assert st == _lib.IRE_OK, lib.ire_last_error()
        lib.ire_shutdown(h)
    else:
        assert st == _lib.IRE_ERR_UNAVAILABLE and b"flags" not in lib.ire_last_error()
    # null handles are rejected, not dereferenced
    assert lib.ire_encode_jpeg_base64_fit(None, None, 1, 5, 7, None, 4096, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_jpeg_base64_fit_device(None, None, 1, 5, 7, 21, 105, None, 4096, None, None) == _lib.IRE_ERR_INVALID_INPUT
